"""Expected results for the causal mask (qgemm_softmax_rows_causal, qgemm_attention_causal, the causal Decoder),
composed in Python from the oracle's primitives: mm_fp32, softmax_rows called per row on its first L_i columns with
zeros after, and attn_oracle's weight and FFN helpers.  TEST INFRASTRUCTURE ONLY.

Query row i sees keys 0 .. L_i - 1, L_i = min(seq_kv, i + q_pos0 + 1).  The masked columns of P are +0 and P V runs
over every key, so a masked key contributes fmaf(+0, v, acc).
"""
import functools

import numpy as np

import attn_oracle
from oracle import oracle as O

# (seq_q, seq_kv, heads, d_k, q_pos0): the smallest shapes at which each mechanism of the kernels can go wrong
SHAPES = (
    (1, 1, 1, 1, 0),           # the smallest possible call
    (33, 33, 2, 24, 0),        # two query tiles with a tail
    (40, 289, 2, 24, 249),     # limits cross the 256-key chunk inside a tile
    (70, 40, 1, 33, 0),        # more queries than keys, with an odd d_k
    (64, 64, 1, 64, 0),        # limits at multiples of 16, 32 and 64
    (512, 512, 1, 64, 0),      # the edge of the fused envelope
    (20, 513, 2, 8, 493),      # the fallback on seq_kv
    (20, 40, 1, 65, 20),       # the fallback on d_k
)
SEED = 211  # Q, K, V of a shape from seeds SEED, SEED + 1, SEED + 2


def limits(seq_q: int, seq_kv: int, q_pos0: int) -> np.ndarray:
    """L_i for i = 0 .. seq_q - 1 (always >= 1)."""
    assert q_pos0 >= 0 and seq_kv >= 1
    return np.minimum(seq_kv, np.arange(seq_q, dtype=np.int64) + q_pos0 + 1)


def softmax_rows_causal(S, seq_q: int, q_pos0: int = 0, scale: float = 1.0) -> np.ndarray:
    """S: a stack of matrices of seq_q rows (any leading shape, last axis w).  Row r is query i = r % seq_q: the
    oracle's softmax_rows on its first L_i columns, +0 after."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    w = S.shape[-1]
    flat = S.reshape(-1, w)
    assert flat.shape[0] % seq_q == 0
    L = limits(seq_q, w, q_pos0)
    P = np.zeros_like(flat)
    for r in range(flat.shape[0]):
        n = int(L[r % seq_q])
        P[r, :n] = O.softmax_rows(np.ascontiguousarray(flat[r:r + 1, :n]), scale)[0]
    return P.reshape(S.shape)


def attention_causal_ref(Q, K, V, n_heads: int, scale: float, q_pos0: int) -> np.ndarray:
    """Per head: mm_fp32, softmax_rows_causal, mm_fp32 over all seq_kv keys."""
    Q, K, V = (np.asarray(a, dtype=np.float32) for a in (Q, K, V))
    seq_q, d = Q.shape
    assert d % n_heads == 0 and K.shape == V.shape and K.shape[1] == d
    dk = d // n_heads
    out = np.empty((seq_q, d), np.float32)
    for h in range(n_heads):
        c = slice(h * dk, (h + 1) * dk)
        S = O.mm_fp32(np.ascontiguousarray(Q[:, c]), np.ascontiguousarray(K[:, c].T))
        P = softmax_rows_causal(S, seq_q, q_pos0, scale)
        out[:, c] = O.mm_fp32(P, np.ascontiguousarray(V[:, c]))
    return out


def qkv(shape, seed: int = SEED):
    seq_q, seq_kv, H, dk, _ = shape
    d = H * dk
    return O.uniform((seq_q, d), seed), O.uniform((seq_kv, d), seed + 1), O.uniform((seq_kv, d), seed + 2)


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def expected(shape) -> np.ndarray:
    """attention_causal_ref on qkv(shape) at the default scale: computed once per process, read-only."""
    Q, K, V = qkv(shape)
    return _frozen(attention_causal_ref(Q, K, V, shape[2], attn_oracle.default_scale(shape[3]), shape[4]))


@functools.lru_cache(maxsize=None)
def expected_unmasked(shape) -> np.ndarray:
    Q, K, V = qkv(shape)
    return _frozen(attn_oracle.attention_ref(Q, K, V, shape[2], attn_oracle.default_scale(shape[3])))


def _self_attention_causal(x, d, H, seed, block):
    """attn_oracle._self_attention with the mask at q_pos0 = 0."""
    dk = d // H
    qkv_ = O.quantized_mm(x, attn_oracle.head_weights(d, dk, H, seed, block, (attn_oracle.WQ, attn_oracle.WK,
                                                                               attn_oracle.WV)))
    heads = attention_causal_ref(qkv_[:, :d], qkv_[:, d:2 * d], qkv_[:, 2 * d:], H, attn_oracle.default_scale(dk), 0)
    t = O.quantized_mm(heads, O.uniform((d, d), O.encoder_weight_seed(seed, block, attn_oracle.WO, 0), -1.0, 1.0))
    return O.add_layernorm_rows(t, heads)


def decoder_forward_causal_ref(X, enc_out, d_model: int, n_heads: int, d_ff: int, n_blocks: int,
                               seed: int) -> np.ndarray:
    """attn_oracle.decoder_forward_ref with the causal mask on every block's self-attention (q_pos0 = 0); the
    cross-attention stays unmasked."""
    d, H = d_model, n_heads
    dk = d // H
    x = np.ascontiguousarray(X, dtype=np.float32)
    enc = np.ascontiguousarray(enc_out, dtype=np.float32)
    for i in range(n_blocks):
        x1 = _self_attention_causal(x, d, H, seed, i)
        q2 = O.quantized_mm(x1, attn_oracle.head_weights(d, dk, H, seed, i, (attn_oracle.WQ2,)))
        kv2 = O.quantized_mm(enc, attn_oracle.head_weights(d, dk, H, seed, i, (attn_oracle.WK2, attn_oracle.WV2)))
        heads2 = attn_oracle.attention_ref(q2, kv2[:, :d], kv2[:, d:], H, attn_oracle.default_scale(dk))
        t = O.quantized_mm(heads2, O.uniform((d, d), O.encoder_weight_seed(seed, i, attn_oracle.WO2, 0), -1.0, 1.0))
        x2 = O.add_layernorm_rows(t, heads2)
        x = attn_oracle._ffn(x2, heads2, d, d_ff, seed, i)
    return x


# the decoder shapes of tests/test_gpu_decoder_causal.py: (seq, enc_seq, d_model, heads, d_ff, blocks)
DECODER_FUSED = (40, 33, 64, 2, 128, 2)
DECODER_FALLBACK = (513, 33, 16, 2, 128, 2)   # self-attention on the three launches (seq 513 > 512)
DECODER_SEED = 223


def decoder_inputs(shape):
    seq, enc_seq, d = shape[:3]
    return O.uniform((seq, d), DECODER_SEED + 1), O.uniform((enc_seq, d), DECODER_SEED + 2)


@functools.lru_cache(maxsize=None)
def decoder_expected(shape, causal: bool = True, rows=None) -> np.ndarray:
    """The decoder's forward on the first `rows` rows of decoder_inputs(shape) (all of them by default)."""
    X, enc = decoder_inputs(shape)
    X = X if rows is None else X[:rows]
    f = decoder_forward_causal_ref if causal else attn_oracle.decoder_forward_ref
    return _frozen(f(X, enc, shape[2], shape[3], shape[4], shape[5], DECODER_SEED))
