"""Expected results for the attention entry point and the decoder counterpart, composed in Python from the
oracle's primitives (oracle/oracle.py): mm_fp32, softmax_rows, quantized_mm, linear, add_layernorm_rows, uniform
and encoder_weight_seed.  TEST INFRASTRUCTURE ONLY.

encoder_forward_ref is the same composition for the encoder; tests/test_attn_oracle_host.py holds it against the
committed C restatement (oracle.encoder_forward) bit for bit, which pins the weight layout and the order of the
steps that decoder_forward_ref shares with it.
"""
import math

import numpy as np

from oracle import oracle as O

# weight kinds (include/qgemm.h): 0..7 the encoder's, 8..11 the decoder's cross-attention
WQ, WK, WV, WO, W1, B1, W2, B2, WQ2, WK2, WV2, WO2 = range(12)


def init_bound(n: int) -> float:
    """fl32(1 / sqrt(n)): the reference's "float max = 1.0f / std::sqrt(n)" with an int n."""
    return float(np.float32(1.0 / math.sqrt(float(n))))


def default_scale(dk: int) -> float:
    return init_bound(dk)  # attention.cuh:64, the same expression


def attention_scores(Q, K, n_heads: int):
    """S_h = Q_h K_h^T per head, the reference's op_mm<float> chain: what attention_ref hands to its softmax."""
    Q, K = (np.asarray(a, dtype=np.float32) for a in (Q, K))
    dk = Q.shape[1] // n_heads
    heads = [slice(h * dk, (h + 1) * dk) for h in range(n_heads)]
    return [O.mm_fp32(np.ascontiguousarray(Q[:, c]), np.ascontiguousarray(K[:, c].T)) for c in heads]


def attention_ref(Q, K, V, n_heads: int, scale: float, exp_tables=None) -> np.ndarray:
    """Per head h (columns h*d_k ..): softmax(Q_h K_h^T * scale) V_h with the reference's op_mm<float> chains.
    exp_tables, when given, holds per head the value to use for exp of every O.softmax_args(S_h, scale) (the
    reference pin's hook, O.softmax_rows_table); otherwise exp is the oracle's own."""
    Q, K, V = (np.asarray(a, dtype=np.float32) for a in (Q, K, V))
    seq_q, d = Q.shape
    assert d % n_heads == 0 and K.shape == V.shape and K.shape[1] == d
    dk = d // n_heads
    out = np.empty((seq_q, d), np.float32)
    for h in range(n_heads):
        c = slice(h * dk, (h + 1) * dk)
        S = O.mm_fp32(np.ascontiguousarray(Q[:, c]), np.ascontiguousarray(K[:, c].T))
        P = O.softmax_rows(S, scale) if exp_tables is None else O.softmax_rows_table(S, exp_tables[h], scale)
        out[:, c] = O.mm_fp32(P, np.ascontiguousarray(V[:, c]))
    return out


def head_weights(d: int, dk: int, n_heads: int, seed: int, block: int, kinds) -> np.ndarray:
    """[W_kind0 | W_kind1 | ...], every kind all heads side by side: one d x d_k tensor per (kind, head)."""
    bd = init_bound(dk)
    cols = [O.uniform((d, dk), O.encoder_weight_seed(seed, block, kind, h), -bd, bd)
            for kind in kinds for h in range(n_heads)]
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def _self_attention(x, d, H, seed, block):
    """The encoder's first half: projections, attention, output projection, add + layernorm."""
    dk = d // H
    qkv = O.quantized_mm(x, head_weights(d, dk, H, seed, block, (WQ, WK, WV)))
    heads = attention_ref(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], H, default_scale(dk))
    t = O.quantized_mm(heads, O.uniform((d, d), O.encoder_weight_seed(seed, block, WO, 0), -1.0, 1.0))
    return O.add_layernorm_rows(t, heads), heads


def _ffn(x, residual, d, dff, seed, block):
    bd, bf = init_bound(d), init_bound(dff)
    w1 = O.uniform((d, dff), O.encoder_weight_seed(seed, block, W1, 0), -bd, bd)
    b1 = O.uniform((dff,), O.encoder_weight_seed(seed, block, B1, 0), -bd, bd)
    w2 = O.uniform((dff, d), O.encoder_weight_seed(seed, block, W2, 0), -bf, bf)
    b2 = O.uniform((d,), O.encoder_weight_seed(seed, block, B2, 0), -bf, bf)
    t = O.linear(O.linear(x, w1, b1, True), w2, b2, False)
    return O.add_layernorm_rows(t, residual)


def encoder_forward_ref(X, d_model: int, n_heads: int, d_ff: int, n_blocks: int, seed: int) -> np.ndarray:
    x = np.ascontiguousarray(X, dtype=np.float32)
    for i in range(n_blocks):
        x1, heads = _self_attention(x, d_model, n_heads, seed, i)
        x = _ffn(x1, heads, d_model, d_ff, seed, i)
    return x


def decoder_forward_ref(X, enc_out, d_model: int, n_heads: int, d_ff: int, n_blocks: int, seed: int) -> np.ndarray:
    """transformer.cu:91-167 with the quantized linears: self-attention, cross-attention (queries from the decoder
    stream, keys and values from enc_out, its own W_O2), FFN with the cross-attention's multiHeadOut as residual."""
    d, H = d_model, n_heads
    dk = d // H
    x = np.ascontiguousarray(X, dtype=np.float32)
    enc = np.ascontiguousarray(enc_out, dtype=np.float32)
    for i in range(n_blocks):
        x1, _ = _self_attention(x, d, H, seed, i)
        q2 = O.quantized_mm(x1, head_weights(d, dk, H, seed, i, (WQ2,)))
        kv2 = O.quantized_mm(enc, head_weights(d, dk, H, seed, i, (WK2, WV2)))
        heads2 = attention_ref(q2, kv2[:, :d], kv2[:, d:], H, default_scale(dk))
        t = O.quantized_mm(heads2, O.uniform((d, d), O.encoder_weight_seed(seed, i, WO2, 0), -1.0, 1.0))
        x2 = O.add_layernorm_rows(t, heads2)
        x = _ffn(x2, heads2, d, d_ff, seed, i)
    return x
