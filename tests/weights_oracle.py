"""Expected results for stacks with caller-supplied weights (qgemm_model_set_weight): the block
chains of tests/attn_oracle.py and tests/causal_oracle.py with explicit weight arrays in place of seeds, composed from
the oracle's primitives (quantized_mm, linear, add_layernorm_rows) and those files' attention oracles.  TEST
INFRASTRUCTURE ONLY.

A weight set is a dict keyed (block, kind): the per-head kinds (Wq, Wk, Wv, Wq2, Wk2, Wv2) hold [n_heads, d_model, d_k],
W_O / W_O2 [d_model, d_model], W1 [d_model, d_ff], W2 [d_ff, d_model], b1 [d_ff], b2 [d_model]; all fp32, y = x W.
tests/test_weights_host.py holds the chains against attn_oracle's seeded ones bit for bit with seeded_weights().
"""
import numpy as np

import attn_oracle
import causal_oracle
from attn_oracle import B1, B2, W1, W2, WK, WK2, WO, WO2, WQ, WQ2, WV, WV2
from oracle import oracle as O

HEAD_KINDS = (WQ, WK, WV, WQ2, WK2, WV2)
ENCODER_KINDS = (WQ, WK, WV, WO, W1, B1, W2, B2)
DECODER_KINDS = ENCODER_KINDS + (WQ2, WK2, WV2, WO2)


def weight_shape(kind: int, d: int, H: int, dff: int) -> tuple:
    """The array of one (block, kind) entry."""
    if kind in HEAD_KINDS:
        return (H, d, d // H)
    return {WO: (d, d), WO2: (d, d), W1: (d, dff), W2: (dff, d), B1: (dff,), B2: (d,)}[kind]


def seeded_weights(d: int, H: int, dff: int, n_blocks: int, seed: int, cross: bool = False) -> dict:
    """The arrays a stack created with `seed` draws: qgemm_fill_uniform at encoder_weight_seed(seed, block, kind, head)
    with the documented bounds (1/sqrt(d_k) per head, U(-1, 1) for W_O / W_O2, 1/sqrt(d_model) for W1 / b1,
    1/sqrt(d_ff) for W2 / b2)."""
    dk = d // H
    bk, bd, bf = attn_oracle.init_bound(dk), attn_oracle.init_bound(d), attn_oracle.init_bound(dff)
    bound = {WO: 1.0, WO2: 1.0, W1: bd, B1: bd, W2: bf, B2: bf}
    out = {}
    for i in range(n_blocks):
        for kind in (DECODER_KINDS if cross else ENCODER_KINDS):
            if kind in HEAD_KINDS:
                out[i, kind] = np.stack([O.uniform((d, dk), O.encoder_weight_seed(seed, i, kind, h), -bk, bk)
                                         for h in range(H)])
            else:
                b = bound[kind]
                out[i, kind] = O.uniform(weight_shape(kind, d, H, dff), O.encoder_weight_seed(seed, i, kind, 0), -b, b)
    return out


def fused(W: dict, block: int, kinds) -> np.ndarray:
    """[W_kind0 | W_kind1 | ...], every kind all heads side by side: attn_oracle.head_weights from arrays."""
    return np.ascontiguousarray(np.concatenate([W[block, kind][h] for kind in kinds
                                                for h in range(W[block, kind].shape[0])], axis=1), dtype=np.float32)


def _self_attention(x, W, i, d, H, causal):
    dk = d // H
    qkv = O.quantized_mm(x, fused(W, i, (WQ, WK, WV)))
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    scale = attn_oracle.default_scale(dk)
    heads = (causal_oracle.attention_causal_ref(q, k, v, H, scale, 0) if causal
             else attn_oracle.attention_ref(q, k, v, H, scale))
    t = O.quantized_mm(heads, W[i, WO])
    return O.add_layernorm_rows(t, heads), heads


def _ffn(x, residual, W, i):
    t = O.linear(O.linear(x, W[i, W1], W[i, B1], True), W[i, W2], W[i, B2], False)
    return O.add_layernorm_rows(t, residual)


def encoder_forward_w(X, W: dict, d_model: int, n_heads: int, n_blocks: int) -> np.ndarray:
    """attn_oracle.encoder_forward_ref on the weight set W."""
    x = np.ascontiguousarray(X, dtype=np.float32)
    for i in range(n_blocks):
        x1, heads = _self_attention(x, W, i, d_model, n_heads, False)
        x = _ffn(x1, heads, W, i)
    return x


def decoder_forward_w(X, enc_out, W: dict, d_model: int, n_heads: int, n_blocks: int, causal: bool = False) -> np.ndarray:
    """attn_oracle.decoder_forward_ref (causal: causal_oracle.decoder_forward_causal_ref) on the weight set W."""
    d, H = d_model, n_heads
    x = np.ascontiguousarray(X, dtype=np.float32)
    enc = np.ascontiguousarray(enc_out, dtype=np.float32)
    for i in range(n_blocks):
        x1, _ = _self_attention(x, W, i, d, H, causal)
        q2 = O.quantized_mm(x1, fused(W, i, (WQ2,)))
        kv2 = O.quantized_mm(enc, fused(W, i, (WK2, WV2)))
        heads2 = attn_oracle.attention_ref(q2, kv2[:, :d], kv2[:, d:], H, attn_oracle.default_scale(d // H))
        t = O.quantized_mm(heads2, W[i, WO2])
        x2 = O.add_layernorm_rows(t, heads2)
        x = _ffn(x2, heads2, W, i)
    return x


def heavy_tailed_weights(d: int, H: int, dff: int, n_blocks: int, seed: int, cross: bool = False) -> dict:
    """Normal(0, 0.1) tensors with a few columns of each scaled by 50: the column scales Cw of one packed weight then
    span a factor of about 50, which one uniform draw at the init bounds never does."""
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(n_blocks):
        for kind in (DECODER_KINDS if cross else ENCODER_KINDS):
            a = (0.1 * rng.standard_normal(weight_shape(kind, d, H, dff))).astype(np.float32)
            if kind not in (B1, B2):
                cols = rng.choice(a.shape[-1], size=max(1, a.shape[-1] // 8), replace=False)
                a[..., cols] *= np.float32(50.0)
            out[i, kind] = a
    return out
