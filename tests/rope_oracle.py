"""Expected results for rotary position embeddings and decoder-only stacks (QGEMM_ARCH_ROPE, QGEMM_ARCH_DECODER_ONLY,
DESIGN.md s27).  TEST INFRASTRUCTURE ONLY.

rope_rows is qgemm_rope_rows' contract of include/qgemm.h in numpy float32, one rounding per step.  The block chains are
those of tests/weights_oracle.py (the reference's block), tests/standard_oracle.py (post-LN) and tests/prenorm_oracle.py
(pre-LN) on their own helpers -- linear, attention, layernorm -- with ONE new step: Q and K of the self-attention are
rotated between the QKV linear and the attention.  The cross-attention is never rotated.  A decoder-only chain is the
encoder's under the causal mask.  mm= as in standard_oracle: None runs every linear on the quantized oracle.
"""
import numpy as np

import attn_oracle
import causal_oracle
import prenorm_oracle as PO
import standard_oracle as SO
import weights_oracle
from attn_oracle import WK, WO, WQ, WV
from standard_oracle import BE1, BK, BO, BQ, BV, G1

F = np.float32
ROPE_COS, ROPE_SIN = 28, 29  # the tables' kinds (include/qgemm.h), block 0's
NORM_FIRST, FINAL_NORM = 0x100, 0x200


def make_tables(max_seq: int, d_k: int):
    """(cos, sin), max_seq x d_k / 2 float32 each, by the creation formula: theta = 10000, in double."""
    i = np.arange(d_k // 2, dtype=np.float64)
    inv = np.array([pow(10000.0, -2.0 * v / d_k) for v in i])
    ang = np.arange(max_seq, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(ang).astype(F), np.sin(ang).astype(F)


def rope_rows(X, groups: int, d_k: int, cos, sin, pos=0):
    """qgemm_rope_rows on a copy of X (rows x groups * d_k): row r at position pos + r, or at pos[r] for an array."""
    X = np.ascontiguousarray(X, dtype=F)
    rows, h = X.shape[0], d_k // 2
    assert X.shape[1] == groups * d_k and d_k % 2 == 0
    p = np.asarray(pos) + np.arange(rows) if np.ndim(pos) == 0 else np.asarray(pos)
    assert p.shape == (rows,) and (p >= 0).all() and (p < len(cos)).all()
    c = np.asarray(cos, F)[p][:, None, :]  # rows x 1 x h
    s = np.asarray(sin, F)[p][:, None, :]
    x = X.reshape(rows, groups, d_k)
    a, b = x[:, :, :h], x[:, :, h:]
    with np.errstate(all="ignore"):
        lo = a * c - b * s  # fl(fl(a c) - fl(b s)): numpy rounds every float32 operation
        hi = b * c + a * s
    y = np.concatenate([lo, hi], axis=2).reshape(rows, groups * d_k)
    assert y.dtype == F
    return y


# ---- the self-attention with the rotation ---------------------------------------------------------------------------
def _projected_heads(x_in, W, i, d, H, causal, mm, rope):
    """attention(rope(Q), rope(K), V) W_O + b_O on the rows x_in; rope = (cos, sin) or None"""
    qkv = SO._linear(x_in, weights_oracle.fused(W, i, (WQ, WK, WV)), SO._cat(W, i, (BQ, BK, BV)), False, mm)
    if rope is not None:
        qkv = np.concatenate([rope_rows(qkv[:, :2 * d], 2 * H, d // H, rope[0], rope[1], 0), qkv[:, 2 * d:]], axis=1)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    scale = attn_oracle.default_scale(d // H)
    heads = (causal_oracle.attention_causal_ref(q, k, v, H, scale, 0) if causal
             else attn_oracle.attention_ref(q, k, v, H, scale))
    return SO._linear(heads, W[i, WO], W[i, BO], False, mm)


def _self_post(x, W, i, d, H, causal, eps, mm, rope):
    """x1 = LN1(x + SelfAttn(x) W_O + b_O)"""
    return SO.layernorm_rows(_projected_heads(x, W, i, d, H, causal, mm, rope), x, W[i, G1], W[i, BE1], eps)


def _self_pre(x, W, i, d, H, causal, eps, mm, rope):
    """x + SelfAttn(LN1(x)) W_O + b_O"""
    n = SO.layernorm_rows(x, None, W[i, G1], W[i, BE1], eps)
    return PO._add(x, _projected_heads(n, W, i, d, H, causal, mm, rope))


def _forward(X, enc_out, W, d, H, n_blocks, arch, causal, activation, eps, mm, rope):
    x = np.ascontiguousarray(X, dtype=F)
    enc = None if enc_out is None else np.ascontiguousarray(enc_out, dtype=F)
    pre = bool(arch & NORM_FIRST)
    assert arch & 0xff == 1, "the standard block"
    for i in range(n_blocks):
        if pre:
            x = _self_pre(x, W, i, d, H, causal, eps, mm, rope)
            if enc is not None:
                x = PO._add(x, PO._cross_attention(x, enc, W, i, d, H, eps, mm))
            x = PO._add(x, PO._ffn(x, W, i, activation, eps, mm))
        else:
            x = _self_post(x, W, i, d, H, causal, eps, mm, rope)
            if enc is not None:
                x = SO._cross_attention(x, enc, W, i, d, H, eps, mm)
            x = SO._ffn(x, W, i, activation, eps, mm)
    return PO._finish(x, W, bool(arch & FINAL_NORM), eps) if pre else x


def encoder_forward_rope(X, W, d_model, n_heads, n_blocks, rope, arch=1, activation="relu", eps=1e-5, mm=None):
    """An encoder with rotated Q and K; rope = (cos, sin); arch: 1, 0x101 or 0x301."""
    return _forward(X, None, W, d_model, n_heads, n_blocks, arch, False, activation, eps, mm, rope)


def decoder_forward_rope(X, enc_out, W, d_model, n_heads, n_blocks, rope, arch=1, causal=True, activation="relu",
                         eps=1e-5, mm=None):
    """A decoder with cross-attention: the self-attention's Q and K rotated, the cross-attention's not."""
    return _forward(X, enc_out, W, d_model, n_heads, n_blocks, arch, causal, activation, eps, mm, rope)


def decoder_only_forward(X, W, d_model, n_heads, n_blocks, arch=1, causal=True, rope=None, activation="relu", eps=1e-5,
                         mm=None):
    """A decoder-only stack: the encoder's blocks under the decoder's mask.  arch: the base in the low byte (0: the
    reference's block on weights_oracle's chain) and the pre-LN bits; rope = (cos, sin) or None."""
    if arch & 0xff == 0:
        assert rope is None and mm is None
        x = np.ascontiguousarray(X, dtype=F)
        for i in range(n_blocks):
            x1, heads = weights_oracle._self_attention(x, W, i, d_model, n_heads, causal)
            x = weights_oracle._ffn(x1, heads, W, i)
        return x
    return _forward(X, None, W, d_model, n_heads, n_blocks, arch, causal, activation, eps, mm, rope)
