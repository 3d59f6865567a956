"""Expected results for Llama-style blocks (QGEMM_ARCH_RMSNORM, QGEMM_ARCH_GATED_FFN): the contracts of
qgemm_rmsnorm_rows and qgemm_glu_rows of include/qgemm.h in numpy float32 -- every step one IEEE fp32 operation, the row
sum in standard_oracle's order, exp as np.exp(float64).astype(float32) -- and ONE stack forward for any combination of
the architecture bits.  TEST INFRASTRUCTURE ONLY.

The forward reuses, by import, standard_oracle (linear, LayerNorm, GELU, the sum order), prenorm_oracle (the residual
add), rope_oracle (the projected, rotated self-attention) and the attention oracles; it swaps only the norm and the
FFN.  A weight set is prenorm_oracle's plus, per block, (i, W3) [d_model, d_ff] and (i, B3) [d_ff]; an RMS chain never
reads a beta.  mm= as in standard_oracle: None runs every linear on the quantized oracle.
"""
import numpy as np

import attn_oracle
import prenorm_oracle as PO
import rope_oracle as RO
import standard_oracle as SO
import weights_oracle
from attn_oracle import B1, B2, W1, W2, WK2, WO2, WQ2, WV2
from prenorm_oracle import BEF, GF
from standard_oracle import BE1, BE2, BE3, BK2, BO2, BQ2, BV2, G1, G2, G3

F = np.float32
W3, B3 = 30, 31  # the up projection and its bias (include/qgemm.h)
STANDARD, NORM_FIRST, FINAL_NORM, DECODER_ONLY, ROPE, RMSNORM, GATED_FFN = 1, 0x100, 0x200, 0x400, 0x800, 0x2000, 0x4000
LLAMA = STANDARD | NORM_FIRST | FINAL_NORM | DECODER_ONLY | ROPE | RMSNORM | GATED_FFN  # 0x6F01
ACTIVATIONS = ("relu", "gelu_tanh", "silu")


# ---- the row kernels --------------------------------------------------------------------------------------------------
def rmsnorm_rows(A, B, gamma, eps, rowsum=SO.rowsum_registers):
    """qgemm_rmsnorm_rows: Y = RMSNorm(A + B), B may be None."""
    A = np.ascontiguousarray(A, dtype=F)
    gamma, eps = np.asarray(gamma, F), F(eps)
    w = A.shape[-1]
    with np.errstate(all="ignore"):
        v = A if B is None else A + np.ascontiguousarray(B, dtype=F)
        v = v.reshape(-1, w)
        ms = rowsum(v * v) / F(w)
        r = F(1.0) / np.sqrt(ms + eps)
        y = (v * r[:, None]) * gamma[None, :]
    assert y.dtype == F
    return y.reshape(A.shape)


def prenorm_rms_rows(A, B, gamma, eps):
    """qgemm_prenorm_rms_pack_a before its pack: (S, RMSNorm(S)) with S = fl(A + B), B may be None (S = A)."""
    A = np.ascontiguousarray(A, dtype=F)
    with np.errstate(all="ignore"):
        S = A.copy() if B is None else A + np.ascontiguousarray(B, dtype=F)
    return S, rmsnorm_rows(S, None, gamma, eps)


def silu(X):
    """x sigmoid(x): e = fl32(exp((double)(-x))), fl(x / fl(1 + e))"""
    x = np.ascontiguousarray(X, dtype=F)
    with np.errstate(all="ignore"):
        e = np.exp((-x).astype(np.float64)).astype(F)
        y = x / (F(1.0) + e)
    assert y.dtype == F
    return y


def act_rows(G, activation):
    assert activation in ACTIVATIONS
    g = np.ascontiguousarray(G, dtype=F)
    if activation == "relu":
        return np.where(g < 0, F(0), g)  # the GEMM epilogue's: NaN and -0 pass
    return SO.gelu_rows(g) if activation == "gelu_tanh" else silu(g)


def glu_rows(X, activation):
    """qgemm_glu_rows: X rows x 2w, [gate | up]; act(gate) * up, rows x w."""
    X = np.asarray(X, dtype=F)
    w = X.shape[1] // 2
    assert X.shape[1] == 2 * w
    with np.errstate(all="ignore"):
        h = act_rows(X[:, :w], activation) * X[:, w:]
    assert h.dtype == F
    return np.ascontiguousarray(h)


# ---- float64 formulas the oracle is held against (tests/test_gated_host.py) -------------------------------------------
def rmsnorm_f64(A, B, gamma, eps):
    v = np.asarray(A, np.float64) + (0.0 if B is None else np.asarray(B, np.float64))
    return v / np.sqrt((v * v).mean(axis=-1, keepdims=True) + float(F(eps))) * np.asarray(gamma, np.float64)


def silu_f64(X):
    x = np.asarray(X, np.float64)
    return x / (1.0 + np.exp(-x))


# ---- weights ----------------------------------------------------------------------------------------------------------
def gated_weights(d: int, H: int, dff: int, n_blocks: int, seed: int, cross: bool = False) -> dict:
    """prenorm_oracle.prenorm_weights (with the final norm) plus a heavy-tailed W3 and a random b3 per block."""
    W = PO.prenorm_weights(d, H, dff, n_blocks, seed, cross, final_norm=True)
    rng = np.random.default_rng(seed + 15485863)
    for i in range(n_blocks):
        up = (0.1 * rng.standard_normal((d, dff))).astype(F)
        up[:, rng.choice(dff, 3, replace=False)] *= F(50.0)
        W[i, W3] = up
        W[i, B3] = (0.2 * rng.standard_normal(dff)).astype(F)
    return W


def init_scale_weights(d: int, H: int, dff: int, n_blocks: int, seed: int) -> dict:
    """A weight set at a trained model's scale instead of gated_weights' heavy tails, for the accuracy statement of
    tests/test_gated_host.py: every matrix U(-1, 1) / sqrt(fan_in), every gamma around 1, every bias and beta around 0.
    Encoder kinds, W3 / b3 and the final norm."""
    rng = np.random.default_rng(seed)
    W, dk = {}, d // H

    def u(shape, fan_in):
        return (rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan_in)).astype(F)

    def vec(n, around=0.0):
        return (around + 0.2 * rng.standard_normal(n)).astype(F)

    for i in range(n_blocks):
        for kind in (attn_oracle.WQ, attn_oracle.WK, attn_oracle.WV):
            W[i, kind] = u((H, d, dk), d)
        W[i, attn_oracle.WO], W[i, W1], W[i, W3], W[i, W2] = u((d, d), d), u((d, dff), d), u((d, dff), d), u((dff, d), dff)
        W[i, B1], W[i, B3], W[i, B2] = vec(dff), vec(dff), vec(d)
        for kind in (SO.BQ, SO.BK, SO.BV, SO.BO, BE1, BE3):
            W[i, kind] = vec(d)
        W[i, G1], W[i, G3] = vec(d, 1.0), vec(d, 1.0)
    W[0, GF], W[0, BEF] = vec(d, 1.0), vec(d)
    return W


def w1_fused(W, i):
    """[W1 | W3], d_model x 2 d_ff: what the block's packed W1 holds on a gated model"""
    return np.ascontiguousarray(np.concatenate([W[i, W1], W[i, W3]], axis=1), dtype=F)


# ---- the stack forward ------------------------------------------------------------------------------------------------
def _norm(x, B, W, i, g, be, rms, eps):
    return rmsnorm_rows(x, B, W[i, g], eps) if rms else SO.layernorm_rows(x, B, W[i, g], W[i, be], eps)


def _cross_heads(x_in, enc, W, i, d, H, mm):
    """CrossAttn(x_in, enc) W_O2 + b_O2, never rotated"""
    q2 = SO._linear(x_in, weights_oracle.fused(W, i, (WQ2,)), W[i, BQ2], False, mm)
    kv2 = SO._linear(enc, weights_oracle.fused(W, i, (WK2, WV2)), SO._cat(W, i, (BK2, BV2)), False, mm)
    heads2 = attn_oracle.attention_ref(q2, kv2[:, :d], kv2[:, d:], H, attn_oracle.default_scale(d // H))
    return SO._linear(heads2, W[i, WO2], W[i, BO2], False, mm)


def _ffn(x_in, W, i, activation, gated, mm):
    """act(x W1 + b1) W2 + b2, or gated (act(x W1 + b1) * (x W3 + b3)) W2 + b2 with gate and up from ONE linear"""
    if gated:
        gu = SO._linear(x_in, w1_fused(W, i), SO._cat(W, i, (B1, B3)), False, mm)
        h = glu_rows(gu, activation)
    else:
        assert activation in ("relu", "gelu_tanh")
        h = SO._linear(x_in, W[i, W1], W[i, B1], activation == "relu", mm)
        if activation == "gelu_tanh":
            h = SO.gelu_rows(h)
    return SO._linear(h, W[i, W2], W[i, B2], False, mm)


def forward(X, enc_out, W, d_model, n_heads, n_blocks, arch, causal=False, activation="relu", eps=1e-5, mm=None,
            rope=None):
    """The stack on the standard block with any of NORM_FIRST, FINAL_NORM, RMSNORM and GATED_FFN in `arch` (the
    DECODER_ONLY and ROPE bits are not read: enc_out = None is a stack without cross-attention, rope = (cos, sin) or
    None says whether Q and K are rotated)."""
    assert arch & 0xff == STANDARD
    d, H = d_model, n_heads
    pre, rms, gated = bool(arch & NORM_FIRST), bool(arch & RMSNORM), bool(arch & GATED_FFN)
    x = np.ascontiguousarray(X, dtype=F)
    enc = None if enc_out is None else np.ascontiguousarray(enc_out, dtype=F)
    for i in range(n_blocks):
        if pre:
            n = _norm(x, None, W, i, G1, BE1, rms, eps)
            x = PO._add(x, RO._projected_heads(n, W, i, d, H, causal, mm, rope))
            if enc is not None:
                x = PO._add(x, _cross_heads(_norm(x, None, W, i, G2, BE2, rms, eps), enc, W, i, d, H, mm))
            x = PO._add(x, _ffn(_norm(x, None, W, i, G3, BE3, rms, eps), W, i, activation, gated, mm))
        else:
            x = _norm(RO._projected_heads(x, W, i, d, H, causal, mm, rope), x, W, i, G1, BE1, rms, eps)
            if enc is not None:
                x = _norm(_cross_heads(x, enc, W, i, d, H, mm), x, W, i, G2, BE2, rms, eps)
            x = _norm(_ffn(x, W, i, activation, gated, mm), x, W, i, G3, BE3, rms, eps)
    if pre and arch & FINAL_NORM:
        x = _norm(x, None, W, 0, GF, BEF, rms, eps)
    return x
