"""Expected results for the standard post-LN block (qgemm_model_create with QGEMM_ARCH_STANDARD): the
two row kernels' contracts of include/qgemm.h in numpy float32 -- every step one IEEE fp32 operation, exp as
np.exp(float64).astype(float32) as beam_oracle.py has it -- and the three block chains on the oracle's primitives
(O.linear, the attention oracles of attn_oracle.py / causal_oracle.py).  TEST INFRASTRUCTURE ONLY.

A weight set is weights_oracle.py's dict keyed (block, kind) plus the standard architecture's vectors, kinds 12 .. 25,
[d_model] each.  The chains take mm=: None runs every linear on the quantized oracle (O.linear), a callable
mm(x, W) -> x W runs the same wiring on that product (tests/test_standard_host.py: a plain fp32 matmul against torch).
"""
import math

import numpy as np

import attn_oracle
import causal_oracle
import weights_oracle
from attn_oracle import B1, B2, W1, W2, WK, WK2, WO, WO2, WQ, WQ2, WV, WV2
from oracle import oracle as O

# the standard architecture's kinds (include/qgemm.h), [d_model] each; BQ2 .. BE2 on a decoder
(BQ, BK, BV, BO, G1, BE1, G3, BE3, BQ2, BK2, BV2, BO2, G2, BE2) = range(12, 26)
ENCODER_VECTOR_KINDS = (BQ, BK, BV, BO, G1, BE1, G3, BE3)
DECODER_VECTOR_KINDS = ENCODER_VECTOR_KINDS + (BQ2, BK2, BV2, BO2, G2, BE2)
GAMMA_KINDS = (G1, G2, G3)

F = np.float32
GELU_C1 = F(2.0 * math.sqrt(2.0 / math.pi))  # fl32(2 sqrt(2/pi))
assert GELU_C1.view(np.uint32) == 0x3FCC422A
GELU_C3 = F(0.044715)


# ---- the sums' order -------------------------------------------------------------------------------------------------
def _butterfly(p):
    """Six steps p[l] = fl(p[l] + p[l ^ off]), off = 32 .. 1, for every l at once; p: [rows, 64] float32."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lanes ^ off]
    assert (p.view(np.uint32) == p[:, :1].view(np.uint32)).all() or np.isnan(p).any()
    return p[:, 0]


def rowsum_registers(v):
    """The contract's row sum as the register-resident launch lays it out: lane l holds float4 columns l, l + 64, ..;
    the row is padded to whole 64 x 4 chunks with -0, the identity of the sum.  v: [rows, w] float32."""
    v = np.ascontiguousarray(v, dtype=F)
    rows, w = v.shape
    chunks = (w + 255) // 256
    pad = np.full((rows, chunks * 256), -0.0, F)
    pad[:, :w] = v
    x = pad.reshape(rows, chunks, 64, 4)  # element c = 4 (l + 64 i) + e at [i, l, e]
    p = np.zeros((rows, 64), F)           # +0
    for i in range(chunks):
        for e in range(4):
            p = p + x[:, i, :, e]
    return _butterfly(p)


def rowsum_fallback(v):
    """The same sum as the fallback launch states it: element by element in increasing c into partial (c / 4) % 64, no
    padding.  Must agree with rowsum_registers bit for bit (tests/test_standard_host.py)."""
    v = np.ascontiguousarray(v, dtype=F)
    rows, w = v.shape
    p = np.zeros((rows, 64), F)
    for c in range(w):
        l = (c // 4) % 64
        p[:, l] = p[:, l] + v[:, c]
    return _butterfly(p)


# ---- the two row kernels ---------------------------------------------------------------------------------------------
def layernorm_rows(A, B, gamma, beta, eps, rowsum=rowsum_registers):
    """qgemm_layernorm_rows: Y = LN(A + B), B may be None."""
    A = np.ascontiguousarray(A, dtype=F)
    gamma, beta, eps = np.asarray(gamma, F), np.asarray(beta, F), F(eps)
    w = A.shape[-1]
    with np.errstate(all="ignore"):
        v = A if B is None else A + np.ascontiguousarray(B, dtype=F)
        v = v.reshape(-1, w)
        fw = F(w)
        mean = rowsum(v) / fw
        d = v - mean[:, None]
        var = rowsum(d * d) / fw
        rstd = F(1.0) / np.sqrt(var + eps)
        y = (d * rstd[:, None]) * gamma[None, :] + beta[None, :]
    assert y.dtype == F
    return y.reshape(A.shape)


def gelu_rows(X):
    """qgemm_gelu_rows: x sigmoid(2u), the tanh-form GELU."""
    x = np.ascontiguousarray(X, dtype=F)
    with np.errstate(all="ignore"):
        t = x * GELU_C1
        q = (x * x) * GELU_C3 + F(1.0)
        z = t * q
        e = np.exp((-z).astype(np.float64)).astype(F)
        g = x / (F(1.0) + e)
    assert g.dtype == F
    return g


# ---- float64 formulas the oracle is held against (tests/test_standard_host.py) ---------------------------------------
def layernorm_f64(A, B, gamma, beta, eps):
    v = np.asarray(A, np.float64) + (0.0 if B is None else np.asarray(B, np.float64))
    mean = v.mean(axis=-1, keepdims=True)
    var = ((v - mean) ** 2).mean(axis=-1, keepdims=True)
    return (v - mean) / np.sqrt(var + float(F(eps))) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def gelu_tanh_f64(X):
    x = np.asarray(X, np.float64)
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


# ---- weights ---------------------------------------------------------------------------------------------------------
def standard_weights(d: int, H: int, dff: int, n_blocks: int, seed: int, cross: bool = False) -> dict:
    """weights_oracle.heavy_tailed_weights plus random vectors of the new kinds: gamma around 1, biases and beta around
    0, none of them at its creation value."""
    W = weights_oracle.heavy_tailed_weights(d, H, dff, n_blocks, seed, cross)
    rng = np.random.default_rng(seed + 7919)
    for i in range(n_blocks):
        for kind in (DECODER_VECTOR_KINDS if cross else ENCODER_VECTOR_KINDS):
            a = (0.2 * rng.standard_normal(d)).astype(F)
            W[i, kind] = a + F(1.0) if kind in GAMMA_KINDS else a
    return W


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().float().numpy())


def torch_layer_weights(layers, n_heads: int) -> dict:
    """The weight set of a list of torch.nn.TransformerEncoderLayer / TransformerDecoderLayer (norm_first=False): what
    load_torch_layer loads, block by block."""
    W = {}
    for i, layer in enumerate(layers):
        cross = hasattr(layer, "multihead_attn")
        d = layer.self_attn.embed_dim
        dk = d // n_heads

        def attn(a, wk, bk, wo, bo):
            Wi, bi = _np(a.in_proj_weight), _np(a.in_proj_bias)
            for j in range(3):
                W[i, wk[j]] = np.stack([Wi[j * d + h * dk:j * d + (h + 1) * dk].T for h in range(n_heads)])
                W[i, bk[j]] = bi[j * d:(j + 1) * d]
            W[i, wo], W[i, bo] = _np(a.out_proj.weight).T, _np(a.out_proj.bias)

        attn(layer.self_attn, (WQ, WK, WV), (BQ, BK, BV), WO, BO)
        W[i, G1], W[i, BE1] = _np(layer.norm1.weight), _np(layer.norm1.bias)
        if cross:
            attn(layer.multihead_attn, (WQ2, WK2, WV2), (BQ2, BK2, BV2), WO2, BO2)
            W[i, G2], W[i, BE2] = _np(layer.norm2.weight), _np(layer.norm2.bias)
        W[i, W1], W[i, B1] = _np(layer.linear1.weight).T, _np(layer.linear1.bias)
        W[i, W2], W[i, B2] = _np(layer.linear2.weight).T, _np(layer.linear2.bias)
        n = layer.norm3 if cross else layer.norm2
        W[i, G3], W[i, BE3] = _np(n.weight), _np(n.bias)
        for key in [k for k in W if k[0] == i]:
            W[key] = np.ascontiguousarray(W[key], dtype=F)
    return W


# ---- the block chains ------------------------------------------------------------------------------------------------
def _linear(x, Wm, b, relu, mm):
    if mm is None:
        return O.linear(x, Wm, b, relu)
    y = np.asarray(mm(x, Wm), F) + np.asarray(b, F)
    return np.where(y < 0, F(0), y) if relu else y


def _cat(W, i, kinds):
    return np.ascontiguousarray(np.concatenate([W[i, k] for k in kinds]), dtype=F)


def _self_attention(x, W, i, d, H, causal, eps, mm):
    """x1 = LN1(x + SelfAttn(x) W_O + b_O)"""
    qkv = _linear(x, weights_oracle.fused(W, i, (WQ, WK, WV)), _cat(W, i, (BQ, BK, BV)), False, mm)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    scale = attn_oracle.default_scale(d // H)
    heads = (causal_oracle.attention_causal_ref(q, k, v, H, scale, 0) if causal
             else attn_oracle.attention_ref(q, k, v, H, scale))
    t = _linear(heads, W[i, WO], W[i, BO], False, mm)
    return layernorm_rows(t, x, W[i, G1], W[i, BE1], eps)


def _cross_attention(x1, enc, W, i, d, H, eps, mm):
    """x2 = LN2(x1 + CrossAttn(x1, enc) W_O2 + b_O2)"""
    q2 = _linear(x1, weights_oracle.fused(W, i, (WQ2,)), W[i, BQ2], False, mm)
    kv2 = _linear(enc, weights_oracle.fused(W, i, (WK2, WV2)), _cat(W, i, (BK2, BV2)), False, mm)
    heads2 = attn_oracle.attention_ref(q2, kv2[:, :d], kv2[:, d:], H, attn_oracle.default_scale(d // H))
    t = _linear(heads2, W[i, WO2], W[i, BO2], False, mm)
    return layernorm_rows(t, x1, W[i, G2], W[i, BE2], eps)


def _ffn(x, W, i, activation, eps, mm):
    """y = LN3(x + act(x W1 + b1) W2 + b2)"""
    assert activation in ("relu", "gelu_tanh")
    h = _linear(x, W[i, W1], W[i, B1], activation == "relu", mm)
    if activation == "gelu_tanh":
        h = gelu_rows(h)
    t = _linear(h, W[i, W2], W[i, B2], False, mm)
    return layernorm_rows(t, x, W[i, G3], W[i, BE3], eps)


def encoder_forward_std(X, W: dict, d_model: int, n_heads: int, n_blocks: int, activation: str = "relu",
                        eps: float = 1e-5, mm=None) -> np.ndarray:
    x = np.ascontiguousarray(X, dtype=F)
    for i in range(n_blocks):
        x1 = _self_attention(x, W, i, d_model, n_heads, False, eps, mm)
        x = _ffn(x1, W, i, activation, eps, mm)
    return x


def decoder_forward_std(X, enc_out, W: dict, d_model: int, n_heads: int, n_blocks: int, causal: bool = False,
                        activation: str = "relu", eps: float = 1e-5, mm=None) -> np.ndarray:
    x = np.ascontiguousarray(X, dtype=F)
    enc = np.ascontiguousarray(enc_out, dtype=F)
    for i in range(n_blocks):
        x1 = _self_attention(x, W, i, d_model, n_heads, causal, eps, mm)
        x2 = _cross_attention(x1, enc, W, i, d_model, n_heads, eps, mm)
        x = _ffn(x2, W, i, activation, eps, mm)
    return x
