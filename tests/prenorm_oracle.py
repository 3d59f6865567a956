"""Expected results for the pre-LN block (QGEMM_ARCH_STANDARD | QGEMM_ARCH_NORM_FIRST [| QGEMM_ARCH_FINAL_NORM],
DESIGN.md s26): the chains of tests/standard_oracle.py rewired norm-first, on its layernorm_rows, gelu_rows and linear /
attention helpers and on the quantized chain of tests/weights_oracle.py.  No new numerical definition: every LN is
standard_oracle.layernorm_rows (B = None), every residual add one float32 add.  TEST INFRASTRUCTURE ONLY.

  x = x + SelfAttn(LN1(x)) W_O + b_O
  x = x + CrossAttn(LN2(x), enc) W_O2 + b_O2          (decoder)
  x = x + act(LN3(x) W1 + b1) W2 + b2
  after the last block:  y = LNf(x)   or   y = x

A weight set is standard_oracle's (kinds 12 .. 25 keep their meaning: gamma1 / beta1 belong to the LN in front of the
self-attention, 2 to the one in front of the cross-attention, 3 to the one in front of the FFN) plus, with a final norm,
(0, GF) and (0, BEF), [d_model] each.  mm= as in standard_oracle: None runs every linear on the quantized oracle.
"""
import numpy as np

import attn_oracle
import causal_oracle
import standard_oracle as SO
import weights_oracle
from attn_oracle import B1, B2, W1, W2, WK, WK2, WO, WO2, WQ, WQ2, WV, WV2
from standard_oracle import BE1, BE2, BE3, BK, BK2, BO, BO2, BQ, BQ2, BV, BV2, G1, G2, G3

GF, BEF = 26, 27  # the final norm's gamma and beta (include/qgemm.h), block 0's
F = np.float32


# ---- the boundary kernel ----------------------------------------------------------------------------------------------
def prenorm_rows(A, B, gamma, beta, eps):
    """qgemm_prenorm_pack_a before its pack: (S, LN(S)) with S = fl(A + B), B may be None (S = A).  The packed bytes the
    entry point writes are pack_a's of the second value, which the device never stores."""
    A = np.ascontiguousarray(A, dtype=F)
    with np.errstate(all="ignore"):
        S = A.copy() if B is None else A + np.ascontiguousarray(B, dtype=F)
    return S, SO.layernorm_rows(S, None, gamma, beta, eps)


# ---- weights ----------------------------------------------------------------------------------------------------------
def prenorm_weights(d: int, H: int, dff: int, n_blocks: int, seed: int, cross: bool = False, final_norm: bool = True) -> dict:
    """standard_oracle.standard_weights plus, with a final norm, random gamma_f around 1 and beta_f around 0."""
    W = SO.standard_weights(d, H, dff, n_blocks, seed, cross)
    if final_norm:
        rng = np.random.default_rng(seed + 104729)
        W[0, GF] = (0.2 * rng.standard_normal(d)).astype(F) + F(1.0)
        W[0, BEF] = (0.2 * rng.standard_normal(d)).astype(F)
    return W


def torch_model_weights(layers, n_heads: int, final_norm=None) -> dict:
    """The weight set of a list of torch.nn layers with norm_first=True and the LayerNorm behind them, if any: what
    load_torch_layer and load_torch_final_norm load.  The norms map to the kinds exactly as on post-LN layers."""
    W = SO.torch_layer_weights(layers, n_heads)
    if final_norm is not None:
        W[0, GF] = np.ascontiguousarray(final_norm.weight.detach().cpu().float().numpy())
        W[0, BEF] = np.ascontiguousarray(final_norm.bias.detach().cpu().float().numpy())
    return W


# ---- the block chains -------------------------------------------------------------------------------------------------
def _self_attention(x, W, i, d, H, causal, eps, mm):
    """SelfAttn(LN1(x)) W_O + b_O"""
    n = SO.layernorm_rows(x, None, W[i, G1], W[i, BE1], eps)
    qkv = SO._linear(n, weights_oracle.fused(W, i, (WQ, WK, WV)), SO._cat(W, i, (BQ, BK, BV)), False, mm)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    scale = attn_oracle.default_scale(d // H)
    heads = (causal_oracle.attention_causal_ref(q, k, v, H, scale, 0) if causal
             else attn_oracle.attention_ref(q, k, v, H, scale))
    return SO._linear(heads, W[i, WO], W[i, BO], False, mm)


def _cross_attention(x, enc, W, i, d, H, eps, mm):
    """CrossAttn(LN2(x), enc) W_O2 + b_O2: keys and values from enc as given"""
    n = SO.layernorm_rows(x, None, W[i, G2], W[i, BE2], eps)
    q2 = SO._linear(n, weights_oracle.fused(W, i, (WQ2,)), W[i, BQ2], False, mm)
    kv2 = SO._linear(enc, weights_oracle.fused(W, i, (WK2, WV2)), SO._cat(W, i, (BK2, BV2)), False, mm)
    heads2 = attn_oracle.attention_ref(q2, kv2[:, :d], kv2[:, d:], H, attn_oracle.default_scale(d // H))
    return SO._linear(heads2, W[i, WO2], W[i, BO2], False, mm)


def _ffn(x, W, i, activation, eps, mm):
    """act(LN3(x) W1 + b1) W2 + b2"""
    assert activation in ("relu", "gelu_tanh")
    n = SO.layernorm_rows(x, None, W[i, G3], W[i, BE3], eps)
    h = SO._linear(n, W[i, W1], W[i, B1], activation == "relu", mm)
    if activation == "gelu_tanh":
        h = SO.gelu_rows(h)
    return SO._linear(h, W[i, W2], W[i, B2], False, mm)


def _add(x, t):
    y = x + np.asarray(t, F)  # one float32 add per element
    assert y.dtype == F
    return y


def _finish(x, W, final_norm, eps):
    return SO.layernorm_rows(x, None, W[0, GF], W[0, BEF], eps) if final_norm else x


def encoder_forward_pre(X, W: dict, d_model: int, n_heads: int, n_blocks: int, activation: str = "relu",
                        final_norm: bool = True, eps: float = 1e-5, mm=None) -> np.ndarray:
    x = np.ascontiguousarray(X, dtype=F)
    for i in range(n_blocks):
        x = _add(x, _self_attention(x, W, i, d_model, n_heads, False, eps, mm))
        x = _add(x, _ffn(x, W, i, activation, eps, mm))
    return _finish(x, W, final_norm, eps)


def decoder_forward_pre(X, enc_out, W: dict, d_model: int, n_heads: int, n_blocks: int, causal: bool = False,
                        activation: str = "relu", final_norm: bool = True, eps: float = 1e-5, mm=None) -> np.ndarray:
    x = np.ascontiguousarray(X, dtype=F)
    enc = np.ascontiguousarray(enc_out, dtype=F)
    for i in range(n_blocks):
        x = _add(x, _self_attention(x, W, i, d_model, n_heads, causal, eps, mm))
        x = _add(x, _cross_attention(x, enc, W, i, d_model, n_heads, eps, mm))
        x = _add(x, _ffn(x, W, i, activation, eps, mm))
    return _finish(x, W, final_norm, eps)
