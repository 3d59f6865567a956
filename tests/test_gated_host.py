"""Llama-style blocks without a GPU: tests/gated_oracle.py against float64 formulas, the RMS norm against
the LayerNorm where the two must agree and where they must not, the whole quantized Llama block against a float64 Llama
block written here, and the refusals of the new architecture bits, kinds and entry points.

Every bound below is a multiple of an error MEASURED on the CPU with these fixed, seeded inputs: 4x for the float32
oracle against float64 -- the margin covers another machine's libm, nothing else -- and 2x for the quantized chain,
whose error is the int8 quantization's and does not move with the library."""
import ctypes

import numpy as np
import pytest

import gated_oracle as GO
import rope_oracle as RO
import standard_oracle as SO
from attn_oracle import B1, B2, W1, W2, WK, WO, WQ, WV
from standard_oracle import BK, BO, BQ, BV, G1, G3
from util import assert_bits_equal

F = np.float32

# ---- 1. the oracle's RMS norm and SiLU against float64 -----------------------------------------------------------------
# measured maximum absolute error of rmsnorm_rows over 8 rows of normal * 3 + 0.5 (gamma random), per width
RMS_MEASURED = {1: 1.259e-7, 2: 9.667e-8, 3: 1.366e-7, 4: 1.127e-7, 5: 1.583e-7, 64: 3.018e-7, 100: 4.566e-7,
                255: 3.531e-7, 256: 3.823e-7, 257: 5.748e-7, 1024: 4.772e-7, 1028: 6.226e-7, 2048: 4.000e-7,
                4096: 4.425e-7}
# measured maximum error of silu over 64 x 4096 values of normal * 10, relative to max(|y|, 2^-126), where exp(-x) is
# finite
SILU_MEASURED = 1.710e-7


def _rows(rows, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, w)) * 3.0 + 0.5).astype(F)


@pytest.mark.parametrize("w", sorted(RMS_MEASURED))
def test_oracle_rmsnorm_against_float64(w):
    A, B = _rows(8, w, 100 + w), _rows(8, w, 200 + w)
    gamma = (1.0 + 0.2 * np.random.default_rng(300 + w).standard_normal(w)).astype(F)
    err = float(np.abs(GO.rmsnorm_rows(A, B, gamma, 1e-5).astype(np.float64) - GO.rmsnorm_f64(A, B, gamma, 1e-5)).max())
    print(f"RMS w={w}: max abs error {err:.3e}")
    assert err <= 4 * RMS_MEASURED[w]
    got = GO.rmsnorm_rows(A, None, gamma, 1e-5)   # B = None is RMSNorm(A)
    assert np.abs(got.astype(np.float64) - GO.rmsnorm_f64(A, None, gamma, 1e-5)).max() <= 4 * RMS_MEASURED[w]
    S, N = GO.prenorm_rms_rows(A, B, gamma, 1e-5)
    assert_bits_equal(S, A + B, "prenorm_rms_rows: S")
    assert_bits_equal(N, GO.rmsnorm_rows(A, B, gamma, 1e-5), "prenorm_rms_rows: the norm of S")


@pytest.mark.parametrize("w", [1, 3, 4, 5, 64, 100, 255, 256, 257, 260, 1024, 1028, 4095, 4096])
def test_sum_order_layouts_agree(w):
    v = _rows(3, w, 400 + w)
    v[1, 0] = -0.0
    gamma = np.full(w, 1.25, F)
    assert_bits_equal(GO.rmsnorm_rows(v, None, gamma, 1e-5, rowsum=SO.rowsum_registers),
                      GO.rmsnorm_rows(v, None, gamma, 1e-5, rowsum=SO.rowsum_fallback), f"RMS w={w}")


def test_oracle_silu_against_float64():
    X = (np.random.default_rng(7).standard_normal((64, 4096)) * 10.0).astype(F)
    got, want = GO.silu(X).astype(np.float64), GO.silu_f64(X)
    far = X.astype(np.float64) < -88.0   # exp(-x) passes FLT_MAX: x / inf = -0 for a true value below |x| / FLT_MAX
    assert np.abs(got[far] - want[far]).max(initial=0.0) <= 2.0 ** -120
    err = float((np.abs(got - want)[~far] / np.maximum(np.abs(want[~far]), 2.0 ** -126)).max())
    print(f"SiLU: max relative error {err:.3e}")
    assert err <= 4 * SILU_MEASURED


def test_oracle_special_values():
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -100.0, 100.0], F)
    s = GO.silu(x)
    assert s[0] == 0 and not np.signbit(s[0]) and s[1] == 0 and np.signbit(s[1])
    assert s[2] == np.inf and np.isnan(s[3]) and np.isnan(s[4])
    assert s[5] == 0 and np.signbit(s[5]) and s[6] == F(100.0)
    r = GO.act_rows(x, "relu")
    assert r[1] == 0 and np.signbit(r[1]) and r[2] == np.inf and r[3] == 0 and np.isnan(r[4]) and r[5] == 0
    # glu: the product's own rules -- 0 * inf is NaN, a NaN on either side sticks
    X = np.array([[1.0, 0.0, np.nan, 2.0, np.inf, np.inf, 3.0, np.nan]], F)   # gate 1, 0, NaN, 2 | up inf, inf, 3, NaN
    h = GO.glu_rows(X, "silu")
    assert h[0, 0] == np.inf and np.isnan(h[0, 1]) and np.isnan(h[0, 2]) and np.isnan(h[0, 3])
    for act in GO.ACTIVATIONS:
        G = _rows(4, 16, 5)
        assert_bits_equal(GO.glu_rows(G, act), GO.act_rows(G[:, :8], act) * G[:, 8:], f"glu_rows {act}")


# ---- 2. RMS against LayerNorm --------------------------------------------------------------------------------------------
def test_rms_is_layernorm_on_a_zero_mean_row_and_not_on_a_shifted_one():
    """With gamma = 1, beta = 0 and a row whose mean is 0 both norms are v / sqrt(mean(v^2) + eps).  The row is built
    as [a, -a], so its float32 mean is 0 up to the rounding of the partial sums (about 2^-24 of the largest partial,
    divided by w); LN then subtracts that and both results differ by a few float32 roundings of values of order 1:
    1e-5 absolute is two orders above that and four below the values.  Shifting the row by 3 moves the LayerNorm not
    at all and the RMS norm by about the shift over the row's scale: the check can tell the two apart."""
    w = 256
    a = _rows(5, w // 2, 31) - F(0.5)
    v = np.concatenate([a, -a], axis=1)
    one, zero = np.ones(w, F), np.zeros(w, F)
    ln, rms = SO.layernorm_rows(v, None, one, zero, 1e-5), GO.rmsnorm_rows(v, None, one, 1e-5)
    assert np.abs(ln.astype(np.float64) - rms).max() <= 1e-5
    shifted = v + F(3.0)
    ln_s, rms_s = SO.layernorm_rows(shifted, None, one, zero, 1e-5), GO.rmsnorm_rows(shifted, None, one, 1e-5)
    assert np.abs(ln_s.astype(np.float64) - ln).max() <= 1e-5
    assert np.abs(rms_s.astype(np.float64) - ln_s).max() > 0.1


# ---- 3. the quantized Llama block against a float64 Llama block ---------------------------------------------------------
D, H, DFF, BLOCKS, SEQ = 64, 4, 200, 2, 9
DK = D // H
# relative Frobenius errors of gated_oracle's chain (arch 0x6F01, SiLU) against llama_f64, measured on the CPU on
# gated_oracle.init_scale_weights: the fp32 wiring and the quantized chain
LLAMA_WIRING_MEASURED = 1.107e-7
LLAMA_QUANT_MEASURED = 1.279e-2
# (on the same weights and tables the LayerNorm + ungated chain: 0.487 with relu, 0.451 with GELU; RMS alone 0.347, the
# gate alone 0.344 -- all more than ten times the bound.  On gated_weights' heavy tails, columns scaled by 50, the
# quantized chain itself is at 0.22: that set is for bit-exactness on the device, not for an accuracy statement)


def llama_f64(X, W, tables, eps):
    """Pre-norm, RMSNorm, rotate_half RoPE, causal attention, SwiGLU and a final RMSNorm in float64, with the biases
    the weight set carries; nothing of the oracle's but the weight set."""
    x = np.asarray(X, np.float64)
    cos, sin = (np.asarray(t, np.float64)[:x.shape[0]] for t in tables)
    h = DK // 2

    def rms(v, g):
        return v / np.sqrt((v * v).mean(axis=-1, keepdims=True) + eps) * np.asarray(g, np.float64)

    def rot(t):  # rows x d_k, one head
        a, b = t[:, :h], t[:, h:]
        return np.concatenate([a * cos - b * sin, b * cos + a * sin], axis=1)

    mask = np.triu(np.ones((x.shape[0], x.shape[0]), bool), 1)
    for i in range(BLOCKS):
        n = rms(x, W[i, G1])
        heads = []
        for j in range(H):
            q, k, v = (n @ W[i, kind][j].astype(np.float64) + W[i, bk][j * DK:(j + 1) * DK]
                       for kind, bk in ((WQ, BQ), (WK, BK), (WV, BV)))
            s = rot(q) @ rot(k).T / np.sqrt(DK)
            s[mask] = -np.inf
            p = np.exp(s - s.max(axis=1, keepdims=True))
            heads.append(p / p.sum(axis=1, keepdims=True) @ v)
        x = x + np.concatenate(heads, axis=1) @ W[i, WO].astype(np.float64) + W[i, BO]
        n = rms(x, W[i, G3])
        gate = n @ W[i, W1].astype(np.float64) + W[i, B1]
        up = n @ W[i, GO.W3].astype(np.float64) + W[i, GO.B3]
        x = x + (gate / (1.0 + np.exp(-gate)) * up) @ W[i, W2].astype(np.float64) + W[i, B2]
    return rms(x, W[0, GO.GF])


def _rel_fro(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want))


def test_quantized_llama_block_against_float64(oracle):
    W = GO.init_scale_weights(D, H, DFF, BLOCKS, 23)
    X = _rows(SEQ, D, 21) / F(3.0)
    tables = RO.make_tables(16, DK)
    want = llama_f64(X, W, tables, float(F(1e-5)))

    def chain(arch, activation, mm=None):
        return _rel_fro(GO.forward(X, None, W, D, H, BLOCKS, arch, True, activation, 1e-5, mm, tables), want)

    # the fp32 wiring first: the same chain on a plain float32 matmul is float64's up to float32 rounding
    wired = chain(GO.LLAMA, "silu", lambda x, w: np.matmul(x, w, dtype=F))
    print(f"Llama wiring: relative Frobenius error {wired:.3e}")
    assert wired <= 4 * LLAMA_WIRING_MEASURED
    err = chain(GO.LLAMA, "silu")
    # the same weights through the LayerNorm + ungated chain, and with one of the two bits alone: the test must be able
    # to tell the wiring apart
    others = {"LayerNorm + ungated relu": chain(GO.LLAMA & ~(GO.RMSNORM | GO.GATED_FFN), "relu"),
              "LayerNorm + ungated GELU": chain(GO.LLAMA & ~(GO.RMSNORM | GO.GATED_FFN), "gelu_tanh"),
              "RMS alone": chain(GO.LLAMA & ~GO.GATED_FFN, "relu"), "the gate alone": chain(GO.LLAMA & ~GO.RMSNORM, "silu")}
    print(f"quantized Llama block: relative Frobenius error {err:.3e}; " +
          ", ".join(f"{k} {v:.3e}" for k, v in others.items()))
    bound = 2 * LLAMA_QUANT_MEASURED
    assert err <= bound
    for what, e in others.items():
        assert e > 10 * bound, what


def test_the_bits_are_independent(oracle):
    """RMSNORM alone and GATED_FFN alone are chains of their own, and neither is the Llama chain."""
    W = GO.gated_weights(D, H, DFF, BLOCKS, 23)
    X = _rows(SEQ, D, 21) / F(3.0)
    outs = [GO.forward(X, None, W, D, H, BLOCKS, 1 | bits, False, "relu") for bits in (0, GO.RMSNORM, GO.GATED_FFN,
                                                                                        GO.RMSNORM | GO.GATED_FFN)]
    for a in range(4):
        for b in range(a + 1, 4):
            assert np.abs(outs[a] - outs[b]).max() > 1e-3
    # without either bit the forward is the older oracles', bit for bit
    assert_bits_equal(outs[0], SO.encoder_forward_std(X, W, D, H, BLOCKS, "relu"), "post-LN, no new bit")
    assert_bits_equal(GO.forward(X, None, W, D, H, BLOCKS, 0x301, True, "gelu_tanh"),
                      RO.decoder_only_forward(X, W, D, H, BLOCKS, 0x301, True, None, "gelu_tanh"), "pre-LN, no new bit")


# ---- 4. refusals before any GPU call --------------------------------------------------------------------------------------
def _desc(qg, **kw):
    d = dict(size=ctypes.sizeof(qg.ModelDesc), cross=0, d_model=8, n_heads=2, d_ff=8, n_blocks=1, max_seq=4,
             max_enc_seq=0, seed=1, flags=0, n_slots=0, max_rows=0, arch=qg.QGEMM_ARCH_STANDARD,
             activation=qg.QGEMM_ACT_RELU, ln_eps=1e-5)
    d.update(kw)
    return qg.ModelDesc(**d)


@pytest.mark.parametrize("kw", [
    dict(arch=0x2000), dict(arch=0x4000), dict(arch=0x6000), dict(arch=0x1001), dict(arch=0x8001), dict(arch=0x7001),
    dict(arch=0x10001), dict(activation=3), dict(arch=0x6001, activation=3), dict(arch=0x2001, activation=2),
    dict(arch=1, activation=2), dict(arch=0x101, activation=2), dict(arch=0x4001, d_ff=16388),
    dict(arch=0x4001, activation=2, d_ff=16388), dict(size=60, arch=0x6001),
    dict(arch=0x4001, d_model=2, n_heads=1, d_ff=8200, max_rows=1 << 17),   # 2^17 rows x 2 d_ff columns pass int32
], ids=lambda kw: ",".join(f"{k}={v:#x}" if k == "arch" else f"{k}={v}" for k, v in kw.items()))
def test_model_create_refusals(qg, kw):
    L = qg.load()
    h = ctypes.c_void_p(5)
    d = _desc(qg, **kw)
    assert ctypes.sizeof(qg.ModelDesc) == 64
    assert L.qgemm_model_create(ctypes.byref(d), ctypes.byref(h)) == qg.HIP_ERROR_INVALID_VALUE
    assert not h.value


def test_python_keyword_refusals(qg):
    for kw in (dict(norm="rms"), dict(gated_ffn=True), dict(arch="standard", norm="root"),
               dict(arch="standard", activation="silu"), dict(arch="standard", norm="rms", activation="silu"),
               dict(arch="standard", gated_ffn=True, activation="swish")):
        with pytest.raises(AssertionError):
            qg.Encoder(8, 2, 8, 1, 4, **kw)
        with pytest.raises(AssertionError):
            qg.Decoder(8, 2, 8, 1, 4, 0, decoder_only=True, **kw)


P = 4096  # a non-null pointer that a refused call never reads


def test_row_entry_point_refusals(qg):
    L, bad = qg.load(), qg.HIP_ERROR_INVALID_VALUE
    rn = L.qgemm_rmsnorm_rows
    assert rn(0, P, P, 1e-5, P, 1, 8, None) == bad
    assert rn(P, P, 0, 1e-5, P, 1, 8, None) == bad
    assert rn(P, P, P, 1e-5, 0, 1, 8, None) == bad
    assert rn(P, P, P, 1e-5, P, 1, 0, None) == bad
    assert rn(P, P, P, 1e-5, P, 1, 4097, None) == bad
    assert rn(P, P, P, 1e-5, P, -1, 8, None) == bad
    assert rn(P, 0, P, 1e-5, P, 0, 8, None) == 0      # rows == 0; B may be null
    rp = L.qgemm_rmsnorm_pack_a
    assert rp(0, P, P, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert rp(P, P, 0, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert rp(P, P, P, 1e-5, 0, 1, 8, 127.0, P, None) == bad
    assert rp(P, P, P, 1e-5, P, 1, 8, 127.0, 0, None) == bad
    assert rp(P, P, P, 1e-5, P, 1, 0, 127.0, P, None) == bad
    assert rp(P, P, P, 1e-5, P, 1, 4097, 127.0, P, None) == bad
    assert rp(P, P, P, 1e-5, P, -1, 8, 127.0, P, None) == bad
    assert rp(P, 0, P, 1e-5, P, 0, 8, 127.0, P, None) == 0
    pp = L.qgemm_prenorm_rms_pack_a
    assert pp(0, P, P, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert pp(P, P, 0, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert pp(P, P, P, 1e-5, P, 1, 8, 127.0, 0, None) == bad
    assert pp(P, P, P, 1e-5, P, 1, 0, 127.0, P, None) == bad
    assert pp(P, P, P, 1e-5, P, 1, 4097, 127.0, P, None) == bad
    assert pp(P, P, P, 1e-5, P, -1, 8, 127.0, P, None) == bad
    assert pp(P, 0, P, 1e-5, 0, 0, 8, 127.0, P, None) == 0      # rows == 0; B and S may be null
    g = L.qgemm_glu_rows
    assert g(0, 16, P, 8, 1, 8, 2, None) == bad
    assert g(P, 16, 0, 8, 1, 8, 2, None) == bad
    assert g(P, -1, P, 8, 1, 8, 2, None) == bad
    assert g(P, 16, P, -1, 1, 8, 2, None) == bad
    assert g(P, 16, P, 8, 1, 0, 2, None) == bad
    assert g(P, 16, P, 8, -1, 8, 2, None) == bad
    assert g(P, 16, P, 8, 1, 8, 3, None) == bad
    assert g(P, 16, P, 8, 1, 8, -1, None) == bad
    assert g(P, 15, P, 8, 2, 8, 2, None) == bad      # two rows closer than 2w
    assert g(P, 16, P, 7, 2, 8, 2, None) == bad
    assert g(P, 16, P, 8, 0, 8, 2, None) == 0
    gp = L.qgemm_glu_pack_a
    assert gp(0, 16, 1, 8, 2, 127.0, P, None) == bad
    assert gp(P, 16, 1, 8, 2, 127.0, 0, None) == bad
    assert gp(P, -1, 1, 8, 2, 127.0, P, None) == bad
    assert gp(P, 16, 1, 0, 2, 127.0, P, None) == bad
    assert gp(P, 32770, 1, 16385, 2, 127.0, P, None) == bad
    assert gp(P, 16, -1, 8, 2, 127.0, P, None) == bad
    assert gp(P, 16, 1, 8, 3, 127.0, P, None) == bad
    assert gp(P, 16, 1, 8, -1, 127.0, P, None) == bad
    assert gp(P, 15, 2, 8, 2, 127.0, P, None) == bad   # x_stride_h < 2k with m > 1
    assert gp(P, 16, 0, 8, 2, 127.0, P, None) == 0


def test_constants_and_exported_names(qg):
    assert (qg.QGEMM_ARCH_RMSNORM, qg.QGEMM_ARCH_GATED_FFN, qg.QGEMM_ACT_SILU) == (0x2000, 0x4000, 2)
    assert (qg.KIND_W3, qg.KIND_B3) == (30, 31) == (GO.W3, GO.B3)
    assert qg.ACTIVATIONS["silu"] == 2
    for name in ("qgemm_rmsnorm_rows", "qgemm_rmsnorm_pack_a", "qgemm_prenorm_rms_pack_a", "qgemm_glu_rows",
                 "qgemm_glu_pack_a"):
        assert name in qg.EXPORTED_SYMBOLS and hasattr(qg.load(), name)
    for name in ("rmsnorm_rows", "rmsnorm_pack_a", "prenorm_rms_pack_a", "glu_rows", "glu_pack_a"):
        assert callable(getattr(qg, name))
    assert GO.LLAMA == 0x6F01
