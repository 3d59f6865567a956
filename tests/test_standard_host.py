"""The standard post-LN block without a GPU: tests/standard_oracle.py against float64 formulas and
against torch.nn's layers, the sum order's two layouts, and the refusals of the new entry points.

Every bound below is a multiple of an error MEASURED on the CPU with these fixed, seeded inputs (the table in DESIGN.md
s25 records the same figures): 4x for the float32 oracle against float64 and for the fp32 wiring against torch -- the
margin covers another machine's libm and BLAS summation order, nothing else -- and 2x for the quantized chain against
torch, whose error is the int8 quantization's and does not move with the library."""
import ctypes
import math

import numpy as np
import pytest

import standard_oracle as SO
import weights_oracle
from util import assert_bits_equal

F = np.float32
D, H, DFF, SEQ, ENC_SEQ, LAYERS = 64, 4, 128, 9, 7, 2

# ---- 1. the oracle's LN and GELU against float64 ------------------------------------------------------------------------
# measured maximum absolute error of layernorm_rows over 8 rows of normal * 3 + 0.5 (gamma, beta random), per width
LN_MEASURED = {1: 0.0, 2: 1.546e-7, 3: 2.202e-7, 4: 2.859e-7, 5: 1.856e-7, 64: 4.825e-7, 100: 4.795e-7, 255: 4.128e-7,
               256: 5.418e-7, 257: 5.441e-7, 1024: 6.732e-7, 1028: 6.668e-7, 2048: 5.876e-7, 4096: 7.881e-7}
# measured maximum error of gelu_rows over 64 x 4096 such values, relative to max(|g|, 2^-126), where exp(-z) is finite
# (z reaches -88 there and fl(t q) carries its rounding into the exponent: about 88 x 2^-24 x a few)
GELU_MEASURED = 1.082e-5


def _rows(rows, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, w)) * 3.0 + 0.5).astype(F)


@pytest.mark.parametrize("w", sorted(LN_MEASURED))
def test_oracle_layernorm_against_float64(w):
    A, B = _rows(8, w, 100 + w), _rows(8, w, 200 + w)
    rng = np.random.default_rng(300 + w)
    gamma = (1.0 + 0.2 * rng.standard_normal(w)).astype(F)
    beta = (0.2 * rng.standard_normal(w)).astype(F)
    got = SO.layernorm_rows(A, B, gamma, beta, 1e-5)
    want = SO.layernorm_f64(A, B, gamma, beta, 1e-5)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"LN w={w}: max abs error {err:.3e}")
    assert err <= 4 * LN_MEASURED[w]
    # B = None is LN(A)
    got = SO.layernorm_rows(A, None, gamma, beta, 1e-5)
    assert np.abs(got.astype(np.float64) - SO.layernorm_f64(A, None, gamma, beta, 1e-5)).max() <= 4 * LN_MEASURED[w]


def test_oracle_gelu_against_float64():
    X = _rows(64, 4096, 7)
    got = SO.gelu_rows(X).astype(np.float64)
    x = X.astype(np.float64)
    # the same function in its stable float64 form, x sigmoid(2u); the tanh form agrees with it to float64 rounding
    # where tanh has not saturated
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    want = x / (1.0 + np.exp(-2.0 * u))
    mid = np.abs(x) < 3
    assert np.abs(want[mid] - SO.gelu_tanh_f64(x)[mid]).max() < 1e-14
    # where exp(-z) passes FLT_MAX (2u < -88) the contract gives x / inf = -0 for a true value below |x| / FLT_MAX:
    # an absolute statement there, the relative error everywhere else
    far = 2.0 * u < -88.0
    assert far.any() and np.abs(got[far] - want[far]).max() <= 2.0 ** -120
    err = float((np.abs(got - want)[~far] / np.maximum(np.abs(want[~far]), 2.0 ** -126)).max())
    print(f"GELU: max relative error {err:.3e}")
    assert err <= 4 * GELU_MEASURED


def test_oracle_gelu_special_values():
    g = SO.gelu_rows(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -100.0, 100.0], F))
    assert g[0] == 0 and not np.signbit(g[0]) and g[1] == 0 and np.signbit(g[1])
    assert g[2] == np.inf and np.isnan(g[3]) and np.isnan(g[4])
    assert g[5] == 0 and np.signbit(g[5]) and g[6] == F(100.0)


# ---- 4. the sum order: the register layout and the fallback layout agree -------------------------------------------------
@pytest.mark.parametrize("w", [1, 3, 4, 5, 64, 100, 255, 256, 257, 260, 1024, 1028, 4095, 4096])
def test_sum_order_layouts_agree(w):
    v = _rows(3, w, 400 + w)
    v[1, 0] = -0.0
    a, b = SO.rowsum_registers(v), SO.rowsum_fallback(v)
    assert_bits_equal(a, b, f"rowsum w={w}")
    gamma, beta = np.full(w, 1.25, F), np.full(w, -0.5, F)
    assert_bits_equal(SO.layernorm_rows(v, None, gamma, beta, 1e-5, rowsum=SO.rowsum_registers),
                      SO.layernorm_rows(v, None, gamma, beta, 1e-5, rowsum=SO.rowsum_fallback), f"LN w={w}")
    # independent of rows: a row alone gives the bits it has among others
    assert_bits_equal(SO.rowsum_registers(v[1:2]), a[1:2], "one row")


def test_sum_order_is_not_the_sequential_chain():
    """The contract's order is its own: on a long row it differs from the left-to-right chain in some bits."""
    v = _rows(16, 4096, 5)
    seq = np.zeros(16, F)
    for c in range(4096):
        seq = seq + v[:, c]
    assert (SO.rowsum_registers(v).view(np.uint32) != seq.view(np.uint32)).any()


# ---- 2. and 3. the chains against torch ----------------------------------------------------------------------------------
# relative Frobenius errors measured on the CPU, keyed (decoder, activation): the fp32 wiring and the quantized chain
WIRING_MEASURED = {(False, "relu"): 1.593e-7, (False, "gelu_tanh"): 1.647e-7, (True, "relu"): 1.976e-7,
                   (True, "gelu_tanh"): 1.881e-7}
QUANT_MEASURED = {(False, "relu"): 1.270e-2, (False, "gelu_tanh"): 1.523e-2, (True, "relu"): 1.687e-2,
                  (True, "gelu_tanh"): 1.729e-2}
# (the reference-architecture chain on the same matrices: 1.45, 1.80, 1.59 and 1.54 -- two orders above the bound)


def _torch_layers(decoder: bool, activation: str):
    import torch
    import torch.nn.functional as Fn
    torch.manual_seed(11 + (2 if decoder else 0) + (1 if activation == "relu" else 0))
    act = Fn.relu if activation == "relu" else (lambda x: Fn.gelu(x, approximate="tanh"))
    cls = torch.nn.TransformerDecoderLayer if decoder else torch.nn.TransformerEncoderLayer
    layers = [cls(D, H, dim_feedforward=DFF, dropout=0.0, activation=act, norm_first=False) for _ in range(LAYERS)]
    with torch.no_grad():
        for layer in layers:
            layer.eval()
            for name, p in layer.named_parameters():
                if "norm" in name and name.endswith("weight"):
                    p.copy_(1.0 + 0.2 * torch.randn_like(p))   # gamma != 1
                elif name.endswith("bias"):
                    p.copy_(0.2 * torch.randn_like(p))         # beta and every bias != 0
    return layers


def _torch_forward(layers, X, enc):
    import torch
    with torch.no_grad():
        x = torch.from_numpy(X)
        for layer in layers:
            if enc is None:
                x = layer(x)
            else:
                mask = torch.nn.Transformer.generate_square_subsequent_mask(x.shape[0])
                x = layer(x, torch.from_numpy(enc), tgt_mask=mask)
        return x.numpy()


def _rel_fro(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want.astype(np.float64)))


def _chain(W, X, enc, activation, mm):
    if enc is None:
        return SO.encoder_forward_std(X, W, D, H, LAYERS, activation, 1e-5, mm)
    return SO.decoder_forward_std(X, enc, W, D, H, LAYERS, True, activation, 1e-5, mm)


@pytest.fixture(scope="module", params=sorted(WIRING_MEASURED))
def torch_case(request, oracle):
    decoder, activation = request.param
    layers = _torch_layers(decoder, activation)
    X = _rows(SEQ, D, 21) / F(3.0)
    enc = _rows(ENC_SEQ, D, 22) / F(3.0) if decoder else None
    return request.param, layers, SO.torch_layer_weights(layers, H), X, enc, _torch_forward(layers, X, enc)


def test_wiring_against_torch_fp32(torch_case):
    key, _, W, X, enc, want = torch_case
    got = _chain(W, X, enc, key[1], lambda x, w: np.matmul(x, w, dtype=F))
    err = _rel_fro(got, want)
    print(f"wiring {key}: relative Frobenius error {err:.3e}")
    assert err <= 4 * WIRING_MEASURED[key]


def test_quantized_chain_against_torch(torch_case):
    key, _, W, X, enc, want = torch_case
    err = _rel_fro(_chain(W, X, enc, key[1], None), want)
    # the same matrices through the reference architecture's chain: the test must be able to tell the wiring apart
    ref = (weights_oracle.encoder_forward_w(X, W, D, H, LAYERS) if enc is None
           else weights_oracle.decoder_forward_w(X, enc, W, D, H, LAYERS, causal=True))
    err_ref = _rel_fro(ref, want)
    print(f"quantized {key}: relative Frobenius error {err:.3e}; the reference-arch chain {err_ref:.3e}")
    bound = 2 * QUANT_MEASURED[key]
    assert err <= bound
    assert err_ref > 10 * bound


# ---- 5. refusals before any GPU call -------------------------------------------------------------------------------------
def _desc(qg, **kw):
    d = dict(size=ctypes.sizeof(qg.ModelDesc), cross=0, d_model=8, n_heads=2, d_ff=8, n_blocks=1, max_seq=4,
             max_enc_seq=0, seed=1, flags=0, n_slots=0, max_rows=0, arch=qg.QGEMM_ARCH_STANDARD,
             activation=qg.QGEMM_ACT_RELU, ln_eps=1e-5)
    d.update(kw)
    return qg.ModelDesc(**d)


@pytest.mark.parametrize("kw", [
    dict(size=0), dict(size=60), dict(arch=2), dict(arch=-1), dict(activation=2), dict(activation=-1),
    dict(arch=0, activation=1), dict(ln_eps=-1e-5), dict(ln_eps=float("nan")), dict(cross=2),
    dict(flags=1), dict(n_slots=2), dict(n_slots=-1), dict(max_rows=-1), dict(d_model=1), dict(n_heads=3),
    dict(max_seq=0), dict(max_seq=4097), dict(cross=1, max_enc_seq=0), dict(cross=1, max_enc_seq=4, flags=8),
    dict(cross=1, max_enc_seq=4, flags=2), dict(cross=1, max_enc_seq=4, flags=1, n_slots=2),
    dict(cross=1, max_enc_seq=4, flags=9, n_slots=65),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_model_create_refusals(qg, kw):
    L = qg.load()
    h = ctypes.c_void_p(5)
    d = _desc(qg, **kw)
    assert L.qgemm_model_create(ctypes.byref(d), ctypes.byref(h)) == qg.HIP_ERROR_INVALID_VALUE
    assert not h.value


def test_model_create_null_pointers(qg):
    L = qg.load()
    h = ctypes.c_void_p()
    d = _desc(qg)
    assert L.qgemm_model_create(None, ctypes.byref(h)) == qg.HIP_ERROR_INVALID_VALUE
    assert L.qgemm_model_create(ctypes.byref(d), None) == qg.HIP_ERROR_INVALID_VALUE
    assert L.qgemm_model_info(None, ctypes.byref(d)) == qg.HIP_ERROR_INVALID_VALUE


P = 4096  # a non-null pointer that a refused call never reads


def test_row_entry_point_refusals(qg):
    L, bad = qg.load(), qg.HIP_ERROR_INVALID_VALUE
    ln = L.qgemm_layernorm_rows
    assert ln(0, P, P, P, 1e-5, P, 1, 8, None) == bad
    assert ln(P, P, 0, P, 1e-5, P, 1, 8, None) == bad
    assert ln(P, P, P, 0, 1e-5, P, 1, 8, None) == bad
    assert ln(P, P, P, P, 1e-5, 0, 1, 8, None) == bad
    assert ln(P, P, P, P, 1e-5, P, 1, 0, None) == bad
    assert ln(P, P, P, P, 1e-5, P, 1, 4097, None) == bad
    assert ln(P, P, P, P, 1e-5, P, -1, 8, None) == bad
    assert ln(P, 0, P, P, 1e-5, P, 0, 8, None) == 0      # rows == 0; B may be null
    lp = L.qgemm_layernorm_pack_a
    assert lp(0, P, P, P, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert lp(P, P, 0, P, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert lp(P, P, P, 0, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert lp(P, P, P, P, 1e-5, 0, 1, 8, 127.0, P, None) == bad
    assert lp(P, P, P, P, 1e-5, P, 1, 8, 127.0, 0, None) == bad
    assert lp(P, P, P, P, 1e-5, P, 1, 0, 127.0, P, None) == bad
    assert lp(P, P, P, P, 1e-5, P, 1, 4097, 127.0, P, None) == bad
    assert lp(P, P, P, P, 1e-5, P, -1, 8, 127.0, P, None) == bad
    assert lp(P, 0, P, P, 1e-5, P, 0, 8, 127.0, P, None) == 0
    g = L.qgemm_gelu_rows
    assert g(0, 8, P, 8, 1, 8, None) == bad
    assert g(P, 8, 0, 8, 1, 8, None) == bad
    assert g(P, -1, P, 8, 1, 8, None) == bad
    assert g(P, 8, P, -1, 1, 8, None) == bad
    assert g(P, 8, P, 8, 1, 0, None) == bad
    assert g(P, 8, P, 8, -1, 8, None) == bad
    assert g(P, 8, P, 8, 0, 8, None) == 0
    gp = L.qgemm_gelu_pack_a
    assert gp(0, 8, 1, 8, 127.0, P, None) == bad
    assert gp(P, 8, 1, 8, 127.0, 0, None) == bad
    assert gp(P, -1, 1, 8, 127.0, P, None) == bad
    assert gp(P, 8, 1, 0, 127.0, P, None) == bad
    assert gp(P, 16385, 1, 16385, 127.0, P, None) == bad
    assert gp(P, 8, -1, 8, 127.0, P, None) == bad
    assert gp(P, 8, 0, 8, 127.0, P, None) == 0


def test_python_refuses_unknown_names(qg):
    with pytest.raises(AssertionError):
        qg.Encoder(8, 2, 8, 1, 4, arch="pre-ln")
    with pytest.raises(AssertionError):
        qg.Encoder(8, 2, 8, 1, 4, arch="standard", activation="gelu_erf")
    assert (qg.KIND_BQ, qg.KIND_BO, qg.KIND_G1, qg.KIND_BE3, qg.KIND_BQ2, qg.KIND_BE2) == (12, 15, 16, 19, 20, 25)
