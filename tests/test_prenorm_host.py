"""The pre-LN block without a GPU: tests/prenorm_oracle.py against torch.nn's norm_first=True layers
chained by hand plus a final LayerNorm, and the refusals of the new architecture bits, keywords and entry points.

Every bound is a multiple of an error MEASURED on the CPU with these fixed, seeded inputs (the table in DESIGN.md s26
records the same figures), as tests/test_standard_host.py does: 4x for the fp32 wiring against torch -- the margin covers
another machine's libm and BLAS summation order, nothing else -- and 2x for the quantized chain, whose error is the int8
quantization's and does not move with the library."""
import ctypes

import numpy as np
import pytest

import prenorm_oracle as PO
import standard_oracle as SO

F = np.float32
D, H, DFF, SEQ, ENC_SEQ, LAYERS = 64, 4, 128, 9, 7, 2

# relative Frobenius errors measured on the CPU, keyed (decoder, activation, final_norm): the fp32 wiring and the
# quantized chain
WIRING_MEASURED = {
    (False, "relu", False): 1.043e-7, (False, "relu", True): 1.389e-7,
    (False, "gelu_tanh", False): 1.220e-7, (False, "gelu_tanh", True): 1.422e-7,
    (True, "relu", False): 1.323e-7, (True, "relu", True): 1.513e-7,
    (True, "gelu_tanh", False): 1.437e-7, (True, "gelu_tanh", True): 1.462e-7,
}
QUANT_MEASURED = {
    (False, "relu", False): 1.316e-2, (False, "relu", True): 1.640e-2,
    (False, "gelu_tanh", False): 1.679e-2, (False, "gelu_tanh", True): 1.206e-2,
    (True, "relu", False): 2.058e-2, (True, "relu", True): 1.356e-2,
    (True, "gelu_tanh", False): 1.723e-2, (True, "gelu_tanh", True): 1.247e-2,
}
# (the post-LN chain of standard_oracle on the same tensors, in the order of the rows above: 0.506, 0.568, 0.576, 0.613,
# 0.599, 0.640, 0.622, 0.626 -- at least 14x the bound it must clear by 10x)


def _rows(rows, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, w)) * 3.0 + 0.5).astype(F)


def torch_model(decoder: bool, activation: str, final_norm: bool):
    """LAYERS torch.nn layers with norm_first=True, every gamma != 1 and every bias and beta != 0, and the LayerNorm
    behind them (None without a final norm)."""
    import torch
    import torch.nn.functional as Fn
    torch.manual_seed(31 + (4 if decoder else 0) + (2 if activation == "relu" else 0) + (1 if final_norm else 0))
    act = Fn.relu if activation == "relu" else (lambda x: Fn.gelu(x, approximate="tanh"))
    cls = torch.nn.TransformerDecoderLayer if decoder else torch.nn.TransformerEncoderLayer
    layers = [cls(D, H, dim_feedforward=DFF, dropout=0.0, activation=act, norm_first=True) for _ in range(LAYERS)]
    norm = torch.nn.LayerNorm(D, eps=1e-5) if final_norm else None
    with torch.no_grad():
        for m in layers + ([norm] if final_norm else []):
            m.eval()
            for name, p in m.named_parameters():
                if name.endswith("bias"):
                    p.copy_(0.2 * torch.randn_like(p))         # beta and every bias != 0
                elif "norm" in name or m is norm:
                    p.copy_(1.0 + 0.2 * torch.randn_like(p))   # gamma != 1
    return layers, norm


def torch_forward(layers, norm, X, enc):
    import torch
    with torch.no_grad():
        x = torch.from_numpy(X)
        for layer in layers:
            if enc is None:
                x = layer(x)
            else:
                mask = torch.nn.Transformer.generate_square_subsequent_mask(x.shape[0])
                x = layer(x, torch.from_numpy(enc), tgt_mask=mask)
        return (x if norm is None else norm(x)).numpy()


def rel_fro(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want.astype(np.float64)))


def inputs(decoder: bool):
    X = _rows(SEQ, D, 21) / F(3.0)
    return X, (_rows(ENC_SEQ, D, 22) / F(3.0) if decoder else None)


def chain(W, X, enc, activation, final_norm, mm):
    if enc is None:
        return PO.encoder_forward_pre(X, W, D, H, LAYERS, activation, final_norm, 1e-5, mm)
    return PO.decoder_forward_pre(X, enc, W, D, H, LAYERS, True, activation, final_norm, 1e-5, mm)


def case_id(key):
    return f"{'dec' if key[0] else 'enc'}-{key[1]}-{'lnf' if key[2] else 'nolnf'}"


@pytest.fixture(scope="module", params=sorted(WIRING_MEASURED), ids=case_id)
def torch_case(request, oracle):
    decoder, activation, final_norm = request.param
    layers, norm = torch_model(decoder, activation, final_norm)
    X, enc = inputs(decoder)
    return request.param, PO.torch_model_weights(layers, H, norm), X, enc, torch_forward(layers, norm, X, enc)


def test_wiring_against_torch_fp32(torch_case):
    key, W, X, enc, want = torch_case
    err = rel_fro(chain(W, X, enc, key[1], key[2], lambda x, w: np.matmul(x, w, dtype=F)), want)
    print(f"pre-LN wiring {key}: relative Frobenius error {err:.3e}")
    assert err <= 4 * WIRING_MEASURED[key]


def test_quantized_chain_against_torch(torch_case):
    key, W, X, enc, want = torch_case
    err = rel_fro(chain(W, X, enc, key[1], key[2], None), want)
    # the same tensors through the post-LN chain: the test must be able to tell the wirings apart
    post = (SO.encoder_forward_std(X, W, D, H, LAYERS, key[1]) if enc is None
            else SO.decoder_forward_std(X, enc, W, D, H, LAYERS, True, key[1]))
    err_post = rel_fro(post, want)
    print(f"pre-LN quantized {key}: relative Frobenius error {err:.3e}; the post-LN chain {err_post:.3e}")
    bound = 2 * QUANT_MEASURED[key]
    assert err <= bound
    assert err_post > 10 * bound


def test_boundary_oracle_is_the_post_ln_kernels():
    """prenorm_rows restates nothing: S is one add, and its LN is layernorm_rows(A, B) bit for bit."""
    rng = np.random.default_rng(5)
    A, B = _rows(5, 100, 1), _rows(5, 100, 2)
    g, b = (1.0 + 0.2 * rng.standard_normal(100)).astype(F), (0.2 * rng.standard_normal(100)).astype(F)
    S, Y = PO.prenorm_rows(A, B, g, b, 1e-5)
    assert np.array_equal(S.view(np.uint32), (A + B).view(np.uint32))
    assert np.array_equal(Y.view(np.uint32), SO.layernorm_rows(A, B, g, b, 1e-5).view(np.uint32))
    S, Y = PO.prenorm_rows(A, None, g, b, 1e-5)
    assert np.array_equal(S.view(np.uint32), A.view(np.uint32))
    assert np.array_equal(Y.view(np.uint32), SO.layernorm_rows(A, None, g, b, 1e-5).view(np.uint32))


# ---- refusals before any GPU call -------------------------------------------------------------------------------------
def _desc(qg, **kw):
    d = dict(size=ctypes.sizeof(qg.ModelDesc), cross=0, d_model=8, n_heads=2, d_ff=8, n_blocks=1, max_seq=4,
             max_enc_seq=0, seed=1, flags=0, n_slots=0, max_rows=0, arch=0x301, activation=qg.QGEMM_ACT_RELU, ln_eps=1e-5)
    d.update(kw)
    return qg.ModelDesc(**d)


@pytest.mark.parametrize("kw", [
    dict(arch=0x100),                 # NORM_FIRST on the reference architecture
    dict(arch=0x201),                 # FINAL_NORM without NORM_FIRST
    dict(arch=0x401),                 # a bit above the low byte that is no modifier
    dict(arch=0x101, activation=2),   # a good arch, an unknown activation
    dict(arch=0x301, n_heads=3),      # a good arch and activation: refused for the head count alone
    dict(arch=0x300), dict(arch=0x102), dict(arch=0x10101), dict(arch=-0x100 | 1),
], ids=lambda kw: ",".join(f"{k}={v:#x}" if k == "arch" else f"{k}={v}" for k, v in kw.items()))
def test_model_create_refusals(qg, kw):
    L = qg.load()
    h = ctypes.c_void_p(5)
    d = _desc(qg, **kw)
    assert L.qgemm_model_create(ctypes.byref(d), ctypes.byref(h)) == qg.HIP_ERROR_INVALID_VALUE
    assert not h.value


def test_python_keyword_refusals(qg):
    with pytest.raises(AssertionError):
        qg.Encoder(8, 2, 8, 1, 4, arch="standard", final_norm=True)                  # without norm_first
    with pytest.raises(AssertionError):
        qg.Encoder(8, 2, 8, 1, 4, norm_first=True)                                   # arch="reference"
    with pytest.raises(AssertionError):
        qg.Decoder(8, 2, 8, 1, 4, 4, arch="reference", norm_first=True, final_norm=True)
    with pytest.raises(AssertionError):
        qg.Decoder(8, 2, 8, 1, 4, 4, arch="standard", final_norm=True)
    with pytest.raises(AssertionError):
        qg.Encoder(8, 2, 8, 1, 4, arch="pre-ln", norm_first=True)                    # still no architecture's name
    assert (qg.KIND_GF, qg.KIND_BEF) == (26, 27)
    assert (qg.QGEMM_ARCH_NORM_FIRST, qg.QGEMM_ARCH_FINAL_NORM) == (0x100, 0x200)
    for name in ("qgemm_prenorm_pack_a", "qgemm_add_rows"):
        assert name in qg.EXPORTED_SYMBOLS


P = 4096  # a non-null pointer that a refused call never reads


def test_row_entry_point_refusals(qg):
    L, bad = qg.load(), qg.HIP_ERROR_INVALID_VALUE
    pp = L.qgemm_prenorm_pack_a
    assert pp(0, P, P, P, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert pp(P, P, 0, P, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert pp(P, P, P, 0, 1e-5, P, 1, 8, 127.0, P, None) == bad
    assert pp(P, P, P, P, 1e-5, P, 1, 8, 127.0, 0, None) == bad
    assert pp(P, P, P, P, 1e-5, P, 1, 0, 127.0, P, None) == bad
    assert pp(P, P, P, P, 1e-5, P, 1, 4097, 127.0, P, None) == bad
    assert pp(P, P, P, P, 1e-5, P, -1, 8, 127.0, P, None) == bad
    assert pp(P, 0, P, P, 1e-5, 0, -1, 8, 127.0, P, None) == bad   # (a null B and a null S are no excuse)
    assert pp(P, 0, P, P, 1e-5, 0, 0, 8, 127.0, P, None) == 0      # rows == 0; B and S may be null
    ar = L.qgemm_add_rows
    assert ar(0, P, P, 1, 8, None) == bad
    assert ar(P, 0, P, 1, 8, None) == bad
    assert ar(P, P, 0, 1, 8, None) == bad
    assert ar(P, P, P, 1, 0, None) == bad
    assert ar(P, P, P, 1, 4097, None) == bad
    assert ar(P, P, P, -1, 8, None) == bad
    assert ar(P, P, P, 0, 8, None) == 0
