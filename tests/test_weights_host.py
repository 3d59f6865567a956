"""Caller-supplied weights without a GPU: the weight-array oracles against the seeded ones, the window
contract restated on the oracle's quantization, and every argument refusal that needs no handle."""
import ctypes

import numpy as np
import pytest

import attn_oracle
import causal_oracle
import weights_oracle as WO_

D, H, DFF, BLOCKS, SEQ, ENC_SEQ, SEED = 40, 5, 72, 2, 9, 7, 31


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_encoder_forward_w_is_the_seeded_oracle(oracle):
    X = oracle.uniform((SEQ, D), 1)
    W = WO_.seeded_weights(D, H, DFF, BLOCKS, SEED)
    got = WO_.encoder_forward_w(X, W, D, H, BLOCKS)
    want = attn_oracle.encoder_forward_ref(X, D, H, DFF, BLOCKS, SEED)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("causal", [False, True])
def test_decoder_forward_w_is_the_seeded_oracle(oracle, causal):
    X, enc = oracle.uniform((SEQ, D), 2), oracle.uniform((ENC_SEQ, D), 3)
    W = WO_.seeded_weights(D, H, DFF, BLOCKS, SEED, cross=True)
    got = WO_.decoder_forward_w(X, enc, W, D, H, BLOCKS, causal=causal)
    ref = causal_oracle.decoder_forward_causal_ref if causal else attn_oracle.decoder_forward_ref
    want = ref(X, enc, D, H, DFF, BLOCKS, SEED)
    assert np.array_equal(_bits(got), _bits(want))


def test_heavy_tailed_weights_spread_the_column_scales(oracle):
    """What the GPU tests load: finite outputs, and column scales of one packed weight a factor > 20 apart."""
    W = WO_.heavy_tailed_weights(D, H, DFF, BLOCKS, 5, cross=True)
    cw = oracle.absmax_cols(WO_.fused(W, 0, (attn_oracle.WQ, attn_oracle.WK, attn_oracle.WV)))
    assert cw.max() / cw.min() > 20
    X, enc = oracle.uniform((SEQ, D), 2), oracle.uniform((ENC_SEQ, D), 3)
    assert np.isfinite(WO_.decoder_forward_w(X, enc, W, D, H, BLOCKS, causal=True)).all()
    assert np.isfinite(WO_.encoder_forward_w(X, W, D, H, BLOCKS)).all()


WINDOWS = ((0, 5), (5, 11), (16, 16), (32, 8))


@pytest.mark.parametrize("range_", [127.0, 100.0])
def test_window_contract_on_the_oracle(oracle, range_):
    """Columns of the oracle's B quantization are independent: Cw[j] and column j of Wq are the same whether the
    column stands in the assembled matrix, in any other matrix, or in its window packed alone -- with a zero column,
    a NaN, an +-inf and a negative seed inside windows."""
    k, n = 65, 40
    W = oracle.uniform((k, n), 7, -3.0, 3.0)
    W[:, 3] = 0.0
    W[9, 7] = np.nan
    W[20, 18] = np.inf
    W[21, 33] = -np.inf
    W[0, 6] = -2.9
    X = oracle.uniform((2, k), 8)
    _, full = oracle.quantized_mm(X, W, range_, intermediates=True)
    other = oracle.uniform((k, n), 9, -0.5, 0.5)
    for c0, nc in WINDOWS:
        sl = slice(c0, c0 + nc)
        M = other.copy()
        M[:, sl] = W[:, sl]
        _, emb = oracle.quantized_mm(X, M, range_, intermediates=True)
        _, alone = oracle.quantized_mm(X, np.ascontiguousarray(W[:, sl]), range_, intermediates=True)
        for got in (emb["Cw"][sl], alone["Cw"]):
            assert np.array_equal(_bits(got), _bits(full["Cw"][sl]))
        assert np.array_equal(emb["Wq"][:, sl], full["Wq"][:, sl]) and np.array_equal(alone["Wq"], full["Wq"][:, sl])
    assert sum(nc for _, nc in WINDOWS) == n


def test_pack_b_window_refusals(qg):
    """Everything outside the envelope is hipErrorInvalidValue before any launch (fake pointers: nothing runs)."""
    L = qg.load()
    f = L.qgemm_pack_b_window
    ok = dict(B=4096, dt=qg.QGEMM_F32, sh=40, sw=1, k=64, n=40, c0=5, nc=11, r=127.0, p=8192)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["B"], a["dt"], a["sh"], a["sw"], a["k"], a["n"], a["c0"], a["nc"], a["r"], a["p"], None)

    bad = [dict(B=None), dict(p=None), dict(dt=2), dict(dt=-1), dict(sh=-1), dict(sw=-1), dict(k=0), dict(k=16385),
           dict(c0=-1), dict(nc=0), dict(c0=30, nc=11), dict(c0=2**31 - 1, nc=2), dict(n=0)]
    for kw in bad:
        assert call(**kw) == qg.HIP_ERROR_INVALID_VALUE, kw
    # the plan query applies the same envelope and launches nothing
    name = ctypes.c_char_p()
    g = L.qgemm_pack_b_window_plan
    assert g(None, 0, 40, 1, 64, 40, 5, 11, ctypes.byref(name)) == qg.HIP_ERROR_INVALID_VALUE
    assert g(4096, 3, 40, 1, 64, 40, 5, 11, ctypes.byref(name)) == qg.HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("ptr,dt,sh,sw,nc,path", [
    (4096, 0, 1, 64, 11, "f32, k-contiguous"),
    (4096, 1, 1, 64, 11, "bf16, k-contiguous"),
    (4096, 0, 1, 65, 11, "f32, generic"),        # columns 260 B apart: not 16-byte aligned
    (4096, 1, 1, 68, 11, "bf16, generic"),       # 136 B apart
    (4096, 0, 1, 65, 1, "f32, k-contiguous"),    # one column: its stride does not count
    (4100, 0, 1, 64, 11, "f32, generic"),        # misaligned base
    (4100, 0, 40, 1, 11, "f32, n-contiguous"),   # n-contiguous needs no alignment
    (4098, 1, 40, 1, 11, "bf16, n-contiguous"),
    (4096, 0, 80, 2, 11, "f32, generic"),
])
def test_pack_b_window_plan_names_the_source_path(qg, ptr, dt, sh, sw, nc, path):
    name = ctypes.c_char_p()
    assert qg.load().qgemm_pack_b_window_plan(ptr, dt, sh, sw, 64, 40, 5, nc, ctypes.byref(name)) == 0
    assert name.value.decode() == f"pack_b_window<{path}>"


def test_model_calls_refuse_a_null_handle(qg):
    L = qg.load()
    i = ctypes.c_int()
    p = ctypes.c_void_p()
    assert L.qgemm_model_weight_shape(None, 0, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)) == 1
    assert L.qgemm_model_set_weight(None, 0, 0, 0, 4096, 0, 8, 1, None) == 1
    assert L.qgemm_model_packed_weight(None, 0, 0, ctypes.byref(p), ctypes.byref(i), ctypes.byref(i)) == 1
    assert L.qgemm_model_bias(None, 0, 5, ctypes.byref(p), ctypes.byref(i)) == 1
