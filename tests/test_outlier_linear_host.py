"""qgemm_linear_outlier (the LLM.int8() decomposition on a cached weight) without a GPU: the symbols, the workspace
size, the argument checks that return before any launch, and the Python wrapper's asserts."""
import ctypes

import pytest


def test_symbols_are_exported_and_declared(qg):
    L = qg.load()
    for name in ("qgemm_linear_outlier_workspace_size", "qgemm_linear_outlier"):
        assert name in qg.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name}: argtypes declared in load()"
    assert L.qgemm_linear_outlier_workspace_size.restype is ctypes.c_size_t
    assert L.qgemm_linear_outlier.restype is ctypes.c_int
    assert len(L.qgemm_linear_outlier.argtypes) == 14
    text = open(qg.HEADER_PATH).read()
    assert "qgemm_linear_outlier_workspace_size(int m, int n, int k);" in text
    assert "int qgemm_linear_outlier(const float *X, int64_t x_stride_h, int m, int k, const void *packed_w, int n," in text


@pytest.mark.parametrize("m,n,k", [(-1, 4, 4), (4, -1, 4), (4, 4, 0), (4, 4, -3)])
def test_workspace_size_is_zero_for_invalid_dims(qg, m, n, k):
    assert qg.load().qgemm_linear_outlier_workspace_size(m, n, k) == 0


# fast-path shapes, 64- / 32-tile plans, a split-K plan, K past one pass of the index kernel, K % 4 != 0, empty M / N
@pytest.mark.parametrize("m,n,k", [(4096, 4096, 4096), (2560, 4096, 128), (300, 200, 512), (64, 96, 130),
                                   (72, 40, 33000), (2048, 4096, 16384), (512, 1024, 4096), (1, 1, 1), (0, 8, 8),
                                   (8, 0, 8)])
def test_workspace_holds_the_linear_workspace_and_the_index(qg, m, n, k):
    L = qg.load()
    need = L.qgemm_linear_outlier_workspace_size(m, n, k)
    # the prepacked chain's workspace, and ahead of it at least the count + column list (k + 1 ints) and X' (m x k)
    assert need >= L.qgemm_linear_workspace_size(m, n, k) + 4 * (k + 1) + 4 * m * k
    # no W' slot: smaller than qgemm_mm_outlier's, which also holds W' (k x n_pad fp32) and a packed B
    assert need <= L.qgemm_mm_outlier_workspace_size(m, n, k)
    if n > 0:
        assert need < L.qgemm_mm_outlier_workspace_size(m, n, k)


def _call(L, X=8, xsh=4, m=4, k=4, pw=8, n=4, bias=None, relu=0, t=6.0, Y=8, ysh=4, ws=8, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = L.qgemm_linear_outlier_workspace_size(m, n, k)
    return L.qgemm_linear_outlier(X, xsh, m, k, pw, n, bias, relu, t, Y, ysh, ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [
    dict(X=None), dict(pw=None), dict(Y=None), dict(ws=None),
    dict(m=-1), dict(n=-1), dict(k=0),
    dict(t=-1.0), dict(t=float("nan")),
    dict(relu=1),                          # relu without a bias
    dict(ws_bytes=16),                     # short workspace
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_arguments_return_before_any_launch(qg, kw):
    """The pointers are never dereferenced (they are not device pointers): every case returns hipErrorInvalidValue
    from the argument checks, with no GPU in the machine."""
    assert _call(qg.load(), **kw) == qg.HIP_ERROR_INVALID_VALUE


def test_empty_problem_returns_success(qg):
    L = qg.load()
    assert _call(L, m=0, ws=None, ws_bytes=0) == 0
    assert _call(L, n=0, ws=None, ws_bytes=0) == 0
    assert _call(L, m=0, t=-1.0) == qg.HIP_ERROR_INVALID_VALUE  # the checks come before the early return


def test_wrapper_refuses_a_weight_packed_with_another_range(qg):
    import torch
    buf = torch.empty(qg.load().qgemm_packed_size(8, 8), dtype=torch.uint8)
    pw = qg.Packed(buf, 8, 8, 100.0)
    X = torch.zeros((4, 8), dtype=torch.float32)
    # the range is checked first, so the assert fires without a GPU
    with pytest.raises(AssertionError, match="range 127"):
        qg.linear_outlier(X, pw, 6.0)
