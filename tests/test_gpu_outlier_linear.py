"""GPU parity of qgemm_linear_outlier: the LLM.int8() decomposition on a CACHED weight (include/qgemm.h, DESIGN.md
"Outlier decomposition on a cached weight").  Every output bit and the outlier count, on the fast path (column mask,
masked X-only pack, the 256-tile GEMM with the chain on the weight's dequantized rows in its epilogue) and on the
fallback (index, X' materialised, the plain chain, the correction kernel).

The expected value is composed from what the oracle already exports (`_compose`): the plain chain on X' and the full
W, the outlier rows of W dequantized from the chain's own Wq / Cw in float32 numpy operations (one rounding each), and
the oracle's sequential-k fmaf chain over the outlier columns.
"""
import ctypes

import numpy as np
import pytest
import torch

from util import assert_bits_equal, bits

pytestmark = pytest.mark.gpu

F32 = np.float32


def _dev(a, device):
    return torch.from_numpy(np.array(a, dtype=a.dtype, order="C", copy=True)).to(device)


def _with_outliers(oracle, M, N, K, cols, seed):
    X, W = oracle.inputs(M, N, K, seed)
    rng = np.random.default_rng(seed)
    for c in cols:
        rows = rng.choice(M, size=max(1, M // 50), replace=False)
        X[rows, c] = rng.choice([-1.0, 1.0], size=rows.size).astype(np.float32) * rng.uniform(7, 60, rows.size)
    return X.astype(np.float32), W


def _chain(oracle, Xo, Wd):
    """Co: the fmaf chain from +0 over the columns of Xo in ascending order, by oracle.mm_fp32.  That function is the
    reference's tiled op_mm: past K it runs fmaf(+0, +0, acc) up to the next multiple of its 32-wide tile, which turns a
    sum of -0 into +0.  The chain defined in include/qgemm.h has no such steps, so the operands are padded here to a
    multiple of 32 columns with -0 * +0 -- fmaf(-0, +0, acc) = acc for every acc, -0 included (the kernels' own padding
    rule) -- and mm_fp32 adds no step of its own.  Every other bit is mm_fp32's."""
    n = Xo.shape[1]
    pad = -n % 32
    Xo = np.concatenate([Xo, np.full((Xo.shape[0], pad), -0.0, F32)], axis=1)
    Wd = np.concatenate([Wd, np.zeros((pad, Wd.shape[1]), F32)], axis=0)
    return oracle.mm_fp32(np.ascontiguousarray(Xo), np.ascontiguousarray(Wd))


def _compose(oracle, X, W, t=6.0, bias=None, relu=False):
    """(Y, count) of linear_outlier(X, pack_b(W), t, bias, relu) as include/qgemm.h defines it."""
    cols = np.flatnonzero((~(np.abs(X) <= F32(t))).any(axis=0))
    Xp = X.copy()
    Xp[:, cols] = 0
    O8, im = oracle.quantized_mm(Xp, W, 127.0, intermediates=True)
    O = O8
    if len(cols):
        Wd = (im["Wq"][cols].astype(F32) * im["Cw"][None, :]) * (F32(1) / F32(127))
        assert Wd.dtype == F32
        O = O8 + _chain(oracle, X[:, cols], Wd)
    if bias is not None:
        O = O + bias[None, :].astype(F32)
    if relu:
        O = np.where(O < 0, F32(0), O)
    assert O.dtype == F32
    return O, len(cols)


def _plan(qg, M, N, K):
    t = ctypes.c_int(0)
    splits = qg.load().qgemm_gemm_plan(M, N, K, ctypes.byref(t), None)
    return t.value, splits


def _on_fast_plan(qg, M, N, K):
    return _plan(qg, M, N, K) == (256, 1) and K % 4 == 0 and K <= 4096


# one data set and one composed value per shape, shared by the tests below (never modified)
_CASES = {}


def _case(oracle, M, N, K, cols, seed=9):
    key = (M, N, K, tuple(cols), seed)
    if key not in _CASES:
        X, W = _with_outliers(oracle, M, N, K, cols, seed)
        want, cnt = _compose(oracle, X, W)
        assert cnt == len(cols)
        for a in (X, W, want):
            a.setflags(write=False)
        _CASES[key] = (X, W, want)
    return _CASES[key]


FAST = [(2560, 4096, 128, [0, 31, 32, 127]),               # the seed column, mask-word edges, the last column
        (2500, 4000, 132, [0, 1, 31, 32, 63, 131]),        # ragged in M, N and K
        (2560, 4096, 1024, list(range(7, 1024, 37))),      # 28 columns: the loop past 8, a count not divisible by 4
        (512, 16384, 256, [3, 100, 255])]                  # >= 64-KiB output rows: the LDS-image stores
FALLBACK = [(300, 200, 512, [3, 77, 400]),                 # small tiles
            (64, 96, 130, [0, 129]),                       # K % 4 != 0
            (72, 40, 33000, [0, 31, 32767, 32768, 32999])]  # K > 4096: 1032 mask words, two passes of the index kernel
SPLIT = (128, 512, 4096, [5, 2048, 4095])                  # 64-tiles, split-K


@pytest.mark.parametrize("M,N,K,cols", FAST)
def test_fast_path_bit_exact(qg, oracle, device, M, N, K, cols):
    assert _on_fast_plan(qg, M, N, K), _plan(qg, M, N, K)
    X, W, want = _case(oracle, M, N, K, cols)
    Y, cnt = qg.linear_outlier(_dev(X, device), qg.pack_b(_dev(W, device)), 6.0)
    assert cnt == len(cols)
    assert_bits_equal(Y.cpu().numpy(), want, f"linear_outlier fast path {M}x{N}x{K}")


@pytest.mark.parametrize("relu", [False, True])
def test_fast_path_bias_and_relu(qg, oracle, device, relu):
    M, N, K, cols = FAST[1]
    X, W, _ = _case(oracle, M, N, K, cols)
    b = oracle.uniform((N,), 77, -0.5, 0.5)
    want, wcnt = _compose(oracle, X, W, 6.0, b, relu)
    Y, cnt = qg.linear_outlier(_dev(X, device), qg.pack_b(_dev(W, device)), 6.0, bias=_dev(b, device), relu=relu)
    assert cnt == wcnt == len(cols)
    if relu:
        assert (want == 0).any() and (want > 0).any()
    assert_bits_equal(Y.cpu().numpy(), want, f"linear_outlier fast path, bias, relu={relu}")


def _strided_check(qg, oracle, device, M, N, K, cols, xpad, ypad):
    X, W, want = _case(oracle, M, N, K, cols)
    Xbig = torch.full((M, K + xpad), 1000.0, device=device)  # an outlier in every gap column, were one read
    Xbig[:, :K] = _dev(X, device)
    sentinel = np.float32(-123.25)
    Ybig = torch.full((M, N + ypad), float(sentinel), device=device)
    Y, cnt = qg.linear_outlier(Xbig[:, :K], qg.pack_b(_dev(W, device)), 6.0, Y=Ybig[:, :N])
    assert cnt == len(cols)
    got = Ybig.cpu().numpy()
    assert_bits_equal(got[:, :N], want, f"linear_outlier strided views {M}x{N}x{K}")
    assert (bits(got[:, N:]) == bits(np.full((M, ypad), sentinel))).all(), "bytes between the rows of Y were written"


def test_fast_path_strided_views(qg, oracle, device):
    M, N, K, cols = FAST[0]
    assert _on_fast_plan(qg, M, N, K)
    _strided_check(qg, oracle, device, M, N, K, cols, xpad=8, ypad=4)  # 16-B aligned rows: still the fast path


@pytest.mark.parametrize("M,N,K,cols", FALLBACK)
def test_fallback_bit_exact(qg, oracle, device, M, N, K, cols):
    assert not _on_fast_plan(qg, M, N, K), _plan(qg, M, N, K)
    X, W, want = _case(oracle, M, N, K, cols)
    Y, cnt = qg.linear_outlier(_dev(X, device), qg.pack_b(_dev(W, device)), 6.0)
    assert cnt == len(cols)
    assert_bits_equal(Y.cpu().numpy(), want, f"linear_outlier fallback {M}x{N}x{K}")


def test_fallback_small_tiles_claim(qg):
    assert _plan(qg, 300, 200, 512)[0] in (32, 64)
    assert _plan(qg, 64, 96, 130)[0] in (32, 64)
    assert _plan(qg, 72, 40, 33000)[0] in (32, 64)


def test_fallback_split_k_bias_relu(qg, oracle, device):
    M, N, K, cols = SPLIT
    tile, splits = _plan(qg, M, N, K)
    assert splits > 1 and tile == 64, (tile, splits)
    X, W, _ = _case(oracle, M, N, K, cols)
    b = oracle.uniform((N,), 78, -0.5, 0.5)
    want, wcnt = _compose(oracle, X, W, 6.0, b, True)
    Y, cnt = qg.linear_outlier(_dev(X, device), qg.pack_b(_dev(W, device)), 6.0, bias=_dev(b, device), relu=True)
    assert cnt == wcnt == len(cols)
    assert (want == 0).any() and (want > 0).any()
    assert_bits_equal(Y.cpu().numpy(), want, "linear_outlier fallback, split-K, bias + relu")


def test_fallback_strided_views(qg, oracle, device):
    M, N, K, cols = FALLBACK[0]
    _strided_check(qg, oracle, device, M, N, K, cols, xpad=3, ypad=5)  # rows off 16 B


def test_fallback_misaligned_base(qg, oracle, device):
    """An X view whose base is 4 B off a 16-B boundary, on a shape whose plan is the fast path's: the vector loads of
    the mask and the pack are not possible, so the call takes the fallback -- same bits."""
    M, N, K, cols = FAST[0]
    assert _plan(qg, M, N, K) == (256, 1)
    X, W, want = _case(oracle, M, N, K, cols)
    buf = torch.empty(M * K + 1, device=device)
    Xv = buf[1:].view(M, K)
    Xv.copy_(_dev(X, device))
    assert Xv.data_ptr() % 16 == 4
    Y, cnt = qg.linear_outlier(Xv, qg.pack_b(_dev(W, device)), 6.0)
    assert cnt == len(cols)
    assert_bits_equal(Y.cpu().numpy(), want, "linear_outlier, misaligned X base")


@pytest.mark.parametrize("M,N,K", [(65600, 24, 36), (65600, 24, 38)])  # fast path; K % 4 != 0: the fallback
def test_more_than_65535_rows_bias_relu(qg, oracle, device, M, N, K):
    """More rows than a grid's y extent, with bias + relu: the fallback's correction kernel strides the rows over
    65 535 blocks.  Outliers in the first and the last row and a NaN between them, everything else below 1."""
    assert _on_fast_plan(qg, M, N, K) == (K % 4 == 0), _plan(qg, M, N, K)
    X, W = oracle.inputs(M, N, K, 16)
    X[0, 0], X[M - 1, K - 1], X[40000, 17] = 7.5, -11.0, np.nan
    b = oracle.uniform((N,), 80, -0.5, 0.5)
    want, wcnt = _compose(oracle, X, W, 6.0, b, True)
    assert wcnt == 3
    Y, cnt = qg.linear_outlier(_dev(X, device), qg.pack_b(_dev(W, device)), 6.0, bias=_dev(b, device), relu=True)
    assert cnt == 3
    assert np.isnan(want[40000]).all() and (want == 0).any() and (want > 0).any()
    assert_bits_equal(Y.cpu().numpy(), want, f"linear_outlier {M}x{N}x{K}, bias + relu")


@pytest.mark.parametrize("M,N,K", [(2560, 4096, 128), (300, 200, 516)])  # fast path; fallback
def test_no_outliers_is_qgemm_linear(qg, oracle, device, M, N, K):
    X, W = oracle.inputs(M, N, K, 10)
    b = oracle.uniform((N,), 79, -0.5, 0.5)
    Xd, pw, bd = _dev(X, device), qg.pack_b(_dev(W, device)), _dev(b, device)
    for bias, relu in ((None, False), (bd, False), (bd, True)):
        Y, cnt = qg.linear_outlier(Xd, pw, 6.0, bias=bias, relu=relu)
        assert cnt == 0
        plain = qg.linear(Xd, pw, bias=bias, relu=relu)
        assert_bits_equal(Y.cpu().numpy(), plain.cpu().numpy(), f"no outliers = qgemm_linear {M}x{N}x{K} relu={relu}")
    want, wcnt = _compose(oracle, X, W)
    assert wcnt == 0
    assert_bits_equal(qg.linear_outlier(Xd, pw, 6.0)[0].cpu().numpy(), want, "no outliers, the composition")


@pytest.mark.parametrize("ncols", [0, 1, 3])
def test_chain_keeps_negative_zero(qg, oracle, device, ncols):
    """The construction of test_gpu_outlier.py::test_outlier_chain_keeps_negative_zero for the cached weight: O8[5, 11]
    is -0 (acc < 0 times an outer product that underflows to +0) and the chain at [5, 11] underflows to -0, so
    O = fl(-0 + -0) = -0; a count that is not a multiple of 4 pads the MFMA step with -0 * +0, which leaves the -0 sum
    alone; with no outlier column O8 is stored with no add (fl(-0 + +0) would be +0).  W[c, 11] is 1e-25 here, not the
    1e-30 of that test: 1e-30 quantizes to 0 against Cw[11] = 1e-25, and a dequantized +0 would make the chain +0; at
    1e-25 the row dequantizes to ~1e-25 and -1e-30 * 1e-25 still underflows to -0."""
    M, N, K = 2560, 4096, 128
    assert _on_fast_plan(qg, M, N, K)
    X, W = oracle.inputs(M, N, K, 12)
    cols = [7, 40, 90][:ncols]
    X[5, :] = 0.0
    X[5, 1] = 1e-22
    W[:, 11] = 0.0
    W[1, 11] = -1e-25
    for c in cols:
        X[100, c] = 50.0
        X[5, c] = -1e-30
        W[c, 11] = 1e-25
    want, wcnt = _compose(oracle, X, W)
    assert wcnt == ncols
    assert want[5, 11] == 0.0 and np.signbit(want[5, 11]), "the composed value is -0"
    Y, cnt = qg.linear_outlier(_dev(X, device), qg.pack_b(_dev(W, device)), 6.0)
    assert cnt == ncols
    assert_bits_equal(Y.cpu().numpy(), want, f"linear_outlier chain -0, {ncols} columns")


@pytest.mark.parametrize("M,N,K", [(2560, 4096, 128), (40, 50, 60)])  # fast path; fallback
def test_nan_column_is_an_outlier(qg, oracle, device, M, N, K):
    X, W = oracle.inputs(M, N, K, 7)
    X[3, 11] = np.nan
    X[M - 1, K - 1] = -9.0
    want, wcnt = _compose(oracle, X, W)
    assert wcnt == 2
    Y, cnt = qg.linear_outlier(_dev(X, device), qg.pack_b(_dev(W, device)), 6.0)
    assert cnt == 2
    assert np.isnan(want[3]).all() and not np.isnan(want[4]).any()
    assert_bits_equal(Y.cpu().numpy(), want, f"linear_outlier NaN column {M}x{N}x{K}")


def _raw(L, Xd, pw, Y, ws, stream, M, N, K):
    return L.qgemm_linear_outlier(Xd.data_ptr(), Xd.stride(0), M, K, pw.buf.data_ptr(), N, None, 0, 6.0, Y.data_ptr(),
                                  Y.stride(0), ws.data_ptr(), ws.numel(), stream)


def _count(L, K, ws):
    cnt = ctypes.c_int(-1)
    assert L.qgemm_outlier_count(K, ws.data_ptr(), ctypes.byref(cnt)) == 0
    return cnt.value


GRAPH = (2560, 4096, 512)


def test_graph_capture_and_repeat(qg, oracle, device):
    """The call allocates nothing and does not synchronize: captured in a HIP graph as the FIRST call on its stream and
    replayed; then 20 eager calls on the same workspace give the same bits every time (race screen of the mask / count /
    column-list hand-offs between the three launches)."""
    M, N, K = GRAPH
    cols = [0, 5, 77, 300, 511]
    X, W, want = _case(oracle, M, N, K, cols, 12)
    L = qg.load()
    Xd, pw = _dev(X, device), qg.pack_b(_dev(W, device))
    ws = torch.empty(L.qgemm_linear_outlier_workspace_size(M, N, K), dtype=torch.uint8, device=device)
    Y = torch.full((M, N), float("nan"), device=device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert _raw(L, Xd, pw, Y, ws, s.cuda_stream, M, N, K) == 0
    for _ in range(3):
        Y.fill_(float("nan"))
        ws.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _count(L, K, ws) == len(cols)
        assert_bits_equal(Y.cpu().numpy(), want, "linear_outlier graph replay")
    wd = _dev(want, device).view(torch.int32)
    for i in range(20):
        assert _raw(L, Xd, pw, Y, ws, s.cuda_stream, M, N, K) == 0
        s.synchronize()
        assert torch.equal(Y.view(torch.int32), wd), f"linear_outlier repeat {i}"
    assert _count(L, K, ws) == len(cols)


@pytest.mark.parametrize("M,N,K", [GRAPH, (300, 200, 516)])  # fast path; fallback
def test_concurrent_streams(qg, oracle, device, M, N, K):
    """Two streams, each with its own workspace, weight and outlier columns, run calls at the same time: nothing is
    shared between calls."""
    L = qg.load()
    cases = []
    for i, cols in enumerate(([0, 5, 77], [3, 300, 511, 64])):
        X, W, want = _case(oracle, M, N, K, cols, 21 + i)
        cases.append((_dev(X, device), qg.pack_b(_dev(W, device)), want, len(cols),
                      torch.empty(L.qgemm_linear_outlier_workspace_size(M, N, K), dtype=torch.uint8, device=device),
                      torch.full((M, N), float("nan"), device=device), torch.cuda.Stream(device)))
    torch.cuda.synchronize()
    for _ in range(8):
        for Xd, pw, _, _, ws, Y, s in cases:
            assert _raw(L, Xd, pw, Y, ws, s.cuda_stream, M, N, K) == 0
    torch.cuda.synchronize()
    for i, (_, _, want, n, ws, Y, _) in enumerate(cases):
        assert _count(L, K, ws) == n
        assert_bits_equal(Y.cpu().numpy(), want, f"linear_outlier stream {i}, {M}x{N}x{K}")


def test_decomposition_reduces_quantization_error(qg, oracle, device):
    """The point of LLM.int8(), with the weight cached: against the fp32 product, the mean |E| of the decomposition is
    below the plain prepacked linear's.  The composition measured 0.1193 against 0.2026 on the CPU, and the device
    value is bit-equal to it."""
    X, W = _with_outliers(oracle, 256, 256, 1024, [10, 500, 900], 8)
    ref = oracle.mm_fp32(X, W)
    Xd, pw = _dev(X, device), qg.pack_b(_dev(W, device))
    plain = qg.linear(Xd, pw).cpu().numpy()
    Y, cnt = qg.linear_outlier(Xd, pw, 6.0)
    assert cnt == 3
    e_plain = np.abs(ref - plain).mean()
    e_dec = np.abs(ref - Y.cpu().numpy()).mean()
    print(f"mean |E|: plain {e_plain:.4f}, linear_outlier {e_dec:.4f}")
    assert e_dec < 0.75 * e_plain, (e_dec, e_plain)
