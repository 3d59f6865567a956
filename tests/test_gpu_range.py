"""`range` other than 127 through every fp32 entry point that takes it, against the CPU oracle, bit for bit.

`range` reaches every pack body as inv_divide(range, c) and every GEMM epilogue as inv_r2 = fl(1 / fl(range * range));
the rest of the GPU suite passes 127.0 only.  Here the oracle (which takes range_) gives every expected value: O and Acc
bit-identical, Xq / Wq byte-identical, scales value-identical.  With range > 127 the int8 cast saturates on both sides
for a large share of the elements (asserted on the oracle's own Xq first, so that no case passes vacuously), and the
int8 MFMA meets operands full of -128.  Outputs are pre-filled with NaN.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_bf16 import BF16, _assert_plan, _bits, _want_bits, assert_bf16_equal
from util import assert_bits_equal, assert_values_equal

pytestmark = pytest.mark.gpu

RANGES = [1.0, 15.5, 63.0, 128.0, 200.0, 1000.0]  # 127.0 is covered everywhere else


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _plant(X, W):
    """The signed-seed quirk as the parity tests plant it: first elements that are negative and the largest magnitude
    of their row / column (the absmax then comes from the OTHER elements, and the seed itself saturates)."""
    if X is not None:
        X[::4, 0] = -2.5
    if W is not None:
        W[0, ::3] = -1.75
    return X, W


def _check_saturation(q, seeds, r, what):
    """The CPU preconditions on the oracle's own quantized operand q (seeds: mask of the absmax seeds, the first
    element of every row of X / column of W)."""
    if r >= 200.0:
        hi, lo = float((q == 127).mean()), float((q == -128).mean())
        assert hi >= 0.10 and lo >= 0.10, f"{what}: {hi:.3f} of the elements at 127, {lo:.3f} at -128"
    if r == 128.0:
        assert ((q == 127) | (q == -128)).any(), f"{what}: nothing saturates"
    if r == 1.0:
        # a negative seed may lie outside its row's absmax (the planted ones do, 2.5 or 1.75 times) and then goes past
        # -1; every other element is at most the absmax in magnitude
        vals = set(np.unique(q[~seeds]).tolist())
        assert vals == {-1, 0, 1}, f"{what}: values {sorted(vals)}"


# ---------------------------------------------------------------------------------- 1. pack intermediates
# one K in each class of the fp32 row dispatch (pack.hip rows_regs): 5 generic (row stride no multiple of 4), 260 two
# chunks per lane, 2052 sixteen, 4100 block per row, 16388 streaming
PACK_K = [5, 260, 2052, 4100, 16388]
# seeds (of the X / W generators) fixed on the CPU so that the preconditions hold at the smallest cases as well: with
# 9 x 5 elements the shares at 127 / -128 scatter widely around the 18 % a large matrix gives
PACK_SEED = 7000


def _check_pack_a(qg, oracle, device, X, r, what):
    M, K = X.shape
    _, ref = oracle.quantized_mm(X, np.ones((K, 1), np.float32), r, intermediates=True)
    seeds = np.zeros(X.shape, bool)
    seeds[:, 0] = True
    _check_saturation(ref["Xq"], seeds, r, what)
    pa = qg.pack_a(_dev(X, device), r)
    torch.cuda.synchronize()
    assert_values_equal(pa.scale[:M].cpu().numpy(), ref["Cx"], f"{what} Cx")
    q = pa.q.cpu().numpy()
    assert (q[:M, :K] == ref["Xq"]).all(), f"{what} Xq: {int((q[:M, :K] != ref['Xq']).sum())} bytes differ"
    assert not q[M:].any() and not q[:, K:].any(), f"{what}: padding not zero"
    assert not pa.scale[M:].cpu().numpy().any(), f"{what}: padding scales not zero"


def _check_pack_b(qg, oracle, device, W, r, what):
    K, N = W.shape
    _, ref = oracle.quantized_mm(np.ones((1, K), np.float32), W, r, intermediates=True)
    seeds = np.zeros(W.shape, bool)
    seeds[0, :] = True
    _check_saturation(ref["Wq"], seeds, r, what)
    pb = qg.pack_b(_dev(W, device), r)
    torch.cuda.synchronize()
    assert_values_equal(pb.scale[:N].cpu().numpy(), ref["Cw"], f"{what} Cw")
    q = pb.q.cpu().numpy()
    assert (q[:N, :K] == ref["Wq"].T).all(), f"{what} Wq: {int((q[:N, :K] != ref['Wq'].T).sum())} bytes differ"
    assert not q[N:].any() and not q[:, K:].any(), f"{what}: padding not zero"
    assert not pb.scale[N:].cpu().numpy().any(), f"{what}: padding scales not zero"


@pytest.mark.parametrize("r", RANGES)
@pytest.mark.parametrize("K", PACK_K)
def test_pack_a_range(qg, oracle, device, K, r):
    for M in (9, 300):
        X, _ = _plant(oracle.uniform((M, K), PACK_SEED + K + M), None)
        _check_pack_a(qg, oracle, device, X, r, f"pack_a {M}x{K} range {r}")


@pytest.mark.parametrize("r", RANGES)
def test_pack_a_range_staged_rows(qg, oracle, device, r):
    """2048 padded rows: the 8-rows-per-block form that stages the packed rows in LDS."""
    M, K = 2048, 512
    X, _ = _plant(oracle.uniform((M, K), PACK_SEED + 1), None)
    _check_pack_a(qg, oracle, device, X, r, f"pack_a staged {M}x{K} range {r}")


@pytest.mark.parametrize("r", RANGES)
@pytest.mark.parametrize("K", PACK_K)
def test_pack_b_range(qg, oracle, device, K, r):
    """Row-major W: the column-maxima pass and the transposing quantize pass, vector (N = 72) and scalar (N = 70)."""
    for N in (72, 70):
        _, W = _plant(None, oracle.uniform((K, N), PACK_SEED + 3 * K + N))
        _check_pack_b(qg, oracle, device, W, r, f"pack_b {K}x{N} range {r}")


# ---------------------------------------------------------------------------------- 2. the drop-in
def fused_pack_path(m, n, k, xsh=None, wsh=None):
    """The pack launches op_mm_quantize_ws chooses for row-major X (row stride xsh) and W (row stride wsh) from 16-B
    aligned bases -- a restatement of launch_pack_single_pass_kind / launch_pack_two_pass / rows_regs (pack.hip), so
    that each test states the path its shape is there for."""
    xsh, wsh = k if xsh is None else xsh, n if wsh is None else wsh
    if k < 2 or (xsh % 4 and m > 1) or n % 4 or wsh % 4:
        return "separate"
    if k > 16384:
        rows = "streaming"
    elif k > 4096:
        rows = "block"
    else:
        rows = str(next(c for c in (1, 2, 4, 8, 16) if (k // 4 + 63) // 64 <= c))
    if k <= 4096:
        can8 = n % 8 == 0 and (k * wsh + 8) * 4 < 1 << 31
        can16 = n % 16 == 0
        can32 = n % 32 == 0 and (k * wsh + 32) * 4 < 1 << 31
        kind = 32 if can32 and n >= 16384 and k > 2048 else 8 if (can8 and n <= 8192 and k > 1024) or not can16 else 16
        if kind != 8 or can8:
            return f"single{kind}"
    return "colmax+cols_then_rows" if rows == "block" else f"rows{rows}+colmax,cols"


# (M, N, K) -> the fused pack path the shape is there for
FUSED_SHAPES = [
    ((100, 208, 300), "single16"),
    ((70, 200, 600), "single8"),
    ((33, 24, 4096), "single8"),
    ((5, 16384, 2052), "single32"),
    ((70, 100, 600), "rows4+colmax,cols"),          # n % 8 == 4: the single pass declines
    ((64, 96, 4100), "colmax+cols_then_rows"),      # K > 4096
    ((9, 24, 16388), "rowsstreaming+colmax,cols"),  # K > 16384
    ((70, 201, 600), "separate"),                   # n % 4 != 0
]


@functools.lru_cache(maxsize=None)
def _drop_in_inputs(M, N, K):
    from oracle import oracle as O
    return _plant(*O.inputs(M, N, K, 211))


@pytest.mark.parametrize("r", [1.0, 63.0, 200.0])
@pytest.mark.parametrize("shape,path", FUSED_SHAPES, ids=[p[1] + "-" + "x".join(map(str, p[0])) for p in FUSED_SHAPES])
def test_drop_in_range(qg, oracle, device, shape, path, r):
    """op_quantized_mm(X, W, O, r) and op_mm_quantize_ws on a workspace full of 0xFF: every output bit."""
    M, N, K = shape
    assert fused_pack_path(M, N, K) == path
    X, W = _drop_in_inputs(M, N, K)
    want = oracle.quantized_mm(X, W, r)
    Xd, Wd = _dev(X, device), _dev(W, device)
    O = torch.full((M, N), float("nan"), device=device)
    qg.op_quantized_mm(Xd, Wd, O, r)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"{M}x{N}x{K} range {r}")
    L = qg.load()
    ws = torch.full((L.op_mm_quantize_workspace_size(M, N, K),), 255, dtype=torch.uint8, device=device)
    O = torch.full((M, N), float("nan"), device=device)
    assert L.op_mm_quantize_ws(Xd.data_ptr(), K, 1, Wd.data_ptr(), N, 1, O.data_ptr(), N, 1, M, N, K, r, ws.data_ptr(),
                               ws.numel(), qg._stream(device)) == 0
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"{M}x{N}x{K} range {r}, caller workspace")


# ---------------------------------------------------------------------------------- 3. every GEMM plan
# (m, n, k), the plan qgemm_gemm_plan must report (tile, splits) and the 64-tile ring depth (test_gpu_bf16._assert_plan).
# The unsplit 256-tile shape has K = 192 (4 k-blocks) and so reaches gemm_i8_fm's plain form; the row-finish form that
# the same plan takes from 8 k-blocks on has these axes in test_gpu_row_finish_matrix.py
PLAN_SHAPES = [
    ((250, 1000, 200), 32, 1, None),
    ((130, 70, 640), 64, 1, 3),
    ((2000, 1990, 130), 64, 1, 2),
    ((70, 100, 4100), 64, 2, 3),
    ((4000, 2500, 192), 256, 1, None),
    ((2048, 4096, 2048), 256, 2, None),
]
PLAN_IDS = ["x".join(map(str, s[0])) for s in PLAN_SHAPES]


@functools.lru_cache(maxsize=4)
def _plan_case(m, n, k, r):
    """Inputs of one plan shape and the oracle's chain on them at range r, shared by the tests and never changed."""
    from oracle import oracle as O
    X, W = _plant(*O.inputs(m, n, k, 223))
    out, ref = O.quantized_mm(X, W, r, intermediates=True)
    return X, W, out, ref


_PACKED = {}


def _packed(qg, device, m, n, k, r):
    """The shape's operands packed with r, once; only the latest shape is kept."""
    key = (m, n, k, r)
    if key not in _PACKED:
        _PACKED.clear()
        X, W, _, _ = _plan_case(m, n, k, r)
        _PACKED[key] = (qg.pack_a(_dev(X, device), r), qg.pack_b(_dev(W, device), r))
    return _PACKED[key]


@pytest.mark.parametrize("r", [63.0, 200.0])
@pytest.mark.parametrize("shape,tile,splits,depth", PLAN_SHAPES, ids=PLAN_IDS)
def test_mm_packed_range_every_plan(qg, oracle, device, shape, tile, splits, depth, r):
    """mm_packed on operands packed with r: O and the raw accumulators.  At 200 the operands are full of +-127 / -128."""
    _assert_plan(qg, shape, tile, splits, depth)
    m, n, k = shape
    _, _, want, ref = _plan_case(m, n, k, r)
    if r == 200.0:
        _check_saturation(ref["Xq"], None, r, f"{shape} Xq")
        _check_saturation(ref["Wq"], None, r, f"{shape} Wq")
    pa, pb = _packed(qg, device, m, n, k, r)
    assert pa.range == r and pb.range == r
    O = torch.full((m, n), float("nan"), device=device)
    qg.mm_packed(pa, pb, O)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"{shape} range {r} mm_packed")
    acc = qg.mm_packed_i32(pa, pb).cpu().numpy()
    assert (acc == ref["Acc"]).all(), f"{shape} range {r} Acc: {int((acc != ref['Acc']).sum())} differ"


@pytest.mark.parametrize("shape,tile,splits,depth", [PLAN_SHAPES[1], PLAN_SHAPES[4]], ids=[PLAN_IDS[1], PLAN_IDS[4]])
def test_mm_packed_range_bf16_output(qg, oracle, device, shape, tile, splits, depth):
    """The same GEMM with a bf16 output at range 200: the oracle's fp32 output rounded once on the CPU."""
    _assert_plan(qg, shape, tile, splits, depth)
    m, n, k = shape
    r = 200.0
    _, _, want, _ = _plan_case(m, n, k, r)
    pa, pb = _packed(qg, device, m, n, k, r)
    C = torch.full((m, n), float("nan"), dtype=BF16, device=device)
    out = qg.mm_packed(pa, pb, C, out_dtype=BF16)
    torch.cuda.synchronize()
    assert out.dtype == BF16
    assert_bf16_equal(_bits(C), _want_bits(want), f"{shape} range {r} mm_packed bf16")


# ---------------------------------------------------------------------------------- 4. two extremes
@pytest.mark.parametrize("shape,tile,splits,depth", [PLAN_SHAPES[1], PLAN_SHAPES[4]], ids=[PLAN_IDS[1], PLAN_IDS[4]])
def test_range_so_large_that_its_square_overflows(qg, oracle, device, shape, tile, splits, depth):
    """range = 1e20: fl(range * range) is inf, inv_r2 = +0, and every finite product becomes a zero with its sign."""
    _assert_plan(qg, shape, tile, splits, depth)
    m, n, k = shape
    r = 1e20
    X, W = _drop_in_inputs(m, n, k)
    want = oracle.quantized_mm(X, W, r)
    zero = want == 0
    assert (zero & np.signbit(want)).any() and (zero & ~np.signbit(want)).any(), "expected +0 and -0 outputs"
    O = torch.full((m, n), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, r)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"{shape} range 1e20")


@pytest.mark.parametrize("shape,tile,splits,depth", [PLAN_SHAPES[1], PLAN_SHAPES[4]], ids=[PLAN_IDS[1], PLAN_IDS[4]])
def test_range_so_small_that_only_seeds_survive(qg, oracle, device, shape, tile, splits, depth):
    """range = 2^-20: an element within its row's absmax gives |x * fl(range / absmax)| <= 2^-20 (1 + 2^-23) < 1, so it
    quantizes to 0; only a signed seed far outside the absmax (planted here at 3e6 times it) keeps a nonzero byte."""
    _assert_plan(qg, shape, tile, splits, depth)
    m, n, k = shape
    r = 2.0 ** -20
    X, W = (a.copy() for a in _drop_in_inputs(m, n, k))
    X[::4, 0] = -3.0e6
    W[0, ::3] = -3.0e6
    want, ref = oracle.quantized_mm(X, W, r, intermediates=True)
    assert not ref["Xq"][:, 1:].any() and not ref["Wq"][1:].any(), "only the seeds may quantize to nonzero"
    assert ref["Xq"][::4, 0].all() and ref["Wq"][0, ::3].all() and (want != 0).any()
    O = torch.full((m, n), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, r)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"{shape} range 2^-20")
