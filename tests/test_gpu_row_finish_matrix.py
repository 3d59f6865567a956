"""Every instantiation, edge, tile map, output layout and range of gemm_i8_fm's row-finish form, bit for bit.

test_gpu_row_finish.py shows that the form is reached and exact at one shape per K-form.  This module runs what that
file leaves out (each instantiation is scheduled on its own and can be wrong on its own, for a
fraction of its outputs):

1. all twelve instantiations -- {loop-free, residue 0, 1, 2} x {none, bias, bias + relu} -- at full and at ragged tiles;
2. the guarded stores of a looped form at the thinnest edges (one row, one lane quad, a cut inside a lane's columns);
3. tile maps: one tile column, fewer tile rows than a group, a workgroup count that is no multiple of 8;
4. the plan matrix of test_gpu_layouts.py / test_gpu_range.py on a shape that takes the form: the output layouts on
   both sides of the launcher's decision (paired-store outputs run row-finish, every other layout the plain kernel of
   the same plan), ranges 63 and 200 and the two extreme ranges;
5. accumulators beyond 2^24, which the epilogue's int32 -> float conversion has to round;
6. the benchmark's K = 4096 under bias + relu with every tile row computing the same 256 rows;
7. repeated launches, launches next to a streaming copy on a second stream, and replays of a captured graph.

Every expected value is the CPU oracle's and every comparison is assert_bits_equal (or exact integer equality for the
raw accumulators); there is no tolerance.  Every case asserts its plan through qgemm_gemm_plan before it launches:
tile 256, one slice, and "row-finish" in the kernel's name exactly when K qualifies.  The plan names the kernel by K;
which outputs of such a shape leave the form is launch_fm's decision, restated here in _row_finish_output so that
each layout case states the kernel it is there for.

The unsplit 256-tile plan starts at 160 tiles, so the base shapes are 2560 x 4096 (10 x 16 full tiles) and
2600 x 4000 (11 x 16 tiles, the last row and the last column ragged).
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from test_gpu_layouts import OUT_LAYOUTS, _check_untouched, _strided_out
from test_gpu_range import _check_saturation, _plant
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

FULL, RAGGED = (2560, 4096), (2600, 4000)
POISON = np.float32(np.nan).view(np.int32).item()  # the bits torch.full(..., nan) stores

EPILOGUES = {"none": (False, False), "bias": (True, False), "bias_relu": (True, True)}


def _round_up(x, m):
    return (x + m - 1) // m * m


def _dev(a, device):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(device)  # torch takes no read-only array


# ---------------------------------------------------------------------------------- the launcher's arithmetic
def _k_form(k):
    """launch_fm's choice for this K (gemm_i8.hip): k_pad / 64 k-blocks, pre = k-blocks - 6 sub-steps that prefetch two
    ahead, rest = pre % 3, and a loop when pre holds a whole group of three.  None below the 7 k-blocks the form
    needs (k_pad is a multiple of 128, so 8 is the fewest); else (pre, rest, loop)."""
    blocks = _round_up(k, 128) // 64
    if blocks < 7:
        return None
    pre = blocks - 6
    return pre, pre % 3, pre > 2


def _instantiation(k):
    """The K-form as the launcher tells its four kernels apart: "loop-free", or the residue of a looped form."""
    pre, rest, loop = _k_form(k)
    return f"residue {rest}" if loop else "loop-free"


def _row_finish_output(k, sh, sw, offset):
    """Whether launch_fm sends an fp32 output with strides (sh, sw) at element `offset` of a 16-B aligned buffer to the
    row-finish kernel: the paired-store path (unit column stride, rows a multiple of 4 floats, 16-B aligned base) with
    rows below the 16384-float switch to the LDS-image stores, at a K that qualifies."""
    return _k_form(k) is not None and sw == 1 and sh % 4 == 0 and offset % 4 == 0 and sh < 16384


def _plan(qg, m, n, k):
    tile, name = ctypes.c_int(0), ctypes.c_char_p()
    splits = qg.load().qgemm_gemm_plan(m, n, k, ctypes.byref(tile), ctypes.byref(name))
    return tile.value, splits, name.value.decode()


def _assert_plan(qg, m, n, k):
    """Tile 256, one slice, "row-finish" in the name exactly when K qualifies -- and every K of this module does."""
    tile, splits, name = _plan(qg, m, n, k)
    assert (tile, splits) == (256, 1), (m, n, k, tile, splits)
    assert ("row-finish" in name) == (_k_form(k) is not None), (m, n, k, name)
    assert _k_form(k) is not None, f"K = {k} does not reach the row-finish form"


# ---------------------------------------------------------------------------------- shared inputs and expected outputs
@functools.lru_cache(maxsize=3)
def _inputs(m, n, k):
    """X, W and a bias of one shape, shared by its tests and never changed."""
    from oracle import oracle as O
    X, W = O.inputs(m, n, k, 7200 + k + m)
    X[::7, 0] = -1.5  # the absmax seed quirk and int8 saturation in some rows
    b = O.uniform((n,), 7300 + k, -0.5, 0.5)
    for a in (X, W, b):
        a.setflags(write=False)
    return X, W, b


@functools.lru_cache(maxsize=4)
def _expected(m, n, k, epi):
    """The oracle's output of _inputs(m, n, k) under one epilogue.  For bias + relu the CPU precondition that both relu
    branches are really taken: between 30 % and 70 % of the outputs are exactly zero (50 % measured)."""
    from oracle import oracle as O
    X, W, b = _inputs(m, n, k)
    bias, relu = EPILOGUES[epi]
    want = O.linear(X, W, b, relu) if bias else O.quantized_mm(X, W)
    if relu:
        zeros = float((want == 0).mean())
        assert 0.30 <= zeros <= 0.70, f"{m}x{n}x{k}: {zeros:.3f} of the relu outputs are zero"
    want.setflags(write=False)
    return want


_ON_DEVICE = {}


def _on_device(qg, device, m, n, k):
    """_inputs(m, n, k) on the device -- X, the packed W and the bias -- for the latest shape only."""
    if (m, n, k) not in _ON_DEVICE:
        _ON_DEVICE.clear()
        X, W, b = _inputs(m, n, k)
        _ON_DEVICE[(m, n, k)] = (_dev(X, device), qg.pack_b(_dev(W, device)), _dev(b, device))
    return _ON_DEVICE[(m, n, k)]


def _linear(qg, device, m, n, k, epi, Y):
    bias, relu = EPILOGUES[epi]
    Xd, pw, bd = _on_device(qg, device, m, n, k)
    qg.linear(Xd, pw, bias=bd if bias else None, relu=relu, Y=Y)


# ---------------------------------------------------------------------------------- 1. all twelve instantiations
# K -> k-blocks, pre, form: 512 -> 8, 2, loop-free; 640 -> 10, 4, residue 1 (the loop runs once); 768 -> 12, 6, residue 0
# (twice); 896 -> 14, 8, residue 2 (twice); 1024 -> 16, 10, residue 1 again, with three runs of the loop
INST_CASES = [(s, k, e) for s in (FULL, RAGGED) for k in (512, 640, 768, 896) for e in EPILOGUES] + \
             [(s, 1024, "bias_relu") for s in (FULL, RAGGED)]

assert [_k_form(k) for k in (512, 640, 768, 896, 1024)] == \
    [(2, 2, False), (4, 1, True), (6, 0, True), (8, 2, True), (10, 1, True)]
_COVERED = {(_instantiation(k), e, s == RAGGED) for s, k, e in INST_CASES}
_ALL = set(itertools.product(("loop-free", "residue 0", "residue 1", "residue 2"), EPILOGUES, (False, True)))
assert _COVERED == _ALL and len(_ALL) == 24, f"instantiations without a case: {sorted(_ALL - _COVERED)}"


@pytest.mark.parametrize("shape,K,epi", INST_CASES, ids=[f"{s[0]}x{s[1]}x{k}-{e}" for s, k, e in INST_CASES])
def test_every_instantiation(qg, oracle, device, shape, K, epi):
    """pack_b + linear into a NaN-filled Y: each K-form under each epilogue, at full tiles and at ragged ones."""
    M, N = shape
    _assert_plan(qg, M, N, K)
    want = _expected(M, N, K, epi)
    Y = torch.full((M, N), float("nan"), device=device)
    _linear(qg, device, M, N, K, epi, Y)
    torch.cuda.synchronize()
    assert_bits_equal(Y.cpu().numpy(), want, f"row finish {_instantiation(K)} {epi} {M}x{N}x{K}")


# ---------------------------------------------------------------------------------- 2. edges of the guarded stores
# a wave owns 128 x 128 of the tile (wave row / column 0 and 1) and a lane four adjacent columns of a row
EDGE_SHAPES = [
    (2561, 4096),  # one valid row in the last tile row; wave row 1 has none
    (2689, 4096),  # 129 valid rows: wave row 1 has exactly one
    (2560, 3844),  # four valid columns in the last tile column: one lane quad
    (2560, 3972),  # 132 valid columns: wave column 1 has four
    (2560, 4001),  # the cut falls inside a lane's four columns; rows of 4008 floats keep the launch on the form
]


@pytest.mark.parametrize("M,N", EDGE_SHAPES, ids=[f"{m}x{n}" for m, n in EDGE_SHAPES])
def test_guarded_store_edges(qg, oracle, device, M, N):
    """K = 640 (a looped form), bias + relu, into a view of a NaN-filled buffer with 8 spare rows and 4 to 7 spare
    floats per row: everything outside the M x N view still holds the NaN afterwards."""
    K, epi = 640, "bias_relu"
    _assert_plan(qg, M, N, K)
    stride = _round_up(N, 4) + 4
    assert _row_finish_output(K, stride, 1, 0)
    want = _expected(M, N, K, epi)
    buf = torch.full((M + 8, stride), float("nan"), device=device)
    Y = buf[:M, :N]
    assert Y.data_ptr() % 16 == 0 and Y.stride() == (stride, 1)
    _linear(qg, device, M, N, K, epi, Y)
    torch.cuda.synchronize()
    what = f"row finish edge {M}x{N}x{K}"
    assert_bits_equal(Y.contiguous().cpu().numpy(), want, what)
    outside = torch.ones(buf.shape, dtype=torch.bool, device=device)
    outside[:M, :N] = False
    written = int((buf.view(torch.int32)[outside] != POISON).sum())
    assert written == 0, f"{what}: {written} elements outside the view were written"


# ---------------------------------------------------------------------------------- 3. tile maps
TILE_MAPS = [
    (41216, 256),  # 161 x 1 tiles: one tile column, 161 % 8 == 1
    (768, 13824),  # 3 x 54: fewer tile rows than a group of 4, 162 % 8 == 2; rows of 55296 B, below the wide-row switch
    (2560, 4352),  # 10 x 17: xcd_remap's remainder branch at the base tile-row count, 170 % 8 == 2
]


@pytest.mark.parametrize("M,N", TILE_MAPS, ids=[f"{m}x{n}" for m, n in TILE_MAPS])
def test_tile_maps(qg, oracle, device, M, N):
    K = 512
    _assert_plan(qg, M, N, K)
    tiles = (M // 256) * (N // 256)
    assert M % 256 == 0 and N % 256 == 0 and tiles % 8 != 0 and _row_finish_output(K, N, 1, 0)
    X, W, _ = _inputs(M, N, K)
    want = _expected(M, N, K, "none")
    O = torch.full((M, N), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, 127.0)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"row finish tile map {M}x{N}x{K}")


# ---------------------------------------------------------------------------------- 4. the plan matrix
K4 = 512


@functools.lru_cache(maxsize=2)
def _range_case(m, n, k, r):
    """Planted inputs of one shape and the oracle's chain on them at range r, shared and never changed."""
    from oracle import oracle as O
    X, W = _plant(*O.inputs(m, n, k, 7400 + m))
    out, ref = O.quantized_mm(X, W, r, intermediates=True)
    return X, W, out, ref


_PACKED = {}


def _packed(qg, device, m, n, k, r):
    """The shape's operands packed with r, once; only the latest is kept."""
    key = (m, n, k, r)
    if key not in _PACKED:
        _PACKED.clear()
        X, W, _, _ = _range_case(m, n, k, r)
        _PACKED[key] = (qg.pack_a(_dev(X, device), r), qg.pack_b(_dev(W, device), r))
    return _PACKED[key]


ROW_FINISH_LAYOUTS = ("contiguous", "rows_n+4", "rows_16380")
PLAIN_LAYOUTS = ("rows_n+1", "rows_n+4_offset_1", "column_major", "every_other_column", "rows_16384")
assert set(ROW_FINISH_LAYOUTS) | set(PLAIN_LAYOUTS) == set(OUT_LAYOUTS)
LAYOUT_CASES = [(FULL, lay) for lay in OUT_LAYOUTS] + [(RAGGED, "rows_n+4"), (RAGGED, "rows_n+1")]


@pytest.mark.parametrize("shape,layout", LAYOUT_CASES, ids=[f"{s[0]}x{s[1]}-{lay}" for s, lay in LAYOUT_CASES])
def test_output_layouts_around_the_form(qg, oracle, device, shape, layout):
    """mm_packed into every output layout: the three paired-store layouts run the row-finish kernel, the five others
    the plain kernel of the same plan; the same bits either way, and nothing outside the matrix is written."""
    M, N = shape
    _assert_plan(qg, M, N, K4)
    sh, sw, off = OUT_LAYOUTS[layout](M, N)
    assert _row_finish_output(K4, sh, sw, off) == (layout in ROW_FINISH_LAYOUTS), layout
    pa, pb = _packed(qg, device, M, N, K4, 127.0)
    flat, C = _strided_out(M, N, sh, sw, off, device)
    assert flat.data_ptr() % 16 == 0 and C.data_ptr() % 16 == (4 if off else 0)
    qg.mm_packed(pa, pb, C)
    torch.cuda.synchronize()
    what = f"{M}x{N}x{K4} {layout}"
    assert_bits_equal(C.contiguous().cpu().numpy(), _range_case(M, N, K4, 127.0)[2], what)
    _check_untouched(flat, M, N, sh, sw, off, what)


@pytest.mark.parametrize("r", [63.0, 200.0])
def test_mm_packed_range(qg, oracle, device, r):
    """mm_packed on operands packed with r: O and the raw accumulators.  At 200 the operands are full of 127 / -128."""
    M, N = FULL
    _assert_plan(qg, M, N, K4)
    _, _, want, ref = _range_case(M, N, K4, r)
    if r == 200.0:
        _check_saturation(ref["Xq"], None, r, f"{M}x{N}x{K4} Xq")
        _check_saturation(ref["Wq"], None, r, f"{M}x{N}x{K4} Wq")
    pa, pb = _packed(qg, device, M, N, K4, r)
    assert pa.range == r and pb.range == r
    O = torch.full((M, N), float("nan"), device=device)
    qg.mm_packed(pa, pb, O)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"{M}x{N}x{K4} range {r} mm_packed")
    acc = qg.mm_packed_i32(pa, pb).cpu().numpy()
    assert (acc == ref["Acc"]).all(), f"{M}x{N}x{K4} range {r} Acc: {int((acc != ref['Acc']).sum())} differ"


def test_drop_in_range_63(qg, oracle, device):
    M, N = FULL
    _assert_plan(qg, M, N, K4)
    X, W, want, _ = _range_case(M, N, K4, 63.0)
    O = torch.full((M, N), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, 63.0)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"{M}x{N}x{K4} range 63 drop-in")


def test_range_so_large_that_its_square_overflows(qg, oracle, device):
    """range = 1e20: fl(range * range) is inf, inv_r2 = +0, and every finite product becomes a zero with its sign."""
    M, N = FULL
    _assert_plan(qg, M, N, K4)
    r = 1e20
    X, W = _range_case(M, N, K4, 63.0)[:2]
    want = oracle.quantized_mm(X, W, r)
    zero = want == 0
    assert (zero & np.signbit(want)).any() and (zero & ~np.signbit(want)).any(), "expected +0 and -0 outputs"
    O = torch.full((M, N), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, r)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"{M}x{N}x{K4} range 1e20")


def test_range_so_small_that_only_seeds_survive(qg, oracle, device):
    """range = 2^-20: only a signed seed far outside its row's / column's absmax (3e6 times it) keeps a nonzero byte."""
    M, N = FULL
    _assert_plan(qg, M, N, K4)
    r = 2.0 ** -20
    X, W = (a.copy() for a in _range_case(M, N, K4, 63.0)[:2])
    X[::4, 0] = -3.0e6
    W[0, ::3] = -3.0e6
    want, ref = oracle.quantized_mm(X, W, r, intermediates=True)
    assert not ref["Xq"][:, 1:].any() and not ref["Wq"][1:].any(), "only the seeds may quantize to nonzero"
    assert ref["Xq"][::4, 0].all() and ref["Wq"][0, ::3].all() and (want != 0).any()
    O = torch.full((M, N), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, r)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"{M}x{N}x{K4} range 2^-20")


# ---------------------------------------------------------------------------------- 5. accumulators beyond 2^24
def test_accumulators_beyond_2_24(qg, oracle, device):
    """2560 x 4096 x 1536 (24 k-blocks, residue 0) with |x|, |w| in [0.75, 1): every quantized operand is 95 .. 127 in
    magnitude and every |acc| about 1536 * 111^2 = 19 million, above 2^24 = 16.8 million, where every second integer
    is no float -- the epilogue's int32 -> float conversion has to round (to nearest even, as the oracle's cast).  Rows
    of X alternate in sign and every third column of W is negative, so half the accumulators are negative."""
    M, N, K = 2560, 4096, 1536
    _assert_plan(qg, M, N, K)
    assert _k_form(K) == (18, 0, True)
    X = oracle.uniform((M, K), 7501, 0.75, 1.0)
    W = oracle.uniform((K, N), 7502, 0.75, 1.0)
    X[1::2] *= -1.0
    W[:, ::3] *= -1.0
    b = oracle.uniform((N,), 7503, -0.5, 0.5)
    want, ref = oracle.quantized_mm(X, W, 127.0, intermediates=True)
    acc = ref["Acc"].astype(np.int64)
    assert (np.abs(acc) > 1 << 24).all(), f"min |acc| = {int(np.abs(acc).min())}"
    inexact = float((acc.astype(np.float32).astype(np.int64) != acc).mean())
    assert inexact >= 0.40, f"{inexact:.3f} of the accumulators are inexact in fp32"
    assert 0.45 <= float((acc < 0).mean()) <= 0.55
    Xd = _dev(X, device)
    pa, pb = qg.pack_a(Xd), qg.pack_b(_dev(W, device))
    O = torch.full((M, N), float("nan"), device=device)
    qg.mm_packed(pa, pb, O)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, "accumulators beyond 2^24, mm_packed")
    got = qg.mm_packed_i32(pa, pb).cpu().numpy()
    assert (got == ref["Acc"]).all(), f"accumulators beyond 2^24, Acc: {int((got != ref['Acc']).sum())} differ"
    Y = torch.full((M, N), float("nan"), device=device)
    qg.linear(Xd, pb, bias=_dev(b, device), Y=Y)
    torch.cuda.synchronize()
    assert_bits_equal(Y.cpu().numpy(), oracle.linear(X, W, b, False), "accumulators beyond 2^24, linear with bias")


# ---------------------------------------------------------------------------------- 6. position independence at long K
def test_long_k_every_tile_row_alike(qg, oracle, device):
    """K = 4096 (the benchmark's; residue 1, 19 runs of the loop) under bias + relu with X's 256 rows repeated ten
    times: a row's output depends on that row and on W alone, so the expected output is the oracle's 256 rows, tiled,
    and a tile row that differs from the others shows."""
    M, N, K, reps = 2560, 4096, 4096, 10
    _assert_plan(qg, M, N, K)
    assert _k_form(K) == (58, 1, True)
    X, W, b = _inputs(M // reps, N, K)
    want = _expected(M // reps, N, K, "bias_relu")
    Xd = _dev(X, device).repeat(reps, 1)
    assert Xd.shape == (M, K)
    Y = torch.full((M, N), float("nan"), device=device)
    qg.linear(Xd, qg.pack_b(_dev(W, device)), bias=_dev(b, device), relu=True, Y=Y)
    torch.cuda.synchronize()
    assert_bits_equal(Y.cpu().numpy(), np.tile(want, (reps, 1)), f"row finish {M}x{N}x{K}, ten equal tile rows")


# ---------------------------------------------------------------------------------- 7. repeats, a busy neighbour, capture
REPEATS = 20


class _Launch:
    """qgemm_linear with bias + relu at 2560 x 4096 x K on a stream of its own, workspace allocated once (so that the
    calls neither allocate nor touch another stream), and the expected output on the device as int32 bits."""

    def __init__(self, qg, device, K):
        self.M, self.N = FULL
        self.K = K
        _assert_plan(qg, self.M, self.N, K)
        self.L = qg.load()
        self.want = _expected(self.M, self.N, K, "bias_relu")
        self.Xd, self.pw, self.bd = _on_device(qg, device, self.M, self.N, K)
        self.ws = torch.empty(self.L.qgemm_linear_workspace_size(self.M, self.N, K), dtype=torch.uint8, device=device)
        self.Y = torch.full((self.M, self.N), float("nan"), device=device)
        self.want_bits = _dev(self.want, device).view(torch.int32)
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream(device)

    def __call__(self):
        rc = self.L.qgemm_linear(self.Xd.data_ptr(), self.K, self.M, self.K, self.pw.buf.data_ptr(), self.N,
                                 self.bd.data_ptr(), 1, self.Y.data_ptr(), self.N, self.ws.data_ptr(), self.ws.numel(),
                                 self.stream.cuda_stream)
        assert rc == 0

    def check_on_host(self, what):
        assert_bits_equal(self.Y.cpu().numpy(), self.want, what)


@pytest.mark.parametrize("K", [512, 640, 768, 896])
def test_repeated_launches(qg, oracle, device, K):
    """20 eager calls on one stream into the same Y, refilled with NaN ahead of each, every result compared on the
    device; the first mismatch ends the run."""
    run = _Launch(qg, device, K)
    with torch.cuda.stream(run.stream):
        for i in range(REPEATS):
            run.Y.fill_(float("nan"))
            run()
            if not torch.equal(run.Y.view(torch.int32), run.want_bits):
                run.check_on_host(f"row finish {_instantiation(K)} repeat {i}")  # says how many differ
                raise AssertionError(f"repeat {i} differs from the expected bits on the device")
    run.stream.synchronize()
    run.check_on_host(f"row finish {_instantiation(K)} after {REPEATS} repeats")


def test_repeated_launches_next_to_a_streaming_copy(qg, oracle, device):
    """The same 20 calls at K = 640 while a second stream copies between two 256-MiB buffers, 20 times: nothing waits
    for the host in between, so the copies and the GEMMs share the chip.  Each call's count of differing outputs
    stays on the device until both streams have been synchronised."""
    K = 640
    run = _Launch(qg, device, K)
    src = torch.zeros(256 << 20, dtype=torch.uint8, device=device)
    dst = torch.empty_like(src)
    differ = torch.full((REPEATS,), -1, dtype=torch.int64, device=device)
    torch.cuda.synchronize()
    other = torch.cuda.Stream(device)
    for i in range(REPEATS):
        with torch.cuda.stream(other):
            dst.copy_(src)
        with torch.cuda.stream(run.stream):
            run.Y.fill_(float("nan"))
            run()
            differ[i] = (run.Y.view(torch.int32) != run.want_bits).sum()
    run.stream.synchronize()
    other.synchronize()
    counts = differ.cpu().tolist()
    run.check_on_host(f"row finish {_instantiation(K)} next to a streaming copy, last of {REPEATS} calls")
    assert counts == [0] * REPEATS, f"outputs that differ, call by call: {counts}"


@pytest.mark.parametrize("K", [512, 896])
def test_graph_capture_and_replay(qg, oracle, device, K):
    """The launch (X's pack and the GEMM) captured in a single-stream graph, after one eager call on that stream, and
    replayed three times into a Y that is refilled with NaN ahead of each replay."""
    run = _Launch(qg, device, K)
    with torch.cuda.stream(run.stream):
        run()
        run.stream.synchronize()
        run.check_on_host(f"row finish {_instantiation(K)} ahead of the capture")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=run.stream):
            run()
    for i in range(3):
        run.Y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        run.check_on_host(f"row finish {_instantiation(K)} graph replay {i}")
