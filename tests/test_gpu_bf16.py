"""bf16 activations and outputs on the prepacked path (qgemm_pack_a_dt / qgemm_mm_packed_dt / qgemm_linear_dt).

The arithmetic is the fp32 chain's; only its two ends change.  So the expected result of every case is the unchanged
CPU oracle run on the WIDENED input (bf16 -> fp32 is exact) and rounded once to bf16 on the CPU
(torch.from_numpy(Y).to(torch.bfloat16): round to nearest even).  Every comparison is on the bf16 bit patterns,
except that NaNs only have to sit at the same places.  Outputs are pre-filled with NaN; for strided outputs the
elements outside the logical matrix must still hold it afterwards.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from util import assert_bits_equal, assert_values_equal

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
POISON = 0x7FC0  # the bf16 NaN the output buffers are filled with
# the bf16 row stride from which gemm_i8_fm's bf16 output takes the LDS-image stores (gemm_i8.hip kBf16WideRowsMin)
WIDE_MIN = 16384


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _to_bf16(a):
    """fp32 numpy -> bf16 CPU tensor, round to nearest even."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF16)


def _widen(xb):
    """bf16 CPU tensor -> fp32 numpy, exact."""
    return xb.float().numpy()


def _bits(t):
    """bf16 tensor (any device, any strides) -> uint16 numpy of its logical elements."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _want_bits(y32):
    return _bits(_to_bf16(y32))


def _is_nan(b):
    return (b & 0x7FFF) > 0x7F80


def assert_bf16_equal(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    gn, wn = _is_nan(got), _is_nan(want)
    assert (gn == wn).all(), f"{what}: NaN positions differ ({int((gn != wn).sum())} places)"
    bad = (got != want) & ~gn
    if bad.any():
        idx = np.argwhere(bad)[:5]
        eg = [(tuple(i), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in idx]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bf16 values differ in bits, e.g. {eg}")


def _plan(qg, m, n, k):
    t, name = ctypes.c_int(0), ctypes.c_char_p()
    splits = qg.load().qgemm_gemm_plan(m, n, k, ctypes.byref(t), ctypes.byref(name))
    return t.value, splits, name.value.decode()


@functools.lru_cache(maxsize=None)
def _case(m, n, k, seed, xscale=1.0, wscale=1.0):
    """Inputs of one shape, shared by its tests and never changed: bf16 X (CPU tensor), its widened copy, W, b."""
    from oracle import oracle as O
    X, W = O.inputs(m, n, k, seed)
    xb = _to_bf16(X * np.float32(xscale))
    W = (W * np.float32(wscale)).astype(np.float32)
    b = O.uniform((n,), 7 * seed + 3, -0.5, 0.5)
    return xb, _widen(xb), W, b


@functools.lru_cache(maxsize=None)
def _want(m, n, k, seed, mode, xscale=1.0, wscale=1.0):
    """fp32 oracle output for mode 0 (no bias), 1 (bias), 2 (bias + relu) on the widened X."""
    from oracle import oracle as O
    _, xw, W, b = _case(m, n, k, seed, xscale, wscale)
    return O.linear(xw, W, b if mode else None, mode == 2)


_PACKED_W = {}


def _packed_w(qg, device, key):
    """The shape's weight, packed once from fp32 and shared by its tests."""
    if key not in _PACKED_W:
        _PACKED_W[key] = qg.pack_b(_dev(_case(*key)[2], device))
    return _PACKED_W[key]


def _strided_out(m, n, stride, offset, device):
    """A NaN-filled flat bf16 buffer and the m x n view into it at `offset` with row stride `stride`."""
    flat = torch.full((offset + (m - 1) * stride + n + 16,), float("nan"), dtype=BF16, device=device)
    assert int(_bits(flat[:1])[0]) == POISON
    return flat, torch.as_strided(flat, (m, n), (stride, 1), offset)


def _check_untouched(flat, m, n, stride, offset, what):
    b = _bits(flat)
    mask = np.ones(b.shape, bool)
    idx = offset + np.arange(m)[:, None] * stride + np.arange(n)[None, :]
    mask[idx.ravel()] = False
    assert (b[mask] == POISON).all(), f"{what}: {int((b[mask] != POISON).sum())} elements outside the matrix were written"


def _run_linear(qg, device, m, n, k, seed, mode, stride=None, offset=0, xscale=1.0, wscale=1.0, x_f32=False,
                bias=None, want=None):
    """One bf16-output linear against the oracle.  bias / want: a test's own bias vector and the oracle output for
    it (mode says whether relu follows)."""
    xb, xw, W, b = _case(m, n, k, seed, xscale, wscale)
    b = b if bias is None else bias
    pw = _packed_w(qg, device, (m, n, k, seed, xscale, wscale))
    stride = n if stride is None else stride
    flat, Y = _strided_out(m, n, stride, offset, device)
    Xd = _dev(xw, device) if x_f32 else xb.to(device)
    out = qg.linear(Xd, pw, bias=_dev(b, device) if mode else None, relu=mode == 2, Y=Y)
    torch.cuda.synchronize()
    assert out.dtype == BF16
    what = f"linear bf16 {m}x{n}x{k} mode {mode} stride {stride} offset {offset}"
    want = _want(m, n, k, seed, mode, xscale, wscale) if want is None else want
    assert_bf16_equal(_bits(Y), _want_bits(want), what)
    _check_untouched(flat, m, n, stride, offset, what)


# ---------------------------------------------------------------------------------- 1. pack intermediates
def _check_pack(qg, oracle, device, xb_view_dev, xw, what, packed=None):
    """scale[:M], q[:M, :K] against the oracle's Cx / Xq of the widened X; padding zero."""
    M, K = xw.shape
    _, ref = oracle.quantized_mm(xw, np.ones((K, 1), np.float32), intermediates=True)
    pa = qg.pack_a(xb_view_dev) if packed is None else packed
    torch.cuda.synchronize()
    assert_values_equal(pa.scale[:M].cpu().numpy(), ref["Cx"], f"{what} Cx")
    q = pa.q.cpu().numpy()
    assert (q[:M, :K] == ref["Xq"]).all(), f"{what} Xq: {int((q[:M, :K] != ref['Xq']).sum())} bytes differ"
    assert not q[M:].any() and not q[:, K:].any(), f"{what}: padding not zero"
    assert not pa.scale[M:].cpu().numpy().any(), f"{what}: padding scales not zero"


# K: the issue's list, plus the value on each side of every boundary of the bf16 dispatch (pack.hip rows_regs):
# 8-element chunks per lane 1 | 2 | 4 | 8 at 519|520, 1031|1032, 2055|2056; one wave per row | block per row at
# 4096|4097; block per row | streaming at 32768|32769
PACK_K = [1, 2, 7, 8, 9, 255, 256, 264, 1000, 4096, 4104, 5003, 16384, 16392, 40000,
          519, 520, 1031, 1032, 2055, 2056, 4097, 32768, 32769]


@pytest.mark.parametrize("K", PACK_K)
def test_pack_a_bf16_intermediates(qg, oracle, device, K):
    for M in (1, 9, 300):
        xb = _to_bf16(oracle.uniform((M, K), 1000 + K + M, -2.0, 2.0))
        _check_pack(qg, oracle, device, xb.to(device), _widen(xb), f"pack_a bf16 {M}x{K}")


@pytest.mark.parametrize("K", [512, 4096])
def test_pack_a_bf16_staged_rows(qg, oracle, device, K):
    """2048 padded rows: the 8-rows-per-block form that stages the packed rows in LDS."""
    M = 2048
    xb = _to_bf16(oracle.uniform((M, K), 2000 + K, -2.0, 2.0))
    _check_pack(qg, oracle, device, xb.to(device), _widen(xb), f"pack_a bf16 staged {M}x{K}")


@pytest.mark.parametrize("M,K", [(9, 264), (300, 1000), (2048, 512)])
def test_pack_a_bf16_unaligned_views(qg, oracle, device, M, K):
    # a row stride that is no multiple of 8 elements
    xb = _to_bf16(oracle.uniform((M, K + 3), 3000 + K, -2.0, 2.0))
    xd = xb.to(device)
    _check_pack(qg, oracle, device, xd[:, :K], _widen(xb[:, :K]), f"row stride {K + 3}")
    # a view that starts one element in: 2-byte aligned only
    xb = _to_bf16(oracle.uniform((M, K + 8), 3100 + K, -2.0, 2.0))
    xd = xb.to(device)
    v = xd[:, 1:K + 1]
    assert v.data_ptr() % 4 == 2
    _check_pack(qg, oracle, device, v, _widen(xb[:, 1:K + 1]), "X[:, 1:]")
    # a_stride_w = 2 through the C entry point
    xb = _to_bf16(oracle.uniform((M, 2 * K), 3200 + K, -2.0, 2.0))
    xd = xb.to(device)
    p = qg.Packed(qg._alloc_packed(M, K, device), M, K, 127.0)
    rc = qg.load().qgemm_pack_a_dt(xd.data_ptr(), qg.QGEMM_BF16, 2 * K, 2, M, K, 127.0, p.buf.data_ptr(),
                                   qg._stream(device))
    assert rc == 0
    _check_pack(qg, oracle, device, None, _widen(xb[:, ::2]), "a_stride_w = 2", packed=p)
    # and through the wrapper (a strided torch view)
    _check_pack(qg, oracle, device, xd[:, ::2], _widen(xb[:, ::2]), "X[:, ::2]")


# ---------------------------------------------------------------------------------- 2. special values
@pytest.mark.parametrize("K", [264, 1000, 5003])
def test_bf16_special_values(qg, oracle, device, K):
    """The seed quirk with int8 saturation, a zero row, NaN / +-inf rows, the bf16 maximum and bf16 subnormals:
    Cx, Xq and the final bf16 Y."""
    M, N = 12, 72
    X = oracle.uniform((M, K), 41 + K)
    X[0, 0] = -3.0                      # first element negative and the largest magnitude
    X[1, :] = 0.0
    X[2, K // 2] = np.nan
    X[3, 0] = np.nan                    # a NaN seed sticks
    X[4, 5 % K] = np.inf
    X[5, K - 1] = -np.inf
    X[6, 3] = 3.3895313892515355e38     # the bf16 maximum
    X[7, 0] = -3.3895313892515355e38
    X[8, :] = oracle.uniform((K,), 43) * np.float32(1e-39)   # bf16 subnormals (and zeros)
    X[9, 1:] = X[9, 1:] * np.float32(1e-39)                  # one normal seed among subnormals
    X[10, :] = -0.0
    xb = _to_bf16(X)
    xw = _widen(xb)
    sub = np.abs(xw[8]) < np.float32(1.1754944e-38)
    assert (sub & (xw[8] != 0)).any(), "row 8 must hold bf16 subnormals"
    assert np.isinf(xw[4]).any() and np.isnan(xw[2]).any() and xw[6, 3] == np.float32(3.3895313892515355e38)
    _check_pack(qg, oracle, device, xb.to(device), xw, f"special values K={K}")
    W = oracle.uniform((K, N), 45 + K)
    b = oracle.uniform((N,), 47, -0.5, 0.5)
    pw = qg.pack_b(_dev(W, device))
    for mode in (0, 1, 2):
        Y = torch.full((M, N), float("nan"), dtype=BF16, device=device)
        qg.linear(xb.to(device), pw, bias=_dev(b, device) if mode else None, relu=mode == 2, Y=Y)
        torch.cuda.synchronize()
        want = oracle.linear(xw, W, b if mode else None, mode == 2)
        assert_bf16_equal(_bits(Y), _want_bits(want), f"special values K={K} mode {mode}")


# ---------------------------------------------------------------------------------- 3. every GEMM plan
# (m, n, k), the plan qgemm_gemm_plan must report (tile, splits) and, for 64-tiles, the ring depth the launcher
# derives from the tile count (<= 512 tiles: 3 stages)
PLAN_SHAPES = [
    ((256, 1024, 256), 32, 1, None),
    ((250, 1000, 200), 32, 1, None),
    ((100, 200, 300), 64, 1, 3),
    ((130, 70, 640), 64, 1, 3),
    ((2048, 2048, 256), 64, 1, 2),
    ((2000, 1990, 130), 64, 1, 2),
    ((64, 64, 4096), 64, 2, 3),
    ((70, 100, 4100), 64, 2, 3),
    ((4096, 2560, 128), 256, 1, None),
    ((4000, 2500, 192), 256, 1, None),
    ((2048, 4096, 2048), 256, 2, None),
    ((2560, 16384, 128), 256, 1, None),
]


def _assert_plan(qg, shape, tile, splits, depth):
    m, n, k = shape
    t, s, name = _plan(qg, m, n, k)
    assert (t, s) == (tile, splits), f"{shape}: plan is tile {t} splits {s} ({name})"
    assert name.startswith("gemm_i8_fm" if tile == 256 else f"gemm_i8_small<{tile}>")
    if depth is not None:
        tiles = -(-m // 64) * -(-n // 64)
        assert (tiles <= 512) == (depth == 3)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["plain", "bias", "bias_relu"])
@pytest.mark.parametrize("shape,tile,splits,depth", PLAN_SHAPES, ids=[str(s[0]) for s in PLAN_SHAPES])
def test_every_plan_bf16_output(qg, oracle, device, shape, tile, splits, depth, mode):
    _assert_plan(qg, shape, tile, splits, depth)
    m, n, k = shape
    _run_linear(qg, device, m, n, k, 11, mode)


@pytest.mark.parametrize("mode", [0, 2], ids=["plain", "bias_relu"])
def test_wide_row_buffer_bf16(qg, oracle, device, mode):
    """(4096, 2560, 128) written into a buffer whose rows are 16 384 elements long."""
    _assert_plan(qg, (4096, 2560, 128), 256, 1, None)
    _run_linear(qg, device, 4096, 2560, 128, 11, mode, stride=16384)


@pytest.mark.parametrize("stride", [WIDE_MIN - 8, WIDE_MIN])
def test_both_sides_of_the_bf16_wide_row_switch(qg, oracle, device, stride):
    """Full 256-tiles with the output's row stride just below the switch point (exchanged 16-B register stores) and
    at it (LDS-image stores)."""
    _assert_plan(qg, (2048, 4096, 128), 256, 1, None)
    _run_linear(qg, device, 2048, 4096, 128, 13, 1, stride=stride)


# ---------------------------------------------------------------------------------- 4. output alignment
@pytest.mark.parametrize("shape,tile", [((100, 200, 300), 64), ((4096, 2560, 128), 256)], ids=["64", "256"])
def test_bf16_output_alignment(qg, oracle, device, shape, tile):
    m, n, k = shape
    assert _plan(qg, m, n, k)[0] == tile
    _run_linear(qg, device, m, n, k, 11, 1, stride=n + 1)            # odd row stride
    _run_linear(qg, device, m, n, k, 11, 1, stride=n + 8, offset=1)  # rows 16-B periodic, base at an odd element
    _run_linear(qg, device, m, n, k, 11, 1, stride=n + 8, offset=8)  # aligned again, padded rows


@pytest.mark.parametrize("shape,tile", [((100, 203, 300), 64), ((4000, 2500, 192), 256)], ids=["64", "256"])
def test_bf16_output_n_not_multiple_of_8(qg, oracle, device, shape, tile):
    m, n, k = shape
    assert n % 8 != 0 and _plan(qg, m, n, k)[0] == tile
    _run_linear(qg, device, m, n, k, 11, 2)
    _run_linear(qg, device, m, n, k, 11, 2, stride=n + 4)


# ---------------------------------------------------------------------------------- 5. rounding
TIE_SEED = 5  # chosen on the CPU: see the precondition below


def test_bf16_rounding_ties(qg, oracle, device):
    """fp32 outputs that lie exactly between two bf16 values must go to the even one."""
    m, n, k = 2048, 2048, 256
    y = _want(m, n, k, TIE_SEED, 0)
    u = y.view(np.uint32)
    ties = (u & 0xFFFF) == 0x8000
    odd = ((u >> 16) & 1) == 1
    assert ties.sum() >= 8 and (ties & odd).sum() >= 1 and (ties & ~odd).sum() >= 1, \
        f"seed {TIE_SEED}: {int(ties.sum())} ties, {int((ties & odd).sum())} with an odd upper half"
    _run_linear(qg, device, m, n, k, TIE_SEED, 0)


@pytest.mark.parametrize("shape", [(130, 70, 640), (4000, 2500, 192)], ids=["64", "256"])
def test_bf16_rounding_overflow(qg, oracle, device, shape):
    """Finite fp32 outputs past the bf16 maximum become +-inf; those between the maximum and the half-way point stay
    at the maximum.  The dequantize alone cannot produce them: fl(float(acc) * fl(Cx * Cw)) already overflows to inf
    before the multiplication by 1 / range^2, so its finite results end near 2e34.  X and W are therefore scaled
    until the GEMM's own outputs are large (and some infinite), and a bias between the bf16 maximum (0x7f7f0000) and
    the fp32 maximum carries the finite ones into the last bf16 binade."""
    m, n, k = shape
    s = 3.0e15
    xb, xw, W, _ = _case(m, n, k, 17, s, s)
    lo, hi = np.float32(3.3895e38), np.float32(3.4028e38)
    b = oracle.uniform((n,), 171, float(lo), float(hi))
    b[1::2] = -b[1::2]
    y = oracle.linear(xw, W, b, False)
    u = y.view(np.uint32) & 0x7FFFFFFF
    over = (u >= 0x7F7F8000) & (u < 0x7F800000)   # finite, rounds to inf (the tie goes to the even 0x7f80)
    near = (u > 0x7F7F0000) & (u < 0x7F7F8000)    # finite, rounds down to the bf16 maximum
    assert over.sum() >= 16 and near.sum() >= 16, f"{int(over.sum())} outputs past the bf16 maximum, {int(near.sum())} near it"
    w = _want_bits(y)
    assert ((w[over] & 0x7FFF) == 0x7F80).all() and ((w[near] & 0x7FFF) == 0x7F7F).all()
    _run_linear(qg, device, m, n, k, 17, 1, xscale=s, wscale=s, bias=b, want=y)


@pytest.mark.parametrize("shape", [(130, 70, 640), (4000, 2500, 192)], ids=["64", "256"])
def test_bf16_rounding_subnormals(qg, oracle, device, shape):
    """fp32-subnormal outputs stay subnormal in bf16 (nothing is flushed)."""
    m, n, k = shape
    s = float(np.sqrt(1.0e-38 * 3.0 / np.sqrt(k)))  # output sigma ~ 1e-38
    y = _want(m, n, k, 19, 0, s, s)
    sub = (y != 0) & (np.abs(y) < np.float32(1.1754944e-38))
    assert sub.sum() >= 64, f"only {int(sub.sum())} subnormal fp32 outputs"
    w = _want_bits(y)
    wsub = ((w & 0x7F80) == 0) & ((w & 0x7F) != 0)
    assert wsub.sum() >= 64, "the expected bf16 values hold subnormals too"
    _run_linear(qg, device, m, n, k, 19, 0, xscale=s, wscale=s)


# ---------------------------------------------------------------------------------- 6. the four type combinations
@pytest.mark.parametrize("shape", [(100, 200, 300), (4096, 2560, 128)], ids=["64", "256"])
def test_four_type_combinations(qg, oracle, device, shape):
    m, n, k = shape
    L = qg.load()
    xb, xw, W, b = _case(m, n, k, 11)
    pw = _packed_w(qg, device, (m, n, k, 11, 1.0, 1.0))
    bd = _dev(b, device)
    X32 = oracle.uniform((m, k), 23)  # an fp32 X that is NOT bf16-representable
    want32 = oracle.linear(X32, W, b, True)
    # bf16 -> bf16 and bf16 -> fp32
    _run_linear(qg, device, m, n, k, 11, 2)
    Y = qg.linear(xb.to(device), pw, bias=bd, relu=True, out_dtype=torch.float32)
    assert Y.dtype == torch.float32
    assert_bits_equal(Y.cpu().numpy(), _want(m, n, k, 11, 2), "bf16 -> fp32")
    # fp32 -> bf16
    Y = qg.linear(_dev(X32, device), pw, bias=bd, relu=True, out_dtype=BF16)
    assert Y.dtype == BF16
    assert_bf16_equal(_bits(Y), _want_bits(want32), "fp32 -> bf16")
    # fp32 -> fp32 through the _dt entry points: bit-identical to qgemm_linear / qgemm_mm_packed
    Xd = _dev(X32, device)
    ws = torch.empty(max(1, L.qgemm_linear_workspace_size(m, n, k)), dtype=torch.uint8, device=device)
    Y0 = torch.full((m, n), float("nan"), device=device)
    Y1 = torch.full((m, n), float("nan"), device=device)
    s = qg._stream(device)
    assert L.qgemm_linear(Xd.data_ptr(), k, m, k, pw.buf.data_ptr(), n, bd.data_ptr(), 1, Y0.data_ptr(), n,
                          ws.data_ptr(), ws.numel(), s) == 0
    assert L.qgemm_linear_dt(Xd.data_ptr(), qg.QGEMM_F32, k, m, k, pw.buf.data_ptr(), n, bd.data_ptr(), 1, Y1.data_ptr(),
                             qg.QGEMM_F32, n, ws.data_ptr(), ws.numel(), s) == 0
    torch.cuda.synchronize()
    assert_bits_equal(Y1.cpu().numpy(), Y0.cpu().numpy(), "qgemm_linear_dt(F32, F32) vs qgemm_linear")
    assert_bits_equal(Y0.cpu().numpy(), want32, "qgemm_linear")
    pa = qg.pack_a(Xd)
    pa_dt = qg.Packed(qg._alloc_packed(m, k, device), m, k, 127.0)
    assert L.qgemm_pack_a_dt(Xd.data_ptr(), qg.QGEMM_F32, k, 1, m, k, 127.0, pa_dt.buf.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(pa.q_raw, pa_dt.q_raw) and torch.equal(pa.scale.view(torch.int32), pa_dt.scale.view(torch.int32))
    C0 = qg.mm_packed(pa, pw)
    C1 = torch.full((m, n), float("nan"), device=device)
    assert L.qgemm_mm_packed_dt(pa.buf.data_ptr(), pw.buf.data_ptr(), C1.data_ptr(), qg.QGEMM_F32, n, 1, m, n, k, 127.0,
                                s) == 0
    torch.cuda.synchronize()
    assert_bits_equal(C1.cpu().numpy(), C0.cpu().numpy(), "qgemm_mm_packed_dt(F32) vs qgemm_mm_packed")
    # mm_packed with a bf16 output: the plain chain, rounded
    Cb = qg.mm_packed(qg.pack_a(xb.to(device)), pw, out_dtype=BF16)
    assert Cb.dtype == BF16
    assert_bf16_equal(_bits(Cb), _want_bits(_want(m, n, k, 11, 0)), "mm_packed bf16")
    # empty outputs are no-ops (pointers must still be non-null, as for qgemm_linear): nothing is written
    Ye = torch.full((m, n), float("nan"), dtype=BF16, device=device)
    xbd = xb.to(device)
    assert L.qgemm_linear_dt(xbd.data_ptr(), 1, k, 0, k, pw.buf.data_ptr(), n, None, 0, Ye.data_ptr(), 1, n,
                             ws.data_ptr(), ws.numel(), s) == 0
    assert L.qgemm_linear_dt(xbd.data_ptr(), 1, k, m, k, pw.buf.data_ptr(), 0, None, 0, Ye.data_ptr(), 1, n,
                             ws.data_ptr(), ws.numel(), s) == 0
    torch.cuda.synchronize()
    assert (_bits(Ye) == POISON).all()


# ---------------------------------------------------------------------------------- 7. graph capture
def test_linear_dt_graph_capture(qg, oracle, device):
    """qgemm_linear_dt (bf16 in and out) with an explicit workspace, captured and replayed on changed input."""
    L = qg.load()
    m, n, k = 512, 1024, 1024
    W = oracle.uniform((k, n), 31)
    b = oracle.uniform((n,), 33, -0.5, 0.5)
    pw = qg.pack_b(_dev(W, device))
    bd = _dev(b, device)
    xs = [_to_bf16(oracle.uniform((m, k), 35 + i)) for i in range(3)]
    Xd = xs[0].to(device)
    Y = torch.full((m, n), float("nan"), dtype=BF16, device=device)
    ws = torch.empty(max(1, L.qgemm_linear_workspace_size(m, n, k)), dtype=torch.uint8, device=device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert L.qgemm_linear_dt(Xd.data_ptr(), qg.QGEMM_BF16, k, m, k, pw.buf.data_ptr(), n, bd.data_ptr(), 1,
                                     Y.data_ptr(), qg.QGEMM_BF16, n, ws.data_ptr(), ws.numel(), s.cuda_stream) == 0
    for i in (1, 2):
        Xd.copy_(xs[i].to(device))
        Y.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bf16_equal(_bits(Y), _want_bits(oracle.linear(_widen(xs[i]), W, b, True)), f"graph replay {i}")
