"""GPU check of qgemm_pack_b_window against qgemm_pack_b, byte for byte.  Every case pre-fills the
destination with pack_b of a DIFFERENT matrix, packs windows into it and compares the scale and q regions WHOLE with
pack_b of the assembled matrix (the other matrix with the windows' columns replaced): a wrong byte inside a window and
a stray write outside one both show.  The reserved region between them is unspecified and not compared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WINDOWS_40 = ((0, 5), (5, 11), (16, 16), (32, 8))   # unaligned, inside one 16-row group, a whole group, a tail
WINDOWS_300 = ((0, 257), (257, 43))                 # across the 256-row pad boundary
KS = (1, 15, 64, 65, 200, 4224)
SOURCES = ("k-contiguous", "n-contiguous", "generic", "misaligned")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _matrix(k, n, seed, scale=1.0):
    """k x n fp32 on the host whose values are exact in bf16, so the bf16 source widens to the same matrix."""
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn((k, n), generator=g)).to(torch.bfloat16).to(torch.float32)


def _source(cols, kind, dtype, device):
    """The window's k x ncols values (on the device, in the source type) laid out for one source path: (the tensor as
    pack_b_window takes it, its layout)."""
    k, nc = cols.shape
    if kind == "n-contiguous":        # a column slice of a wider row-major matrix
        wide = torch.zeros((k, nc + 3), dtype=dtype, device=device)
        wide[:, 2:2 + nc] = cols
        return wide[:, 2:2 + nc], "kn"
    if kind == "generic":             # every second row and column of a larger one
        big = torch.zeros((2 * k, 2 * nc), dtype=dtype, device=device)
        big[::2, ::2] = cols
        return big[::2, ::2], "kn"
    # [out, in] rows, each padded to a multiple of 16 elements so that every row starts 16-byte aligned ...
    kp = (k + 15) // 16 * 16
    off = 0 if kind == "k-contiguous" else 1   # ... and, misaligned, the whole tensor one element further on
    flat = torch.zeros(nc * kp + 16, dtype=dtype, device=device)
    B = flat[off:off + nc * kp].view(nc, kp)[:, :k]
    B.copy_(cols.t())
    return B, "nk"


def _expect_path(kind, dtype):
    return f"pack_b_window<{'bf16' if dtype == torch.bfloat16 else 'f32'}, {'generic' if kind == 'misaligned' else kind}>"


def _run(qg, device, base, W, windows, kind, dtype, range_=127.0):
    """Pre-fill with pack_b(base), pack W's windows, compare with pack_b of the assembled matrix."""
    k, n = base.shape
    packed = qg.pack_b(base.to(device), range=range_)
    want = base.to(device)
    for c0, nc in windows:
        cols = W[:, c0:c0 + nc].to(device).to(dtype)
        B, layout = _source(cols, kind, dtype, device)
        assert qg.pack_b_window_plan(B, packed, c0, layout=layout) == _expect_path(kind, dtype)
        assert qg.pack_b_window(B, packed, c0, layout=layout, range=range_) is packed
        want[:, c0:c0 + nc] = cols.to(torch.float32)   # the source widened exactly, a NaN's payload included
    ref = qg.pack_b(want, range=range_)
    torch.cuda.synchronize()
    what = f"k={k} n={n} {kind} {dtype} windows={windows}"
    assert torch.equal(packed.scale.view(torch.int32), ref.scale.view(torch.int32)), f"scale region differs: {what}"
    if not torch.equal(packed.q_raw, ref.q_raw):
        bad = (packed.q != ref.q).nonzero()
        raise AssertionError(f"q region differs: {what}: {bad.shape[0]} bytes, first (row, k) {bad[:4].tolist()}")


@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("kind", SOURCES)
@pytest.mark.parametrize("k", KS)
def test_windows_that_cover_the_weight_reproduce_pack_b(qg, device, k, kind, dtype):
    _run(qg, device, _matrix(k, 40, 1, 0.3), _matrix(k, 40, 2), WINDOWS_40, kind, dtype)


@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("kind", SOURCES)
@pytest.mark.parametrize("k", (65, 200))
def test_windows_across_the_row_pad_boundary(qg, device, k, kind, dtype):
    _run(qg, device, _matrix(k, 300, 3, 0.3), _matrix(k, 300, 4), WINDOWS_300, kind, dtype)


@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("kind", SOURCES)
@pytest.mark.parametrize("k", (1, 65, 200))
def test_zero_column_nan_and_infinities(qg, device, k, kind, dtype):
    """A column of zeros (its scale is the seed's zero, every product NaN -> 0), a NaN (skipped by the absmax, packed
    as 0), +inf (scale inf, range / inf = 0) and -inf, as the seed row too (k = 1: every special is a seed), and a
    negative seed larger in magnitude than every candidate."""
    W = _matrix(k, 40, 5)
    W[:, 2] = 0.0
    W[:, 12] = -0.0
    W[5 % k, 7] = float("nan")
    W[k - 1, 20] = float("inf")
    W[0, 33] = float("-inf")
    W[k // 2, 34] = float("-inf")
    W[0, 36] = -100.0
    _run(qg, device, _matrix(k, 40, 6, 0.3), W, WINDOWS_40, kind, dtype)


@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("kind", SOURCES)
def test_range_100_saturates_as_pack_b(qg, device, kind, dtype):
    """range 100, with a negative seed far larger in magnitude than its column's candidates: Cw is the candidates'
    maximum (the signed seed loses the comparison), so seed * (100 / Cw) leaves int8 and saturates, as pack_b's does."""
    W = _matrix(65, 40, 7)
    W[0, 9] = -64.0
    W[0, 37] = -512.0
    _run(qg, device, _matrix(65, 40, 8, 0.3), W, WINDOWS_40, kind, dtype, range_=100.0)


@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("kind", SOURCES)
@pytest.mark.parametrize("k,c0", [(65, 7), (200, 16), (16384, 39)])
def test_one_column_window_leaves_the_rest(qg, device, k, c0, kind, dtype):
    """One column replaced (k = 16384: the longest k of the envelope): the other 39 stay the pre-fill's."""
    _run(qg, device, _matrix(k, 40, 9, 0.3), _matrix(k, 40, 10), ((c0, 1),), kind, dtype)
