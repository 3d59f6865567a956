"""qgemm_rmsnorm_rows / qgemm_rmsnorm_pack_a / qgemm_prenorm_rms_pack_a on the device: Y and S against
tests/gated_oracle.py bit for bit, the packed views against qgemm_pack_a of the kernel's own Y byte for byte on
pre-poisoned buffers, padding rows and columns included.  The widths stand on both sides of every edge of the kernel's
three register budgets (1024, 2048, 4096 floats) and of its float4 column (w % 4)."""
import numpy as np
import pytest
import torch

import gated_oracle as GO
from util import assert_bits_equal

pytestmark = pytest.mark.gpu
F = np.float32
WIDTHS = [1, 3, 4, 255, 256, 260, 1024, 1028, 2048, 2052, 4096]


def _case(rows, w, seed):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((rows, w)) * 3.0 + 0.5).astype(F)
    B = rng.standard_normal((rows, w)).astype(F)
    gamma = (1.0 + 0.2 * rng.standard_normal(w)).astype(F)
    return A, B, gamma


def _dev(a, device, misalign=False):
    """The array on the device; misalign: its base pointer one float past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if not misalign:
        return t
    big = torch.empty(t.numel() + 1, dtype=torch.float32, device=device)
    view = big[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _poisoned(qg, rows, w, device, range_):
    return qg.Packed(torch.full((qg.load().qgemm_packed_size(rows, w),), 0xA5, dtype=torch.uint8, device=device), rows, w,
                     range_)


def _sum(A, B):
    with np.errstate(all="ignore"):
        return A.copy() if B is None else A + B


def _same_pack(packed, want, what):
    torch.cuda.synchronize()
    assert_bits_equal(packed.scale.cpu().numpy(), want.scale.cpu().numpy(), f"{what}: scale")
    assert torch.equal(packed.q_raw, want.q_raw), f"{what}: packed bytes differ from pack_a(rmsnorm_rows(A, B))"


def _run(qg, device, A, B, gamma, eps, what, misalign=False, want=None, ranges=(127.0,)):
    """The three entry points on one case: rows against the oracle, both pack forms against pack_a of the rows."""
    rows, w = A.shape
    Ad, gd = _dev(A, device, misalign), _dev(gamma, device)
    Bd = None if B is None else _dev(B, device)
    want = GO.rmsnorm_rows(A, B, gamma, eps) if want is None else want
    Y = qg.rmsnorm_rows(Ad, Bd, gd, eps, Y=torch.full((rows, w), float("nan"), device=device))
    assert_bits_equal(Y.cpu().numpy(), want, f"{what}: rmsnorm_rows")
    for r in ranges:
        ref = qg.pack_a(Y, range=r)
        Y2, packed = qg.rmsnorm_pack_a(Ad, Bd, gd, eps, range=r, out=_poisoned(qg, rows, w, device, r))
        assert_bits_equal(Y2.cpu().numpy(), want, f"{what}: rmsnorm_pack_a's Y")
        _same_pack(packed, ref, f"{what}: rmsnorm_pack_a range {r}")
        Sd = torch.full((rows, w), float("nan"), device=device)
        S, packed = qg.prenorm_rms_pack_a(Ad, Bd, gd, eps, S=Sd, range=r, out=_poisoned(qg, rows, w, device, r))
        assert S is Sd
        _same_pack(packed, ref, f"{what}: prenorm_rms_pack_a range {r}")
        assert_bits_equal(Sd.cpu().numpy(), _sum(A, B), f"{what}: S")
    assert_bits_equal(Ad.cpu().numpy(), A, f"{what}: A is left alone")
    return want


@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("w", WIDTHS)
def test_rmsnorm_matches_oracle(qg, device, w, rows):
    """The register path where w % 4 == 0 and the fallback elsewhere; 5 and 9 rows leave a partial block of the four
    rows per workgroup; B given and NULL; ranges 127 and 100."""
    A, B, gamma = _case(rows, w, 1000 * w + rows)
    _run(qg, device, A, B, gamma, 1e-5, f"w={w} rows={rows}", ranges=(127.0, 100.0))
    _run(qg, device, A, None, gamma, 1e-5, f"w={w} rows={rows} B=None")


@pytest.mark.parametrize("w", [4, 256, 1024, 1028, 2052, 4096])
def test_misaligned_base_takes_the_fallback_with_the_same_bits(qg, device, w):
    A, B, gamma = _case(5, w, 77 + w)
    want = _run(qg, device, A, B, gamma, 1e-5, f"aligned w={w}")
    _run(qg, device, A, B, gamma, 1e-5, f"misaligned w={w}", misalign=True, want=want)
    # a misaligned S alone sends the norm-first form down the fallback
    Sd = _dev(np.full_like(A, np.nan), device, True)
    _, packed = qg.prenorm_rms_pack_a(_dev(A, device), _dev(B, device), _dev(gamma, device), 1e-5, S=Sd)
    _same_pack(packed, qg.pack_a(_dev(want, device)), f"misaligned S w={w}")
    assert_bits_equal(Sd.cpu().numpy(), A + B, "misaligned S")


@pytest.mark.parametrize("w", [255, 1024])
@pytest.mark.parametrize("alias", ["A", "B"])
def test_outputs_may_alias_an_input(qg, device, w, alias):
    A, B, gamma = _case(9, w, 500 + w)
    want = GO.rmsnorm_rows(A, B, gamma, 1e-5)
    ref = qg.pack_a(_dev(want, device))
    for form in ("rows", "pack", "pre", "pre-none"):
        Ad, Bd, gd = (_dev(a, device) for a in (A, B, gamma))
        out = Ad if alias == "A" else Bd
        if form == "rows":
            qg.rmsnorm_rows(Ad, Bd, gd, 1e-5, Y=out)
        elif form == "pack":
            _, packed = qg.rmsnorm_pack_a(Ad, Bd, gd, 1e-5, Y=out)
            _same_pack(packed, ref, f"Y is {alias}")
        else:
            _, packed = qg.prenorm_rms_pack_a(Ad, Bd, gd, 1e-5, S=None if form == "pre-none" else out)
            _same_pack(packed, ref, f"{form}, S is {alias}")
        if form == "pre-none":
            assert_bits_equal(Ad.cpu().numpy(), A, "S = None: A is left alone")
            assert_bits_equal(Bd.cpu().numpy(), B, "S = None: B is left alone")
        else:
            assert_bits_equal(out.cpu().numpy(), A + B if form == "pre" else want, f"{form}: output over {alias}")


@pytest.mark.parametrize("w", [5, 256])
def test_zero_row_with_eps_zero(qg, device, w):
    """ms = 0, r = 1 / sqrt(0) = inf, 0 * inf = NaN -- what the operations give; with an eps the row is zeros."""
    A, B, gamma = _case(3, w, 600 + w)
    A[1], B[1] = F(1.5), F(-1.5)
    want = _run(qg, device, A, B, gamma, 0.0, f"zero row eps=0 w={w}")
    assert np.isnan(want[1]).all()
    want = _run(qg, device, A, B, gamma, 1e-5, f"zero row w={w}")
    assert not want[1].any()


@pytest.mark.parametrize("w", [7, 1024])
def test_non_finite_values(qg, device, w):
    A, B, gamma = _case(6, w, 700 + w)
    A[0, w // 2] = np.nan
    A[1, 0] = np.inf
    B[1, 0] = -np.inf     # inf - inf: S itself holds a NaN
    A[2, w - 1] = -np.inf
    B[3, 1] = np.inf
    _run(qg, device, A, B, gamma, 1e-5, "NaN / inf in the row")
    A, B, gamma = _case(6, w, 800 + w)
    gamma[0], gamma[w - 1] = np.nan, np.inf
    _run(qg, device, A, B, gamma, 1e-5, "NaN / inf in gamma")


@pytest.mark.parametrize("w", [3, 260, 2048])
def test_rows_beside_the_call_and_past_the_view_are_untouched(qg, device, w):
    rows = 5
    A, B, gamma = _case(rows, w, 900 + w)
    ref = qg.pack_a(_dev(GO.rmsnorm_rows(A, B, gamma, 1e-5), device))
    Ap, Bp, Sp = (torch.full((9, w), float("nan"), device=device) for _ in range(3))
    Ap[2:7].copy_(_dev(A, device))
    Bp[2:7].copy_(_dev(B, device))
    nbytes, guard = qg.load().qgemm_packed_size(rows, w), 256
    big = torch.full((nbytes + 2 * guard,), 0x5A, dtype=torch.uint8, device=device)
    out = qg.Packed(big[guard:guard + nbytes], rows, w, qg.DEFAULT_RANGE)
    _, packed = qg.prenorm_rms_pack_a(Ap[2:7], Bp[2:7], _dev(gamma, device), 1e-5, S=Sp[2:7], out=out)
    _same_pack(packed, ref, f"embedded w={w}")
    assert_bits_equal(Sp[2:7].cpu().numpy(), A + B, "S's rows")
    for t, nm in ((Sp, "S"), (Ap, "A"), (Bp, "B")):
        assert torch.isnan(torch.cat([t[:2], t[7:]])).all(), f"rows beside {nm} were written"
    assert (big[:guard] == 0x5A).all() and (big[guard + nbytes:] == 0x5A).all(), "bytes past the packed view were written"
