"""qgemm_prenorm_pack_a / qgemm_add_rows on the device: S against fl32(A + B) bit for bit, the packed
view against qgemm_pack_a of qgemm_layernorm_rows' own Y byte for byte on a pre-poisoned buffer -- the post-LN kernel
that tests/test_gpu_layernorm_std.py holds against tests/standard_oracle.py -- and against the oracle's LN itself."""
import numpy as np
import pytest
import torch

import standard_oracle as SO
from test_gpu_layernorm_std import WIDTHS, _case, _dev, _poisoned
from util import assert_bits_equal

pytestmark = pytest.mark.gpu
F = np.float32


def _sum(A, B):
    with np.errstate(all="ignore"):
        return A.copy() if B is None else A + B


def _want_pack(qg, device, A, B, gamma, beta, eps):
    """pack_a(layernorm_rows(A, B, ..)) from the post-LN kernel on aligned copies, whose Y is the oracle's bit for bit."""
    Y = qg.layernorm_rows(_dev(A, device), None if B is None else _dev(B, device), _dev(gamma, device),
                          _dev(beta, device), eps)
    assert_bits_equal(Y.cpu().numpy(), SO.layernorm_rows(A, B, gamma, beta, eps), "layernorm_rows against the oracle")
    want = qg.pack_a(Y)
    torch.cuda.synchronize()
    return want


def _check_pack(packed, want, what):
    torch.cuda.synchronize()
    assert_bits_equal(packed.scale.cpu().numpy(), want.scale.cpu().numpy(), f"{what}: scale")
    assert torch.equal(packed.q_raw, want.q_raw), f"{what}: packed bytes differ from pack_a(layernorm_rows(A, B))"


def _run(qg, device, A, B, gamma, beta, eps, what, want=None, mis_a=False, mis_s=False, s_is=None):
    """One call with S = a NaN-filled buffer of its own (s_is None), A or B ("A" / "B"), or no S at all ("none")."""
    rows, w = A.shape
    Ad, gd, bd = _dev(A, device, mis_a), _dev(gamma, device), _dev(beta, device)
    Bd = None if B is None else _dev(B, device)
    Sd = {None: _dev(np.full((rows, w), np.nan, F), device, mis_s), "A": Ad, "B": Bd, "none": None}[s_is]
    want = _want_pack(qg, device, A, B, gamma, beta, eps) if want is None else want
    S, packed = qg.prenorm_pack_a(Ad, Bd, gd, bd, eps, S=Sd, out=_poisoned(qg, rows, w, device))
    _check_pack(packed, want, what)
    if Sd is not None:
        assert S is Sd
        assert_bits_equal(Sd.cpu().numpy(), _sum(A, B), f"{what}: S")
    if s_is != "A":
        assert_bits_equal(Ad.cpu().numpy(), A, f"{what}: A is left alone")
    return want


@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("w", WIDTHS)
def test_prenorm_matches_the_post_ln_kernel(qg, device, w, rows):
    """The register path where w % 4 == 0, the fallback elsewhere; S aliasing A, S aliasing B and no S give the same
    packed bytes; padding rows and columns of the packed view on a 0x5A-poisoned buffer."""
    A, B, gamma, beta = _case(rows, w, 1000 * w + rows)
    want = _run(qg, device, A, B, gamma, beta, 1e-5, f"w={w} rows={rows}")
    for s_is in ("A", "B", "none"):
        _run(qg, device, A, B, gamma, beta, 1e-5, f"w={w} rows={rows} S={s_is}", want=want, s_is=s_is)


@pytest.mark.parametrize("w", [3, 4, 64, 257, 1024, 2048, 4096])
def test_without_b(qg, device, w):
    A, _, gamma, beta = _case(5, w, 300 + w)
    want = _run(qg, device, A, None, gamma, beta, 1e-5, f"B=None w={w}")          # S = A, a copy
    _run(qg, device, A, None, gamma, beta, 1e-5, f"B=None S=None w={w}", want=want, s_is="none")
    _run(qg, device, A, None, gamma, beta, 1e-5, f"B=None S=A w={w}", want=want, s_is="A")


@pytest.mark.parametrize("w", [4, 64, 1024, 1028, 4096])
def test_misaligned_base_takes_the_fallback_with_the_same_bits(qg, device, w):
    A, B, gamma, beta = _case(5, w, 77 + w)
    want = _run(qg, device, A, B, gamma, beta, 1e-5, f"aligned w={w}")
    _run(qg, device, A, B, gamma, beta, 1e-5, f"misaligned A w={w}", want=want, mis_a=True)
    _run(qg, device, A, B, gamma, beta, 1e-5, f"misaligned S w={w}", want=want, mis_s=True)
    # add_rows through the same two paths
    for mis_a, mis_s in ((True, False), (False, True)):
        S = qg.add_rows(_dev(A, device, mis_a), _dev(B, device), S=_dev(np.zeros_like(A), device, mis_s))
        assert_bits_equal(S.cpu().numpy(), A + B, f"add_rows misaligned {'A' if mis_a else 'S'} w={w}")


@pytest.mark.parametrize("w", [7, 1024])
def test_non_finite_values(qg, device, w):
    A, B, gamma, beta = _case(6, w, 700 + w)
    A[0, w // 2] = np.nan
    A[1, 0] = np.inf
    B[1, 0] = -np.inf     # inf - inf: S itself holds a NaN
    A[2, w - 1] = -np.inf
    B[3, 1] = np.inf
    _run(qg, device, A, B, gamma, beta, 1e-5, "NaN / inf in the row")
    _run(qg, device, A, B, gamma, beta, 1e-5, "NaN / inf in the row, S = B", s_is="B")
    S = qg.add_rows(_dev(A, device), _dev(B, device))
    assert_bits_equal(S.cpu().numpy(), _sum(A, B), "add_rows with NaN / inf")


@pytest.mark.parametrize("w", [5, 256])
def test_constant_row_with_eps_zero(qg, device, w):
    """d = 0, rstd = inf, 0 * inf = NaN -- what the operations give; S is the constant."""
    A, B, gamma, beta = _case(3, w, 600 + w)
    A[1], B[1] = F(1.5), F(0.25)
    assert np.isnan(SO.layernorm_rows(A, B, gamma, beta, 0.0)[1]).all()
    _run(qg, device, A, B, gamma, beta, 0.0, f"constant row eps=0 w={w}")


@pytest.mark.parametrize("w", [3, 100, 1024, 2048])
def test_rows_beside_s_and_past_the_view_are_untouched(qg, device, w):
    """A, B and S are rows 2 .. 6 of NaN-filled parents of 9 rows; the packed view sits between NaN-filled guard
    bytes: nothing outside the 5 rows of S and the view's own bytes changes."""
    rows = 5
    A, B, gamma, beta = _case(rows, w, 900 + w)
    want = _want_pack(qg, device, A, B, gamma, beta, 1e-5)
    parents = [torch.full((9, w), float("nan"), device=device) for _ in range(3)]
    Ap, Bp, Sp = parents
    Ap[2:7].copy_(_dev(A, device))
    Bp[2:7].copy_(_dev(B, device))
    nbytes = qg.load().qgemm_packed_size(rows, w)
    guard = 256
    big = torch.full((nbytes + 2 * guard,), 0x5A, dtype=torch.uint8, device=device)
    out = qg.Packed(big[guard:guard + nbytes], rows, w, qg.DEFAULT_RANGE)
    _, packed = qg.prenorm_pack_a(Ap[2:7], Bp[2:7], _dev(gamma, device), _dev(beta, device), 1e-5, S=Sp[2:7], out=out)
    _check_pack(packed, want, f"embedded w={w}")
    assert_bits_equal(Sp[2:7].cpu().numpy(), A + B, "S's rows")
    for t, nm in ((Sp, "S"), (Ap, "A"), (Bp, "B")):
        outside = torch.cat([t[:2], t[7:]])
        assert torch.isnan(outside).all(), f"rows beside {nm} were written"
    assert_bits_equal(Ap[2:7].cpu().numpy(), A, "A's rows")
    assert (big[:guard] == 0x5A).all() and (big[guard + nbytes:] == 0x5A).all(), "bytes past the packed view were written"
    # add_rows in the same parents, in place over A's rows
    qg.add_rows(Ap[2:7], Bp[2:7], S=Ap[2:7])
    assert_bits_equal(Ap[2:7].cpu().numpy(), A + B, "add_rows in place")
    assert torch.isnan(torch.cat([Ap[:2], Ap[7:]])).all(), "add_rows wrote beside its rows"


@pytest.mark.parametrize("rows", [1, 9])
@pytest.mark.parametrize("w", WIDTHS)
def test_add_rows(qg, device, w, rows):
    A, B, _, _ = _case(rows, w, 2000 * w + rows)
    Ad, Bd = _dev(A, device), _dev(B, device)
    S = qg.add_rows(Ad, Bd, S=torch.full((rows, w), float("nan"), device=device))
    assert_bits_equal(S.cpu().numpy(), A + B, f"add_rows w={w} rows={rows}")
    assert_bits_equal(Ad.cpu().numpy(), A, "A is left alone")
    assert qg.add_rows(Ad, Bd, S=Ad) is Ad                      # S aliasing A
    assert_bits_equal(Ad.cpu().numpy(), A + B, f"add_rows in place w={w} rows={rows}")
    assert_bits_equal(Bd.cpu().numpy(), B, "B is left alone")
