"""qgemm_layernorm_rows / qgemm_layernorm_pack_a on the device against tests/standard_oracle.py bit for bit, and the
fused pack against qgemm_pack_a of the kernel's own Y byte for byte."""
import numpy as np
import pytest
import torch

import standard_oracle as SO
from util import assert_bits_equal

pytestmark = pytest.mark.gpu
F = np.float32
WIDTHS = [1, 3, 4, 64, 100, 257, 1024, 1028, 2048, 4096]


def _case(rows, w, seed):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((rows, w)) * 3.0 + 0.5).astype(F)
    B = rng.standard_normal((rows, w)).astype(F)
    gamma = (1.0 + 0.2 * rng.standard_normal(w)).astype(F)
    beta = (0.2 * rng.standard_normal(w)).astype(F)
    return A, B, gamma, beta


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


def _poisoned(qg, rows, w, device):
    p = qg.Packed(torch.full((qg.load().qgemm_packed_size(rows, w),), 0x5A, dtype=torch.uint8, device=device), rows, w,
                  qg.DEFAULT_RANGE)
    return p


def _check_pack(qg, Yd, packed, what):
    """The scale and q regions equal pack_a(Y)'s, padding rows and columns included."""
    want = qg.pack_a(Yd)
    torch.cuda.synchronize()
    assert_bits_equal(packed.scale.cpu().numpy(), want.scale.cpu().numpy(), f"{what}: scale")
    assert torch.equal(packed.q_raw, want.q_raw), f"{what}: packed bytes differ from pack_a(Y)"


def _run_both(qg, device, A, B, gamma, beta, eps, what, misalign=False, want=None):
    Ad, gd, bd = _dev(A, device, misalign), _dev(gamma, device), _dev(beta, device)
    Bd = None if B is None else _dev(B, device)
    want = SO.layernorm_rows(A, B, gamma, beta, eps) if want is None else want
    Y = qg.layernorm_rows(Ad, Bd, gd, bd, eps)
    assert_bits_equal(Y.cpu().numpy(), want, f"{what}: layernorm_rows")
    rows, w = A.shape
    Y2, packed = qg.layernorm_pack_a(Ad, Bd, gd, bd, eps, out=_poisoned(qg, rows, w, device))
    assert_bits_equal(Y2.cpu().numpy(), want, f"{what}: layernorm_pack_a's Y")
    _check_pack(qg, Y2, packed, what)
    return want


@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("w", WIDTHS)
def test_layernorm_matches_oracle(qg, device, w, rows):
    """Every width takes the register path where w % 4 == 0 and the fallback elsewhere; rows that are no multiple of
    16 leave padding rows in the packed view, checked on a pre-poisoned buffer."""
    A, B, gamma, beta = _case(rows, w, 1000 * w + rows)
    _run_both(qg, device, A, B, gamma, beta, 1e-5, f"w={w} rows={rows}")


@pytest.mark.parametrize("w", [4, 64, 1024, 1028, 4096])
def test_misaligned_base_takes_the_fallback_with_the_same_bits(qg, device, w):
    A, B, gamma, beta = _case(5, w, 77 + w)
    want = _run_both(qg, device, A, B, gamma, beta, 1e-5, f"aligned w={w}")
    _run_both(qg, device, A, B, gamma, beta, 1e-5, f"misaligned w={w}", misalign=True, want=want)


@pytest.mark.parametrize("w", [3, 64, 257, 2048])
def test_without_b(qg, device, w):
    A, _, gamma, beta = _case(5, w, 300 + w)
    _run_both(qg, device, A, None, gamma, beta, 1e-5, f"B=None w={w}")


@pytest.mark.parametrize("w", [100, 1024])
@pytest.mark.parametrize("alias", ["A", "B"])
def test_output_may_alias_an_input(qg, device, w, alias):
    A, B, gamma, beta = _case(9, w, 500 + w)
    want = SO.layernorm_rows(A, B, gamma, beta, 1e-5)
    for pack in (False, True):
        Ad, Bd, gd, bd = (_dev(a, device) for a in (A, B, gamma, beta))
        Yd = Ad if alias == "A" else Bd
        if pack:
            _, packed = qg.layernorm_pack_a(Ad, Bd, gd, bd, 1e-5, Y=Yd)
            _check_pack(qg, Yd, packed, f"Y is {alias}")
        else:
            qg.layernorm_rows(Ad, Bd, gd, bd, 1e-5, Y=Yd)
        assert_bits_equal(Yd.cpu().numpy(), want, f"Y is {alias}, pack={pack}")


@pytest.mark.parametrize("eps", [1e-5, 0.0])
@pytest.mark.parametrize("w", [5, 256])
def test_constant_row(qg, device, w, eps):
    """eps = 0 on a constant row: d = 0, rstd = inf, 0 * inf = NaN -- what the operations give."""
    A, B, gamma, beta = _case(3, w, 600 + w)
    A[1], B[1] = F(1.5), F(0.25)
    want = _run_both(qg, device, A, B, gamma, beta, eps, f"constant row eps={eps}")
    if eps == 0.0:
        assert np.isnan(want[1]).all()
    else:
        assert_bits_equal(want[1], beta + F(0.0) * gamma, "constant row: beta")


@pytest.mark.parametrize("w", [7, 1024])
def test_non_finite_values(qg, device, w):
    A, B, gamma, beta = _case(6, w, 700 + w)
    A[0, w // 2] = np.nan
    A[1, 0] = np.inf
    A[2, w - 1] = -np.inf
    _run_both(qg, device, A, B, gamma, beta, 1e-5, "NaN / inf in the row")
    A, B, gamma, beta = _case(6, w, 800 + w)
    gamma[0], gamma[w - 1] = np.nan, np.inf
    _run_both(qg, device, A, B, gamma, beta, 1e-5, "NaN / inf in gamma")
    A, B, gamma, beta = _case(6, w, 900 + w)
    beta[0], beta[w // 2] = -np.inf, np.nan
    _run_both(qg, device, A, B, gamma, beta, 1e-5, "NaN / inf in beta")
