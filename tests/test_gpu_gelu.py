"""qgemm_gelu_rows on the device against tests/standard_oracle.py bit for bit, and qgemm_gelu_pack_a against
qgemm_pack_a(gelu_rows(X)) byte for byte over the scale and q regions."""
import numpy as np
import pytest
import torch

import standard_oracle as SO
from util import assert_bits_equal

pytestmark = pytest.mark.gpu
F = np.float32
KS = [1, 15, 64, 65, 200, 4096, 16384]


def _x(m, k, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m, k)) * 3.0 + 0.5).astype(F)


def _poisoned(qg, m, k, device):
    return qg.Packed(torch.full((qg.load().qgemm_packed_size(m, k),), 0xA5, dtype=torch.uint8, device=device), m, k,
                     qg.DEFAULT_RANGE)


def _check(qg, device, Xd, want, what, range_=None):
    """gelu_rows == the oracle; gelu_pack_a == pack_a(gelu_rows), on a pre-poisoned buffer."""
    range_ = qg.DEFAULT_RANGE if range_ is None else range_
    G = qg.gelu_rows(Xd)
    assert_bits_equal(G.cpu().numpy(), want, f"{what}: gelu_rows")
    m, k = Xd.shape
    got = qg.gelu_pack_a(Xd, range=range_, out=_poisoned(qg, m, k, device))
    ref = qg.pack_a(G, range=range_)
    torch.cuda.synchronize()
    assert_bits_equal(got.scale.cpu().numpy(), ref.scale.cpu().numpy(), f"{what}: scale")
    assert torch.equal(got.q_raw, ref.q_raw), f"{what}: packed bytes differ from pack_a(gelu_rows(X))"
    return G


@pytest.mark.parametrize("m", [1, 7, 33])
@pytest.mark.parametrize("k", KS)
def test_gelu_matches_oracle(qg, device, k, m):
    X = _x(m, k, 10 * k + m)
    _check(qg, device, torch.from_numpy(X).to(device), SO.gelu_rows(X), f"m={m} k={k}")


@pytest.mark.parametrize("k,stride", [(15, 17), (64, 96), (200, 203), (4096, 4100)])
def test_strided_rows(qg, device, k, stride):
    """A row stride that keeps every row 16-byte aligned (96, 4100) and one that does not (17, 203)."""
    X = _x(7, stride, 3 * k)
    Xd = torch.from_numpy(X).to(device)[:, :k]
    assert Xd.stride(0) == stride
    G = _check(qg, device, Xd, SO.gelu_rows(X[:, :k]), f"k={k} stride={stride}")
    # and a strided destination
    Y = torch.zeros((7, stride), dtype=torch.float32, device=device)
    qg.gelu_rows(Xd, Y=Y[:, :k])
    assert torch.equal(Y[:, :k], G) and not Y[:, k:].any()


@pytest.mark.parametrize("k", [15, 200, 4096])
def test_negative_first_element_seeds_the_absmax(qg, device, k):
    """The seed quirk on the GELU'd values: the SIGNED first element starts the maximum and the candidates are
    magnitudes, so a negative first element loses to every candidate however small.  Row 0: g[0] = -0.17 (GELU's
    minimum, at x = -0.75) is the row's largest magnitude, the rest are gelu(-3.5) = -8e-4: Cx = 8e-4 and g[0]
    saturates at -128.  Row 1: the same with one large positive element, Cx = gelu(2).  Row 2: x[0] = +0.75 wins as
    itself."""
    X = np.full((3, k), -3.5, F)
    X[:2, 0] = -0.75
    X[2, 0] = 0.75
    X[1, k // 2] = 2.0
    Xd = torch.from_numpy(X).to(device)
    _check(qg, device, Xd, SO.gelu_rows(X), f"seed k={k}")
    packed = qg.gelu_pack_a(Xd)
    scale = packed.scale.cpu().numpy()
    g = SO.gelu_rows(X)
    assert abs(g[0, 0]) > 100 * abs(g[0, 1])
    assert scale[0] == -g[0, 1] and scale[1] == g[1, k // 2] and scale[2] == g[2, 0]
    assert int(packed.q[0, 0]) == -128


@pytest.mark.parametrize("k", [8, 200])
def test_special_values(qg, device, k):
    X = _x(6, k, 91)
    X[0, :8] = [np.nan, 1.0, np.inf, -np.inf, -0.0, 0.0, 100.0, -100.0]
    X[1, 0] = np.nan     # a NaN seed sticks
    X[2, 0] = -0.0
    X[3, 1] = np.inf
    X[4] = np.linspace(-100.0, 100.0, k, dtype=F)
    X[5] = -np.abs(X[5]) * F(30.0)
    want = SO.gelu_rows(X)
    assert np.isnan(want[0, 0]) and np.isnan(want[0, 3]) and want[0, 2] == np.inf
    assert want[0, 4] == 0 and np.signbit(want[0, 4]) and want[0, 7] == 0 and np.signbit(want[0, 7])
    _check(qg, device, torch.from_numpy(X).to(device), want, f"special k={k}")


@pytest.mark.parametrize("m,k", [(7, 65), (33, 4096)])
def test_range_100(qg, device, m, k):
    X = _x(m, k, 5 * k)
    _check(qg, device, torch.from_numpy(X).to(device), SO.gelu_rows(X), f"range 100 m={m} k={k}", range_=100.0)
