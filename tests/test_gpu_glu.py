"""qgemm_glu_rows on the device against tests/gated_oracle.py bit for bit, and qgemm_glu_pack_a against
qgemm_pack_a(glu_rows(X)) byte for byte over the scale and q regions, for the three activations.  A row
of X is [gate: k | up: k]; the ks stand on both sides of the pack's register budgets (1024, 4096, 16384 floats) and of
its float4 column (k % 4)."""
import numpy as np
import pytest
import torch

import gated_oracle as GO
from util import assert_bits_equal

pytestmark = pytest.mark.gpu
F = np.float32
KS = [1, 15, 64, 65, 200, 1024, 1028, 4096, 4100, 16384]
ACTS = list(GO.ACTIVATIONS)


def _x(m, k2, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m, k2)) * 3.0 + 0.5).astype(F)


def _poisoned(qg, m, k, device, range_):
    return qg.Packed(torch.full((qg.load().qgemm_packed_size(m, k),), 0xA5, dtype=torch.uint8, device=device), m, k, range_)


def _check(qg, device, Xd, want, act, what, range_=None):
    """glu_rows == the oracle; glu_pack_a == pack_a(glu_rows), on a pre-poisoned buffer."""
    range_ = qg.DEFAULT_RANGE if range_ is None else range_
    m, k = Xd.shape[0], Xd.shape[1] // 2
    G = qg.glu_rows(Xd, act, Y=torch.full((m, k), float("nan"), device=device))
    assert_bits_equal(G.cpu().numpy(), want, f"{what}: glu_rows")
    got = qg.glu_pack_a(Xd, act, range=range_, out=_poisoned(qg, m, k, device, range_))
    ref = qg.pack_a(G, range=range_)
    torch.cuda.synchronize()
    assert_bits_equal(got.scale.cpu().numpy(), ref.scale.cpu().numpy(), f"{what}: scale")
    assert torch.equal(got.q_raw, ref.q_raw), f"{what}: packed bytes differ from pack_a(glu_rows(X))"
    return G


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("m", [1, 7, 33])
@pytest.mark.parametrize("k", KS)
def test_glu_matches_oracle(qg, device, k, m, act):
    """Contiguous rows of 2k floats: an odd k on the aligned base leaves the gate aligned and the up half not."""
    X = _x(m, 2 * k, 10 * k + m)
    _check(qg, device, torch.from_numpy(X).to(device), GO.glu_rows(X, act), act, f"{act} m={m} k={k}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("k,pad", [(15, 8), (15, 1), (64, 8), (64, 1), (200, 8), (200, 1), (4096, 8), (4096, 1)])
def test_strided_rows(qg, device, k, pad, act):
    """A row stride that keeps every row 16-byte aligned (2k + 8) and one that does not (2k + 1)."""
    stride = 2 * k + pad
    X = _x(7, stride, 3 * k + pad)
    Xd = torch.from_numpy(X).to(device)[:, :2 * k]
    assert Xd.stride(0) == stride
    G = _check(qg, device, Xd, GO.glu_rows(X[:, :2 * k], act), act, f"{act} k={k} stride={stride}")
    # and a strided destination
    Y = torch.zeros((7, k + pad), dtype=torch.float32, device=device)
    qg.glu_rows(Xd, act, Y=Y[:, :k])
    assert torch.equal(Y[:, :k], G) and not Y[:, k:].any()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("k", [64, 1028])
def test_misaligned_base_gives_the_same_bits(qg, device, k, act):
    X = _x(5, 2 * k, 40 + k)
    big = torch.empty(X.size + 1, dtype=torch.float32, device=device)
    Xd = big[1:].view(X.shape)
    Xd.copy_(torch.from_numpy(X))
    assert Xd.data_ptr() % 16 == 4
    _check(qg, device, Xd, GO.glu_rows(X, act), act, f"{act} misaligned k={k}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("k", [15, 200, 4096])
def test_negative_first_element_seeds_the_absmax(qg, device, k, act):
    """The seed quirk on the PRODUCT: the signed h[0] starts the maximum and the candidates are magnitudes, so a negative
    first element loses to every candidate however small.  Every gate is 1 (act(1) > 0 for all three activations).
    Row 0: up[0] = -2 makes h[0] the row's largest magnitude, the rest are act(1) * 1e-3: Cx is that small value and
    h[0] saturates at -128.  Row 1: the same with one large positive element, which wins.  Row 2: up[0] = +2 wins as
    itself."""
    X = np.full((3, 2 * k), 1.0, F)
    X[:, k:] = F(1e-3)
    X[:2, k] = -2.0
    X[2, k] = 2.0
    X[1, k + k // 2] = 5.0
    Xd = torch.from_numpy(X).to(device)
    h = GO.glu_rows(X, act)
    _check(qg, device, Xd, h, act, f"{act} seed k={k}")
    packed = qg.glu_pack_a(Xd, act)
    scale = packed.scale.cpu().numpy()
    assert h[0, 0] < 0 and abs(h[0, 0]) > 100 * abs(h[0, 1])
    assert scale[0] == h[0, 1] and scale[1] == h[1, k // 2] and scale[2] == h[2, 0]
    assert int(packed.q[0, 0]) == -128


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("k", [8, 200])
def test_special_values(qg, device, k, act):
    """NaN, +-inf, +-0 and +-100 in the gate with ordinary ups, in up with ordinary gates, and in both."""
    special = np.array([np.nan, 1.0, np.inf, -np.inf, -0.0, 0.0, 100.0, -100.0], F)
    X = _x(7, 2 * k, 91)
    X[0, :8] = special                 # the gate
    X[1, k:k + 8] = special            # up
    X[2, :8] = special                 # both: inf * 0, -inf * -0, NaN * NaN ..
    X[2, k:k + 8] = special[::-1]
    X[3, 0] = np.nan                   # a NaN seed sticks
    X[4, k] = -0.0                     # a -0 seed
    X[5, :k] = np.linspace(-100.0, 100.0, k, dtype=F)
    X[6, :k] = -np.abs(X[6, :k]) * F(30.0)
    want = GO.glu_rows(X, act)
    assert np.isnan(want[0, 0]) and np.isnan(want[1, 0]) and np.isnan(want[3, 0])
    if act == "silu":
        assert np.isnan(want[0, 3])    # silu(-inf) = -inf / inf
    if act == "relu":
        assert want[0, 3] == 0         # relu(-inf) = 0, times a finite up
    _check(qg, device, torch.from_numpy(X).to(device), want, act, f"{act} special k={k}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("m,k", [(7, 65), (33, 4096)])
def test_range_100(qg, device, m, k, act):
    X = _x(m, 2 * k, 5 * k)
    _check(qg, device, torch.from_numpy(X).to(device), GO.glu_rows(X, act), act, f"{act} range 100 m={m} k={k}", range_=100.0)
