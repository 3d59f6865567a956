"""GPU parity of qgemm_logsumexp_rows against tests/beam_oracle.py, bit for bit.  S is a window of a NaN-filled parent
(a base 4 bytes off a 16-byte boundary and an odd row stride, so that the scalar head, the float4 body and the scalar
tail of a block's loads all run and nothing outside a row may be read).  Widths: below, at and above one 1024-column
tree block, several blocks with a ragged last one, and the two split plans (8200: 2 parts, 36877: many parts with a
short last part); row counts on both sides of the plan's 256-row threshold."""
import functools

import numpy as np
import pytest
import torch

import beam_oracle as BO
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

NAN, INF = np.float32("nan"), np.float32("inf")
WIDTHS = (1, 2, 1023, 1024, 1025, 2049, 4099, 8200, 36877)
SHAPES = [(3, w) for w in WIDTHS] + [(1, 1024), (1, 8200), (1, 36877), (32, 1025), (32, 8200), (32, 36877),
                                     (300, 1), (300, 1025), (300, 4099)]


def _window(rows_np, device):
    """The rows as a window of a NaN-filled device parent: (parent, view)."""
    rows, w = rows_np.shape
    stride = w + 3 if (w + 3) % 2 else w + 4
    parent = torch.full((1 + rows * stride + 7,), float("nan"), device=device)
    view = torch.as_strided(parent, (rows, w), (stride, 1), storage_offset=1)
    view.copy_(torch.from_numpy(np.array(rows_np)))
    assert view.data_ptr() % 16 == 4 and stride % 2 == 1
    return parent, view


def _check(qg, device, S, what):
    want = BO.logsumexp_rows_ref(S)
    parent, view = _window(S, device)
    before = parent.clone()
    mx, logz = qg.logsumexp_rows(view)
    torch.cuda.synchronize()
    assert_bits_equal(mx.cpu().numpy(), want[0], f"{what}: mx")
    assert_bits_equal(logz.cpu().numpy(), want[1], f"{what}: logz")
    assert torch.equal(parent.view(torch.int32), before.view(torch.int32)), f"{what}: S is const"
    return mx, logz


@pytest.mark.parametrize("rows,w", SHAPES)
def test_random_rows(qg, oracle, device, rows, w):
    if w in (8200, 36877) and rows <= 32:
        assert qg.logsumexp_rows_plan(rows, w) > 1, "the split plan"
    else:
        assert qg.logsumexp_rows_plan(rows, w) == 1
    _check(qg, device, O.uniform((rows, w), 900 + rows + w, -8.0, 8.0), f"{rows} x {w}")


@functools.lru_cache(maxsize=None)
def _value_cases(w):
    """One row per case (read-only)."""
    rng = np.random.default_rng(w)
    base = O.uniform((9, w), 950 + w, -8.0, 8.0)
    S = base.copy()
    S[1] = O.uniform((w,), 951 + w, -200.0, 0.0)                       # e goes subnormal and reaches +0
    S[2] = 1.25                                                        # all columns equal
    S[3] = -INF
    S[3, w // 2] = 3.0                                                 # one candidate: logz = +0
    S[4, rng.random(w) < 0.3] = -INF                                   # planted -inf
    S[5, rng.random(w) < 0.3] = NAN
    S[5, 0] = NAN                                                      # NaN, also at column 0
    S[6, [w // 3, w - 1]] = INF                                        # +inf: logz NaN
    S[7] = NAN
    S[7, ::2] = -INF                                                   # no candidate
    S[8, [0, w - 1]] = 8.0                                             # the maximum at both ends, twice
    S.flags.writeable = False
    return S


@pytest.mark.parametrize("w", [1, 5, 1025, 4099, 8200])
def test_value_cases(qg, oracle, device, w):
    S = _value_cases(w)
    mx, logz = _check(qg, device, S, f"value cases at {w}")
    mx, logz = mx.cpu().numpy(), logz.cpu().numpy()
    assert mx[3] == 3 and logz[3].view(np.uint32) == 0
    assert np.isnan(logz[6]) and mx[6] == INF
    assert mx[7] == -INF and logz[7] == -INF


def test_one_row_alone_and_among_300(qg, oracle, device):
    """The split plan of one row (w 8200: two parts) and the unsplit plan of 300 rows give the same bits."""
    w = 8200
    many = O.uniform((300, w), 977, -8.0, 8.0)
    assert qg.logsumexp_rows_plan(1, w) > 1 and qg.logsumexp_rows_plan(300, w) == 1
    _, one = _window(many[5:6], device)
    _, all_ = _window(many, device)
    a, b = qg.logsumexp_rows(one), qg.logsumexp_rows(all_)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y[5:6].view(torch.int32))
    want = BO.logsumexp_rows_ref(many[:8])
    assert_bits_equal(b[0][:8].cpu().numpy(), want[0], "mx")
    assert_bits_equal(b[1][:8].cpu().numpy(), want[1], "logz")
