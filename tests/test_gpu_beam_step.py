"""GPU parity of qgemm_beam_step against tests/beam_oracle.py: parents, tokens and the bits of the scores.  Widths 97
(fewer columns than a workgroup has threads), 1000 (one workgroup per row) and 8200 (the selection and the log-sum-exp
both split in two, the selection's seam between columns 4099 and 4100).  The logits are windows of a NaN-filled parent
with a base off 16 bytes and an odd row stride."""
import numpy as np
import pytest
import torch

import beam_oracle as BO
import head_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

NAN, INF = np.float32("nan"), np.float32("inf")
SHAPES = [(1, 1), (1, 2), (2, 3), (4, 8), (8, 4)]
WIDTHS = (97, 1000, 8200)


def _window(rows_np, device):
    rows, w = rows_np.shape
    stride = w + 3 if (w + 3) % 2 else w + 4
    parent = torch.full((1 + rows * stride + 7,), float("nan"), device=device)
    view = torch.as_strided(parent, (rows, w), (stride, 1), storage_offset=1)
    view.copy_(torch.from_numpy(np.array(rows_np)))
    return view


def _dev(a, device, dtype):
    return None if a is None else torch.from_numpy(np.asarray(a, dtype)).to(device)


def _check(qg, device, S, beams, scores_in=None, prev=None, eos=-1, what=""):
    want = BO.beam_step_ref(S, beams, scores_in, prev, eos)
    got = qg.beam_step(_window(S, device), beams, _dev(scores_in, device, np.float32), _dev(prev, device, np.int32), eos)
    torch.cuda.synchronize()
    par, tok, sc = (t.cpu().numpy() for t in got)
    assert np.array_equal(par, want[0]), f"{what}: parents\n{par}\n{want[0]}"
    assert np.array_equal(tok, want[1]), f"{what}: tokens\n{tok}\n{want[1]}"
    assert_bits_equal(sc, want[2], f"{what}: scores")
    assert not np.isnan(sc).any()
    groups = sc.reshape(-1, beams)
    assert (groups[:, :-1] >= groups[:, 1:]).all(), f"{what}: scores_out is non-increasing within a group"
    return par, tok, sc


def _logits(rows, w, seed):
    S = O.uniform((rows, w), seed, -8.0, 8.0)
    rng = np.random.default_rng(seed)
    S[rng.integers(0, rows, 3 * rows), rng.integers(0, w, 3 * rows)] = NAN
    S[rng.integers(0, rows, 3 * rows), rng.integers(0, w, 3 * rows)] = -INF
    return S


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("groups,beams", SHAPES)
def test_random_states(qg, oracle, device, groups, beams, w):
    rows = groups * beams
    if w == 8200:
        assert qg.beam_step_plan(groups, beams, w) == (2, 2), "both launches split"
    else:
        assert qg.beam_step_plan(groups, beams, w) == (1, 1)
    S = _logits(rows, w, 1000 + 10 * rows + w)
    rng = np.random.default_rng(rows + w)
    _check(qg, device, S, beams, what="the start")                             # scores_in NULL
    scores = (-5 * rng.random(rows)).astype(np.float32)
    scores[rng.random(rows) < 0.2] = -INF                                      # dead beams
    eos = 7
    prev = rng.integers(0, w, rows).astype(np.int32)
    prev[rng.random(rows) < 0.3] = eos                                         # finished beams
    _check(qg, device, S, beams, scores, prev, eos, "a mixed state")
    _check(qg, device, S, beams, scores, prev, -1, "eos < 0")
    _check(qg, device, S, beams, scores, None, eos, "prev == NULL")


@pytest.mark.parametrize("w", WIDTHS)
def test_one_beam_is_the_argmax(qg, oracle, device, w):
    S = _logits(16, w, 1100 + w)
    S[:, 0] = np.where(np.isnan(S[:, 0]), np.float32(0.5), S[:, 0])            # column 0 is no NaN
    S[3, :] = 1.25
    S[4, w // 2:] = 9.0
    S[5, :] = -INF                                                             # no candidate: token 0, as the argmax
    par, tok, sc = _check(qg, device, S, 1, what="beams = 1")
    assert np.array_equal(tok, head_oracle.argmax_rows_ref(S)[0]) and not par.any()
    got = qg.argmax_rows(_window(S, device))[0]
    assert np.array_equal(got.cpu().numpy(), tok)


@pytest.mark.parametrize("w", WIDTHS)
def test_ties(qg, oracle, device, w):
    """Equal values across the beams-th place of a row, across the selection's part seam, between beams with identical
    rows and scores, and between candidates whose c rounds to the same value."""
    beams = 4
    seam = 4100 if w == 8200 else w // 2
    row = O.uniform((w,), 1200 + w, -8.0, 0.0)
    row[[seam - 1, seam, seam + 1, 2, w - 1, seam + 7]] = 5.0                   # six equal maxima: places 4 and 5 lose
    S = np.stack([row, row, O.uniform((w,), 1201 + w, -8.0, 8.0), row])
    par, tok, sc = _check(qg, device, S, beams, np.array([-1, -1, -1, -1], np.float32), what="identical beams")
    assert par.tolist() == [0, 0, 0, 0] and tok.tolist() == sorted([2, seam - 1, seam, seam + 1])
    par, tok, sc = _check(qg, device, S, beams, np.array([-1, -1, -30, -0.5], np.float32), what="the last beam leads")
    assert par.tolist() == [3, 3, 3, 3]
    big = np.full(4, -2.0 ** 25, np.float32)                                   # swallows every lp within half an ulp
    S2 = np.full((4, w), 1.0, np.float32)                                      # uniform rows: lp = -log w
    par, tok, sc = _check(qg, device, S2, beams, big, what="c rounds to equal values")
    assert par.tolist() == [0, 0, 0, 0] and tok.tolist() == [0, 1, 2, 3] and len(set(sc.tolist())) == 1


@pytest.mark.parametrize("w", WIDTHS)
def test_finished_dead_and_short_groups(qg, oracle, device, w):
    beams, eos = 2, 3
    S = _logits(8, w, 1300 + w)
    S[4] = NAN
    S[4, 5] = 2.0                                                              # group 2: one candidate in all
    S[5] = -INF
    S[6:8] = NAN                                                               # group 3: none
    scores = np.array([-1.0, -0.25, -1.0, -40.0, -2.0, -3.0, -1.0, -1.0], np.float32)
    prev = np.array([0, eos, 0, eos, 0, 0, 0, 0], np.int32)
    par, tok, sc = _check(qg, device, S, beams, scores, prev, eos, "held beams")
    assert (par[0], tok[0]) == (1, eos) and sc[0] == np.float32(-0.25)         # outranks: kept first, score frozen
    assert eos not in tok[2:4].tolist() or par[2:4].tolist() == [0, 0]         # outranked by beam 0's two candidates
    assert par[4:6].tolist() == [0, 1] and tok[4:6].tolist() == [5, 0] and sc[5] == -INF
    assert par[6:8].tolist() == [0, 1] and tok[6:8].tolist() == [0, 0] and (sc[6:8] == -INF).all()
    dead = np.array([-INF, NAN, -INF, -1.0, -INF, -INF, -1.0, -INF], np.float32)
    par, tok, sc = _check(qg, device, S, beams, dead, None, -1, "dead beams")
    assert (sc[0:2] == -INF).all() and par[2:4].tolist() == [1, 1]


def test_more_beams_than_columns(qg, oracle, device):
    S = np.array([[1.0, 2.0, NAN]] * 8, np.float32)
    par, tok, sc = _check(qg, device, S, 8, what="the start, beams > w")
    assert tok.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and par.tolist() == [0, 0, 2, 3, 4, 5, 6, 7] and (sc[2:] == -INF).all()
    _check(qg, device, S, 8, np.linspace(-1, -2, 8).astype(np.float32), what="beams > w")
    S1 = np.array([[0.5]] * 4, np.float32)
    _check(qg, device, S1, 4, np.zeros(4, np.float32), what="w = 1")


def test_refusals_launch_nothing(qg, device):
    S = torch.zeros((4, 16), device=device)
    out = (torch.full((4,), -7, dtype=torch.int32, device=device), torch.full((4,), -7, dtype=torch.int32, device=device),
           torch.full((4,), -7.0, device=device))
    with pytest.raises(AssertionError):
        qg.beam_step(S, 3, out=out)                                            # rows no multiple of beams
    S9 = torch.zeros((9, 16), device=device)
    with pytest.raises(qg.QGemmError):
        qg.beam_step(S9, 9)                                                    # beams > 8
    L = qg.load()
    rc = L.qgemm_beam_step(S.data_ptr(), 16, 2, 2, 16, None, None, -1, out[0].data_ptr(), out[1].data_ptr(),
                           out[2].data_ptr(), None, 0, None)
    assert rc == qg.HIP_ERROR_INVALID_VALUE                                    # no workspace
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == -7).all() for t in out)
