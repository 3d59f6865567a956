"""Beam search without a GPU: the rules of qgemm_logsumexp_rows and qgemm_beam_step on the oracle's side (the tree sum
by hand, against math.fsum and under padding; beams = 1 against the argmax oracle; a worked example of every rule of
the step), the plan and workspace queries (they need no device) and every refusal that can be reached without a device
through the loaded library."""
import ctypes
import math

import numpy as np
import pytest

import beam_oracle as BO
import head_oracle
from oracle import oracle as O

F32 = np.float32
NAN, INF = float("nan"), float("inf")


def _bits(x):
    return np.asarray(x, F32).reshape(-1).view(np.uint32).tolist()


def test_tree_sum_by_hand():
    """5 values: ((a + b) + (c + d)) + ((e + 0) + (0 + 0)), then +0 subtrees all the way up to 1024 leaves."""
    a, b, c, d, e = (F32(v) for v in (1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 1.0))
    want = F32(F32(F32(a + b) + F32(c + d)) + e)
    # 1 + 2^-24 rounds to 1 (ties to even); 2^-24 + 2^-24 = 2^-23; 1 + 2^-23 is exact; + 1 -> 2 + 2^-23 rounds to 2
    assert F32(a + b) == F32(1.0) and F32(c + d) == F32(2.0 ** -23)
    assert F32(F32(a + b) + F32(c + d)) == F32(1.0 + 2.0 ** -23)
    assert want == F32(2.0)
    assert _bits(BO.tree_sum([a, b, c, d, e])) == _bits(want)
    # a left-to-right sum differs: ((1 + 2^-24) + 2^-24) + 2^-24 stays 1, + 1 = 2 -- same here, so use another order
    assert _bits(BO.tree_sum([b, c, a, d, e])) == _bits(F32(F32(F32(b + c) + F32(a + d)) + e))
    assert BO.tree_sum([]) == 0 and BO.tree_sum([3.5]) == F32(3.5)
    assert np.isnan(BO.tree_sum([1.0, NAN, 2.0]))


def test_tree_sum_against_fsum():
    rng = np.random.default_rng(11)
    for w in (1, 7, 1000, 1024, 1025, 5000, 36877):
        e = rng.random(w, dtype=F32)
        exact = math.fsum(e.tolist())
        assert abs(float(BO.tree_sum(e)) - exact) <= w * 2.0 ** -24 * exact, w


def test_padding_with_no_candidates_changes_nothing():
    row = O.uniform((1000,), 801, -8.0, 8.0)
    want = BO.logsumexp_rows_ref(row[None])
    for w in (1024, 3000):
        padded = np.full(w, -np.inf, F32)
        padded[:1000] = row
        got = BO.logsumexp_rows_ref(padded[None])
        assert _bits(got[0]) == _bits(want[0]) and _bits(got[1]) == _bits(want[1]), w


def test_logsumexp_corner_rows():
    mx, logz = BO.logsumexp_rows_ref(np.array([[NAN, -INF, NAN], [NAN, 2.5, -INF], [1.0, INF, 0.0], [3.0, 3.0, 3.0]], F32))
    assert mx[0] == -INF and logz[0] == -INF                                   # no candidate
    assert mx[1] == F32(2.5) and _bits(logz[1]) == _bits(F32(0.0))             # one candidate: log(1) = +0
    assert mx[2] == INF and np.isnan(logz[2])                                  # +inf: fl(inf - inf)
    assert mx[3] == 3 and logz[3] == F32(math.log(3.0))
    assert _bits(BO.logsumexp_rows_ref(np.array([[0.0, -0.0]], F32))[0]) == _bits(F32(0.0))    # the lower index's bits
    assert _bits(BO.logsumexp_rows_ref(np.array([[-0.0, 0.0]], F32))[0]) == _bits(F32(-0.0))


def test_one_beam_is_the_argmax():
    S = O.uniform((40, 257), 701, -3.0, 3.0)
    rng = np.random.default_rng(5)
    S[rng.integers(0, 40, 60), rng.integers(1, 257, 60)] = np.nan     # never at column 0
    S[rng.integers(0, 40, 60), rng.integers(0, 257, 60)] = -np.inf
    S[3, :] = 1.25
    S[4, 100:] = 10.0
    want = head_oracle.argmax_rows_ref(S)[0]
    par, tok, sc = BO.beam_step_ref(S, 1)
    assert np.array_equal(tok, want) and not par.any()
    mx, logz = BO.logsumexp_rows_ref(S)
    lp = (S[np.arange(40), want] - mx).astype(F32) - logz
    assert _bits(sc) == _bits(F32(0.0) + lp.astype(F32))


def _lp(row, t):
    mx, logz = BO.logsumexp_rows_ref(np.asarray([row], F32))
    return F32(F32(F32(row[t]) - mx[0]) - logz[0])


def test_beam_step_rules_worked():
    A = [0.0, 3.0, NAN, 1.0, 3.0, -INF]                 # order: 1, 4, 3, 0; 2 and 5 are no candidates
    B = [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]
    # the start: beam 0 alone is live, so both places come from it; the tie 1 / 4 goes to the lower column
    par, tok, sc = BO.beam_step_ref(np.array([A, B], F32), 2)
    assert par.tolist() == [0, 0] and tok.tolist() == [1, 4]
    assert _bits(sc) == _bits([F32(0.0) + _lp(A, 1), F32(0.0) + _lp(A, 4)]) and sc[0] == sc[1]
    # two beams with identical rows and scores: equal c, the lower beam's candidates first
    par, tok, sc = BO.beam_step_ref(np.array([A, A], F32), 2, scores_in=[-1.0, -1.0])
    assert par.tolist() == [0, 0] and tok.tolist() == [1, 4]
    par, tok, sc = BO.beam_step_ref(np.array([B, A], F32), 2, scores_in=[-1.0, -1.0])
    assert par.tolist() == [1, 1] and tok.tolist() == [1, 4]             # A's best beat B's uniform 1/6
    # a finished beam that outranks (score -0.5) and one that is outranked (score -9)
    par, tok, sc = BO.beam_step_ref(np.array([A, B], F32), 2, scores_in=[-1.0, -0.5], prev=[0, 5], eos=5)
    assert par.tolist() == [1, 0] and tok.tolist() == [5, 1] and sc[0] == F32(-0.5)
    par, tok, sc = BO.beam_step_ref(np.array([A, B], F32), 2, scores_in=[-1.0, -9.0], prev=[0, 5], eos=5)
    assert par.tolist() == [0, 0] and tok.tolist() == [1, 4]
    # eos < 0 or prev None: nobody is finished
    for kw in (dict(prev=[0, 5], eos=-1), dict(prev=None, eos=5)):
        par, tok, sc = BO.beam_step_ref(np.array([B, B], F32), 2, scores_in=[-1.0, -0.5], **kw)
        assert par.tolist() == [1, 1] and tok.tolist() == [0, 1]
    # a dead beam (-inf, NaN) contributes nothing; a group with one candidate; a group with none
    par, tok, sc = BO.beam_step_ref(np.array([A, B, B, B], F32), 2, scores_in=[-INF, NAN, -INF, 0.0])
    assert par.tolist() == [0, 1, 1, 1] and tok.tolist() == [0, 0, 0, 1]
    assert sc[0] == -INF and sc[1] == -INF and sc[2] == sc[3] == _lp(B, 0)
    one = [NAN, -INF, 7.0, -INF, NAN, -INF]
    par, tok, sc = BO.beam_step_ref(np.array([one, one], F32), 2, scores_in=[-2.0, -INF])
    assert par.tolist() == [0, 1] and tok.tolist() == [2, 0] and _bits(sc) == _bits([F32(-2.0), -INF])
    # beams > w
    par, tok, sc = BO.beam_step_ref(np.array([[1.0, 2.0]] * 3, F32), 3)
    assert par.tolist() == [0, 0, 2] and tok.tolist() == [1, 0, 0] and sc[2] == -INF
    # scores that make c round to equal values: 2^25 swallows lp, the lower place wins
    par, tok, sc = BO.beam_step_ref(np.array([A, B], F32), 2, scores_in=[-2.0 ** 25, -2.0 ** 25])
    assert par.tolist() == [0, 0] and tok.tolist() == [1, 4] and sc[0] == sc[1] == F32(-2.0 ** 25)
    par, tok, sc = BO.beam_step_ref(np.array([A, B, B], F32), 3, scores_in=[-2.0 ** 25, -2.0 ** 25, -2.0 ** 25])
    # A's third column (lp about -2.8) rounds one ulp (4) down, B's (-log 6) round to -2^25 itself: beam 1's first wins
    assert par.tolist() == [0, 0, 1] and tok.tolist() == [1, 4, 0] and sc[2] == F32(-2.0 ** 25)


def _lse_plan(L, rows, w):
    parts = ctypes.c_int(-1)
    return L.qgemm_logsumexp_rows_plan(rows, w, ctypes.byref(parts)), parts.value


def test_plans_and_workspaces(qg):
    L = qg.load()
    bad = qg.HIP_ERROR_INVALID_VALUE
    assert _lse_plan(L, 32, 4099) == (0, 1) and _lse_plan(L, 300, 36877) == (0, 1)
    assert _lse_plan(L, 32, 8200)[1] == 2 and _lse_plan(L, 32, 36877)[1] > 1 and _lse_plan(L, 1, 36877)[1] > 1
    assert qg.logsumexp_rows_plan(3, 36877) == _lse_plan(L, 3, 36877)[1]
    for rows in (1, 2, 3, 16, 32, 64, 255, 256, 300, 5000):
        for w in (1, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8200, 32768, 36877, 131072, 1 << 24):
            rc, parts = _lse_plan(L, rows, w)
            nblk = -(-w // 1024)
            assert rc == 0 and 1 <= parts <= 64, (rows, w, parts)
            assert parts == 1 or (rows < 256 and nblk // parts >= 4), (rows, w, parts)      # whole blocks, >= 4 each
            ws = L.qgemm_logsumexp_rows_workspace_size(rows, w)
            assert ws == (0 if parts == 1 else 8 * rows * parts + 4 * rows * nblk)
    assert L.qgemm_logsumexp_rows_plan(0, 8, None) == 0
    for rows, w in ((1, 0), (-1, 8), (1, (1 << 24) + 1)):
        assert _lse_plan(L, rows, w)[0] == bad and L.qgemm_logsumexp_rows_workspace_size(rows, w) == 0
    with pytest.raises(qg.QGemmError):
        qg.logsumexp_rows_plan(1, 0)
    for groups, beams in ((1, 1), (1, 2), (2, 3), (4, 8), (8, 4), (8, 8), (64, 1), (0, 4)):
        for w in (1, 97, 1000, 4096, 8191, 8200, 32768, 36877, 1 << 24):
            rows = groups * beams
            sp, lp = ctypes.c_int(-1), ctypes.c_int(-1)
            assert L.qgemm_beam_step_plan(groups, beams, w, ctypes.byref(sp), ctypes.byref(lp)) == 0
            assert sp.value == qg.sample_rows_plan(rows, w, beams) and lp.value == _lse_plan(L, rows, w)[1]
            assert qg.beam_step_plan(groups, beams, w) == (sp.value, lp.value)
            lse = -(-L.qgemm_logsumexp_rows_workspace_size(rows, w) // 8) * 8
            lists = 8 * rows * sp.value * beams if sp.value > 1 else 0
            assert L.qgemm_beam_step_workspace_size(groups, beams, w) == lists + lse + 4 * rows * (2 + 2 * beams)
    assert L.qgemm_beam_step_plan(1, 1, 8, None, None) == 0
    for groups, beams, w in ((1, 0, 8), (1, 9, 8), (-1, 1, 8), (9, 8, 8), (65, 1, 8), (1, 1, 0), (1, 1, (1 << 24) + 1)):
        assert L.qgemm_beam_step_plan(groups, beams, w, None, None) == bad, (groups, beams, w)
        assert L.qgemm_beam_step_workspace_size(groups, beams, w) == 0
    with pytest.raises(qg.QGemmError):
        qg.beam_step_plan(1, 9, 8)


def test_new_symbols_are_exported(qg):
    L = qg.load()
    for name in ("qgemm_logsumexp_rows_plan", "qgemm_logsumexp_rows_workspace_size", "qgemm_logsumexp_rows",
                 "qgemm_beam_step_plan", "qgemm_beam_step_workspace_size", "qgemm_beam_step", "qgemm_head_beam_step",
                 "qgemm_decoder_gather_slots", "qgemm_decoder_generate_beam"):
        assert name in qg.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    for name in ("logsumexp_rows", "logsumexp_rows_plan", "beam_step", "beam_step_plan", "beam_hypotheses"):
        assert hasattr(qg, name)
    assert hasattr(qg.Head, "beam_step")
    for name in ("gather_slots", "generate_beam", "beam_fork"):
        assert hasattr(qg.Decoder, name)


def test_argument_checks_need_no_gpu(qg):
    """Every refusal that does not depend on a decoder's or a head's state comes before any device call: the pointers
    here are never dereferenced.  (The refusals that need a live decoder are in the GPU tests.)"""
    L = qg.load()
    bad = qg.HIP_ERROR_INVALID_VALUE
    S, A, B, C, WS = 4096, 8192, 12288, 16384, 20480                  # stand-ins for device pointers

    def lse(s=S, stride=8, rows=1, w=8, mx=A, logz=B, ws=None, ws_bytes=0):
        return L.qgemm_logsumexp_rows(s, stride, rows, w, mx, logz, ws, ws_bytes, None)

    assert lse(rows=0) == 0                                           # the arguments above are fine: nothing to do
    assert lse(s=None) == bad and lse(mx=None) == bad and lse(logz=None) == bad
    assert lse(w=0) == bad and lse(w=(1 << 24) + 1, stride=1 << 25) == bad and lse(rows=-1) == bad
    assert lse(stride=7) == bad
    wide = dict(rows=2, w=36877, stride=36877)
    need = L.qgemm_logsumexp_rows_workspace_size(2, 36877)
    assert need > 0
    assert lse(**wide) == bad and lse(ws=WS, ws_bytes=need - 1, **wide) == bad and lse(ws=WS + 4, ws_bytes=need, **wide) == bad

    need = L.qgemm_beam_step_workspace_size(1, 2, 8)

    def step(s=S, stride=8, groups=1, beams=2, w=8, par=A, tok=B, sc=C, ws=WS, ws_bytes=need):
        return L.qgemm_beam_step(s, stride, groups, beams, w, None, None, -1, par, tok, sc, ws, ws_bytes, None)

    assert step(groups=0) == 0
    assert step(s=None) == bad and step(par=None) == bad and step(tok=None) == bad and step(sc=None) == bad
    assert step(beams=0) == bad and step(beams=9) == bad and step(groups=-1) == bad and step(groups=33) == bad
    assert step(w=0) == bad and step(w=(1 << 24) + 1, stride=1 << 25) == bad and step(stride=7) == bad
    assert step(ws=None) == bad and step(ws_bytes=need - 1) == bad and step(ws=WS + 4) == bad
    assert L.qgemm_head_beam_step(None, 16, 4, 1, 2, None, None, -1, A, B, C, None) == bad
    ints = (ctypes.c_int * 2)(0, 1)
    assert L.qgemm_decoder_gather_slots(None, 1, 2, ints, ints, A, ints, None) == bad
    assert L.qgemm_decoder_generate_beam(None, None, 1, 2, ints, ints, A, 1, None, None, -1, A, B, C, None) == bad


def test_beam_hypotheses_backtracks(qg):
    tokens = np.array([[5, 6, 7, 8], [9, 3, 1, 2], [4, 3, 0, 0]], np.int32)
    parents = np.array([[0, 0, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1]], np.int32)
    scores = np.array([[-1, -2, -1, -2], [-2, -3, -2, -3], [-3, -3.5, -np.inf, -4]], np.float32)
    hyp = qg.beam_hypotheses(tokens, parents, scores, eos=3, beams=2)
    assert hyp[0] == ([6, 9, 4], -3.0)                  # place 0 <- parent 0 (row 0 at step 1) <- parent 1 (row 1 at step 0)
    assert hyp[1] == ([5, 3], -3.5)                     # held after the end token: cut there
    assert hyp[2] == ([], -np.inf)                      # a dead place
    assert hyp[3] == ([7, 2, 0], -4.0)                  # group 1: place 1 <- parent 1 (row 3) <- parent 0 (row 2)
