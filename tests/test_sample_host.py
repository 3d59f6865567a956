"""Sampled token choice without a GPU: the rules of qgemm_sample_rows on the oracle's side (worked examples, the greedy
case against the argmax oracle, the draw's generator, the draw's frequencies), the launch plan query
(qgemm_sample_rows_plan needs no device) and every refusal of the contract through the loaded library."""
import ctypes
import math

import numpy as np
import pytest

import head_oracle
import sample_oracle as SO
from oracle import oracle as O

NAN, INF = float("nan"), float("inf")
ROW = [0.5, NAN, 2.0, -INF, 1.0, 2.0, -0.0, 0.0]


def _one(row, top_k, **kw):
    idx, top_idx, top_prob, n_kept = SO.sample_rows_ref(np.array([row], np.float32), top_k, **kw)
    return int(idx[0]), top_idx[0].tolist(), top_prob[0], int(n_kept[0])


def test_worked_examples(oracle):
    tok, cols, p, n = _one(ROW, 4, seed=1, counter0=0)
    assert cols == [2, 5, 4, 0] and n == 4 and tok == 2
    assert [f"{x:.8f}" for x in p] == ["0.38594994", "0.38594994", "0.14198305", "0.08611707"]
    assert _one(ROW, 4, temperature=0.7, top_p=0.5)[3] == 2
    assert _one(ROW, 4, temperature=0.7, top_p=1e-6)[3] == 1
    assert _one(ROW, 4, temperature=0.7, top_p=1.0)[3] == 4
    assert _one(ROW, 8)[1] == [2, 5, 4, 0, 6, 7, -1, -1]          # -0 before +0 by index, NaN and -inf never listed
    tok, cols, p, n = _one([1, INF, 3, INF], 3)
    assert cols == [1, 3, 2] and np.isnan(p).all() and n == 3 and tok == 1
    tok, cols, p, n = _one([NAN, -INF], 2)
    assert tok == 0 and n == 0 and cols == [-1, -1] and not p.any()
    assert _one(ROW, 4, temperature=0)[1] == [2, -1, -1, -1]      # temperature 0: top_k taken as 1
    assert _one(ROW, 4, seed=1, prev=[7], eos=7)[0] == 7 and _one(ROW, 4, seed=1, prev=[6], eos=7)[0] == 2


def test_top_k_one_is_the_argmax(oracle):
    S = O.uniform((40, 257), 701, -3.0, 3.0)
    rng = np.random.default_rng(5)
    S[rng.integers(0, 40, 60), rng.integers(1, 257, 60)] = np.nan     # never at column 0
    S[rng.integers(0, 40, 60), rng.integers(0, 257, 60)] = -np.inf
    S[3, :] = 1.25                                                    # a row of equal values
    S[4, 100:] = 10.0                                                 # a long tie for the maximum
    want = head_oracle.argmax_rows_ref(S)[0]
    for t in (1.0, 0.3, 0.0):
        got = SO.sample_rows_ref(S, 1, temperature=t, seed=9)
        assert np.array_equal(got[0], want) and np.array_equal(got[1][:, 0], want) and (got[3] == 1).all()


def test_uniform_at_is_the_fill(oracle):
    for seed in (0, 1, 123, 2 ** 63 + 5):
        fill = O.uniform((500,), seed, 0.0, 1.0)
        assert all(SO.uniform_at(seed, i) == fill[i] for i in range(500))
    # the extreme draws tests/test_gpu_sample.py uses
    assert SO.uniform_at(123, 10386508) == np.float32(1 - 2.0 ** -24)
    assert SO.uniform_at(123, 10561121) == np.float32(2.0 ** -23)


def test_draw_frequencies(oracle):
    """20 000 counters on the worked example's row at temperature 0.7: every token's count within 4 sigma of n p."""
    k_one, inv_t = SO.inv_temperature(0.7)
    cols, p, c = SO.row_list(ROW, 4, inv_t)
    n = SO.nucleus(c, 1.0)
    assert k_one is None and n == 4
    draws = 20000
    u = O.uniform((draws,), 77, 0.0, 1.0)                             # uniform_at(77, i), checked above
    counts = np.bincount([SO.draw(c, n, u[i]) for i in range(draws)], minlength=4)
    for j in range(4):
        pj = float(p[j])
        sigma = math.sqrt(draws * pj * (1 - pj))
        assert abs(counts[j] - draws * pj) <= 4 * sigma, (j, counts.tolist(), pj)


def _plan(L, rows, w, top_k):
    parts = ctypes.c_int(-1)
    rc = L.qgemm_sample_rows_plan(rows, w, top_k, ctypes.byref(parts))
    return rc, parts.value


def test_sample_rows_plan(qg):
    L = qg.load()
    bad = qg.HIP_ERROR_INVALID_VALUE
    assert _plan(L, 64, 1000, 50) == (0, 1)
    assert _plan(L, 1, 131072, 50)[1] > 1 and qg.sample_rows_plan(1, 131072, 50) == _plan(L, 1, 131072, 50)[1]
    assert _plan(L, 3, 36877, 64)[1] >= 8                             # the split case of tests/test_gpu_sample.py
    for rows in (1, 2, 3, 16, 64, 65, 255, 256, 257, 5000):
        for w in (1, 4095, 4096, 8191, 8192, 32768, 36877, 70001, 131072, 1 << 24):
            for top_k in (1, 2, 50, 1000, 1024):
                rc, parts = _plan(L, rows, w, top_k)
                assert rc == 0 and 1 <= parts <= 64, (rows, w, top_k, parts)
                assert parts == 1 or (rows < 256 and w // parts >= 4096), (rows, w, top_k, parts)
                ws = L.qgemm_sample_rows_workspace_size(rows, w, top_k)
                assert ws == (0 if parts == 1 else 8 * rows * parts * top_k)   # top_k composites per (row, part)
    assert L.qgemm_sample_rows_plan(0, 8, 1, None) == 0
    for rows, w, top_k in ((1, 0, 1), (-1, 8, 1), (1, (1 << 24) + 1, 1), (1, 8, 0), (1, 8, 1025), (1, 8, -1)):
        assert _plan(L, rows, w, top_k)[0] == bad, (rows, w, top_k)
        assert L.qgemm_sample_rows_workspace_size(rows, w, top_k) == 0
    with pytest.raises(qg.QGemmError):
        qg.sample_rows_plan(1, 8, 0)


def test_new_symbols_are_exported(qg):
    L = qg.load()
    for name in ("qgemm_sample_rows_plan", "qgemm_sample_rows_workspace_size", "qgemm_sample_rows",
                 "qgemm_head_sample_tokens", "qgemm_decoder_generate_sampled"):
        assert name in qg.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    assert hasattr(qg, "sample_rows") and hasattr(qg, "sample_rows_plan")
    assert hasattr(qg.Head, "sample_tokens") and hasattr(qg.Decoder, "generate_sampled")


def test_argument_checks_need_no_gpu(qg):
    """Every refusal of the contract comes before any device call: the pointers here are never dereferenced."""
    L = qg.load()
    bad = qg.HIP_ERROR_INVALID_VALUE
    S, IDX, A, B, WS = 4096, 8192, 12288, 16384, 20480                # stand-ins for device pointers

    def call(s=S, stride=8, rows=1, w=8, top_k=4, top_p=1.0, temp=1.0, counters=None, idx=IDX, top_idx=None,
             top_prob=None, ws=None, ws_bytes=0):
        return L.qgemm_sample_rows(s, stride, rows, w, top_k, top_p, temp, 0, 0, counters, None, -1, idx, top_idx,
                                   top_prob, None, ws, ws_bytes, None)

    assert call(rows=0) == 0                                          # the arguments above are fine: nothing to do
    assert call(s=None) == bad and call(idx=None) == bad
    assert call(top_k=0) == bad and call(top_k=1025) == bad
    assert call(top_p=0.0) == bad and call(top_p=1.5) == bad and call(top_p=NAN) == bad and call(top_p=-0.5) == bad
    assert call(temp=-1.0) == bad and call(temp=INF) == bad and call(temp=NAN) == bad
    assert call(w=0) == bad and call(w=(1 << 24) + 1, stride=1 << 25) == bad and call(rows=-1) == bad
    assert call(stride=7) == bad                                      # a row stride below w
    assert call(top_idx=A) == bad and call(top_prob=B) == bad         # the list's two arrays come together
    assert call(rows=65, counters=(ctypes.c_uint64 * 65)()) == bad    # per-row counters travel by value: 64 at most
    wide = dict(rows=1, w=131072, stride=131072, top_k=50)
    need = L.qgemm_sample_rows_workspace_size(1, 131072, 50)
    assert need > 0
    assert call(**wide) == bad                                        # split, no workspace
    assert call(ws=WS, ws_bytes=need - 1, **wide) == bad              # a short one
    assert call(ws=WS + 4, ws_bytes=need, **wide) == bad              # not 8-byte aligned
    assert L.qgemm_head_sample_tokens(None, 16, 4, 1, 4, 1.0, 1.0, 0, 0, None, None, -1, 16, None) == bad
    assert L.qgemm_decoder_generate_sampled(None, None, 1, None, None, 1, None, 4, 1.0, 1.0, 0, None, -1, None,
                                            None) == bad
