"""GPU parity of qgemm_sample_rows against sample_oracle (the rules of include/qgemm.h restated): the tokens, the
sorted list, the bits of its probabilities and the nucleus length, exactly.  Every case draws with 16 counters, so
that different ranks of the list are reached.  S is a window of a NaN-filled parent (a base off 16 bytes and an odd
row stride unless a case asks for aligned rows) and must come back unchanged.

Where this kernel can go wrong is the selection: equal values at the k-th place of the list, of which only the lowest
indices may pass, across the seams of its loads (the 4 columns of a 16-byte load, the 1024 columns of a workgroup's
pass, the parts of a split row); columns that are no candidates (NaN, -inf); fewer candidates than top_k.  Random rows
carry all of these -- every second row lies on a grid of 17 values -- and test_planted_rows places them one by one."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sample_oracle as SO
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

NAN, INF = np.float32("nan"), np.float32("inf")
SEED = 11
COUNTER0S = tuple(1000 * d + 7 for d in range(16))
SPLIT_W = 36877                                   # 9 parts of 4100 columns at 3 rows (asserted below)

# (rows, w, top_k, top_p, temperature, aligned rows): every width, row count, top_k, top_p and temperature of the list
CASES = [
    (1, 1, 1, 1.0, 1.0, False),
    (3, 2, 2, 0.9, 0.7, False),
    (65, 63, 7, 0.5, 2.0, False),
    (300, 64, 64, 1.0, 1.0, True),
    (3, 65, 1000, 0.9, 1.0, False),               # top_k above w
    (65, 1000, 1024, 0.5, 0.7, False),
    (300, 1000, 7, 1e-6, 1.0, False),
    (3, 4099, 64, 1.0, 0.0, False),               # temperature 0: greedy, the list one long
    (1, 8195, 1000, 0.9, 2.0, False),             # split in two
    (65, 8195, 2, 0.5, 1.0, True),
    (300, 4099, 1024, 0.9, 0.7, False),
    (3, SPLIT_W, 64, 0.9, 0.7, False),
    (3, SPLIT_W, 1024, 1.0, 1.0, True),
    (1, SPLIT_W, 1, 1.0, 1.0, False),
]


@functools.lru_cache(maxsize=None)
def _logits(rows, w, seed=0):
    S = O.uniform((rows, w), 800 + seed + rows + w % 97, -4.0, 4.0)
    rng = np.random.default_rng(rows * 131 + w + seed)
    S[1::2] = np.round(S[1::2] * 2) / 2           # 17 values (-0.0 among them): ties wherever the k-th place falls
    S[rng.random(S.shape) < 0.02] = NAN
    S[rng.random(S.shape) < 0.03] = -INF
    if rows >= 3:
        S[2, 0] = NAN
    S.flags.writeable = False
    return S


def _window(rows_np, device, aligned=False):
    """The rows as a window of a NaN-filled device parent: (parent, view)."""
    n, w = rows_np.shape
    stride, offset = (-(-w // 4) * 4 + 4, 0) if aligned else (w + 1 if w % 2 == 0 else w + 2, 1)
    flat = np.full(offset + n * stride + 3, NAN, np.float32)
    for r in range(n):
        flat[offset + r * stride: offset + r * stride + w] = rows_np[r]
    parent = torch.from_numpy(flat).to(device)
    return parent, torch.as_strided(parent, (n, w), (stride, 1), offset)


def _compare_top(got, want, what):
    (_, ti, tp, nk), (_, want_ti, want_tp, want_nk) = got, want
    ti, nk = ti.cpu().numpy(), nk.cpu().numpy()
    bad = np.flatnonzero((ti != want_ti).any(axis=1))
    assert not len(bad), f"{what}: list of row {bad[0]}: {ti[bad[0]][:12]} want {want_ti[bad[0]][:12]}"
    assert_bits_equal(tp.cpu().numpy(), want_tp, f"{what}: top_prob")
    assert np.array_equal(nk, want_nk), f"{what}: n_kept {nk[nk != want_nk][:4]} want {want_nk[nk != want_nk][:4]}"


def _check(qg, device, S_np, top_k, top_p, temperature, what, aligned=False):
    parent, S = _window(S_np, device, aligned)
    before = parent.clone()
    want = SO.sample_rows_draws(S_np, top_k, top_p, temperature, SEED, COUNTER0S)
    for d, c0 in enumerate(COUNTER0S):
        if d == 0:
            got = qg.sample_rows(S, top_k, top_p, temperature, SEED, c0, return_top=True)
            _compare_top(got, want, what)
            idx = got[0]
        else:
            idx = qg.sample_rows(S, top_k, top_p, temperature, SEED, c0)
        idx = idx.cpu().numpy()
        diff = np.flatnonzero(idx != want[0][d])
        assert not len(diff), f"{what}, counter0 {c0}: rows {diff[:4]} got {idx[diff[:4]]} want {want[0][d][diff[:4]]}"
    assert torch.equal(parent.view(torch.int32), before.view(torch.int32)), f"{what}: S was written"
    return want


@pytest.mark.parametrize("rows,w,top_k,top_p,temperature,aligned", CASES)
def test_against_the_oracle(qg, oracle, device, rows, w, top_k, top_p, temperature, aligned):
    if w == SPLIT_W and rows == 3:
        assert qg.sample_rows_plan(3, w, top_k) >= 8
    if rows >= 256:
        assert qg.sample_rows_plan(rows, w, top_k) == 1
    want = _check(qg, device, _logits(rows, w), top_k, top_p, temperature, f"{rows} x {w}, top_k {top_k}", aligned)
    if top_k >= 7 and top_p >= 0.5 and temperature > 0 and rows * w >= 65 * 63:
        ranks = {int(np.flatnonzero(want[1][r] == want[0][d, r])[0]) for d in range(16) for r in range(rows)
                 if want[3][r]}
        assert len(ranks) >= 3, f"the 16 counters reach several ranks of the list: {sorted(ranks)}"


def _chunk(qg, rows, w, top_k):
    parts = qg.sample_rows_plan(rows, w, top_k)
    return parts, -(-(-(-w // parts)) // 4) * 4     # ceil(w / parts) rounded up to a multiple of 4


def _planted(w, chunk):
    """Rows with values placed one by one; row 0's equal values in ascending column order come back too."""
    base = O.uniform((1, w), 950, -1.0, 1.0)[0]
    seam = chunk if chunk < w else w - 2
    equal = sorted({5, 1028, 1029, 1030, 1031, 1032, 2056, seam - 1, seam, seam + 1, w - 1})
    rows = []

    def add(edit):
        r = base.copy()
        edit(r)
        rows.append(r)

    def put(r, cols, v):
        for c in cols:
            r[c] = v

    add(lambda r: put(r, equal, 5.0))                                  # more equal maxima than places in the list
    add(lambda r: (put(r, equal, 5.0), put(r, [9, 2057, 3000], 6.0)))  # the k-th place inside the equals
    add(lambda r: r.fill(2.5))                                         # every column equal
    add(lambda r: (r.fill(-1.0), put(r, [w // 3], -0.0), put(r, [5, w - 1], 0.0)))   # +0 == -0: by index
    add(lambda r: (r.fill(-1.0), put(r, [w // 3], 0.0), put(r, [5, w - 1], -0.0)))
    rng = np.random.default_rng(w)
    add(lambda r: put(r, np.flatnonzero(rng.random(w) < 0.6), -INF))   # banned columns
    add(lambda r: (put(r, np.flatnonzero(rng.random(w) < 0.3), NAN), put(r, [0], NAN)))   # NaN at column 0 and elsewhere
    add(lambda r: put(r, [w // 2, w - 1], INF))                        # a +inf row: every p NaN, the lowest index wins
    add(lambda r: (r.fill(-INF), put(r, np.flatnonzero(rng.random(w) < 0.5), NAN)))   # no candidate at all
    add(lambda r: (r.fill(-INF), put(r, [seam, 7, w - 1], 1.0), put(r, [seam - 1], 0.5)))  # fewer candidates than top_k
    S = np.stack(rows)
    S.flags.writeable = False
    return S, equal


@pytest.mark.parametrize("w", [4099, SPLIT_W])
@pytest.mark.parametrize("top_k", [7, 64])
def test_planted_rows(qg, oracle, device, w, top_k):
    parts, chunk = _chunk(qg, 10, w, top_k)
    assert parts == (1 if w == 4099 else 9)
    S, equal = _planted(w, chunk)
    assert S.shape[0] == 10
    want = _check(qg, device, S, top_k, 0.9, 0.7, f"planted rows, w {w}, top_k {top_k}")
    # the oracle itself: only the lowest-index equals make the list, in index order
    n_eq = min(top_k, len(equal))
    assert want[1][0, :n_eq].tolist() == equal[:n_eq]
    seam = chunk if chunk < w else w - 2
    assert want[1][1, :3].tolist() == [9, 2057, 3000]
    assert want[1][1, 3:3 + min(top_k - 3, len(equal))].tolist() == equal[:top_k - 3]
    assert want[1][2, :top_k].tolist() == list(range(top_k))
    assert want[1][3, :3].tolist() == sorted([5, w // 3, w - 1])
    assert want[0][:, 7].tolist() == [w // 2] * 16 and np.isnan(want[2][7, :min(top_k, 8)]).all()
    assert (want[0][:, 8] == 0).all() and want[3][8] == 0 and (want[1][8] == -1).all()
    assert want[1][9, :5].tolist() == [7, seam, w - 1, seam - 1, -1]


def test_the_result_does_not_depend_on_the_plan(qg, oracle, device):
    """One logits row sampled alone (many parts) and as row 5 of a 300-row call (one part), with the same counter."""
    w, top_k = SPLIT_W, 64
    assert qg.sample_rows_plan(1, w, top_k) >= 8 and qg.sample_rows_plan(300, w, top_k) == 1
    one = _logits(3, w)[1:2]                                          # a row on the grid: ties at the k-th place
    many = np.ascontiguousarray(np.broadcast_to(_logits(1, w, seed=1), (300, w))).copy()
    many[5] = one[0]
    _, S1 = _window(one, device)
    _, S300 = _window(many, device, aligned=True)
    for c in (0, 12345, 2 ** 40 + 3):
        a = qg.sample_rows(S1, top_k, 0.9, 0.7, SEED, counter0=c + (5 << 32), return_top=True)
        b = qg.sample_rows(S300, top_k, 0.9, 0.7, SEED, counter0=c, return_top=True)
        want = SO.sample_rows_ref(one, top_k, 0.9, 0.7, SEED, counters=[c + (5 << 32)])
        assert int(a[0][0]) == int(b[0][5]) == int(want[0][0])
        _compare_top(a, want, "alone")
        _compare_top(tuple(t[5:6] for t in b), want, "row 5 of 300")


def test_extreme_draws(qg, oracle, device):
    """u = 1 - 2^-24, the greatest value of the generator, and u = 2^-23 (seed 123; counters found by a search over
    2^24 of them): the last and the first ranks of the nucleus."""
    hi, lo = 10386508, 10561121
    assert SO.uniform_at(123, hi) == np.float32(1 - 2.0 ** -24) and SO.uniform_at(123, lo) == np.float32(2.0 ** -23)
    S_np = _logits(8, 1000)
    _, S = _window(S_np, device)
    for top_p in (1.0, 0.5):
        for counter in (hi, lo):
            got = qg.sample_rows(S, 64, top_p, 0.7, 123, counters=[counter] * 8, return_top=True)
            want = SO.sample_rows_ref(S_np, 64, top_p, 0.7, 123, counters=[counter] * 8)
            assert np.array_equal(got[0].cpu().numpy(), want[0]), (top_p, counter)
            _compare_top(got, want, f"top_p {top_p}, counter {counter}")
            rank = [int(np.flatnonzero(want[1][r] == want[0][r])[0]) for r in range(8)]
            if counter == hi:
                assert rank == [int(n) - 1 for n in want[3]], "the greatest u draws the nucleus' last rank"
            else:
                assert rank == [0] * 8


def test_end_token_hold(qg, oracle, device):
    S_np = _logits(65, 1000)
    _, S = _window(S_np, device)
    prev_np = np.where(np.arange(65) % 3 == 0, 5, 3).astype(np.int32)
    prev = torch.from_numpy(prev_np).to(device)
    got = qg.sample_rows(S, 64, 0.9, 0.7, SEED, 3, prev=prev, eos=5).cpu().numpy()
    want = SO.sample_rows_ref(S_np, 64, 0.9, 0.7, SEED, 3, prev=prev_np, eos=5)[0]
    free = SO.sample_rows_ref(S_np, 64, 0.9, 0.7, SEED, 3)[0]
    assert np.array_equal(got, want)
    assert (got[prev_np == 5] == 5).all() and np.array_equal(got[prev_np != 5], free[prev_np != 5])
    assert (free[prev_np == 5] != 5).any(), "the hold changed something"
    assert np.array_equal(qg.sample_rows(S, 64, 0.9, 0.7, SEED, 3, prev=prev).cpu().numpy(), free)   # no end token
    # a row without a candidate is held too
    banned = np.full((2, 9), -INF, np.float32)
    idx = qg.sample_rows(_window(banned, device)[1], 4, prev=torch.tensor([8, 1], dtype=torch.int32, device=device),
                         eos=8)
    assert idx.cpu().numpy().tolist() == [8, 0]


def test_captured_call_replays(qg, oracle, device):
    """Nothing allocated, synchronized or copied: a two-launch call captured as the first work of a fresh stream and
    replayed twice gives the eager call's output (and so repeats its draws)."""
    L = qg.load()
    rows, w, top_k = 3, SPLIT_W, 64
    assert qg.sample_rows_plan(rows, w, top_k) > 1
    S_np = _logits(rows, w)
    parent, S = _window(S_np, device)
    want = SO.sample_rows_ref(S_np, top_k, 0.9, 0.7, SEED, 21)
    need = L.qgemm_sample_rows_workspace_size(rows, w, top_k)
    ws = torch.zeros(need, dtype=torch.uint8, device=device)
    idx = torch.full((rows,), -1, dtype=torch.int32, device=device)
    ti = torch.full((rows, top_k), -2, dtype=torch.int32, device=device)
    tp = torch.full((rows, top_k), float("nan"), device=device)
    nk = torch.full((rows,), -1, dtype=torch.int32, device=device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = L.qgemm_sample_rows(S.data_ptr(), S.stride(0), rows, w, top_k, 0.9, 0.7, SEED, 21, None, None, -1,
                                 idx.data_ptr(), ti.data_ptr(), tp.data_ptr(), nk.data_ptr(), ws.data_ptr(), need,
                                 s.cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -1).all(), "a captured call runs nothing"
    for i in range(2):
        idx.fill_(-1)
        ti.fill_(-2)
        ws.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy(), want[0]), f"replay {i}"
        _compare_top((idx, ti, tp, nk), want, f"replay {i}")
