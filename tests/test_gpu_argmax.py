"""GPU parity of qgemm_argmax_rows: idx and val, bit for bit, against head_oracle.argmax_rows_ref (the reference's
sequential op_argmax chain).  S is always a window of a NaN-filled parent with a row stride above w, idx is prefilled
with -1 and val with NaN.  Two layouts per width: a base that is not 16-byte aligned, and an odd row stride.

Where a kernel like this can go wrong is at the seams of its reduction: between the 4 columns of one 16-byte load, the
256 columns of a wave's pass, the 1024 columns of a workgroup's pass and the parts of a split row.  Equal maxima are
placed on both sides of each seam, for every position the scalar head can shift the seams to, and the lowest index is
expected every time."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import head_oracle
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INVALID = 1
WIDTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099)
SPLIT_WIDTHS = (8195, 70001)     # checked against the plan query below: every row count splits them
ROW_COUNTS = (1, 3, 65)
NAN, INF = np.float32("nan"), np.float32("inf")


def _chunk(qg, rows, w):
    parts = qg.argmax_rows_plan(rows, w)
    return parts, -(-(-(-w // parts)) // 4) * 4     # ceil(w / parts) rounded up to a multiple of 4 (include/qgemm.h)


@functools.lru_cache(maxsize=None)
def _seams(qg, w):
    seams = {4, 256, 1024}
    for rows in ROW_COUNTS:
        parts, chunk = _chunk(qg, rows, w)
        seams |= {p * chunk for p in range(1, min(parts, 3))} | {(parts - 1) * chunk}
    return sorted(c for c in seams if 0 < c < w)


@functools.lru_cache(maxsize=None)
def _cases(qg, w):
    """(S, idx, val): one row per value placement, and the oracle's result on them (computed once, read-only)."""
    base = O.uniform((1, w), 900 + w % 89)[0]
    rows = []

    def add(edit):
        r = base.copy()
        edit(r)
        rows.append(r)

    def put(r, cols, v):
        for c in cols:
            r[c] = v

    add(lambda r: put(r, [0], 2.0))                                   # the maximum at column 0
    add(lambda r: put(r, [w - 1], 2.0))                               # ... and at w - 1
    for c in _seams(qg, w):                                           # equal maxima across every seam
        for shift in range(4):
            a = c - shift
            if a - 1 >= 0:
                add(lambda r, a=a: put(r, [a - 1, a], 3.0))
        add(lambda r, c=c: put(r, [c - 1, c, w - 1], 3.0))            # three of them
    add(lambda r: put(r, [w // 2, w - 1], 3.0))
    add(lambda r: (r.fill(-1.0), put(r, [w // 3], -0.0), put(r, [w - 1], 0.0)))      # -0 first: +0 is not greater
    add(lambda r: (r.fill(-1.0), put(r, [w // 3], 0.0), put(r, [w - 1], -0.0)))
    add(lambda r: r.fill(-INF))                                       # an all -inf row
    add(lambda r: (r.fill(NAN), put(r, [0], -INF)))                   # [-inf, NaN, NaN, ..]
    add(lambda r: (put(r, [0], NAN), put(r, [w - 1], 5.0)))           # NaN at column 0, larger values after it
    rng = np.random.default_rng(w)

    def scatter(r):
        r[rng.random(w) < 0.3] = NAN
        r[0] = -0.5
    add(scatter)                                                      # NaNs scattered elsewhere
    add(lambda r: (scatter(r), put(r, [w - 1], 4.0), put(r, [max(w - 2, 0)], NAN if w > 2 else 4.0)))
    S = np.stack(rows)
    idx, val = head_oracle.argmax_rows_ref(S)
    for a in (S, idx, val):
        a.flags.writeable = False
    return S, idx, val


def _window(rows_np, stride, offset, device):
    """The rows as a window of a NaN-filled device parent: (parent, view)."""
    n, w = rows_np.shape
    flat = np.full(offset + n * stride, NAN, np.float32)
    for r in range(n):
        flat[offset + r * stride: offset + r * stride + w] = rows_np[r]
    parent = torch.from_numpy(flat).to(device)
    return parent, torch.as_strided(parent, (n, w), (stride, 1), offset)


def _layouts(w):
    even = -(-w // 4) * 4 + 4
    return (("unaligned base", even, 1), ("odd stride", w + 1 if w % 2 == 0 else w + 2, 0))


def _run(qg, S_np, want_idx, want_val, stride, offset, device, what):
    parent, S = _window(S_np, stride, offset, device)
    before = parent.clone()
    n = S_np.shape[0]
    idx = torch.full((n,), -1, dtype=torch.int32, device=device)
    val = torch.full((n,), float("nan"), device=device)
    qg.argmax_rows(S, idx, val)
    got_idx, got_val = idx.cpu().numpy(), val.cpu().numpy()
    assert np.array_equal(got_idx, want_idx), f"{what}: idx {got_idx[got_idx != want_idx][:4]} at rows " \
                                               f"{np.flatnonzero(got_idx != want_idx)[:4]}, want " \
                                               f"{want_idx[got_idx != want_idx][:4]}"
    assert np.array_equal(got_val.view(np.uint32), want_val.view(np.uint32)), f"{what}: val bits differ"
    assert torch.equal(parent.view(torch.int32), before.view(torch.int32)), f"{what}: S was written"


def _check_width(qg, w, device):
    S, idx, val = _cases(qg, w)
    n = S.shape[0]
    for name, stride, offset in _layouts(w):
        pick = np.arange(65) % n                       # 65 rows: every placement, some twice
        _run(qg, S[pick], idx[pick], val[pick], stride, offset, device, f"w {w}, 65 rows, {name}")
        for r0 in range(0, n, 3):                      # 3 rows
            sl = slice(r0, min(n, r0 + 3))
            _run(qg, S[sl], idx[sl], val[sl], stride, offset, device, f"w {w}, rows {r0}.., {name}")
        for r in range(n):                             # 1 row
            _run(qg, S[r:r + 1], idx[r:r + 1], val[r:r + 1], stride, offset, device, f"w {w}, row {r} alone, {name}")


@pytest.mark.parametrize("w", WIDTHS)
def test_one_workgroup_per_row(qg, oracle, device, w):
    for rows in ROW_COUNTS:
        assert qg.argmax_rows_plan(rows, w) == 1
    _check_width(qg, w, device)


@pytest.mark.parametrize("w", SPLIT_WIDTHS)
def test_split_rows(qg, oracle, device, w):
    plans = {qg.argmax_rows_plan(rows, w) for rows in ROW_COUNTS}
    assert min(plans) > 1, "every row count splits these widths"
    _check_width(qg, w, device)


def test_the_split_widths_cover_several_plans(qg):
    plans = {qg.argmax_rows_plan(rows, w) for rows in ROW_COUNTS for w in SPLIT_WIDTHS}
    assert len(plans) >= 3 and min(plans) > 1, plans


def test_the_result_does_not_depend_on_the_plan(qg, oracle, device):
    """The same wide rows once among few rows (split) and once among 256 (one workgroup each)."""
    w = SPLIT_WIDTHS[0]
    S, idx, val = _cases(qg, w)
    assert qg.argmax_rows_plan(3, w) > 1 and qg.argmax_rows_plan(256, w) == 1
    pick = np.arange(256) % S.shape[0]
    _run(qg, S[pick], idx[pick], val[pick], w + 5, 3, device, "256 rows")
    _run(qg, S[:3], idx[:3], val[:3], w + 5, 3, device, "3 rows")


def test_argument_checks(qg, oracle, device):
    L = qg.load()
    w = SPLIT_WIDTHS[0]
    S_np = _cases(qg, w)[0][:2]
    parent, S = _window(S_np, w + 1, 0, device)
    idx = torch.full((2,), -1, dtype=torch.int32, device=device)
    val = torch.full((2,), float("nan"), device=device)
    need = L.qgemm_argmax_rows_workspace_size(2, w)
    assert need == 8 * 2 * qg.argmax_rows_plan(2, w)
    ws = torch.zeros(need, dtype=torch.uint8, device=device)
    s = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def call(S_ptr=S.data_ptr(), rows=2, idx_ptr=idx.data_ptr(), val_ptr=val.data_ptr(), ws_ptr=ws.data_ptr(),
             ws_bytes=need, stride=w + 1, width=w):
        return L.qgemm_argmax_rows(S_ptr, stride, rows, width, idx_ptr, val_ptr, ws_ptr, ws_bytes, s)

    assert call(rows=0) == 0                                   # nothing to do, nothing touched
    assert call(ws_bytes=need - 1) == INVALID                  # a short workspace
    assert call(ws_ptr=None) == INVALID
    assert call(S_ptr=None) == INVALID and call(idx_ptr=None) == INVALID
    assert call(rows=-1) == INVALID and call(width=0) == INVALID and call(stride=w - 1) == INVALID
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -1).all() and np.isnan(val.cpu().numpy()).all()
    assert call(val_ptr=None) == 0                             # val is optional
    torch.cuda.synchronize()
    want_idx, _ = head_oracle.argmax_rows_ref(S_np)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.isnan(val.cpu().numpy()).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(val.cpu().numpy().view(np.uint32), _cases(qg, w)[2][:2].view(np.uint32))
