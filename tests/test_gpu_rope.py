"""qgemm_rope_rows / qgemm_rope_rows_varlen on the device (rope.hip), bit for bit against
rope_oracle.rope_rows.  The tables are random, not real cosines, so a swapped c / s or a swapped sign shows; the rows are
a strided window of a NaN-filled parent, which must be unchanged outside the window.  d_k 2, 4, 6 take the pair path,
8 .. 128 the float4 path where the base and the stride are aligned and the pair path where they are not."""
import functools

import numpy as np
import pytest
import torch

import rope_oracle as RO
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
TABLE_ROWS = 24


@functools.lru_cache(maxsize=None)
def _tables(d_k):
    rng = np.random.default_rng(1000 + d_k)
    c, s = (rng.standard_normal((TABLE_ROWS, d_k // 2)).astype(F) for _ in range(2))
    c.flags.writeable = s.flags.writeable = False
    return c, s


def _window(rows, w, device, seed, pad=3, lead=0, extra_rows=0):
    """(parent, view, values): a NaN-filled parent whose window of rows x w floats -- row stride w + pad, `lead` floats
    into the allocation -- holds seeded values."""
    rng = np.random.default_rng(seed)
    vals = (rng.standard_normal((rows, w)) * 2.0).astype(F)
    stride = w + pad
    flat = torch.full(((rows + extra_rows) * stride + lead + 8,), float("nan"), device=device)
    view = flat[lead:lead + rows * stride].view(rows, stride)[:, :w]
    view.copy_(torch.from_numpy(vals))
    return flat, view, vals


def _check_window(flat, view, before, want, what):
    """the window is `want`, every float of the parent outside it is what it was (NaN payloads included)"""
    assert_bits_equal(view.cpu().numpy(), want, what)
    mask = torch.ones_like(flat, dtype=torch.bool)
    lead = (view.data_ptr() - flat.data_ptr()) // 4
    rows, w = view.shape
    idx = (lead + torch.arange(rows, device=flat.device)[:, None] * view.stride(0) +
           torch.arange(w, device=flat.device)[None, :]).reshape(-1)
    mask[idx] = False
    assert torch.equal(flat.view(torch.int32)[mask], before.view(torch.int32)[mask]), f"{what}: outside the window"


@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("groups", [1, 3, 8])
@pytest.mark.parametrize("d_k", [2, 4, 6, 8, 16, 64, 128])
def test_rope_rows_matches_the_oracle(qg, device, d_k, groups, rows):
    cos, sin = _tables(d_k)
    c, s = (torch.from_numpy(np.array(t)).to(device) for t in (cos, sin))
    w = groups * d_k
    for pos0 in (0, 7, TABLE_ROWS - rows):
        # pad 4: an aligned stride (the float4 path where d_k % 8 == 0); pad 3 or a base one float in: the pair path
        for pad, lead in ((4, 0), (3, 0), (4, 1)):
            flat, view, vals = _window(rows, w, device, 7 * d_k + groups + rows + pos0, pad, lead)
            before = flat.clone()
            assert qg.rope_rows(view, groups, d_k, c, s, pos0) is view
            _check_window(flat, view, before, RO.rope_rows(vals, groups, d_k, cos, sin, pos0),
                          f"rope_rows d_k={d_k} groups={groups} rows={rows} pos0={pos0} pad={pad} lead={lead}")


@pytest.mark.parametrize("d_k", [6, 16])
def test_nan_and_inf_inputs(qg, device, d_k):
    cos, sin = _tables(d_k)
    rng = np.random.default_rng(3)
    vals = rng.standard_normal((5, 3 * d_k)).astype(F)
    vals[0, 0], vals[1, d_k // 2], vals[2, 1], vals[3, d_k - 1], vals[4, d_k] = np.nan, np.inf, -np.inf, np.inf, np.nan
    vals[3, d_k // 2 - 1] = np.inf   # inf c - inf s: NaN or inf by the signs, as the operations give
    X = torch.from_numpy(vals).to(device)
    qg.rope_rows(X, 3, d_k, *(torch.from_numpy(np.array(t)).to(device) for t in (cos, sin)), 2)
    assert_bits_equal(X.cpu().numpy(), RO.rope_rows(vals, 3, d_k, cos, sin, 2), f"non-finite inputs d_k={d_k}")


@pytest.mark.parametrize("d_k,pad", [(16, 4), (16, 3), (6, 0)])
def test_varlen_three_sequences_with_gaps(qg, device, d_k, pad):
    """4, 1 and 6 rows at positions 5, 0, 3, two untouched rows between them; equal to per-sequence calls."""
    cos, sin = _tables(d_k)
    c, s = (torch.from_numpy(np.array(t)).to(device) for t in (cos, sin))
    groups, n_rows, pos0, row0 = 3, (4, 1, 6), (5, 0, 3), (0, 6, 9)
    flat, view, vals = _window(15, groups * d_k, device, 77 + d_k, pad)
    view[4:6] = float("nan")
    view[7:9] = float("nan")
    before, alone = flat.clone(), view.clone()
    want = view.cpu().numpy().copy()
    for r0, n, p in zip(row0, n_rows, pos0):
        want[r0:r0 + n] = RO.rope_rows(vals[r0:r0 + n], groups, d_k, cos, sin, p)
        qg.rope_rows(alone[r0:r0 + n], groups, d_k, c, s, p)
    qg.rope_rows_varlen(view, groups, d_k, c, s, row0, n_rows, pos0)
    _check_window(flat, view, before, want, f"varlen d_k={d_k} pad={pad}")
    assert torch.equal(view.contiguous().view(torch.int32), alone.view(torch.int32)), "varlen against rope_rows calls"


def test_varlen_sixty_four_sequences_of_one_row(qg, device):
    d_k, groups = 8, 2
    cos, sin = _tables(d_k)
    flat, view, vals = _window(64, groups * d_k, device, 5, 4)
    pos = [(5 * b) % TABLE_ROWS for b in range(64)]
    c, s = (torch.from_numpy(np.array(t)).to(device) for t in (cos, sin))
    qg.rope_rows_varlen(view, groups, d_k, c, s, list(range(64)), [1] * 64, pos)
    assert_bits_equal(view.cpu().numpy(), RO.rope_rows(vals, groups, d_k, cos, sin, np.array(pos)), "64 sequences")


def test_a_captured_launch_replays_the_same_bits(qg, device):
    L = qg.load()
    d_k, groups, rows = 16, 4, 5
    cos, sin = _tables(d_k)
    c, s = (torch.from_numpy(np.array(t)).to(device) for t in (cos, sin))
    vals = (np.random.default_rng(9).standard_normal((rows, groups * d_k))).astype(F)
    want = RO.rope_rows(vals, groups, d_k, cos, sin, 7)
    src = torch.from_numpy(vals).to(device)
    X = src.clone()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device)
    with torch.cuda.stream(st):
        qg.rope_rows(X, groups, d_k, c, s, 7)   # the warm-up
        st.synchronize()
        assert_bits_equal(X.cpu().numpy(), want, "the eager launch")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            rc = L.qgemm_rope_rows(X.data_ptr(), X.stride(0), rows, groups, d_k, c.data_ptr(), s.data_ptr(), TABLE_ROWS, 7,
                                   st.cuda_stream)
            assert rc == 0
    for i in range(2):
        X.copy_(src)   # the operation is in place: restore the input
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits_equal(X.cpu().numpy(), want, f"replay {i}")
