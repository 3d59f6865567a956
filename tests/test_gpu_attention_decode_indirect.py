"""GPU parity of qgemm_attention_decode_indirect (attention_decode_kernel<., DecodeIndirect>): the decode
attention reading every K / V row through a per-row slab table.  For every sequence three results are compared bit for
bit: the indirect call, attention_decode_batched on slabs gathered on the host (tests/beam_indirect_oracle.gather) and
the CPU oracles on the gathered rows.  The slabs hold finite values only where a table entry of the call points, NaN
everywhere else, and one slab is named by no entry; every output is pre-filled with NaN."""
import ctypes

import numpy as np
import pytest
import torch

import attn_oracle
import beam_indirect_oracle as BI
import causal_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu
INVALID = 1


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _slabs(own, tab_row, seq_kv, n_slabs, d, seed, rows=None):
    """K and V as [n_slabs, rows, d]: seeded values at (own[t][j], j) for every table row t and key j < seq_kv the call
    reads, NaN everywhere else."""
    rows = max(seq_kv) + 3 if rows is None else rows
    K, V = O.uniform((n_slabs, rows, d), seed).copy(), O.uniform((n_slabs, rows, d), seed + 1).copy()
    used = np.zeros((n_slabs, rows), bool)
    for t, n in zip(tab_row, seq_kv):
        ok = own[t, :n] < n_slabs
        used[own[t, :n][ok], np.arange(n)[ok]] = True
    K[~used], V[~used] = np.nan, np.nan
    return K, V


def _random_table(n_rows, width, n_from, seed):
    return np.random.default_rng(seed).integers(0, n_from, (n_rows, width)).astype(np.uint8)


def _want(Q, K, V, H, q_pos0):
    scale = attn_oracle.default_scale(Q.shape[1] // H)
    if q_pos0 is None:
        return attn_oracle.attention_ref(Q, K, V, H, scale)
    return causal_oracle.attention_causal_ref(Q, K, V, H, scale, q_pos0)


def _check(qg, device, Q, K, V, own, H, seq_kv, q_pos0, tab_row, r, what, cpu=True, Qd=None, Kd=None, Vd=None, ownd=None,
           out=None):
    """One indirect call into a NaN-filled output against the batched call on host-gathered slabs and, with cpu,
    against the oracle on every sequence's gathered rows.  Returns the output."""
    n = len(seq_kv)
    rows_of = list(range(n)) if tab_row is None else tab_row
    Qd = _dev(Q, device) if Qd is None else Qd
    Kd = _dev(K, device) if Kd is None else Kd
    Vd = _dev(V, device) if Vd is None else Vd
    ownd = _dev(own, device) if ownd is None else ownd
    out = _nan(Q.shape, device) if out is None else out
    got_t = qg.attention_decode_indirect(Qd, Kd, Vd, H, ownd, seq_kv, q_pos0=q_pos0, tab_row=tab_row, rows_per_seq=r,
                                         O=out)
    assert got_t is out
    got = out.cpu().numpy()
    Kg, Vg = BI.gather(K, own, rows_of, seq_kv), BI.gather(V, own, rows_of, seq_kv)
    flat = _nan(Q.shape, device)
    qg.attention_decode_batched(_dev(Q, device), _dev(Kg, device), _dev(Vg, device), H, seq_kv, q_pos0=q_pos0,
                                rows_per_seq=r, O=flat)
    assert_bits_equal(got, flat.cpu().numpy(), f"{what}: against the batched call on gathered slabs")
    if cpu:
        for b in range(n):
            rows = slice(b * r, (b + 1) * r)
            want = _want(Q[rows], Kg[b, :seq_kv[b]], Vg[b, :seq_kv[b]], H, None if q_pos0 is None else q_pos0[b])
            assert_bits_equal(got[rows], want, f"{what}: sequence {b} against the oracle")
    return got


def test_chunk_boundaries_random_table(qg, oracle, device):
    """Lengths 1, 127, 128, 129 and 300 (one, one, one, two and three chunks: both register-buffer parities), every key's
    slab drawn from five of six slabs, the sequences' table rows permuted inside a larger table."""
    H, dk = 2, 32
    seq_kv, tab_row = [1, 127, 128, 129, 300], [6, 0, 3, 1, 4]
    own = _random_table(7, 303, 5, 700)
    assert (np.diff(own[4, :300].astype(int)) != 0).mean() > 0.7, "the slab changes at nearly every key"
    K, V = _slabs(own, tab_row, seq_kv, 6, H * dk, 701)
    assert np.isnan(K[5]).all() and np.isnan(K[:5]).any()
    Q = O.uniform((5, H * dk), 703)
    got = _check(qg, device, Q, K, V, own, H, seq_kv, [n - 1 for n in seq_kv], tab_row, 1, "chunk boundaries")
    assert np.isfinite(got).all()


def test_slab_changes_at_the_chunk_edges_alone(qg, oracle, device):
    H, dk = 2, 32
    own = np.zeros((1, 300), np.uint8)
    own[0, :128], own[0, 128:256], own[0, 256:] = 2, 0, 3
    K, V = _slabs(own, [0], [300], 5, H * dk, 711)
    Q = O.uniform((1, H * dk), 713)
    assert np.isfinite(_check(qg, device, Q, K, V, own, H, [300], [299], None, 1, "edges")).all()


def test_identity_and_one_other_slab_equal_kv_slot(qg, oracle, device):
    """own[b][j] = b is the batched call with the default slabs, own[b][j] = s[b] the batched call with kv_slot = s."""
    H, dk, r = 2, 16, 2
    seq_kv, q_pos0 = [70, 129, 5], [68, 100, 3]
    Q = O.uniform((3 * r, H * dk), 720)
    for kv_slot in ([0, 1, 2], [3, 0, 3]):
        own = np.repeat(np.array(kv_slot, np.uint8)[:, None], 140, axis=1)
        K, V = _slabs(own, [0, 1, 2], seq_kv, 4, H * dk, 721)
        got = _check(qg, device, Q, K, V, own, H, seq_kv, q_pos0, None, r, f"kv_slot {kv_slot}", cpu=False)
        direct = _nan(Q.shape, device)
        qg.attention_decode_batched(_dev(Q, device), _dev(K, device), _dev(V, device), H, seq_kv, q_pos0=q_pos0,
                                    kv_slot=kv_slot, rows_per_seq=r, O=direct)
        assert_bits_equal(got, direct.cpu().numpy(), f"kv_slot {kv_slot}: against the batched call with kv_slot")
        assert np.isfinite(got).all()


def test_eight_rows_masked_and_three_unmasked(qg, oracle, device):
    seq_kv = [8, 136, 513]
    own = _random_table(3, 513, 3, 730)
    for H, dk, r, q_pos0 in ((2, 8, 8, [0, 100, 505]), (2, 24, 3, None)):
        K, V = _slabs(own, [0, 1, 2], seq_kv, 4, H * dk, 731)
        Q = O.uniform((3 * r, H * dk), 733)
        got = _check(qg, device, Q, K, V, own, H, seq_kv, q_pos0, None, r, f"{r} rows, q_pos0 {q_pos0}")
        assert np.isfinite(got).all()


def test_scalar_load_path_and_column_slices(qg, oracle, device):
    """d_k 12; K / V column slices that start 4 bytes past a 16-byte boundary with an odd row stride (scalar loads)."""
    H, dk, r = 2, 12, 2
    d = H * dk
    seq_kv, tab_row, q_pos0 = [40, 130, 7], [2, 0, 1], [38, 100, 5]
    own = _random_table(3, 133, 3, 740)
    K, V = _slabs(own, tab_row, seq_kv, 4, d, 741)
    Q = O.uniform((3 * r, d), 743)
    wk, wv = (torch.zeros(K.shape[:2] + (d + 5,), device=device) for _ in range(2))
    wk[:, :, 1:1 + d], wv[:, :, 1:1 + d] = _dev(K, device), _dev(V, device)
    sentinel = -12345.5
    wide_o = torch.full((3 * r + 2, d + 11), sentinel, device=device)
    _check(qg, device, Q, K, V, own, H, seq_kv, q_pos0, tab_row, r, "column slices", Kd=wk[:, :, 1:1 + d],
           Vd=wv[:, :, 1:1 + d], out=wide_o[1:1 + 3 * r, 5:5 + d])
    w = wide_o.cpu().numpy()
    mask = np.ones(w.shape, bool)
    mask[1:1 + 3 * r, 5:5 + d] = False
    assert (w[mask] == np.float32(sentinel)).all(), "elements outside the output slice were written"


def test_table_views(qg, oracle, device):
    """A table view whose base is 1 byte past a 16-byte boundary with an odd row stride (the staging copy's offset), and
    a table whose row stride is exactly seq_kv (nothing past a row's entries belongs to it)."""
    H, dk = 2, 16
    seq_kv, q_pos0 = [129, 129, 129], [128, 60, 0]
    own = _random_table(3, 129, 4, 750)
    K, V = _slabs(own, [0, 1, 2], seq_kv, 5, H * dk, 751)
    Q = O.uniform((3, H * dk), 753)
    wide = torch.full((4, 151), 255, dtype=torch.uint8, device=device)
    wide[:3, 1:130] = _dev(own, device)
    view = wide[:3, 1:130]
    assert view.data_ptr() % 16 == 1 and view.stride(0) % 2 == 1
    a = _check(qg, device, Q, K, V, own, H, seq_kv, q_pos0, None, 1, "offset view", ownd=view)
    tight = _dev(own, device)
    assert tight.stride(0) == 129
    b = _check(qg, device, Q, K, V, own, H, seq_kv, q_pos0, None, 1, "stride == seq_kv", cpu=False, ownd=tight)
    assert_bits_equal(a, b, "the two views")
    assert np.isfinite(a).all()


def test_far_end_of_the_table(qg, oracle, device):
    H, dk = 1, 8
    seq_kv = [4096, 3969]
    own = _random_table(2, 4096, 3, 760)
    K, V = _slabs(own, [0, 1], seq_kv, 4, dk, 761, rows=4096)
    Q = O.uniform((2, dk), 763)
    got = _check(qg, device, Q, K, V, own, H, seq_kv, [4095, 3968], None, 1, "4096 and 3969 keys")
    assert np.isfinite(got).all()
    # the same rows from a start 1 byte past a 16-byte boundary: 4096 entries then span 257 aligned pieces
    wide = torch.full((2, 4113), 255, dtype=torch.uint8, device=device)
    wide[:, 1:4097] = _dev(own, device)
    off = _check(qg, device, Q, K, V, own, H, seq_kv, [4095, 3968], None, 1, "4096 keys, offset table", cpu=False,
                 ownd=wide[:, 1:4097])
    assert_bits_equal(off, got, "the offset table")


def test_two_sequences_share_a_table_row(qg, oracle, device):
    H, dk = 2, 8
    own = _random_table(2, 140, 3, 770)
    K, V = _slabs(own, [1, 1], [140, 90], 4, H * dk, 771)
    Q = O.uniform((2, H * dk), 773)
    assert np.isfinite(_check(qg, device, Q, K, V, own, H, [140, 90], [139, 40], [1, 1], 1, "shared row")).all()


def test_entries_that_name_no_slab_read_as_nan_rows(qg, oracle, device):
    """255 and n_slabs itself, at a visible key, at a masked key and in the last chunk: the output is the batched call's
    on slabs with quiet-NaN rows planted there (BI.gather plants them), and the call returns normally.  The
    neighbouring sequence, whose entries are all valid, stays finite."""
    H, dk, n_slabs = 2, 16, 4
    seq_kv, q_pos0 = [300, 300, 200], [299, 150, 199]
    own = _random_table(3, 300, n_slabs, 780)
    own[0, 10], own[0, 290] = 255, n_slabs       # visible, and visible in the last chunk
    own[1, 200] = 255                            # masked (q_pos0 150): P = +0 there, P V still meets the NaN
    K, V = _slabs(own, [0, 1, 2], seq_kv, n_slabs, H * dk, 781)
    Q = O.uniform((3, H * dk), 783)
    got = _check(qg, device, Q, K, V, own, H, seq_kv, q_pos0, None, 1, "invalid entries")
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and np.isfinite(got[2]).all()
    torch.cuda.synchronize()


def test_refusals_touch_nothing(qg, device):
    H, dk, r, n = 2, 8, 1, 2
    d = H * dk
    L = qg.load()
    Q, K, V = (torch.zeros(s, device=device) for s in ((n * r, d), (3, 40, d), (3, 40, d)))
    own = torch.zeros((2, 40), dtype=torch.uint8, device=device)
    out = torch.full((n * r, d), 7.5, device=device)
    ints = lambda v: None if v is None else (ctypes.c_int * len(v))(*v)

    def call(q=Q, k=K, v=V, o=out, table=own.data_ptr(), stride=40, n_slabs=3, tab_row=(0, 1), seq_kv=(40, 9),
             q_pos0=(39, 8), n_seqs=n, rows=r, heads=H, d_k=dk):
        return L.qgemm_attention_decode_indirect(
            None if q is None else q.data_ptr(), d, None if k is None else k.data_ptr(), d, 40 * d,
            None if v is None else v.data_ptr(), d, 40 * d, None if o is None else o.data_ptr(), d, n_seqs, rows, table,
            stride, n_slabs, ints(tab_row), ints(seq_kv), ints(q_pos0), heads, d_k, 1.0, None)

    bad = [dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(seq_kv=None), dict(n_seqs=-1), dict(n_seqs=65),
           dict(rows=0), dict(rows=9), dict(d_k=0), dict(d_k=65), dict(heads=0), dict(seq_kv=(0, 9)),
           dict(seq_kv=(4097, 9), stride=4097), dict(q_pos0=(-1, 0)),
           dict(table=None), dict(n_slabs=0), dict(n_slabs=65), dict(stride=39), dict(tab_row=(0, -1))]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.5).all(), "a refused call wrote the output"
    assert call(n_seqs=0) == 0 and call() == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() != 7.5).all()
