"""GPU parity of the grouped-query decode kernel (attention_decode_gqa_kernel) through
qgemm_attention_gqa, qgemm_attention_decode_batched_gqa and _indirect_gqa: bit for bit tests/attn_oracle.py and
tests/causal_oracle.py on K and V with every head repeated G = n_heads / n_kv_heads times.  Every case first asserts its
plan name; outputs are pre-filled with NaN, the workspace with 0xFF bytes that must stay.  A workgroup owns up to four
query heads of one KV head, stages 128-key chunks and sums in passes of 1024 elements: the shapes stand on both sides
of each of these edges, with full and partial blocks of heads at both row widths."""
import ctypes

import numpy as np
import pytest
import torch

import attn_oracle
import causal_oracle
from decode_table_cases import check_unmasked_tables
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

# (seq_q, seq_kv, heads, kv heads, d_k, q_pos0[, how]); q_pos0 None: no mask
CASES = (
    (1, 1, 2, 1, 64, 0),              # one key
    (1, 129, 3, 1, 128, 128),         # a partial block of 3 heads, one key past a chunk
    (1, 1025, 4, 1, 64, 1024),        # past a 1024-element sum pass, on all four waves
    (1, 4096, 4, 1, 128, 4095),       # the key limit: full LDS at the wide width
    (3, 40, 10, 2, 96, 37),           # G = 5: blocks of 4 and 1, two KV heads, the upper half-wave idle at d_k 96
    (8, 600, 8, 1, 128, 592),         # G = 8: two full blocks
    (4, 100, 7, 1, 32, 10),           # G = 7, narrow, most keys hidden
    (2, 77, 4, 2, 20, None),          # unmasked, d_k no multiple of 4: the scalar loads
    (5, 513, 6, 2, 128, None),
    (2, 140, 6, 2, 128, 138, "slices"),   # K / V as misaligned column slices with an odd stride
    (4, 100, 4, 1, 128, 10, 3),       # +inf in V at a masked key, in a column of the low half ...
    (4, 100, 4, 1, 128, 10, 100),     # ... and of the high half
)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _plan(dk):
    return "attention_decode_gqa_kernel" if dk <= 64 else "attention_decode_gqa_wide_kernel"


def _qkv(seq_q, seq_kv, H, n_kv, dk, seed):
    return O.uniform((seq_q, H * dk), seed), O.uniform((seq_kv, n_kv * dk), seed + 1), O.uniform((seq_kv, n_kv * dk), seed + 2)


def _want(Q, K, V, H, n_kv, q_pos0):
    """the oracle on K and V with every head repeated H / n_kv times"""
    dk = Q.shape[1] // H
    Kr, Vr = (np.repeat(a.reshape(len(a), n_kv, dk), H // n_kv, axis=1).reshape(len(a), -1) for a in (K, V))
    scale = attn_oracle.default_scale(dk)
    if q_pos0 is None:
        return attn_oracle.attention_ref(Q, Kr, Vr, H, scale)
    return causal_oracle.attention_causal_ref(Q, Kr, Vr, H, scale, q_pos0)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_gqa_decode_bit_exact(qg, oracle, device, case):
    """how "slices": K and V 4 bytes past a 16-byte boundary with an odd row stride; how a column: +inf in V there at key
    50, masked for every row -- 0 * inf = NaN in that column of EVERY query head, the rest finite"""
    (seq_q, seq_kv, H, n_kv, dk, q_pos0), how = case[:6], case[6] if len(case) > 6 else None
    assert qg.attention_gqa_plan(seq_q, seq_kv, H, n_kv, dk) == _plan(dk)
    Q, K, V = _qkv(seq_q, seq_kv, H, n_kv, dk, 701)
    if isinstance(how, int):
        V[50, how] = np.inf
    want = _want(Q, K, V, H, n_kv, q_pos0)
    if isinstance(how, int):
        cols = [h * dk + how for h in range(H)]
        assert np.isnan(want[:, cols]).all() and np.isfinite(np.delete(want, cols, axis=1)).all()
    Qd, Kd, Vd = _dev(Q, device), _dev(K, device), _dev(V, device)
    if how == "slices":
        wk, wv = (torch.zeros((seq_kv, n_kv * dk + 7), device=device) for _ in range(2))
        wk[:, 1:1 + n_kv * dk], wv[:, 1:1 + n_kv * dk] = Kd, Vd
        Kd, Vd = wk[:, 1:1 + n_kv * dk], wv[:, 1:1 + n_kv * dk]
    L = qg.load()
    assert L.qgemm_attention_gqa_workspace_size(seq_q, seq_kv, H, n_kv, dk) == 0
    ws = torch.full((64,), 0xFF, dtype=torch.uint8, device=device)
    out = torch.full((seq_q, H * dk), float("nan"), device=device)
    rc = L.qgemm_attention_gqa(Qd.data_ptr(), Qd.stride(0), Kd.data_ptr(), Kd.stride(0), Vd.data_ptr(), Vd.stride(0),
                               out.data_ptr(), out.stride(0), seq_q, seq_kv, H, n_kv, dk, attn_oracle.default_scale(dk),
                               q_pos0 is not None, q_pos0 or 0, ws.data_ptr(), 64,
                               torch.cuda.current_stream(device).cuda_stream)
    assert rc == 0, f"qgemm_attention_gqa returned {rc}"
    assert bool((ws == 0xFF).all()), "the decode launch wrote into the workspace"
    assert_bits_equal(out.cpu().numpy(), want, f"gqa decode attention {case}")


ROWS = 2


def _sequences(seq_kv, H, n_kv, dk):   # per sequence (Q, K, V, q_pos0): the last of its rows sees every key
    return [_qkv(ROWS, n, H, n_kv, dk, 731 + 10 * b) + (max(n - ROWS, 0),) for b, n in enumerate(seq_kv)]


def _check_sequences(qg, call, seqs, H, n_kv, dk, device, what):
    assert qg.attention_gqa_plan(ROWS, max(len(s[1]) for s in seqs), H, n_kv, dk) == _plan(dk)
    out = torch.full((len(seqs) * ROWS, H * dk), float("nan"), device=device)
    call(_dev(np.concatenate([s[0] for s in seqs]), device), [s[3] for s in seqs], out)
    got = out.cpu().numpy()
    for b, (Q, K, V, p) in enumerate(seqs):
        assert_bits_equal(got[b * ROWS:(b + 1) * ROWS], _want(Q, K, V, H, n_kv, p), f"{what}: sequence {b}")
    return got


def _slabs(seqs, slot_of, n_slabs, width):
    """K and V slabs, NaN where no sequence's row lies: row j of sequence b in slab slot_of(b, j)"""
    rows = max(len(s[1]) for s in seqs) + 3
    K, V = (np.full((n_slabs, rows, width), np.nan, np.float32) for _ in range(2))
    for b, (_, Kb, Vb, _) in enumerate(seqs):
        j = np.arange(len(Kb))
        K[slot_of(b, j), j], V[slot_of(b, j), j] = Kb, Vb
    return K, V


@pytest.mark.parametrize("heads", [(8, 2, 128), (6, 2, 64)], ids=str)
def test_batched_and_indirect(qg, oracle, device, heads):
    """3 sequences of 1, 128 and 300 keys: the batched launch on permuted slabs; the indirect launch through a table
    that interleaves two slabs per sequence, with the entry 6 of 6 slabs at the visible key 200 of the last sequence
    (its rows NaN, the others finite); and the identity table, which must give the batched launch's bits."""
    H, n_kv, dk = heads
    seq_kv, kv_slot = [1, 128, 300], [2, 0, 3]
    seqs = _sequences(seq_kv, H, n_kv, dk)
    K, V = _slabs(seqs, lambda b, j: kv_slot[b], 4, n_kv * dk)
    Kd, Vd = _dev(K, device), _dev(V, device)
    batched = _check_sequences(qg, lambda Q, p, out: qg.attention_decode_batched_gqa(
        Q, Kd, Vd, H, n_kv, seq_kv, q_pos0=p, kv_slot=kv_slot, rows_per_seq=ROWS, O=out), seqs, H, n_kv, dk, device, "batched")
    ident = np.repeat(np.arange(4, dtype=np.uint8)[:, None], K.shape[1], axis=1)
    same = _check_sequences(qg, lambda Q, p, out: qg.attention_decode_indirect(
        Q, Kd, Vd, H, _dev(ident, device), seq_kv, q_pos0=p, tab_row=kv_slot, rows_per_seq=ROWS, O=out, n_kv_heads=n_kv),
        seqs, H, n_kv, dk, device, "identity table")
    assert_bits_equal(same, batched, "indirect with the identity table against batched")
    Ki, Vi = _slabs(seqs, lambda b, j: 2 * b + (j & 1), 6, n_kv * dk)
    own = np.full((3, Ki.shape[1]), 255, np.uint8)
    for b, n in enumerate(seq_kv):
        own[b, :n] = 2 * b + (np.arange(n) & 1)
    own[2, 200] = 6
    seqs[2][1][200], seqs[2][2][200] = np.nan, np.nan
    Kd, Vd = _dev(Ki, device), _dev(Vi, device)
    got = _check_sequences(qg, lambda Q, p, out: qg.attention_decode_indirect(
        Q, Kd, Vd, H, _dev(own, device), seq_kv, q_pos0=p, rows_per_seq=ROWS, O=out, n_kv_heads=n_kv),
        seqs, H, n_kv, dk, device, "indirect")
    assert np.isfinite(got[:2 * ROWS]).all() and np.isnan(got[2 * ROWS:]).all()


def test_batched_64_sequences(qg, oracle, device):
    H, n_kv, dk = 6, 2, 64
    seqs = _sequences([1 + (37 * b) % 290 for b in range(64)], H, n_kv, dk)
    K, V = _slabs(seqs, lambda b, j: 63 - b, 64, n_kv * dk)
    Kd, Vd = _dev(K, device), _dev(V, device)
    _check_sequences(qg, lambda Q, p, out: qg.attention_decode_batched_gqa(
        Q, Kd, Vd, H, n_kv, [len(s[1]) for s in seqs], q_pos0=p, kv_slot=[63 - b for b in range(64)], rows_per_seq=ROWS,
        O=out), seqs, H, n_kv, dk, device, "64 sequences")


def test_graph_capture_and_replay(qg, oracle, device):
    """The batched launch allocates nothing, copies nothing and does not synchronize: captured once, replayed twice after
    Q, K and V change, each replay against the oracle."""
    H, n_kv, dk, seq_kv, kv_slot = 6, 2, 128, [100, 129, 9], [1, 2, 0]
    d, w, rows = H * dk, n_kv * dk, 132
    Qs, out = torch.zeros((3 * ROWS, d), device=device), torch.full((3 * ROWS, d), float("nan"), device=device)
    Ks, Vs = torch.zeros((3, rows, w), device=device), torch.zeros((3, rows, w), device=device)
    L = qg.load()
    ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731

    def call(stream):
        assert L.qgemm_attention_decode_batched_gqa(
            Qs.data_ptr(), d, Ks.data_ptr(), w, rows * w, Vs.data_ptr(), w, rows * w, out.data_ptr(), d, 3, ROWS,
            ints(kv_slot), ints(seq_kv), ints([n - ROWS for n in seq_kv]), H, n_kv, dk, attn_oracle.default_scale(dk),
            stream) == 0

    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        call(s.cuda_stream)      # warm-up: module load, first launch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call(s.cuda_stream)
    for i in range(2):
        seqs = [_qkv(ROWS, n, H, n_kv, dk, 761 + 50 * i + 10 * b) for b, n in enumerate(seq_kv)]
        Qs.copy_(_dev(np.concatenate([q for q, _, _ in seqs]), device))
        for (_, Kb, Vb), slot in zip(seqs, kv_slot):
            Ks[slot, :len(Kb)], Vs[slot, :len(Vb)] = _dev(Kb, device), _dev(Vb, device)
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for b, (Q, Kb, Vb) in enumerate(seqs):
            assert_bits_equal(got[b * ROWS:(b + 1) * ROWS], _want(Q, Kb, Vb, H, n_kv, seq_kv[b] - ROWS),
                              f"graph replay {i}, sequence {b}")


# (rows per sequence, seq_kv, heads, kv heads, d_k, sliced): unmasked, two sequences on one K / V history -- 129 and 300
# keys (one key past a chunk; three chunks, so both prefetch buffers and both parities of the K chunk count), G = 3 (a
# block of three heads) and G = 5 (a second block of one head), both widths, vector and element loads
UNMASKED = ((1, (129, 300), 6, 2, 64, False), (3, (300, 129), 10, 2, 20, True),
            (3, (129, 300), 6, 2, 96, False), (1, (300, 129), 10, 2, 128, True))


@pytest.mark.parametrize("case", UNMASKED, ids=str)
def test_unmasked_batched_and_indirect(qg, oracle, device, case):
    """attention_decode_gqa_kernel<false, DecodeMany | DecodeIndirect, 64 | 128> (decode_table_cases.py)"""
    rows, seq_kv, H, n_kv, dk, sliced = case
    assert qg.attention_gqa_plan(rows, max(seq_kv), H, n_kv, dk) == _plan(dk)
    check_unmasked_tables(
        device, rows, seq_kv, H, n_kv, dk, sliced, torch.float32,
        lambda Q, K, V, n, slot, out: qg.attention_decode_batched_gqa(Q, K, V, H, n_kv, n, kv_slot=slot, rows_per_seq=rows, O=out),
        lambda Q, K, V, tab, n, out: qg.attention_decode_indirect(Q, K, V, H, tab, n, rows_per_seq=rows, O=out, n_kv_heads=n_kv),
        lambda Q, K, V: _want(Q, K, V, H, n_kv, None), 761)
