"""GPU parity of the fused grouped-query prefill kernel (attention_fused_gqa_kernel) through
qgemm_attention_varlen_gqa: bit for bit tests/attn_oracle.py and tests/causal_oracle.py on K and V with every head
repeated G = n_heads / n_kv_heads times (_want of tests/test_gpu_attention_decode_gqa.py).  Every case first asserts its
plan name and that the call needs no workspace; outputs are pre-filled with NaN.  The kernel stages 256-key chunks at
row width 64 and 128-key chunks at 128, 32 query rows per workgroup: the shapes stand on both sides of these edges."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attn_oracle
from test_gpu_attention_decode_gqa import _dev, _qkv, _want
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

NARROW, WIDE, PER_SEQ = "attention_fused_gqa_kernel<many>", "attention_fused_gqa_wide_kernel<many>", "per_sequence"

# (seq_q, seq_kv, heads, kv heads, d_k, q_pos0[, how]); q_pos0 None: no mask
CASES = (
    (1, 1, 2, 1, 64, None),                # one key
    (33, 40, 6, 2, 64, 0),                 # two query tiles, the second partial, G = 3, causal
    (9, 257, 8, 2, 64, None),              # one key past a 256-key chunk
    (17, 129, 3, 1, 96, None),             # d_k 96, one key past a 128-key chunk, one KV head
    (40, 512, 4, 2, 128, 472),             # the key limit at the wide width, mask offset, skipped tiles
    (32, 100, 14, 2, 64, 68),              # G = 7
    (2, 50, 32, 1, 16, 48),                # G = 32, decode-shaped, d_k below a k-tile
    (20, 70, 4, 2, 128, None, "views"),    # K / V misaligned with an odd stride, Q / O column slices of wider buffers
    (20, 70, 4, 2, 128, 50, "inf"),        # +inf in V at key 69, masked for rows 0 .. 18
    (20, 70, 4, 2, 128, None, "nan"),      # a NaN in Q row 5 of head 1
)


def _plan(dk):
    return NARROW if dk <= 64 else WIDE


def _slice_of_wider(a, device, extra):
    """a as columns 1 .. of a buffer `extra` columns wider: 4 bytes past a 16-byte boundary, an odd row stride"""
    wide = torch.zeros((a.shape[0], a.shape[1] + extra), device=device)
    wide[:, 1:1 + a.shape[1]] = _dev(a, device)
    return wide[:, 1:1 + a.shape[1]]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_single_sequence_bit_exact(qg, oracle, device, case):
    (seq_q, seq_kv, H, n_kv, dk, q_pos0), how = case[:6], case[6] if len(case) > 6 else None
    assert qg.attention_varlen_gqa_plan([seq_q], [seq_kv], H, n_kv, dk) == _plan(dk)
    ints = lambda v: (ctypes.c_int * 1)(v)  # noqa: E731
    assert qg.load().qgemm_attention_varlen_gqa_workspace_size(1, ints(seq_q), ints(seq_kv), H, n_kv, dk) == 0
    Q, K, V = _qkv(seq_q, seq_kv, H, n_kv, dk, 801)
    if how == "inf":
        V[69, 3] = np.inf
    if how == "nan":
        Q[5, dk + 7] = np.nan
    want = _want(Q, K, V, H, n_kv, q_pos0)
    if how == "inf":   # 0 * inf = NaN wherever the key is masked (row 19 alone sees it: +inf), in every head of KV head 0
        cols = [h * dk + 3 for h in range(H // n_kv)]
        assert np.isnan(want[:19, cols]).all() and np.isinf(want[19, cols]).all()
        assert np.isfinite(np.delete(want, cols, axis=1)).all()
    if how == "nan":   # the NaN stays in its row and head
        bad = np.zeros(want.shape, bool)
        bad[5, dk:2 * dk] = True
        assert np.isnan(want[bad]).all() and np.isfinite(want[~bad]).all()
    Qd, Kd, Vd = _dev(Q, device), _dev(K, device), _dev(V, device)
    out = torch.full((seq_q, H * dk), float("nan"), device=device)
    if how == "views":
        Qd, Kd, Vd = _slice_of_wider(Q, device, 5), _slice_of_wider(K, device, 7), _slice_of_wider(V, device, 7)
        out = torch.full((seq_q, H * dk + 11), float("nan"), device=device)[:, 5:5 + H * dk]
    got = qg.attention_varlen_gqa(Qd, Kd, Vd, H, n_kv, [seq_q], [seq_kv], q_pos0=None if q_pos0 is None else [q_pos0],
                                  O=out)
    assert got is out
    assert_bits_equal(out.cpu().numpy(), want, f"fused gqa prefill {case}")


# four sequences (seq_q, seq_kv, q_pos0): the first empty; sequence 1 reads the first 33 of sequence 2's K / V rows
BATCH = ((0, 5, 0), (33, 33, 0), (7, 300, 293), (64, 512, 448))
Q_ROW0 = (2, 3, 40, 50)            # gaps of 2, 1, 4 and 3 rows in front of the sequences' query rows
KV_ROW0 = (1, 8, 8, 311)


@functools.lru_cache(maxsize=None)
def _batch(H, n_kv, dk, last_kv):
    """NaN-filled parents with the sequences' rows in them and the expected O (NaN where no sequence owns the row)"""
    seqs = BATCH[:3] + ((BATCH[3][0], last_kv, BATCH[3][2]),)
    Q = np.full((Q_ROW0[3] + seqs[3][0] + 2, H * dk), np.nan, np.float32)
    K, V = (np.full((KV_ROW0[3] + last_kv + 2, n_kv * dk), np.nan, np.float32) for _ in range(2))
    want = np.full(Q.shape, np.nan, np.float32)
    for b in (0, 2, 3):
        nq, nkv, _ = seqs[b]
        q, k, v = _qkv(nq, nkv, H, n_kv, dk, 831 + 10 * b)
        Q[Q_ROW0[b]:Q_ROW0[b] + nq], K[KV_ROW0[b]:KV_ROW0[b] + nkv], V[KV_ROW0[b]:KV_ROW0[b] + nkv] = q, k, v
    Q[Q_ROW0[1]:Q_ROW0[1] + 33] = _qkv(33, 1, H, n_kv, dk, 841)[0]
    for b, (nq, nkv, pos) in enumerate(seqs):
        if nq:
            ks = slice(KV_ROW0[b], KV_ROW0[b] + nkv)
            want[Q_ROW0[b]:Q_ROW0[b] + nq] = _want(Q[Q_ROW0[b]:Q_ROW0[b] + nq], K[ks], V[ks], H, n_kv, pos)
    return seqs, Q, K, V, want


def _run_batch(qg, device, H, n_kv, dk, last_kv, plan):
    seqs, Q, K, V, want = _batch(H, n_kv, dk, last_kv)
    seq_q, seq_kv, q_pos0 = ([s[i] for s in seqs] for i in range(3))
    assert qg.attention_varlen_gqa_plan(seq_q, seq_kv, H, n_kv, dk) == plan
    out = torch.full(Q.shape, float("nan"), device=device)
    qg.attention_varlen_gqa(_dev(Q, device), _dev(K, device), _dev(V, device), H, n_kv, seq_q, seq_kv, q_row0=Q_ROW0,
                            kv_row0=KV_ROW0, q_pos0=q_pos0, O=out)
    # every sequence's rows against the oracle on its own views; the rows no sequence owns still NaN
    assert_bits_equal(out.cpu().numpy(), want, f"batch at {H} / {n_kv} x {dk}, last sequence {last_kv} keys")


@pytest.mark.parametrize("dk", [128, 64])
def test_batch_of_four_sequences(qg, oracle, device, dk):
    _run_batch(qg, device, 6, 2, dk, 512, _plan(dk))


def test_outside_the_envelope_runs_per_sequence(qg, oracle, device):
    _run_batch(qg, device, 6, 2, 128, 513, PER_SEQ)


def test_one_head_per_group_is_attention_varlen(qg, oracle, device):
    Q, K, V = (_dev(a, device) for a in _qkv(45, 45, 2, 2, 64, 861))
    args = ([33, 12], [40, 5])
    got = qg.attention_varlen_gqa(Q, K, V, 2, 2, *args, q_pos0=[7, 0])
    assert_bits_equal(got.cpu().numpy(), qg.attention_varlen(Q, K, V, 2, *args, q_pos0=[7, 0]).cpu().numpy(), "G = 1")


def test_graph_capture_and_replay(qg, oracle, device):
    """The fused call allocates nothing, copies nothing and does not synchronize: captured once, each of two replays
    into a freshly NaN-filled O equals the eager call."""
    H, n_kv, dk = 6, 2, 128
    seqs, Q, K, V, _ = _batch(H, n_kv, dk, 512)
    Qd, Kd, Vd = _dev(Q, device), _dev(K, device), _dev(V, device)
    eager, out = (torch.full(Q.shape, float("nan"), device=device) for _ in range(2))
    n = len(seqs)
    ints, longs = (lambda v: (ctypes.c_int * n)(*v)), (lambda v: (ctypes.c_int64 * n)(*v))

    def call(O, stream):
        assert qg.load().qgemm_attention_varlen_gqa(
            Qd.data_ptr(), Qd.stride(0), Kd.data_ptr(), Kd.stride(0), Vd.data_ptr(), Vd.stride(0), O.data_ptr(),
            O.stride(0), n, longs(Q_ROW0), ints([s[0] for s in seqs]), longs(KV_ROW0), ints([s[1] for s in seqs]),
            ints([s[2] for s in seqs]), H, n_kv, dk, attn_oracle.default_scale(dk), None, 0, stream) == 0

    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        call(eager, s.cuda_stream)      # the eager result; also module load and first launch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call(out, s.cuda_stream)
    for i in range(2):
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), eager.cpu().numpy(), f"graph replay {i} against the eager call")
