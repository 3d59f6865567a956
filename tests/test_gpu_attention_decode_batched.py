"""GPU parity of qgemm_attention_decode_batched (attention_decode_batched_kernel): every sequence's rows against
qg.attention on that sequence's own views, on the GPU, and against tests/causal_oracle.py / tests/attn_oracle.py on the
CPU, bit for bit.  The K / V slabs hold NaN past each sequence's seq_kv and one slab is unused and all NaN, so a wrong
slab, length or limit shows; every output is pre-filled with NaN.

The kernel stages K and V in chunks of 128 keys fetched two chunks ahead into two register buffers: the lengths sit on
both sides of a chunk edge, give odd and even chunk counts, and are and are not multiples of 32."""
import ctypes

import numpy as np
import pytest
import torch

import attn_oracle
import causal_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(device)   # a copy: the cached inputs are read-only


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _slabs(seq_kv, kv_slot, d, seed, n_slabs=None, rows=None):
    """K and V as [slabs, rows, d] numpy arrays: sequence b's seq_kv[b] rows in slab kv_slot[b], NaN everywhere else
    (one more slab than sequences unless n_slabs says otherwise)."""
    n = len(seq_kv)
    kv_slot = list(range(n)) if kv_slot is None else kv_slot
    n_slabs = n + 1 if n_slabs is None else n_slabs
    rows = max(seq_kv) + 3 if rows is None else rows
    K = np.full((n_slabs, rows, d), np.nan, np.float32)
    V = np.full((n_slabs, rows, d), np.nan, np.float32)
    for b in range(n):
        K[kv_slot[b], :seq_kv[b]] = O.uniform((seq_kv[b], d), seed + 2 * b)
        V[kv_slot[b], :seq_kv[b]] = O.uniform((seq_kv[b], d), seed + 2 * b + 1)
    return K, V


def _want(Q, K, V, H, q_pos0):
    scale = attn_oracle.default_scale(Q.shape[1] // H)
    if q_pos0 is None:
        return attn_oracle.attention_ref(Q, K, V, H, scale)
    return causal_oracle.attention_causal_ref(Q, K, V, H, scale, q_pos0)


def _check(qg, device, Q, K, V, H, seq_kv, q_pos0, kv_slot, r, what, cpu=True, Qd=None, Kd=None, Vd=None, out=None):
    """One batched call into a NaN-filled output; every sequence against qg.attention on its views (GPU) and, with
    cpu, against the oracle.  Q, K, V: numpy; Qd / Kd / Vd / out: device views to use instead of plain copies."""
    n = len(seq_kv)
    Qd = _dev(Q, device) if Qd is None else Qd
    Kd = _dev(K, device) if Kd is None else Kd
    Vd = _dev(V, device) if Vd is None else Vd
    out = _nan(Q.shape, device) if out is None else out
    got_t = qg.attention_decode_batched(Qd, Kd, Vd, H, seq_kv, q_pos0=q_pos0, kv_slot=kv_slot, rows_per_seq=r, O=out)
    assert got_t is out
    got = out.cpu().numpy()
    for b in range(n):
        slot = b if kv_slot is None else kv_slot[b]
        rows = slice(b * r, (b + 1) * r)
        assert qg.attention_plan(r, seq_kv[b], H, Q.shape[1] // H).startswith("attention_decode")
        one = _nan((r, Q.shape[1]), device)
        qg.attention(Qd[rows], Kd[slot, :seq_kv[b]], Vd[slot, :seq_kv[b]], H, O=one, causal=q_pos0 is not None,
                     q_pos0=None if q_pos0 is None else q_pos0[b])
        assert_bits_equal(got[rows], one.cpu().numpy(), f"{what}: sequence {b} against qg.attention")
        if cpu:
            want = _want(Q[rows], K[slot, :seq_kv[b]], V[slot, :seq_kv[b]], H, None if q_pos0 is None else q_pos0[b])
            assert_bits_equal(got[rows], want, f"{what}: sequence {b} against the oracle")
    return got


def test_chunk_boundaries_masked(qg, oracle, device):
    """Lengths 1, 127, 128, 129 and 300 in permuted slabs: one, one, one, two and three chunks per operand (both
    register-buffer parities), seq % 32 zero and non-zero, L = 1."""
    H, dk = 2, 32
    seq_kv, kv_slot = [1, 127, 128, 129, 300], [4, 0, 3, 1, 2]
    K, V = _slabs(seq_kv, kv_slot, H * dk, 501)
    Q = O.uniform((5, H * dk), 500)
    got = _check(qg, device, Q, K, V, H, seq_kv, [n - 1 for n in seq_kv], kv_slot, 1, "chunk boundaries")
    assert np.isfinite(got).all()


@pytest.mark.parametrize("q_pos0", [[0, 128, 505], [0, 100, 505]], ids=["aligned_to_the_end", "keys_masked_inside"])
def test_eight_rows_masked(qg, oracle, device, q_pos0):
    H, dk, r = 2, 8, 8
    seq_kv = [8, 136, 513]
    if q_pos0[1] == 128:
        assert q_pos0 == [n - r for n in seq_kv]
    K, V = _slabs(seq_kv, None, H * dk, 521)
    Q = O.uniform((3 * r, H * dk), 520)
    got = _check(qg, device, Q, K, V, H, seq_kv, q_pos0, None, r, f"eight rows, q_pos0 {q_pos0}")
    assert np.isfinite(got).all()


def test_unmasked_cross_attention_shape(qg, oracle, device):
    H, dk, r = 2, 24, 3
    seq_kv = [33, 20, 512]
    K, V = _slabs(seq_kv, None, H * dk, 541)
    Q = O.uniform((3 * r, H * dk), 540)
    got = _check(qg, device, Q, K, V, H, seq_kv, None, None, r, "unmasked")
    assert np.isfinite(got).all()


def test_scalar_load_path_and_column_slices(qg, oracle, device):
    """d_k 12, 2 heads; Q the first third of a 3d-wide buffer, O a column slice of a wider sentinel-filled buffer, and
    K / V column slices that start 4 bytes past a 16-byte boundary with an odd row stride (the scalar staging loads)."""
    H, dk, r = 2, 12, 2
    d = H * dk
    seq_kv, kv_slot, q_pos0 = [40, 130, 7], [2, 0, 1], [38, 100, 5]
    K, V = _slabs(seq_kv, kv_slot, d, 561)
    Q = O.uniform((3 * r, d), 560)
    wide_q = torch.zeros((3 * r, 3 * d), device=device)
    wide_q[:, :d] = _dev(Q, device)
    wk, wv = (torch.zeros(K.shape[:2] + (d + 5,), device=device) for _ in range(2))
    wk[:, :, 1:1 + d], wv[:, :, 1:1 + d] = _dev(K, device), _dev(V, device)
    sentinel = -12345.5
    wide_o = torch.full((3 * r + 2, d + 11), sentinel, device=device)
    _check(qg, device, Q, K, V, H, seq_kv, q_pos0, kv_slot, r, "column slices", Qd=wide_q[:, :d],
           Kd=wk[:, :, 1:1 + d], Vd=wv[:, :, 1:1 + d], out=wide_o[1:1 + 3 * r, 5:5 + d])
    w = wide_o.cpu().numpy()
    mask = np.ones(w.shape, bool)
    mask[1:1 + 3 * r, 5:5 + d] = False
    assert (w[mask] == np.float32(sentinel)).all(), "elements outside the output slice were written"


def test_full_batch(qg, device):
    """The cap: 64 sequences x 16 heads x d_k 64, one row each, lengths spread over 1 .. 4096 with exactly one at
    4096.  The largest case: compared with qg.attention on the GPU only."""
    H, dk, n = 16, 64, 64
    d = H * dk
    seq_kv = [1 + (b * 4095) // 63 for b in (int(v) for v in np.arange(n) * 37 % n)]   # a permutation of the spread
    assert sorted(seq_kv)[0] == 1 and sorted(seq_kv)[-2:] == [4031, 4096] and len(set(seq_kv)) == n
    kv_slot = [int(v) for v in (np.arange(n) * 29 + 5) % n]             # another permutation
    g = torch.Generator(device=device).manual_seed(577)
    K = torch.rand((n + 1, 4096, d), device=device, generator=g) * 2 - 1
    V = torch.rand((n + 1, 4096, d), device=device, generator=g) * 2 - 1
    Q = torch.rand((n, d), device=device, generator=g) * 2 - 1
    length = torch.zeros(n + 1, dtype=torch.int64, device=device)      # slab n stays unused: all NaN
    length[torch.tensor(kv_slot, device=device)] = torch.tensor(seq_kv, device=device)
    past = torch.arange(4096, device=device)[None, :, None] >= length[:, None, None]
    K.masked_fill_(past, float("nan"))
    V.masked_fill_(past, float("nan"))
    q_pos0 = [v - 1 for v in seq_kv]
    out = _nan((n, d), device)
    qg.attention_decode_batched(Q, K, V, H, seq_kv, q_pos0=q_pos0, kv_slot=kv_slot, O=out)
    ref = _nan((n, d), device)
    for b in range(n):
        qg.attention(Q[b:b + 1], K[kv_slot[b], :seq_kv[b]], V[kv_slot[b], :seq_kv[b]], H, O=ref[b:b + 1], causal=True,
                     q_pos0=q_pos0[b])
    assert bool(torch.isfinite(ref).all())
    bad = (out.view(torch.int32) != ref.view(torch.int32)).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"sequences {bad} (lengths {[seq_kv[b] for b in bad]}) differ from qg.attention"


def test_non_finite_values_stay_in_their_sequence(qg, oracle, device):
    """An inf in a visible K row and a NaN in a visible V row of sequence 1: that sequence matches qg.attention and the
    oracle, NaN included; its neighbours stay finite."""
    H, dk, r = 2, 8, 2
    seq_kv, q_pos0 = [50, 140, 129], [48, 138, 127]
    K, V = _slabs(seq_kv, None, H * dk, 581)
    K[1, 20, 3] = np.inf
    V[1, 130, 12] = np.nan
    Q = O.uniform((3 * r, H * dk), 580)
    got = _check(qg, device, Q, K, V, H, seq_kv, q_pos0, None, r, "non-finite values")
    assert np.isnan(got[2:4]).any(), "the non-finite values did not reach their own sequence"
    assert np.isfinite(got[:2]).all() and np.isfinite(got[4:]).all()


def test_graph_capture_and_replay(qg, oracle, device):
    """The call allocates nothing, copies nothing to the device and does not synchronize: captured once, replayed after
    the contents of Q, K and V change (the table of the capture -- slots, lengths, offsets -- is replayed)."""
    H, dk, r = 2, 24, 2
    d = H * dk
    seq_kv, kv_slot, q_pos0 = [100, 129, 9], [1, 2, 0], [98, 60, 7]
    rows = max(seq_kv) + 3
    Qs = torch.zeros((3 * r, d), device=device)
    Ks, Vs = torch.zeros((4, rows, d), device=device), torch.zeros((4, rows, d), device=device)
    out = _nan((3 * r, d), device)
    L = qg.load()

    def ints(v):
        return (ctypes.c_int * len(v))(*v)

    def call(stream):
        rc = L.qgemm_attention_decode_batched(Qs.data_ptr(), d, Ks.data_ptr(), d, rows * d, Vs.data_ptr(), d, rows * d,
                                              out.data_ptr(), d, 3, r, ints(kv_slot), ints(seq_kv), ints(q_pos0), H, dk,
                                              attn_oracle.default_scale(dk), stream)
        assert rc == 0

    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        call(s.cuda_stream)      # warm-up: module load, first launch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call(s.cuda_stream)
    for i in range(2):
        K, V = _slabs(seq_kv, kv_slot, d, 601 + 20 * i, n_slabs=4, rows=rows)
        Q = O.uniform((3 * r, d), 600 + 20 * i)
        for dst, src in ((Qs, Q), (Ks, K), (Vs, V)):
            dst.copy_(_dev(src, device))
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for b in range(3):
            one = _nan((r, d), device)
            qg.attention(Qs[b * r:(b + 1) * r], Ks[kv_slot[b], :seq_kv[b]], Vs[kv_slot[b], :seq_kv[b]], H, O=one,
                         causal=True, q_pos0=q_pos0[b])
            assert_bits_equal(got[b * r:(b + 1) * r], one.cpu().numpy(), f"graph replay {i}, sequence {b}")
