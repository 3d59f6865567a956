"""GPU parity of qgemm_attention_varlen (attention_fused_kernel<., FusedMany>): every sequence's rows against
tests/attn_oracle.py / tests/causal_oracle.py on the CPU, one sequence at a time, and against qg.attention on that
sequence's own views on the GPU, bit for bit.

The parent matrices Q, K and V are NaN-filled with gaps between the sequences' rows, so a read that crosses into a gap
or -- through a wrong row offset, length or limit -- reaches an output shows as NaN or as a wrong bit.  Every row of O
that no sequence owns holds a sentinel that must come back untouched.  The plan query is asserted before each case."""
import ctypes

import numpy as np
import pytest
import torch

import attn_cases
import attn_oracle
import causal_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

MANY, PER_SEQ = "attention_fused_kernel<many>", "per_sequence"
SENTINEL = -12345.5
H = 2
# the work map's edges: exactly one and exactly two query tiles (32, 64), one row past a tile (33), a single row, an
# empty sequence in the middle, one key past the 256-key chunk (257), the envelope's last key (512), a single key
EDGE_Q, EDGE_KV = (33, 1, 32, 0, 64, 7), (100, 512, 33, 5, 257, 1)
EDGE_POS0 = (0, 511, 1, 0, 193, 0)


def _dev(a, device):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(device)   # a copy: cached inputs are read-only


def _offsets(counts, gaps):
    """Row offsets of sequences of `counts` rows with gaps[b] rows before sequence b; the total with one last gap."""
    out, at = [], 0
    for b, c in enumerate(counts):
        at += gaps[b % len(gaps)]
        out.append(at)
        at += c
    return out, at + gaps[0]


def _build(seq_q, seq_kv, d, seed, values=None):
    """NaN-filled parents with the sequences' rows in them: (Q, K, V, q_row0, kv_row0).  values[b] = (Q, K, V) of
    sequence b replaces the seeded uniform draw."""
    q_row0, nq = _offsets(seq_q, (2, 1, 3))
    kv_row0, nkv = _offsets(seq_kv, (1, 4, 2))
    Q = np.full((nq, d), np.nan, np.float32)
    K, V = np.full((nkv, d), np.nan, np.float32), np.full((nkv, d), np.nan, np.float32)
    for b, (nqb, nkb) in enumerate(zip(seq_q, seq_kv)):
        q, k, v = (values or {}).get(b) or (O.uniform((nqb, d), seed + 3 * b), O.uniform((nkb, d), seed + 3 * b + 1),
                                            O.uniform((nkb, d), seed + 3 * b + 2))
        Q[q_row0[b]:q_row0[b] + nqb], K[kv_row0[b]:kv_row0[b] + nkb], V[kv_row0[b]:kv_row0[b] + nkb] = q, k, v
    return Q, K, V, q_row0, kv_row0


def _want(Q, K, V, dk, q_pos0):
    scale = attn_oracle.default_scale(dk)
    if q_pos0 is None:
        return attn_oracle.attention_ref(Q, K, V, H, scale)
    return causal_oracle.attention_causal_ref(Q, K, V, H, scale, q_pos0)


def _owned(n_rows, q_row0, seq_q):
    own = np.zeros(n_rows, bool)
    for r0, n in zip(q_row0, seq_q):
        own[r0:r0 + n] = True
    return own


def _check(qg, device, Q, K, V, seq_q, seq_kv, q_row0, kv_row0, q_pos0, what, plan=MANY, cpu=True, Qd=None, Kd=None,
           Vd=None, out=None):
    """One varlen call into a sentinel-filled output; every sequence against the oracle (cpu) and against
    qg.attention on its views (GPU); the rows no sequence owns untouched.  Q, K, V: numpy parents; Qd / Kd / Vd / out:
    device views to use instead of plain copies."""
    d = Q.shape[1]
    dk = d // H
    assert qg.attention_varlen_plan(seq_q, seq_kv, H, dk) == plan, what
    Qd = _dev(Q, device) if Qd is None else Qd
    Kd = _dev(K, device) if Kd is None else Kd
    Vd = _dev(V, device) if Vd is None else Vd
    out = torch.full(Q.shape, SENTINEL, device=device) if out is None else out
    got_t = qg.attention_varlen(Qd, Kd, Vd, H, seq_q, seq_kv, q_row0=q_row0, kv_row0=kv_row0, q_pos0=q_pos0, O=out)
    assert got_t is out
    got = out.cpu().numpy()
    for b, (nq, nkv) in enumerate(zip(seq_q, seq_kv)):
        qs, ks = slice(q_row0[b], q_row0[b] + nq), slice(kv_row0[b], kv_row0[b] + nkv)
        pos = None if q_pos0 is None else q_pos0[b]
        if nq == 0:
            continue
        if cpu:
            assert_bits_equal(got[qs], _want(Q[qs], K[ks], V[ks], dk, pos), f"{what}: sequence {b} against the oracle")
        one = torch.full((nq, d), float("nan"), device=device)
        qg.attention(Qd[qs], Kd[ks], Vd[ks], H, O=one, causal=pos is not None, q_pos0=pos)
        assert_bits_equal(got[qs], one.cpu().numpy(), f"{what}: sequence {b} against qg.attention")
    free = ~_owned(Q.shape[0], q_row0, seq_q)
    assert (got[free] == np.float32(SENTINEL)).all(), f"{what}: rows of O that no sequence owns were written"
    return got


@pytest.mark.parametrize("dk", [24, 64])
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_work_map_edges(qg, oracle, device, dk, masked):
    Q, K, V, q_row0, kv_row0 = _build(EDGE_Q, EDGE_KV, H * dk, 700)
    got = _check(qg, device, Q, K, V, EDGE_Q, EDGE_KV, q_row0, kv_row0, EDGE_POS0 if masked else None,
                 f"work map edges, d_k {dk}, masked {masked}")
    assert np.isfinite(got[_owned(Q.shape[0], q_row0, EDGE_Q)]).all()


def test_a_mask_that_hides_nothing(qg, oracle, device):
    """q_pos0 at and past seq_kv - 1 (the launcher clamps it): the masked call equals the unmasked one bit for bit."""
    dk = 24
    seq_q, seq_kv, q_pos0 = (33, 5, 40), (100, 64, 7), (99, 1000, 2 ** 31 - 1)
    Q, K, V, q_row0, kv_row0 = _build(seq_q, seq_kv, H * dk, 720)
    masked = _check(qg, device, Q, K, V, seq_q, seq_kv, q_row0, kv_row0, q_pos0, "mask hides nothing", cpu=False)
    plain = _check(qg, device, Q, K, V, seq_q, seq_kv, q_row0, kv_row0, None, "no mask")
    assert_bits_equal(masked, plain, "a mask that hides nothing against no mask")


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_one_sequence_equals_attention(qg, oracle, device, masked):
    dk = 64
    seq_q, seq_kv = (70,), (300,)
    Q, K, V, q_row0, kv_row0 = _build(seq_q, seq_kv, H * dk, 730)
    _check(qg, device, Q, K, V, seq_q, seq_kv, q_row0, kv_row0, (230,) if masked else None, "n_seqs = 1")


def test_full_table_of_short_sequences(qg, oracle, device):
    """The cap: 64 sequences, query rows on both sides of the tile boundaries 32 and 64, keys on both sides of 32 and
    64 too, with empty sequences among them and after the last one that has rows."""
    dk = 24
    qs, ks = (31, 32, 33, 1, 63, 64, 65, 0, 2), (1, 31, 33, 64, 65, 32, 7)
    seq_q = [qs[b % len(qs)] for b in range(64)]
    seq_kv = [ks[(5 * b) % len(ks)] for b in range(64)]
    seq_q[62] = seq_q[63] = 0
    q_pos0 = [max(0, kv - q) if b % 3 else b % 5 for b, (q, kv) in enumerate(zip(seq_q, seq_kv))]
    Q, K, V, q_row0, kv_row0 = _build(seq_q, seq_kv, H * dk, 760)
    _check(qg, device, Q, K, V, seq_q, seq_kv, q_row0, kv_row0, q_pos0, "64 sequences")


def test_sequences_that_share_keys(qg, oracle, device):
    """Two sequences read the same K / V rows, a third a prefix of them (a shared prompt)."""
    dk = 24
    seq_q, seq_kv = (33, 40, 9), (100, 100, 60)
    Q, K, V, q_row0, kv_row0 = _build(seq_q, seq_kv, H * dk, 780)
    kv_row0 = [kv_row0[0]] * 3    # everyone reads sequence 0's keys
    _check(qg, device, Q, K, V, seq_q, seq_kv, q_row0, kv_row0, (67, 0, 51), "shared keys")


def test_queries_inside_a_qkv_buffer(qg, oracle, device):
    """The encoder's layout: Q, K and V the thirds of one [Q | K | V] buffer, q_row0 = kv_row0, seq_q = seq_kv."""
    dk = 24
    d = H * dk
    lens = (33, 1, 40, 32, 7)
    row0, n = _offsets(lens, (0,))
    Q, K, V = (np.full((n, d), np.nan, np.float32) for _ in range(3))
    for b, (r0, nb) in enumerate(zip(row0, lens)):
        Q[r0:r0 + nb], K[r0:r0 + nb], V[r0:r0 + nb] = (O.uniform((nb, d), 800 + 3 * b + i) for i in range(3))
    qkv = _dev(np.concatenate([Q, K, V], axis=1), device)
    _check(qg, device, Q, K, V, lens, lens, row0, row0, None, "[Q | K | V] thirds", Qd=qkv[:, :d], Kd=qkv[:, d:2 * d],
           Vd=qkv[:, 2 * d:])


def test_column_slices_that_are_not_16_byte_aligned(qg, oracle, device):
    """d_k 24; Q, K and V column slices that start 4 bytes past a 16-byte boundary with an odd row stride (the scalar
    staging loads), O a column slice of a wider sentinel-filled buffer."""
    dk = 24
    d = H * dk
    seq_q, seq_kv, q_pos0 = (33, 5, 64), (257, 40, 100), (224, 35, 0)
    Q, K, V, q_row0, kv_row0 = _build(seq_q, seq_kv, d, 820)
    wq = torch.zeros((Q.shape[0], d + 5), device=device)
    wk, wv = (torch.zeros((K.shape[0], d + 7), device=device) for _ in range(2))
    wq[:, 1:1 + d], wk[:, 1:1 + d], wv[:, 1:1 + d] = _dev(Q, device), _dev(K, device), _dev(V, device)
    wide_o = torch.full((Q.shape[0], d + 11), SENTINEL, device=device)
    _check(qg, device, Q, K, V, seq_q, seq_kv, q_row0, kv_row0, q_pos0, "column slices", Qd=wq[:, 1:1 + d],
           Kd=wk[:, 1:1 + d], Vd=wv[:, 1:1 + d], out=wide_o[:, 5:5 + d])
    w = wide_o.cpu().numpy()
    assert (w[:, :5] == np.float32(SENTINEL)).all() and (w[:, 5 + d:] == np.float32(SENTINEL)).all(), \
        "columns outside the output slice were written"


@pytest.mark.parametrize("name", attn_cases.ATTENTION_NAMES)
def test_special_values_stay_in_their_sequence(qg, oracle, device, name):
    """attn_cases.py's special-value sets as the middle sequence of three: it matches the oracle, NaN and inf
    included, and the sequences beside it equal what they give without it."""
    seq_q0, seq_kv0, _, dk = attn_cases.ATTN_BASE
    seq_q, seq_kv = (40, seq_q0, 7), (64, seq_kv0, 33)
    special = attn_cases.attention_sets()[name][0]
    Q, K, V, q_row0, kv_row0 = _build(seq_q, seq_kv, H * dk, 840, values={1: special})
    got = _check(qg, device, Q, K, V, seq_q, seq_kv, q_row0, kv_row0, None, name)
    assert_bits_equal(got[q_row0[1]:q_row0[1] + seq_q0], attn_cases.attention_expected(name), f"{name}: the shared expectation")
    for b in (0, 2):
        assert np.isfinite(got[q_row0[b]:q_row0[b] + seq_q[b]]).all(), f"{name}: sequence {b} is not finite"


def _raw_call(qg, Qd, Kd, Vd, out, seq_q, seq_kv, q_row0, kv_row0, q_pos0, dk, ws, ws_bytes, stream):
    n = len(seq_q)
    ints = lambda v: (ctypes.c_int * n)(*v)            # noqa: E731
    longs = lambda v: (ctypes.c_int64 * n)(*v)         # noqa: E731
    return qg.load().qgemm_attention_varlen(
        Qd.data_ptr(), Qd.stride(0), Kd.data_ptr(), Kd.stride(0), Vd.data_ptr(), Vd.stride(0), out.data_ptr(),
        out.stride(0), n, longs(q_row0), ints(seq_q), longs(kv_row0), ints(seq_kv),
        None if q_pos0 is None else ints(q_pos0), H, dk, attn_oracle.default_scale(dk), ws, ws_bytes, stream)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_per_sequence_path(qg, oracle, device, masked):
    """One sequence of 513 keys among fused-size ones: the call loops over the sequences (fused, three launches, decode,
    fused) through a 0xFF-filled workspace exactly as large as the size query says, with guard bytes behind it."""
    dk = 24
    seq_q, seq_kv = (33, 9, 3, 0, 40), (100, 513, 600, 5, 64)
    q_pos0 = (67, 504, 597, 0, 24) if masked else None
    Q, K, V, q_row0, kv_row0 = _build(seq_q, seq_kv, H * dk, 860)
    L = qg.load()
    ints = lambda v: (ctypes.c_int * len(v))(*v)       # noqa: E731
    assert qg.attention_varlen_plan(seq_q, seq_kv, H, dk) == PER_SEQ
    assert [qg.attention_plan(q, kv, H, dk).split("_kernel")[0] for q, kv in zip(seq_q, seq_kv) if q] == \
        ["attention_fused", "three_launches", "attention_decode", "attention_fused"]
    need = L.qgemm_attention_varlen_workspace_size(len(seq_q), ints(seq_q), ints(seq_kv), H, dk)
    assert need == 4 * H * 9 * 513
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=device)
    Qd, Kd, Vd = (_dev(a, device) for a in (Q, K, V))
    out = torch.full(Q.shape, SENTINEL, device=device)
    assert _raw_call(qg, Qd, Kd, Vd, out, seq_q, seq_kv, q_row0, kv_row0, q_pos0, dk, ws.data_ptr(), need - 1, None) == 1
    assert _raw_call(qg, Qd, Kd, Vd, out, seq_q, seq_kv, q_row0, kv_row0, q_pos0, dk, ws.data_ptr(), need, None) == 0
    got = out.cpu().numpy()
    for b, (nq, nkv) in enumerate(zip(seq_q, seq_kv)):
        qs, ks = slice(q_row0[b], q_row0[b] + nq), slice(kv_row0[b], kv_row0[b] + nkv)
        if nq:
            assert_bits_equal(got[qs], _want(Q[qs], K[ks], V[ks], dk, None if q_pos0 is None else q_pos0[b]),
                              f"per sequence, sequence {b}")
    assert (got[~_owned(Q.shape[0], q_row0, seq_q)] == np.float32(SENTINEL)).all()
    assert bool((ws[need:] == 0xFF).all()), "bytes past the workspace size were written"


def test_graph_capture_and_replay(qg, oracle, device):
    """The call allocates nothing, copies nothing to the device and does not synchronize: captured once, replayed after
    the contents of Q, K and V change (the table of the capture -- offsets, lengths, mask offsets -- is replayed)."""
    dk = 24
    seq_q, seq_kv, q_pos0 = (33, 1, 64, 0, 7), (100, 512, 257, 3, 7), (67, 511, 100, 0, 0)
    Q, K, V, q_row0, kv_row0 = _build(seq_q, seq_kv, H * dk, 880)
    Qs, Ks, Vs = (torch.zeros(a.shape, device=device) for a in (Q, K, V))
    out = torch.full(Q.shape, SENTINEL, device=device)
    assert qg.attention_varlen_plan(seq_q, seq_kv, H, dk) == MANY

    def call(stream):
        assert _raw_call(qg, Qs, Ks, Vs, out, seq_q, seq_kv, q_row0, kv_row0, q_pos0, dk, None, 0, stream) == 0

    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        call(s.cuda_stream)      # warm-up: module load, first launch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call(s.cuda_stream)
    for i in range(2):
        Q, K, V, _, _ = _build(seq_q, seq_kv, H * dk, 900 + 40 * i)
        for dst, src in ((Qs, Q), (Ks, K), (Vs, V)):
            dst.copy_(_dev(src, device))
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for b, (nq, nkv) in enumerate(zip(seq_q, seq_kv)):
            qs, ks = slice(q_row0[b], q_row0[b] + nq), slice(kv_row0[b], kv_row0[b] + nkv)
            if nq:
                assert_bits_equal(got[qs], _want(Q[qs], K[ks], V[ks], dk, q_pos0[b]), f"graph replay {i}, sequence {b}")
        assert (got[~_owned(Q.shape[0], q_row0, seq_q)] == np.float32(SENTINEL)).all()


def test_two_calls_back_to_back_with_different_tables(qg, oracle, device):
    """Two calls on one stream without a synchronization between them, the second with other lengths, offsets and
    mask: each carries its own table."""
    dk = 24
    a = ((33, 64, 2), (100, 257, 40), (67, 0, 38))
    b = ((5, 0, 70, 32), (512, 9, 70, 33), None)
    Qa, Ka, Va, qa0, ka0 = _build(a[0], a[1], H * dk, 940)
    Qb, Kb, Vb, qb0, kb0 = _build(b[0], b[1], H * dk, 960)
    dev = [_dev(x, device) for x in (Qa, Ka, Va, Qb, Kb, Vb)]
    out_a = torch.full(Qa.shape, SENTINEL, device=device)
    out_b = torch.full(Qb.shape, SENTINEL, device=device)
    assert qg.attention_varlen_plan(a[0], a[1], H, dk) == MANY and qg.attention_varlen_plan(b[0], b[1], H, dk) == MANY
    qg.attention_varlen(dev[0], dev[1], dev[2], H, a[0], a[1], q_row0=qa0, kv_row0=ka0, q_pos0=a[2], O=out_a)
    qg.attention_varlen(dev[3], dev[4], dev[5], H, b[0], b[1], q_row0=qb0, kv_row0=kb0, q_pos0=b[2], O=out_b)
    torch.cuda.synchronize()
    for (seq_q, seq_kv, pos), (Q, K, V), q0, k0, out in ((a, (Qa, Ka, Va), qa0, ka0, out_a),
                                                        (b, (Qb, Kb, Vb), qb0, kb0, out_b)):
        got = out.cpu().numpy()
        for i, (nq, nkv) in enumerate(zip(seq_q, seq_kv)):
            qs, ks = slice(q0[i], q0[i] + nq), slice(k0[i], k0[i] + nkv)
            if nq:
                assert_bits_equal(got[qs], _want(Q[qs], K[ks], V[ks], dk, None if pos is None else pos[i]),
                                  f"back to back, sequence {i}")
        assert (got[~_owned(Q.shape[0], q0, seq_q)] == np.float32(SENTINEL)).all()


def test_default_offsets_are_the_packed_layout(qg, oracle, device):
    """q_row0 / kv_row0 left out: prefix sums; a fresh O is returned with every row owned."""
    dk = 24
    seq_q, seq_kv = (33, 1, 40), (64, 100, 7)
    d = H * dk
    Q, K, V = O.uniform((sum(seq_q), d), 980), O.uniform((sum(seq_kv), d), 981), O.uniform((sum(seq_kv), d), 982)
    got = qg.attention_varlen(_dev(Q, device), _dev(K, device), _dev(V, device), H, seq_q, seq_kv).cpu().numpy()
    q0 = k0 = 0
    for b, (nq, nkv) in enumerate(zip(seq_q, seq_kv)):
        assert_bits_equal(got[q0:q0 + nq], _want(Q[q0:q0 + nq], K[k0:k0 + nkv], V[k0:k0 + nkv], dk, None),
                          f"packed layout, sequence {b}")
        q0, k0 = q0 + nq, k0 + nkv
