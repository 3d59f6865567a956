"""GPU parity of decode attention over a bf16 K / V cache (attention_decode_kv16_kernel) through
qgemm_attention_decode_batched_kv16 and _indirect_kv16: bit for bit tests/attn_oracle.py and tests/causal_oracle.py on
K and V rounded to bf16 on the CPU, widened, with every head repeated G = n_heads / n_kv_heads times.  Outputs are
pre-filled with NaN.  A workgroup owns up to four query heads of one KV head, stages 256-key chunks and sums in passes
of 1024 elements: the shapes stand on both sides of each of these edges, G = 1 included."""
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

# (rows, seq_kv, heads, kv heads, d_k, q_pos0[, how]); q_pos0 None: no mask
CASES = (
    (1, 1, 1, 1, 64, 0),              # one key, G = 1
    (1, 257, 3, 1, 128, 256),         # one key past a 256-key chunk, a partial block of 3
    (2, 1025, 4, 1, 64, 1023),        # past a 1024-element sum pass, all four waves
    (1, 4096, 4, 1, 128, 4095),       # the key limit, full LDS
    (3, 40, 10, 2, 96, 37),           # G = 5: blocks of 4 and 1, d_k 96
    (8, 600, 8, 1, 128, 592),         # two full blocks, a partial third chunk
    (2, 77, 4, 2, 20, None),          # unmasked, d_k no multiple of 8: element loads
    (2, 300, 6, 2, 128, 298, "slices"),   # K / V one element past a 16-byte boundary with an odd row stride
    (4, 100, 4, 1, 128, 10, 3),       # +inf in V at a masked key, in an odd column of a lane pair ...
    (4, 100, 4, 1, 128, 10, 100),     # ... and in an even one
)


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)


def _f32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _plan(dk):
    return "attention_decode_kv16_kernel" if dk <= 64 else "attention_decode_kv16_wide_kernel"


def _qkv(rows, seq_kv, H, n_kv, dk, seed):
    return O.uniform((rows, H * dk), seed), O.uniform((seq_kv, n_kv * dk), seed + 1), O.uniform((seq_kv, n_kv * dk), seed + 2)


def _want(Q, K, V, H, n_kv, q_pos0):
    """the oracle on K and V rounded to bf16, widened, every head repeated H / n_kv times"""
    dk = Q.shape[1] // H
    Kr, Vr = (np.repeat(_bf16(a).float().numpy().reshape(len(a), n_kv, dk), H // n_kv, axis=1).reshape(len(a), -1)
              for a in (K, V))
    scale = attn_oracle.default_scale(dk)
    if q_pos0 is None:
        return attn_oracle.attention_ref(Q, Kr, Vr, H, scale)
    return causal_oracle.attention_causal_ref(Q, Kr, Vr, H, scale, q_pos0)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_kv16_decode_bit_exact(qg, oracle, device, case):
    """One sequence through the batched entry.  how "slices": K and V 2 bytes past a 16-byte boundary with an odd row
    stride; how a column: +inf in V there at key 50, masked for every row -- 0 * inf = NaN in that column of EVERY query
    head, the rest finite."""
    (rows, seq_kv, H, n_kv, dk, q_pos0), how = case[:6], case[6] if len(case) > 6 else None
    assert qg.attention_decode_kv16_plan(rows, H, n_kv, dk) == _plan(dk)
    Q, K, V = _qkv(rows, seq_kv, H, n_kv, dk, 801)
    if isinstance(how, int):
        V[50, how] = np.inf
    want = _want(Q, K, V, H, n_kv, q_pos0)
    if isinstance(how, int):
        cols = [h * dk + how for h in range(H)]
        assert np.isnan(want[:, cols]).all() and np.isfinite(np.delete(want, cols, axis=1)).all()
    Kd, Vd = _bf16(K).to(device)[None], _bf16(V).to(device)[None]
    if how == "slices":
        wk, wv = (torch.zeros((1, seq_kv, n_kv * dk + 7), dtype=torch.bfloat16, device=device) for _ in range(2))
        wk[:, :, 1:1 + n_kv * dk], wv[:, :, 1:1 + n_kv * dk] = Kd, Vd
        Kd, Vd = wk[:, :, 1:1 + n_kv * dk], wv[:, :, 1:1 + n_kv * dk]
    out = torch.full((rows, H * dk), float("nan"), device=device)
    qg.attention_decode_batched_kv16(_f32(Q, device), Kd, Vd, H, n_kv, [seq_kv],
                                     q_pos0=None if q_pos0 is None else [q_pos0], rows_per_seq=rows, O=out)
    assert_bits_equal(out.cpu().numpy(), want, f"kv16 decode attention {case}")


ROWS = 2


def _sequences(seq_kv, H, n_kv, dk):   # per sequence (Q, K, V, q_pos0): the last of its rows sees every key
    return [_qkv(ROWS, n, H, n_kv, dk, 831 + 10 * b) + (max(n - ROWS, 0),) for b, n in enumerate(seq_kv)]


def _check_sequences(call, seqs, H, n_kv, dk, device, what):
    out = torch.full((len(seqs) * ROWS, H * dk), float("nan"), device=device)
    call(_f32(np.concatenate([s[0] for s in seqs]), device), [s[3] for s in seqs], out)
    got = out.cpu().numpy()
    for b, (Q, K, V, p) in enumerate(seqs):
        assert_bits_equal(got[b * ROWS:(b + 1) * ROWS], _want(Q, K, V, H, n_kv, p), f"{what}: sequence {b}")
    return got


def _slabs(seqs, slot_of, n_slabs, width, device):
    """bf16 K and V slabs on the device, NaN where no sequence's row lies: row j of sequence b in slab slot_of(b, j)"""
    rows = max(len(s[1]) for s in seqs) + 3
    K, V = (np.full((n_slabs, rows, width), np.nan, np.float32) for _ in range(2))
    for b, (_, Kb, Vb, _) in enumerate(seqs):
        j = np.arange(len(Kb))
        K[slot_of(b, j), j], V[slot_of(b, j), j] = Kb, Vb
    return _bf16(K).to(device), _bf16(V).to(device)


@pytest.mark.parametrize("heads", [(8, 2, 128), (6, 2, 64)], ids=str)
def test_batched_and_indirect(qg, oracle, device, heads):
    """3 sequences of 1, 256 and 300 keys: the batched launch on permuted slabs; the indirect launch with the identity
    table, which must give the batched launch's bits; and through a table that interleaves two slabs per sequence, with
    the entry 6 of 6 slabs at the visible key 200 of the last sequence (its rows NaN, the others finite)."""
    H, n_kv, dk = heads
    seq_kv, kv_slot = [1, 256, 300], [2, 0, 3]
    seqs = _sequences(seq_kv, H, n_kv, dk)
    Kd, Vd = _slabs(seqs, lambda b, j: kv_slot[b], 4, n_kv * dk, device)
    batched = _check_sequences(lambda Q, p, out: qg.attention_decode_batched_kv16(
        Q, Kd, Vd, H, n_kv, seq_kv, q_pos0=p, kv_slot=kv_slot, rows_per_seq=ROWS, O=out), seqs, H, n_kv, dk, device, "batched")
    ident = torch.arange(4, dtype=torch.uint8, device=device)[:, None].repeat(1, Kd.shape[1])
    same = _check_sequences(lambda Q, p, out: qg.attention_decode_indirect_kv16(
        Q, Kd, Vd, H, ident, seq_kv, q_pos0=p, tab_row=kv_slot, rows_per_seq=ROWS, O=out, n_kv_heads=n_kv),
        seqs, H, n_kv, dk, device, "identity table")
    assert_bits_equal(same, batched, "indirect with the identity table against batched")
    Kd, Vd = _slabs(seqs, lambda b, j: 2 * b + (j & 1), 6, n_kv * dk, device)
    own = np.full((3, Kd.shape[1]), 255, np.uint8)
    for b, n in enumerate(seq_kv):
        own[b, :n] = 2 * b + (np.arange(n) & 1)
    own[2, 200] = 6
    seqs[2][1][200], seqs[2][2][200] = np.nan, np.nan
    got = _check_sequences(lambda Q, p, out: qg.attention_decode_indirect_kv16(
        Q, Kd, Vd, H, torch.from_numpy(own).to(device), seq_kv, q_pos0=p, rows_per_seq=ROWS, O=out, n_kv_heads=n_kv),
        seqs, H, n_kv, dk, device, "indirect")
    assert np.isfinite(got[:2 * ROWS]).all() and np.isnan(got[2 * ROWS:]).all()


def test_graph_capture_and_replay(qg, oracle, device):
    """The batched launch allocates nothing, copies nothing and does not synchronize: captured once, replayed twice after
    Q, K and V change, each replay against the oracle."""
    H, n_kv, dk, seq_kv, kv_slot = 6, 2, 128, [100, 257, 9], [1, 2, 0]
    d, w, rows = H * dk, n_kv * dk, 260
    Qs, out = torch.zeros((3 * ROWS, d), device=device), torch.full((3 * ROWS, d), float("nan"), device=device)
    Ks, Vs = (torch.zeros((3, rows, w), dtype=torch.bfloat16, device=device) for _ in range(2))
    L = qg.load()
    ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731

    def call(stream):
        assert L.qgemm_attention_decode_batched_kv16(
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
        seqs = [_qkv(ROWS, n, H, n_kv, dk, 861 + 50 * i + 10 * b) for b, n in enumerate(seq_kv)]
        Qs.copy_(_f32(np.concatenate([q for q, _, _ in seqs]), device))
        for (_, Kb, Vb), slot in zip(seqs, kv_slot):
            Ks[slot, :len(Kb)], Vs[slot, :len(Vb)] = _bf16(Kb).to(device), _bf16(Vb).to(device)
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for b, (Q, Kb, Vb) in enumerate(seqs):
            assert_bits_equal(got[b * ROWS:(b + 1) * ROWS], _want(Q, Kb, Vb, H, n_kv, seq_kv[b] - ROWS),
                              f"graph replay {i}, sequence {b}")


# (rows per sequence, seq_kv, heads, kv heads, d_k, sliced): unmasked, two sequences on one K / V history -- 257 and 600
# keys (one key past a 256-key chunk; three chunks, so both prefetch buffers and both parities of the K chunk count),
# G = 3 (a block of three heads), G = 5 (a second block of one head) and G = 1, both widths, 16-byte and element loads
UNMASKED = ((1, (257, 600), 6, 2, 64, False), (3, (600, 257), 10, 2, 20, True),
            (3, (257, 600), 6, 2, 96, False), (1, (600, 257), 10, 2, 128, True), (3, (257, 600), 2, 2, 128, False))


@pytest.mark.parametrize("case", UNMASKED, ids=str)
def test_unmasked_batched_and_indirect(qg, oracle, device, case):
    """attention_decode_kv16_kernel<false, DecodeMany | DecodeIndirect, 64 | 128> (decode_table_cases.py)"""
    rows, seq_kv, H, n_kv, dk, sliced = case
    assert qg.attention_decode_kv16_plan(rows, H, n_kv, dk) == _plan(dk)
    check_unmasked_tables(
        device, rows, seq_kv, H, n_kv, dk, sliced, torch.bfloat16,
        lambda Q, K, V, n, slot, out: qg.attention_decode_batched_kv16(Q, K, V, H, n_kv, n, kv_slot=slot, rows_per_seq=rows, O=out),
        lambda Q, K, V, tab, n, out: qg.attention_decode_indirect_kv16(Q, K, V, H, tab, n, rows_per_seq=rows, O=out, n_kv_heads=n_kv),
        lambda Q, K, V: _want(Q, K, V, H, n_kv, None), 881)
