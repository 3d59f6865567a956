"""GPU parity of the wide decode attention kernel (attention_decode_kernel<., ., 128>) -- the launch
qgemm_attention[_causal], qgemm_attention_decode_batched and _indirect take for seq_q <= 8 at d_k 96 and 128 -- bit for
bit against tests/causal_oracle.py and tests/attn_oracle.py.  Every case first asserts through qgemm_attention_plan
that it lands on that kernel; outputs are pre-filled with NaN, the workspace with 0xFF bytes that must stay.  The
kernel stages 128-key chunks, sums in passes of 1024 elements and carries the P V columns on two waves (0 .. 63,
64 .. 127): the shapes stand on both sides of each of these edges."""
import numpy as np
import pytest
import torch

import attn_oracle
import causal_oracle
from decode_table_cases import check_unmasked_tables
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

WIDE = "attention_decode_wide_kernel"
# (seq_q, seq_kv, heads, d_k, q_pos0[, how]); q_pos0 None: no mask
SHAPES = (
    (1, 1, 1, 96, 0),            # a single key
    (1, 33, 2, 128, 32),         # one key past a 32-key tile
    (1, 129, 1, 128, 128),       # one key past a chunk
    (1, 257, 2, 96, 256),        # one key past two chunks
    (1, 1025, 1, 128, 1024),     # one key past a 1024-element pass of the sum chain
    (1, 4096, 1, 128, 4095),     # the key limit
    (3, 40, 2, 96, 37),          # several query rows
    (8, 600, 2, 128, 592),       # eight rows past 512 keys
    (4, 100, 2, 128, 10),        # every row hides most keys
    (1, 77, 2, 128, None),       # unmasked
    (5, 513, 1, 96, None),
    (2, 140, 1, 128, 138, "slices"),   # the scalar-load path
    (4, 100, 1, 128, 10, 3),     # +inf in V at a masked key, in a column of P V's wave 0 ...
    (4, 100, 1, 128, 10, 100),   # ... and of wave 1
)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _want(Q, K, V, H, q_pos0):
    scale = attn_oracle.default_scale(Q.shape[1] // H)
    if q_pos0 is None:
        return attn_oracle.attention_ref(Q, K, V, H, scale)
    return causal_oracle.attention_causal_ref(Q, K, V, H, scale, q_pos0)


def _run(qg, device, Qd, Kd, Vd, H, q_pos0):
    """qgemm_attention[_causal] on device tensors or views, into a NaN-filled output, with the 0xFF-filled workspace"""
    seq_q, seq_kv, dk = Qd.shape[0], Kd.shape[0], Qd.shape[1] // H
    assert qg.attention_plan(seq_q, seq_kv, H, dk) == WIDE
    L = qg.load()
    need = L.qgemm_attention_workspace_size(seq_q, seq_kv, H, dk)
    ws = torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device=device)
    out = torch.full((seq_q, H * dk), float("nan"), device=device)
    head = (Qd.data_ptr(), Qd.stride(0), Kd.data_ptr(), Kd.stride(0), Vd.data_ptr(), Vd.stride(0), out.data_ptr(),
            out.stride(0), seq_q, seq_kv, H, dk, attn_oracle.default_scale(dk))
    tail = (ws.data_ptr(), need, torch.cuda.current_stream(device).cuda_stream)
    rc = L.qgemm_attention(*head, *tail) if q_pos0 is None else L.qgemm_attention_causal(*head, q_pos0, *tail)
    assert rc == 0, f"the attention call returned {rc}"
    assert bool((ws == 0xFF).all()), "the decode launch wrote into the workspace"
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_wide_decode_bit_exact(qg, oracle, device, shape):
    """how "slices": K and V as column slices 4 bytes past a 16-byte boundary with an odd row stride (the scalar loads);
    how a column: +inf in V there at key 50, masked for every row -- 0 * inf = NaN, the masked tail of P V is not skipped"""
    (seq_q, seq_kv, H, dk, q_pos0), how = shape[:5], shape[5] if len(shape) > 5 else None
    Q, K, V = causal_oracle.qkv(shape[:5], 401)
    if isinstance(how, int):
        V[50, how] = np.inf
    want = _want(Q, K, V, H, q_pos0)
    Kd, Vd = _dev(K, device), _dev(V, device)
    if how == "slices":
        wk, wv = (torch.zeros((seq_kv, H * dk + 7), device=device) for _ in range(2))
        wk[:, 1:1 + H * dk], wv[:, 1:1 + H * dk] = Kd, Vd
        Kd, Vd = wk[:, 1:1 + H * dk], wv[:, 1:1 + H * dk]
    if isinstance(how, int):
        assert np.isnan(want[:, how]).all() and np.isfinite(np.delete(want, how, axis=1)).all()
    assert_bits_equal(_run(qg, device, _dev(Q, device), Kd, Vd, H, q_pos0), want, f"wide decode attention {shape}")


SEQ_KV, ROWS, H, DK = (1, 128, 300), 2, 2, 128   # key counts on both sides of a chunk edge


def _sequences():   # per sequence (Q, K, V, q_pos0): the last of its 2 rows sees every key
    return [causal_oracle.qkv((ROWS, n, H, DK, 0), 431 + 10 * b) + (max(n - ROWS, 0),) for b, n in enumerate(SEQ_KV)]


def _check_sequences(qg, call, seqs, device, what):
    assert qg.attention_plan(ROWS, max(SEQ_KV), H, DK) == WIDE
    out = torch.full((3 * ROWS, H * DK), float("nan"), device=device)
    call(_dev(np.concatenate([s[0] for s in seqs]), device), [s[3] for s in seqs], out)
    got = out.cpu().numpy()
    for b, (Q, K, V, p) in enumerate(seqs):
        assert_bits_equal(got[b * ROWS:(b + 1) * ROWS], _want(Q, K, V, H, p), f"{what}: sequence {b}")
    return got


def test_batched_with_permuted_slabs(qg, oracle, device):
    seqs, kv_slot = _sequences(), [2, 0, 3]
    K, V = (np.full((4, 303, H * DK), np.nan, np.float32) for _ in range(2))
    for (_, Kb, Vb, _), s in zip(seqs, kv_slot):
        K[s, :len(Kb)], V[s, :len(Vb)] = Kb, Vb
    Kd, Vd = _dev(K, device), _dev(V, device)
    _check_sequences(qg, lambda Q, p, out: qg.attention_decode_batched(Q, Kd, Vd, H, list(SEQ_KV), q_pos0=p, kv_slot=kv_slot,
                                                                       rows_per_seq=ROWS, O=out), seqs, device, "batched")


def test_indirect_with_mixed_slabs_and_an_entry_that_names_no_slab(qg, oracle, device):
    """Sequence b's key j lies in slab 2 b + (j & 1); key 200 of the last sequence has the entry 6 of 6 slabs, so that
    K / V row reads as quiet NaNs and, being visible, makes the sequence's rows NaN."""
    seqs = _sequences()
    K, V = (np.full((6, 303, H * DK), np.nan, np.float32) for _ in range(2))
    own = np.full((3, 303), 255, np.uint8)
    for b, (_, Kb, Vb, _) in enumerate(seqs):
        j = np.arange(len(Kb))
        own[b, :len(Kb)] = 2 * b + (j & 1)
        K[own[b, j], j], V[own[b, j], j] = Kb, Vb
    own[2, 200] = 6
    seqs[2][1][200], seqs[2][2][200] = np.nan, np.nan
    Kd, Vd, ownd = _dev(K, device), _dev(V, device), _dev(own, device)
    got = _check_sequences(qg, lambda Q, p, out: qg.attention_decode_indirect(Q, Kd, Vd, H, ownd, list(SEQ_KV), q_pos0=p,
                                                                              rows_per_seq=ROWS, O=out), seqs, device, "indirect")
    assert np.isfinite(got[:2 * ROWS]).all() and np.isnan(got[2 * ROWS:]).all()


# (rows per sequence, seq_kv, heads, d_k, sliced): unmasked, two sequences on one K / V history -- 129 and 300 keys (one
# key past a chunk; three chunks, so both prefetch buffers and both parities of the K chunk count), vector and element loads
UNMASKED = ((1, (129, 300), 2, 128, False), (3, (300, 129), 2, 96, True))


@pytest.mark.parametrize("case", UNMASKED, ids=str)
def test_unmasked_batched_and_indirect(qg, oracle, device, case):
    """attention_decode_kernel<false, DecodeMany | DecodeIndirect, 128> (decode_table_cases.py)"""
    rows, seq_kv, heads, dk, sliced = case
    assert qg.attention_plan(rows, max(seq_kv), heads, dk) == WIDE
    check_unmasked_tables(
        device, rows, seq_kv, heads, heads, dk, sliced, torch.float32,
        lambda Q, K, V, n, slot, out: qg.attention_decode_batched(Q, K, V, heads, n, kv_slot=slot, rows_per_seq=rows, O=out),
        lambda Q, K, V, tab, n, out: qg.attention_decode_indirect(Q, K, V, heads, tab, n, rows_per_seq=rows, O=out),
        lambda Q, K, V: _want(Q, K, V, heads, None), 461)
