"""GPU parity of cache slots and batched steps (qgemm_decoder_create_slots, begin_slot, step_slot, step_batch,
copy_slot, slot_state).  Every sequence's output rows are compared, bit for bit, with
causal_oracle.decoder_forward_causal_ref on that sequence's own inputs and with a plain
Decoder(causal=True, kv_cache=True) stepping that sequence alone on the GPU.  Every step writes into a NaN-filled
output.  Dimensions: those of causal_oracle.DECODER_FUSED unless a test says otherwise."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import causal_oracle
from oracle import oracle as O
from util import assert_bits_equal, bits

pytestmark = pytest.mark.gpu

DIMS = causal_oracle.DECODER_FUSED[2:]   # d_model 64, 2 heads, d_ff 128, 2 blocks
SEED = causal_oracle.DECODER_SEED
INVALID = 1


def _dev(a, device):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(device)   # a copy: the cached inputs are read-only


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _decoder(qg, n_slots, max_seq=40, max_enc_seq=33, dims=DIMS):
    d, H, dff, blocks = dims
    return qg.Decoder(d, H, dff, blocks, max_seq=max_seq, max_enc_seq=max_enc_seq, seed=SEED, causal=True,
                      kv_cache=True, n_slots=n_slots)


@functools.lru_cache(maxsize=None)
def _inputs(b, rows, enc_rows, d=DIMS[0]):
    """Sequence b's own decoder input rows and encoder output (read-only)."""
    X, enc = O.uniform((rows, d), 700 + 10 * b), O.uniform((enc_rows, d), 701 + 10 * b)
    X.flags.writeable = enc.flags.writeable = False
    return X, enc


def _ref(X, enc, dims=DIMS):
    return causal_oracle.decoder_forward_causal_ref(X, enc, *dims, SEED)


def _alone(plain, X, enc, device):
    """The sequence on a plain cached decoder, one row per step: the stacked outputs."""
    plain.begin(_dev(enc, device))
    Xd = _dev(X, device)
    Y = _nan(X.shape, device)
    for p in range(X.shape[0]):
        plain.step(Xd[p:p + 1], Y=Y[p:p + 1])
    return Y.cpu().numpy()


def _batch(dec, slots, rows, device, pos=None, r=1):
    """step_batch on the numpy rows (len(slots) * r x d) into a NaN-filled output; the output as numpy."""
    Y = _nan(rows.shape, device)
    assert dec.step_batch(slots, _dev(rows, device), pos=pos, rows_per_seq=r, Y=Y) is Y
    return Y.cpu().numpy()


def _compare(got, X, enc, plain, device, what, dims=DIMS):
    assert_bits_equal(got, _ref(X, enc, dims), f"{what} against the oracle")
    assert_bits_equal(got, _alone(plain, X, enc, device), f"{what} against a plain decoder alone")


def test_staggered_slots_and_a_shrinking_batch(qg, oracle, device):
    """Three slots with their own inputs and enc_seq 33, 20, 9; slot 0 prefilled with 17 rows, slot 1 with 3, slot 2
    with none; then one row each per step_batch while the batch shrinks [0, 1, 2] -> [1, 2] -> [2] as the sequences
    (19, 7 and 6 rows) end; the slot order is permuted on every other call."""
    total, pre, enc_rows = [19, 7, 6], [17, 3, 0], [33, 20, 9]
    seqs = [_inputs(b, total[b], enc_rows[b]) for b in range(3)]
    dec, plain = _decoder(qg, 3), _decoder(qg, 1)
    try:
        got = [np.full((total[b], DIMS[0]), np.nan, np.float32) for b in range(3)]
        for b in range(3):
            dec.begin_slot(b, _dev(seqs[b][1], device))
            assert dec.slot_filled(b) == 0
            if pre[b]:
                Y = _nan((pre[b], DIMS[0]), device)
                dec.step_slot(b, _dev(seqs[b][0][:pre[b]], device), Y=Y)
                got[b][:pre[b]] = Y.cpu().numpy()
        fill = list(pre)
        call = 0
        while any(fill[b] < total[b] for b in range(3)):
            live = [b for b in range(3) if fill[b] < total[b]]
            if call % 2:
                live = live[::-1]
            out = _batch(dec, live, np.concatenate([seqs[b][0][fill[b]:fill[b] + 1] for b in live]), device)
            for i, b in enumerate(live):
                got[b][fill[b]] = out[i]
                fill[b] += 1
                assert dec.slot_filled(b) == fill[b]
            call += 1
        assert call == 6 and dec.filled == total[0]
        for b in range(3):
            _compare(got[b], *seqs[b], plain, device, f"slot {b}")
    finally:
        dec.close()
        plain.close()


def test_speculative_rows_and_a_per_sequence_rewind(qg, oracle, device):
    """rows_per_seq 4 on two slots (slot 0 after 5 rows, slot 1 from empty), then the same slots one position further
    with other rows -- a rewind of each sequence on its own -- then one-row steps."""
    d = DIMS[0]
    pre = [5, 0]
    first = [_inputs(b, pre[b] + 4, 33 - 13 * b) for b in range(2)]          # the prefill and the first four rows
    alt = [O.uniform((3 + 2, d), 751 + b) for b in range(2)]                 # rows from pre + 1 on: 4 at once, 1 after
    final = [np.concatenate([first[b][0][:pre[b] + 1], alt[b]]) for b in range(2)]
    dec, plain = _decoder(qg, 2), _decoder(qg, 1)
    try:
        for b in range(2):
            dec.begin_slot(b, _dev(first[b][1], device))
        head0 = dec.step_slot(0, _dev(first[0][0][:5], device)).cpu().numpy()
        a = _batch(dec, [0, 1], np.concatenate([first[b][0][pre[b]:] for b in range(2)]), device, r=4)
        assert [dec.slot_filled(b) for b in range(2)] == [9, 4]
        b4 = _batch(dec, [1, 0], np.concatenate([alt[b][:4] for b in (1, 0)]), device, pos=[1, 6], r=4)
        assert [dec.slot_filled(b) for b in range(2)] == [10, 5]
        last = _batch(dec, [0, 1], np.concatenate([alt[b][4:] for b in range(2)]), device)
        assert [dec.slot_filled(b) for b in range(2)] == [11, 6]
        _compare(np.concatenate([head0, a[:4]]), *first[0], plain, device, "slot 0, the first four rows")
        _compare(a[4:], *first[1], plain, device, "slot 1, the first four rows")
        got = [np.concatenate([head0, a[:1], b4[4:], last[:1]]), np.concatenate([a[4:5], b4[:4], last[1:]])]
        for b in range(2):
            assert (bits(_ref(final[b], first[b][1])[pre[b] + 1:pre[b] + 4]) !=
                    bits(_ref(*first[b])[pre[b] + 1:])).any(axis=1).all(), "the rewind changes nothing: a weak test"
            _compare(got[b], final[b], first[b][1], plain, device, f"slot {b} after the rewind")
    finally:
        dec.close()
        plain.close()


def test_crossing_128_keys_inside_the_decoder(qg, oracle, device):
    """d 16, 2 heads, max_seq 140: a slot prefilled to 126 rows and an empty one stepped together through key counts
    127, 128, 129 and 130 (the decode kernel's chunk edge) and 1 .. 4."""
    dims = (16, 2, 32, 2)
    Xa, ea = _inputs(0, 130, 12, 16)
    Xb, eb = _inputs(1, 4, 5, 16)
    dec, plain = _decoder(qg, 2, 140, 12, dims), _decoder(qg, 1, 140, 12, dims)
    try:
        dec.begin_slot(0, _dev(ea, device))
        dec.begin_slot(1, _dev(eb, device))
        head = dec.step_slot(0, _dev(Xa[:126], device)).cpu().numpy()
        outs = [_batch(dec, [0, 1], np.stack([Xa[126 + i], Xb[i]]), device) for i in range(4)]
        assert dec.slot_filled(0) == 130 and dec.slot_filled(1) == 4
        _compare(np.concatenate([head] + [o[:1] for o in outs]), Xa, ea, plain, device, "the long slot", dims)
        _compare(np.concatenate([o[1:] for o in outs]), Xb, eb, plain, device, "the short slot", dims)
    finally:
        dec.close()
        plain.close()


def test_fork_with_copy_slot(qg, oracle, device):
    """copy_slot after 10 rows; source and copy continue with different rows in the same batched steps.  Each equals
    the forward of its own whole sequence, and the source's first rows still answer as before."""
    d = DIMS[0]
    X, enc = _inputs(0, 15, 20)
    Xfork = np.concatenate([X[:10], O.uniform((5, d), 771)])
    dec, plain = _decoder(qg, 3), _decoder(qg, 1)
    try:
        dec.begin_slot(1, _dev(enc, device))
        head = dec.step_slot(1, _dev(X[:10], device)).cpu().numpy()
        assert dec.slot_filled(2) is None
        dec.copy_slot(2, 1)
        assert dec.slot_filled(2) == 10 and dec.slot_filled(1) == 10
        outs = [_batch(dec, [1, 2], np.stack([X[p], Xfork[p]]), device) for p in range(10, 15)]
        again = _nan((1, d), device)
        dec.step_slot(1, _dev(X[9:10], device), pos=9, Y=again)           # rows 0 .. 8 of the source, read once more
        _compare(np.concatenate([head] + [o[:1] for o in outs]), X, enc, plain, device, "the source")
        _compare(np.concatenate([head] + [o[1:] for o in outs]), Xfork, enc, plain, device, "the copy")
        assert_bits_equal(again.cpu().numpy(), head[9:10], "row 9 of the source after the fork went on")
    finally:
        dec.close()
        plain.close()


def test_poisoned_slot_begun_again(qg, oracle, device):
    """Slot 1 is filled to the brim by a NaN sequence, begun again with a shorter enc_out and batched with two healthy
    slots: nothing of the NaN sequence leaks into slot 1's new sequence or into its neighbours."""
    d = DIMS[0]
    seqs = [_inputs(0, 6, 33), _inputs(1, 6, 9), _inputs(2, 6, 20)]
    dec, plain = _decoder(qg, 3), _decoder(qg, 1)
    try:
        dec.begin_slot(1, torch.full((33, d), float("nan"), device=device))
        assert bool(torch.isnan(dec.step_slot(1, torch.full((40, d), float("nan"), device=device))).all())
        for b in range(3):
            dec.begin_slot(b, _dev(seqs[b][1], device))
        assert dec.slot_filled(1) == 0
        outs = [_batch(dec, [0, 1, 2], np.stack([seqs[b][0][p] for b in range(3)]), device) for p in range(6)]
        for b in range(3):
            _compare(np.stack([o[b] for o in outs]), *seqs[b], plain, device, f"slot {b} beside a poisoned slot")
    finally:
        dec.close()
        plain.close()


def test_begin_and_step_drive_slot_0_of_a_slotted_decoder(qg, oracle, device):
    X0, e0 = _inputs(0, 8, 33)
    X1, e1 = _inputs(1, 2, 20)
    dec, plain = _decoder(qg, 2), _decoder(qg, 1)
    try:
        assert dec.filled is None
        dec.begin(_dev(e0, device))
        assert dec.filled == 0 and dec.slot_filled(0) == 0 and dec.slot_filled(1) is None
        a = dec.step(_dev(X0[:5], device)).cpu().numpy()
        assert dec.filled == 5
        dec.begin_slot(1, _dev(e1, device))
        b = _batch(dec, [1, 0], np.stack([X1[0], X0[5]]), device)
        assert dec.filled == 6
        c = _nan((1, DIMS[0]), device)
        dec.step(_dev(X0[6:7], device), Y=c)
        b2 = _batch(dec, [0, 1], np.stack([X0[7], X1[1]]), device)
        assert dec.filled == 8 and dec.slot_filled(1) == 2
        _compare(np.concatenate([a, b[1:], c.cpu().numpy(), b2[:1]]), X0, e0, plain, device, "slot 0")
        _compare(np.concatenate([b[:1], b2[1:]]), X1, e1, plain, device, "slot 1")
    finally:
        dec.close()
        plain.close()


def test_forward_between_two_batched_steps_changes_nothing(qg, oracle, device):
    seqs = [_inputs(0, 4, 33), _inputs(1, 4, 20)]
    other, oenc = _inputs(5, 40, 9)
    dec, plain = _decoder(qg, 2), _decoder(qg, 1)
    try:
        for b in range(2):
            dec.begin_slot(b, _dev(seqs[b][1], device))
        outs = [_batch(dec, [0, 1], np.stack([seqs[b][0][p] for b in range(2)]), device) for p in range(2)]
        fwd = _nan(other.shape, device)
        dec.forward(_dev(other, device), _dev(oenc, device), Y=fwd)
        outs += [_batch(dec, [0, 1], np.stack([seqs[b][0][p] for b in range(2)]), device) for p in range(2, 4)]
        assert_bits_equal(fwd.cpu().numpy(), _ref(other, oenc), "forward on a slotted decoder")
        for b in range(2):
            _compare(np.stack([o[b] for o in outs]), *seqs[b], plain, device, f"slot {b} around a forward")
    finally:
        dec.close()
        plain.close()


def test_more_batched_rows_than_max_seq(qg, oracle, device):
    """Four slots of max_seq 9 stepped with eight rows each: 32 rows through scratch buffers that a one-slot decoder
    sizes for 9 (they hold max(max_seq, 8 * n_slots) rows)."""
    seqs = [_inputs(b, 9, 9) for b in range(4)]
    dec, plain = _decoder(qg, 4, 9, 9), _decoder(qg, 1, 9, 9)
    try:
        for b in range(4):
            dec.begin_slot(b, _dev(seqs[b][1], device))
        a = _batch(dec, [3, 1, 0, 2], np.concatenate([seqs[b][0][:8] for b in (3, 1, 0, 2)]), device, r=8)
        last = _batch(dec, [0, 1, 2, 3], np.stack([seqs[b][0][8] for b in range(4)]), device)
        for i, b in enumerate((3, 1, 0, 2)):
            _compare(np.concatenate([a[8 * i:8 * i + 8], last[b:b + 1]]), *seqs[b], plain, device, f"slot {b}")
    finally:
        dec.close()
        plain.close()


def test_graph_capture_of_one_batched_step(qg, oracle, device):
    """step_batch allocates nothing and does not synchronize: the step of two slots at positions 6 and 2 is captured
    once and replayed with new input rows (a graph replays its positions)."""
    d = DIMS[0]
    seqs = [_inputs(0, 6, 33), _inputs(1, 2, 20)]
    L = qg.load()
    dec, plain = _decoder(qg, 2), _decoder(qg, 1)
    try:
        xs, y = torch.zeros((2, d), device=device), _nan((2, d), device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            for b in range(2):
                dec.begin_slot(b, _dev(seqs[b][1], device))
                dec.step_slot(b, _dev(seqs[b][0], device))
            dec.step_batch([0, 1], xs, Y=y)          # warm-up of the captured call
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = L.qgemm_decoder_step_batch(dec._h, 2, _ints([0, 1]), _ints([6, 2]), 1, xs.data_ptr(), y.data_ptr(),
                                                s.cuda_stream)
                assert rc == 0
        for i in range(2):
            rows = O.uniform((2, d), 791 + i)
            xs.copy_(_dev(rows, device))
            y.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            for b in range(2):
                whole = np.concatenate([seqs[b][0], rows[b:b + 1]])
                want = _alone(plain, whole, seqs[b][1], device)
                assert_bits_equal(got[b:b + 1], want[-1:], f"graph replay {i}, slot {b}")
    finally:
        dec.close()
        plain.close()


def test_argument_checks(qg, oracle, device):
    """Every refused call returns hipErrorInvalidValue before any launch: Y stays NaN, no filled length moves and
    qgemm_decoder_slot_state agrees."""
    d, H, dff, blocks = DIMS
    L = qg.load()
    X, enc = _inputs(0, 40, 33)
    Xd, Ed, Y = _dev(X, device), _dev(enc, device), _nan((40, d), device)
    st = torch.cuda.current_stream(device).cuda_stream

    def batch(h, slots=(0, 1), pos=(4, 0), r=1, n=None, x=Xd.data_ptr(), y=Y.data_ptr(), null=()):
        sl = None if "slots" in null else _ints(list(slots))
        ps = None if "pos" in null else _ints(list(pos))
        return L.qgemm_decoder_step_batch(h, len(slots) if n is None else n, sl, ps, r, x, y, st)

    def state(h, slot):
        e, f = ctypes.c_int(-7), ctypes.c_int(-7)
        return L.qgemm_decoder_slot_state(h, slot, ctypes.byref(e), ctypes.byref(f)), e.value, f.value

    nocache = qg.Decoder(d, H, dff, blocks, 40, 33, seed=SEED, causal=True)
    dec = _decoder(qg, 3)
    try:
        # a decoder without the slots' flags
        assert batch(nocache._h) == INVALID and L.qgemm_decoder_begin_slot(nocache._h, 0, Ed.data_ptr(), 33, st) == INVALID
        assert L.qgemm_decoder_step_slot(nocache._h, 0, Xd.data_ptr(), Y.data_ptr(), 0, 1, st) == INVALID
        assert L.qgemm_decoder_copy_slot(nocache._h, 1, 0, st) == INVALID and state(nocache._h, 0)[0] == INVALID
        # begin_slot
        for slot, e, n in ((-1, Ed.data_ptr(), 33), (3, Ed.data_ptr(), 33), (0, None, 33), (0, Ed.data_ptr(), 0),
                           (0, Ed.data_ptr(), 34)):
            assert L.qgemm_decoder_begin_slot(dec._h, slot, e, n, st) == INVALID, (slot, e, n)
        assert state(dec._h, 0) == (0, 0, 0) and state(dec._h, 3)[0] == INVALID and state(dec._h, -1)[0] == INVALID
        assert L.qgemm_decoder_slot_state(dec._h, 0, None, None) == 0
        assert batch(dec._h) == INVALID                                         # nothing begun
        assert L.qgemm_decoder_copy_slot(dec._h, 1, 0, st) == INVALID           # the source not begun
        assert L.qgemm_decoder_begin_slot(dec._h, 0, Ed.data_ptr(), 33, st) == 0
        assert L.qgemm_decoder_begin_slot(dec._h, 1, Ed.data_ptr(), 20, st) == 0
        assert L.qgemm_decoder_step_slot(dec._h, 0, Xd.data_ptr(), Xd.data_ptr() + 4 * d * 20, 0, 4, st) == 0
        assert state(dec._h, 0) == (0, 33, 4) and state(dec._h, 1) == (0, 20, 0) and state(dec._h, 2) == (0, 0, 0)
        # step_slot
        for slot, pos, n in ((-1, 0, 1), (3, 0, 1), (2, 0, 1), (0, 5, 1), (0, -1, 1), (0, 4, 37), (0, 4, 0)):
            assert L.qgemm_decoder_step_slot(dec._h, slot, Xd.data_ptr(), Y.data_ptr(), pos, n, st) == INVALID
        # step_batch
        assert batch(dec._h, null=("slots",)) == INVALID and batch(dec._h, null=("pos",)) == INVALID
        assert batch(dec._h, x=None) == INVALID and batch(dec._h, y=None) == INVALID
        assert batch(dec._h, slots=(0, 3)) == INVALID and batch(dec._h, slots=(-1, 1)) == INVALID   # out of range
        assert batch(dec._h, slots=(0, 2)) == INVALID                                               # not begun
        assert batch(dec._h, slots=(0, 0)) == INVALID and batch(dec._h, slots=(1, 0, 1), pos=(0, 4, 0)) == INVALID
        assert batch(dec._h, pos=(-1, 0)) == INVALID and batch(dec._h, pos=(5, 0)) == INVALID       # pos > filled
        assert batch(dec._h, pos=(4, 1)) == INVALID
        assert batch(dec._h, n=0) == INVALID and batch(dec._h, n=-1) == INVALID
        assert batch(dec._h, slots=(0, 1, 2, 0), pos=(4, 0, 0, 0)) == INVALID                       # n_seqs > n_slots
        assert batch(dec._h, r=0) == INVALID and batch(dec._h, r=9) == INVALID and batch(dec._h, r=-1) == INVALID
        # copy_slot
        for dst, src in ((0, 0), (3, 0), (-1, 0), (0, 3), (0, -1), (0, 2)):
            assert L.qgemm_decoder_copy_slot(dec._h, dst, src, st) == INVALID, (dst, src)
        assert state(dec._h, 0) == (0, 33, 4) and state(dec._h, 1) == (0, 20, 0) and state(dec._h, 2) == (0, 0, 0)
        # pos + r > max_seq, on a slot filled to the brim less three
        assert L.qgemm_decoder_step_slot(dec._h, 1, Xd.data_ptr(), Xd.data_ptr() + 4 * d * 20, 0, 20, st) == 0
        assert L.qgemm_decoder_copy_slot(dec._h, 2, 1, st) == 0 and state(dec._h, 2) == (0, 20, 20)
        big = _decoder(qg, 2, max_seq=6)
        try:
            for b in range(2):
                assert L.qgemm_decoder_begin_slot(big._h, b, Ed.data_ptr(), 9, st) == 0
            assert L.qgemm_decoder_step_slot(big._h, 0, Xd.data_ptr(), Xd.data_ptr() + 4 * d * 20, 0, 3, st) == 0
            assert batch(big._h, pos=(3, 0), r=4) == INVALID and batch(big._h, pos=(0, 0), r=7) == INVALID
            assert state(big._h, 0) == (0, 9, 3) and state(big._h, 1) == (0, 9, 0)
        finally:
            big.close()
        torch.cuda.synchronize()
        assert bool(torch.isnan(Y).all()), "a refused call wrote into Y"
        assert dec.slot_filled(0) == 4 and dec.slot_filled(1) == 20 and dec.slot_filled(2) == 20
        with pytest.raises(AssertionError):
            qg.Decoder(d, H, dff, blocks, 40, 33, causal=True, kv_cache=False, n_slots=2)
    finally:
        nocache.close()
        dec.close()
