"""GPU parity of Decoder.step_varlen (qgemm_decoder_step_varlen): a prefill of many slots in one call and prefills mixed
with decoding rows.  Every sequence's output rows are compared, bit for bit, with step_slot on a second decoder that
steps that sequence alone on the GPU, and with causal_oracle.decoder_forward_causal_ref on that sequence's own inputs.
Every step writes into a NaN-filled output.  Dimensions: those of causal_oracle.DECODER_FUSED unless a test says
otherwise."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import causal_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

DIMS = causal_oracle.DECODER_FUSED[2:]   # d_model 64, 2 heads, d_ff 128, 2 blocks
SEED = causal_oracle.DECODER_SEED
INVALID = 1


def _dev(a, device):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(device)   # a copy: the cached inputs are read-only


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _ints(v):
    return (ctypes.c_int * max(1, len(v)))(*v)


def _decoder(qg, n_slots, max_rows=None, max_seq=40, max_enc_seq=33, dims=DIMS):
    d, H, dff, blocks = dims
    return qg.Decoder(d, H, dff, blocks, max_seq=max_seq, max_enc_seq=max_enc_seq, seed=SEED, causal=True,
                      kv_cache=True, n_slots=n_slots, max_rows=max_rows)


@functools.lru_cache(maxsize=None)
def _inputs(b, rows, enc_rows, d=DIMS[0]):
    """Sequence b's own decoder input rows and encoder output (read-only)."""
    X, enc = O.uniform((rows, d), 1700 + 10 * b), O.uniform((enc_rows, d), 1701 + 10 * b)
    X.flags.writeable = enc.flags.writeable = False
    return X, enc


def _ref(X, enc, dims=DIMS):
    return causal_oracle.decoder_forward_causal_ref(X, enc, *dims, SEED)


def _varlen(dec, slots, chunks, device, pos=None):
    """step_varlen on the numpy chunks (one per slot) into a NaN-filled output; the outputs split per slot."""
    n_rows = [c.shape[0] for c in chunks]
    X = _dev(np.concatenate(chunks), device)
    Y = _nan(X.shape, device)
    assert dec.step_varlen(slots, X, n_rows, pos=pos, Y=Y) is Y
    out, at, y = [], 0, Y.cpu().numpy()
    for n in n_rows:
        out.append(y[at:at + n])
        at += n
    return out


def _slot(plain, X, device, pos=None):
    Y = _nan(X.shape, device)
    plain.step_slot(0, _dev(X, device), pos=pos, Y=Y)
    return Y.cpu().numpy()


def test_prefill_of_four_slots_then_a_mixed_call_then_step_batch(qg, oracle, device):
    """Prefill 4 slots with (17, 1, 40, 8) rows in one call -- more rows than max_seq: the row budget; slot 2 is then
    full -- then one call that appends (1, 3, -, 9) rows at each slot's own position (slot 2 left out), in another
    slot order; then step_batch continues the sequences that have room by one row.  Every result against step_slot on
    a second decoder and the oracle."""
    pre, more, enc_rows = [17, 1, 40, 8], [1, 3, 0, 9], [33, 20, 9, 1]
    last = [1, 1, 0, 1]     # the row step_batch appends
    total = [pre[b] + more[b] + last[b] for b in range(4)]
    seqs = [_inputs(b, total[b], enc_rows[b]) for b in range(4)]
    dec, plain = _decoder(qg, 4, max_rows=sum(pre)), _decoder(qg, 1)
    assert sum(pre) > 40
    try:
        for b in range(4):
            dec.begin_slot(b, _dev(seqs[b][1], device))
        got = [np.full((total[b], DIMS[0]), np.nan, np.float32) for b in range(4)]
        out = _varlen(dec, [0, 1, 2, 3], [seqs[b][0][:pre[b]] for b in range(4)], device)
        for b in range(4):
            got[b][:pre[b]] = out[b]
        assert [dec.slot_filled(b) for b in range(4)] == pre
        order = [3, 0, 1]
        out = _varlen(dec, order, [seqs[b][0][pre[b]:pre[b] + more[b]] for b in order], device)
        for i, b in enumerate(order):
            got[b][pre[b]:pre[b] + more[b]] = out[i]
        assert [dec.slot_filled(b) for b in range(4)] == [pre[b] + more[b] for b in range(4)]
        # step_batch afterwards continues the same sequences: one row each
        Y = _nan((3, DIMS[0]), device)
        dec.step_batch([0, 1, 3], _dev(np.stack([seqs[b][0][-1] for b in (0, 1, 3)]), device), Y=Y)
        for i, b in enumerate((0, 1, 3)):
            got[b][-1] = Y[i].cpu().numpy()
        assert [dec.slot_filled(b) for b in range(4)] == total
        for b in range(4):
            X, enc = seqs[b]
            assert_bits_equal(got[b], _ref(X, enc), f"slot {b} against the oracle")
            plain.begin(_dev(enc, device))
            alone = np.concatenate([_slot(plain, X[:pre[b]], device)] +
                                   ([_slot(plain, X[pre[b]:pre[b] + more[b]], device)] if more[b] else []) +
                                   ([_slot(plain, X[-1:], device)] if last[b] else []))
            assert_bits_equal(got[b], alone, f"slot {b} against step_slot alone")
    finally:
        dec.close()
        plain.close()


def test_a_rewind(qg, oracle, device):
    """Two slots prefilled with 12 and 20 rows; then slot 0 rewinds to position 5 with 9 other rows while slot 1 goes
    on with 2: each equals the causal forward on its own final sequence."""
    d = DIMS[0]
    first = [_inputs(10 + b, n, 33 - 4 * b) for b, n in enumerate((12, 22))]
    alt = O.uniform((9, d), 1790)
    final0 = np.concatenate([first[0][0][:5], alt])
    dec = _decoder(qg, 2, max_rows=64)
    try:
        for b in range(2):
            dec.begin_slot(b, _dev(first[b][1], device))
        a = _varlen(dec, [0, 1], [first[0][0], first[1][0][:20]], device)
        b_ = _varlen(dec, [1, 0], [first[1][0][20:], alt], device, pos=[20, 5])
        assert [dec.slot_filled(b) for b in range(2)] == [14, 22]
        assert_bits_equal(a[0], _ref(*first[0]), "slot 0 before the rewind")
        assert_bits_equal(np.concatenate([a[0][:5], b_[1]]), _ref(final0, first[0][1]), "slot 0 after the rewind")
        assert_bits_equal(np.concatenate([a[1], b_[0]]), _ref(*first[1]), "slot 1")
    finally:
        dec.close()


def test_refusals_leave_the_slots_alone(qg, device):
    """Repeated slots, pos > filled and the other step_batch rules, every one before the first launch: the output
    stays NaN and no filled length moves."""
    d = DIMS[0]
    L = qg.load()
    dec = _decoder(qg, 3, max_rows=48)
    enc_dec = qg.Encoder(*DIMS, max_seq=8, seed=1)
    try:
        for b in range(2):
            dec.begin_slot(b, _dev(O.uniform((5, d), 1800 + b), device))
        X, Y = torch.zeros((64, d), device=device), _nan((64, d), device)
        dec.step_varlen([0, 1], X[:7], [3, 4])
        f = L.qgemm_decoder_step_varlen

        def rc(slots, pos, n_rows, h=None, n=None, x=X, y=Y):
            return f(dec._h if h is None else h, len(slots) if n is None else n, _ints(slots), _ints(pos),
                     _ints(n_rows), None if x is None else x.data_ptr(), None if y is None else y.data_ptr(), None)

        assert rc([0, 0], [3, 3], [1, 1]) == INVALID, "a repeated slot"
        assert rc([0, 1], [4, 4], [1, 1]) == INVALID, "pos > filled"
        assert rc([0, 1], [3, -1], [1, 1]) == INVALID
        assert rc([0, 1], [3, 4], [1, 0]) == INVALID, "n_rows < 1"
        assert rc([0, 1], [3, 4], [1, 37]) == INVALID, "pos + n > max_seq"
        assert rc([0, 1], [0, 0], [40, 9]) == INVALID, "more rows than the budget of 48"
        assert rc([0, 2], [3, 0], [1, 1]) == INVALID, "slot 2 not begun"
        assert rc([0, 3], [3, 0], [1, 1]) == INVALID and rc([0, -1], [3, 0], [1, 1]) == INVALID
        assert rc([], [], []) == INVALID and rc([0, 1, 2, 0], [0] * 4, [1] * 4) == INVALID
        assert rc([0], [3], [1], x=None) == INVALID and rc([0], [3], [1], y=None) == INVALID
        assert rc([0], [3], [1], h=enc_dec._h) == INVALID, "an encoder"
        assert f(dec._h, 1, None, _ints([3]), _ints([1]), X.data_ptr(), Y.data_ptr(), None) == INVALID
        assert f(dec._h, 1, _ints([0]), None, _ints([1]), X.data_ptr(), Y.data_ptr(), None) == INVALID
        assert f(dec._h, 1, _ints([0]), _ints([3]), None, X.data_ptr(), Y.data_ptr(), None) == INVALID
        torch.cuda.synchronize()
        assert bool(torch.isnan(Y).all()), "a refused step launched something"
        assert [dec.slot_filled(b) for b in range(3)] == [3, 4, None]
        assert rc([1, 0], [0, 0], [8, 40]) == 0, "sum = the budget, pos + n = max_seq"
        assert [dec.slot_filled(b) for b in range(2)] == [40, 8]
    finally:
        dec.close()
        enc_dec.close()


def test_a_prefix_that_crosses_512_keys(qg, oracle, device):
    """causal_oracle.DECODER_FALLBACK's sizes (d_model 16): slot 0 prefilled with 500 rows beside a short slot 1 in one
    table launch per attention; then 13 more rows take slot 0's prefix to 513 keys, so that call's self-attention runs
    sequence by sequence (three launches for slot 0) while its cross-attention stays one launch."""
    shape = causal_oracle.DECODER_FALLBACK
    seq, enc_seq = shape[:2]
    dims = shape[2:]
    H, dk = dims[1], dims[0] // dims[1]
    X0, enc0 = causal_oracle.decoder_inputs(shape)
    X1, enc1 = _inputs(20, 25, 9, d=dims[0])
    assert qg.attention_varlen_plan([500, 20], [500, 20], H, dk) == "attention_fused_kernel<many>"
    assert qg.attention_varlen_plan([13, 5], [513, 25], H, dk) == "per_sequence"
    assert qg.attention_plan(13, 513, H, dk) == "three_launches"
    dec = _decoder(qg, 2, max_rows=520, max_seq=seq, max_enc_seq=enc_seq, dims=dims)
    plain = _decoder(qg, 1, max_seq=seq, max_enc_seq=enc_seq, dims=dims)
    try:
        dec.begin_slot(0, _dev(enc0, device))
        dec.begin_slot(1, _dev(enc1, device))
        a = _varlen(dec, [0, 1], [X0[:500], X1[:20]], device)
        b = _varlen(dec, [1, 0], [X1[20:], X0[500:]], device)
        assert [dec.slot_filled(s) for s in range(2)] == [513, 25]
        got0, got1 = np.concatenate([a[0], b[1]]), np.concatenate([a[1], b[0]])
        assert_bits_equal(got0, causal_oracle.decoder_expected(shape), "slot 0 against the oracle")
        assert_bits_equal(got1, _ref(X1, enc1, dims), "slot 1 against the oracle")
        plain.begin(_dev(enc0, device))
        alone = np.concatenate([_slot(plain, X0[:500], device), _slot(plain, X0[500:], device)])
        assert_bits_equal(got0, alone, "slot 0 against step_slot alone")
    finally:
        dec.close()
        plain.close()
