"""GPU parity of Decoder.step_varlen and step_batch with every one of the 64 cache slots in use, at
batch_cases.WIDE (d_model 128, d_ff 4096, 2 blocks): calls of 2112, 512 and 64 rows, whose linears run other int8 GEMM
plans than the one-slot steps they are compared with (tests/test_batch_plans_host.py holds the table against the
library).  Every slot has its own encoder output of 1 .. 33 rows.  Every slot's output rows are compared, bit for bit,
with a one-slot decoder fed the same rows with begin / step, and for a third of the slots with
causal_oracle.decoder_forward_causal_ref on the slot's whole sequence.  Every step writes into a NaN-filled output."""
import ctypes

import numpy as np
import pytest
import torch

import batch_cases as C
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(device)   # a copy: the cached inputs are read-only


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _decoders(qg):
    """(the 64-slot decoder with a budget of 2112 rows, a one-slot decoder of the same weights)"""
    kw = dict(max_seq=C.DEC_MAX_SEQ, max_enc_seq=C.DEC_MAX_ENC, seed=C.SEED, causal=True, kv_cache=True)
    return qg.Decoder(*C.WIDE, n_slots=C.N_SLOTS, max_rows=C.MAX_ROWS, **kw), qg.Decoder(*C.WIDE, **kw)


def _begin_all(dec, device):
    for b in range(C.N_SLOTS):
        dec.begin_slot(b, _dev(C.slot_enc(b), device))
        assert dec.slot_filled(b) == 0


def _run(dec, call, device):
    """One call of the schedule into a NaN-filled output: {slot: its output rows}."""
    kind, r, slots, pos, n_rows, chunks = call
    X = _dev(np.concatenate(chunks), device)
    Y = _nan(X.shape, device)
    if kind == "varlen":
        assert dec.step_varlen(slots, X, n_rows, pos=pos, Y=Y) is Y
    else:
        assert dec.step_batch(slots, X, pos=pos, rows_per_seq=r, Y=Y) is Y
    y, out, at = Y.cpu().numpy(), {}, 0
    for b, n in zip(slots, n_rows):
        out[b] = y[at:at + n]
        at += n
    assert at == y.shape[0]
    return out


def test_every_slot_through_prefill_batched_steps_and_a_mixed_call(qg, oracle, device):
    """batch_cases.decoder_schedule: one step_varlen prefills the 64 slots in a permuted order (2112 rows), one
    step_batch appends 8 rows to each (512 rows; the eight full slots rewind to position 56 with other rows), one
    appends one row each (64 rows), one step_varlen appends 1 .. 9 rows to the 32 odd slots."""
    calls = C.decoder_schedule()
    assert [sum(c[4]) for c in calls[:3]] == [C.ROWS_64_SEQS, C.ROWS_SLOTS8, C.ROWS_SLOTS]
    dec, plain = _decoders(qg)
    try:
        _begin_all(dec, device)
        got = [_run(dec, call, device) for call in calls]
        assert [dec.slot_filled(b) for b in range(C.N_SLOTS)] == C.final_filled()
        for b in range(C.N_SLOTS):
            plain.begin(_dev(C.slot_enc(b), device))
            for c, pos, rows in C.slot_calls(b):
                one = _nan(rows.shape, device)
                plain.step(_dev(rows, device), pos=pos, Y=one)
                assert_bits_equal(got[c][b], one.cpu().numpy(), f"slot {b}, call {c} against a one-slot decoder")
            assert plain.filled == C.final_filled()[b]
        for b in C.DEC_ORACLE_SLOTS:
            want = C.slot_expected(b)
            for c, _, _ in C.slot_calls(b):
                assert_bits_equal(got[c][b], want[c], f"slot {b}, call {c} against the oracle")
    finally:
        dec.close()
        plain.close()


def test_graph_capture_of_a_64_slot_step(qg, oracle, device):
    """One row for each of the 64 slots at explicit positions (the prefill lengths), captured once and replayed on new
    input rows: every replay rewinds every slot to its captured position."""
    prefill = C.decoder_schedule()[0]
    pos = [C.lens(C.N_SLOTS)[b] for b in range(C.N_SLOTS)]
    slots = list(range(C.N_SLOTS))
    L = qg.load()
    dec, plain = _decoders(qg)
    try:
        xs, y = torch.zeros((C.N_SLOTS, C.D), device=device), _nan((C.N_SLOTS, C.D), device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            _begin_all(dec, device)
            _run(dec, prefill, device)
            dec.step_batch(slots, xs, pos=pos, Y=y)          # warm-up of the captured call
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = L.qgemm_decoder_step_batch(dec._h, C.N_SLOTS, _ints(slots), _ints(pos), 1, xs.data_ptr(),
                                                y.data_ptr(), s.cuda_stream)
                assert rc == 0
        news = [O.uniform((C.N_SLOTS, C.D), 6900 + i) for i in range(2)]
        got = []
        for rows in news:
            xs.copy_(_dev(rows, device))
            y.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got.append(y.cpu().numpy())
        first = {b: rows for b, rows in zip(prefill[2], prefill[5])}
        for b in range(C.N_SLOTS):
            plain.begin(_dev(C.slot_enc(b), device))
            plain.step(_dev(first[b], device))
            for i, rows in enumerate(news):
                want = plain.step(_dev(rows[b:b + 1], device), pos=pos[b]).cpu().numpy()
                assert_bits_equal(got[i][b:b + 1], want, f"graph replay {i}, slot {b}")
    finally:
        dec.close()
        plain.close()
