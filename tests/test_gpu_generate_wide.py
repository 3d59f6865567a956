"""GPU parity of Decoder.generate with 64 sequences: the 64-slot decoder of tests/test_gpu_decoder_batch_plans.py
(batch_cases.WIDE), the head of tests/test_gpu_head_wide.py (vocab 50257, an untied weight with a bias) with E and a
position table of 72 rows.  The slots are prefilled with 0 .. 7 rows, so some start empty; every slot has its own
encoder output.  generate's tokens are compared with head_oracle.generate_ref for every 4th sequence, the first and the
last, and for all 64 with the same sequence generated alone on a one-slot decoder."""
import numpy as np
import pytest
import torch

import batch_cases as C
import causal_oracle
import head_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SLOTS = list(range(C.N_SLOTS))


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


@pytest.fixture(scope="module")
def gen_head(qg, oracle, device):
    (E, P), (W, bias) = C.gen_tables(), C.head_model()
    head = qg.Head(qg.pack_b(_dev(W, device)), C.VOCAB, _dev(bias, device), _dev(E, device), _dev(P, device),
                   max_rows=C.HEAD_MAX_ROWS)
    yield head
    head.close()


def _decoder(qg, n_slots):
    kw = dict(max_seq=C.DEC_MAX_SEQ, max_enc_seq=C.DEC_MAX_ENC, seed=C.SEED, causal=True, kv_cache=True)
    if n_slots == 1:
        return qg.Decoder(*C.WIDE, **kw)
    return qg.Decoder(*C.WIDE, n_slots=n_slots, max_rows=C.MAX_ROWS, **kw)


def _prefill(dec, device):
    """begin_slot on all 64 slots, then one step_varlen with the slots that have prefill rows."""
    for b in SLOTS:
        dec.begin_slot(b, _dev(C.slot_enc(b), device))
    some = [b for b in SLOTS if C.gen_prefill_rows(b)]
    dec.step_varlen(some, _dev(np.concatenate([C.gen_prefill(b) for b in some]), device),
                    [C.gen_prefill_rows(b) for b in some])
    assert [dec.slot_filled(b) for b in SLOTS] == [C.gen_prefill_rows(b) for b in SLOTS]


def _tokens_in(device, order=SLOTS):
    return torch.tensor([C.gen_token_in(b) for b in order], dtype=torch.int32, device=device)


def test_generate_64_sequences(qg, oracle, device, gen_head):
    first = C.gen_first_tokens()
    assert len(set(first.tolist())) >= 32, "a test bug: the sequences must not all choose the same tokens"
    dec, alone = _decoder(qg, C.N_SLOTS), _decoder(qg, 1)
    try:
        _prefill(dec, device)
        out = torch.full((C.GEN_N_NEW, C.N_SLOTS), -1, dtype=torch.int32, device=device)
        assert dec.generate(gen_head, SLOTS, _tokens_in(device), C.GEN_N_NEW, tokens_out=out) is out
        got = out.cpu().numpy()
        assert np.array_equal(got[0], first), f"the first tokens: sequences {np.flatnonzero(got[0] != first)} differ"
        for b in C.GEN_ORACLE_SEQS:
            assert first[b] == C.gen_expected(b)[0]
            assert tuple(got[:, b].tolist()) == C.gen_expected(b), f"sequence {b} against generate_ref"
        assert [dec.slot_filled(b) for b in SLOTS] == [C.gen_prefill_rows(b) + C.GEN_N_NEW for b in SLOTS]
        # every sequence alone on a one-slot decoder
        for b in SLOTS:
            alone.begin(_dev(C.slot_enc(b), device))
            if C.gen_prefill_rows(b):
                alone.step(_dev(C.gen_prefill(b), device))
            one = alone.generate(gen_head, [0], _tokens_in(device, [b]), C.GEN_N_NEW).cpu().numpy()
            assert np.array_equal(one[:, 0], got[:, b]), f"sequence {b} alone: {one[:, 0]} vs {got[:, b]}"
        # the caches hold the rows of exactly the tokens fed, at their positions: one more row on four slots, bit for bit
        E, P = C.gen_tables()
        probe = O.uniform((1, C.D), 7400)
        for b in C.GEN_PROBE_SLOTS:
            assert b in C.GEN_ORACLE_SEQS
            fed = [C.gen_token_in(b)] + list(C.gen_expected(b)[:-1])
            rows = head_oracle.embed_rows_ref(E, fed, P, [C.gen_prefill_rows(b)], rows_per_seq=C.GEN_N_NEW)
            whole = np.concatenate([C.gen_prefill(b), rows, probe])
            ref = causal_oracle.decoder_forward_causal_ref(whole, C.slot_enc(b), *C.WIDE, C.SEED)[-1:]
            assert_bits_equal(dec.step_slot(b, _dev(probe, device)).cpu().numpy(), ref, f"slot {b} after generate")
    finally:
        dec.close()
        alone.close()


def test_a_second_call_in_reverse_order_continues_the_first(qg, oracle, device, gen_head):
    """Three tokens, then three more from the first call's last row with the slots in reverse order: what one call of
    six gives on a fresh prefill."""
    dec = _decoder(qg, C.N_SLOTS)
    try:
        _prefill(dec, device)
        six = dec.generate(gen_head, SLOTS, _tokens_in(device), 2 * C.GEN_N_NEW).cpu().numpy()
        assert [dec.slot_filled(b) for b in SLOTS] == [C.gen_prefill_rows(b) + 2 * C.GEN_N_NEW for b in SLOTS]
        _prefill(dec, device)          # begin_slot starts every sequence again
        a = dec.generate(gen_head, SLOTS, _tokens_in(device), C.GEN_N_NEW)
        back = SLOTS[::-1]
        b = dec.generate(gen_head, back, a[-1].flip(0).contiguous(), C.GEN_N_NEW)
        got = np.concatenate([a.cpu().numpy(), b.cpu().numpy()[:, ::-1]])
        assert np.array_equal(got, six), f"sequences {np.flatnonzero((got != six).any(axis=0))} differ"
        for s in C.GEN_ORACLE_SEQS:
            assert tuple(six[:C.GEN_N_NEW, s].tolist()) == C.gen_expected(s)
        assert len(set(six[-1].tolist())) >= 2
    finally:
        dec.close()
