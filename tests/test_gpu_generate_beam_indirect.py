"""GPU parity of the copy-free beam search (Decoder.generate_beam_indirect) on the model, groups and sizes
of tests/test_gpu_generate_beam.py: nine beam slots begun by beam_begin from three prompt slots, ONE slot set, no K / V
row copied.  Tokens, parents and the bits of the scores are compared with beam_oracle.generate_beam_ref and with
generate_beam (the copy path) on a second decoder; the K / V rows every final place sees through the row table are
compared with the copy path's live set and with the hypothesis replayed alone."""
import ctypes

import numpy as np
import pytest
import torch

import beam_indirect_oracle as BI
import beam_oracle as BO
import test_gpu_generate as G
import test_gpu_generate_beam as B
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

N_NEW, PRE, D, BEAMS, GROUPS, ROWS = B.N_NEW, B.PRE, B.D, B.BEAMS, B.GROUPS, B.ROWS
SLOTS = list(range(ROWS))
SRC = [ROWS, ROWS + 1, ROWS + 2]
N_SLOTS = ROWS + 5                     # slots 12 and 13 are never begun
INVALID = 1


def _decoder(qg, n_slots=N_SLOTS):
    return B._decoder(qg, n_slots)


def _prompts(dec, device, src=SRC, seqs=(0, 1, 2)):
    """Sequence seqs[g] into prompt slot src[g]: begin_slot and, where it has prefill rows, one step_slot."""
    for slot, g in zip(src, seqs):
        dec.begin_slot(slot, G._dev(G._seq(g)[1], device))
        if PRE[g]:
            dec.step_slot(slot, G._dev(G._seq(g)[0], device))


def _start(dec, device, beams=BEAMS, slots=None, src=SRC):
    slots = list(range(GROUPS * beams)) if slots is None else slots
    _prompts(dec, device, src)
    dec.beam_begin(slots, src, None, beams)
    return slots


def _kv(dec, block, slots):
    """[len(slots), max_seq, 2 d_model]: the K and V thirds of the slots' self slabs of one block, as int32 bits."""
    return np.stack([dec.read_slot(block, s)[0][:, D:].contiguous().view(torch.int32).cpu().numpy() for s in slots])


@pytest.mark.parametrize("vocab", [G.VOCAB, 8200])
def test_against_the_oracle_and_the_copy_path(qg, oracle, device, vocab):
    want = B._expected(vocab)
    dec, old, alone = _decoder(qg), B._decoder(qg), B._decoder(qg, 1)
    head = B._head(qg, device, vocab)
    try:
        _prompts(dec, device)
        prompt_before = [[t.clone() for t in dec.read_slot(b, s)] for b in range(2) for s in SRC]
        dec.beam_begin(SLOTS, SRC, None, BEAMS)
        beam_before = [_kv(dec, b, SLOTS) for b in range(2)]
        got = dec.generate_beam_indirect(head, SLOTS, SRC, B._tokens_in(device), N_NEW, BEAMS)
        B._same(got, want, "generate_beam_indirect against generate_beam_ref")
        assert [dec.slot_filled(s) for s in SLOTS] == [PRE[r // BEAMS] + N_NEW for r in range(ROWS)]
        B._prefill(old, device)
        copy = old.generate_beam(head, B.SLOTS_A, B.SLOTS_B, B._tokens_in(device), N_NEW, BEAMS)
        B._same(got, tuple(t.cpu().numpy() for t in copy), "generate_beam_indirect against generate_beam")
        if vocab != G.VOCAB:
            return
        # the rows every final place sees through the table: the copy path's live set (A after six steps), and the
        # hypothesis replayed alone
        table = dec.beam_table().cpu().numpy()
        for b in range(2):
            slabs = _kv(dec, b, range(N_SLOTS))
            live = _kv(old, b, B.SLOTS_A)
            for r in range(ROWS):
                n = PRE[r // BEAMS] + N_NEW
                assert (table[SLOTS[r], :n] < N_SLOTS).all()
                eff = BI.effective(slabs, table[SLOTS[r]], n)
                assert np.array_equal(eff, live[r, :n]), f"place {r} block {b}: the copy path's rows"
                rows = want[3][r]
                if rows is not None:
                    alone.begin_slot(0, G._dev(G._seq(r // BEAMS)[1], device))
                    alone.step_slot(0, G._dev(rows, device))
                    assert np.array_equal(eff, _kv(alone, b, [0])[0, :n]), f"place {r} block {b}: replayed alone"
        # no copy happened: the prompt slots' slabs are as they were, and a beam slot's slab changed only at the rows of
        # its own appends (rows pos .. pos + n_new - 1), which are finite
        after = [[t for t in dec.read_slot(b, s)] for b in range(2) for s in SRC]
        for x, y in zip(prompt_before, after):
            assert torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)) and \
                torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)), "a prompt slot's slab changed"
        for b in range(2):
            now = _kv(dec, b, SLOTS)
            for r in range(ROWS):
                p = PRE[r // BEAMS]
                assert np.array_equal(now[r, :p], beam_before[b][r, :p]), f"place {r}: rows below pos were written"
                assert np.array_equal(now[r, p + N_NEW:], beam_before[b][r, p + N_NEW:]), f"place {r}: rows past the end"
                assert np.isfinite(now[r, p:p + N_NEW].view(np.float32)).all()
                assert (table[SLOTS[r], p:p + N_NEW] < ROWS).all(), "a new row lives in a beam slot's slab"
                assert (table[SLOTS[r], :p] == SRC[r // BEAMS]).all(), "the prompt rows stay in the prompt's slab"
    finally:
        head.close()
        for d in (dec, old, alone):
            d.close()


def test_python_driven_loop(qg, oracle, device):
    """step_batch_indirect + the numpy beam step on read-back logits + beam_reindex, step by step: the one call's rows."""
    want = B._expected()
    dec, head = _decoder(qg), B._head(qg, device)
    try:
        _start(dec, device)
        cross = [SRC[r // BEAMS] for r in range(ROWS)]
        tok = B._tokens_in(device).repeat_interleave(BEAMS).contiguous()
        sc, rows_t, rows_p, rows_s = None, [], [], []
        for t in range(N_NEW):
            pos = [PRE[r // BEAMS] + t for r in range(ROWS)]
            logits = head.logits(dec.step_batch_indirect(SLOTS, cross, head.embed(tok, pos), pos=pos)).cpu().numpy()
            par, ntok, nsc = BO.beam_step_ref(logits, BEAMS, sc, tok.cpu().numpy(), -1)
            dec.beam_reindex(SLOTS, G._dev(par, device), [PRE[g] + t + 1 for g in range(GROUPS)], BEAMS)
            rows_t.append(ntok), rows_p.append(par), rows_s.append(nsc)
            tok, sc = G._dev(ntok, device), nsc
        got = (np.stack(rows_t), np.stack(rows_p), np.stack(rows_s))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert_bits_equal(got[2], want[2], "the Python-driven loop: scores")
    finally:
        head.close()
        dec.close()


def test_two_calls_continue_one(qg, oracle, device):
    want = B._expected()
    dec, head = _decoder(qg), B._head(qg, device)
    try:
        _start(dec, device)
        first = dec.generate_beam_indirect(head, SLOTS, SRC, B._tokens_in(device), 3, BEAMS)
        assert [dec.slot_filled(s) for s in SLOTS] == [PRE[r // BEAMS] + 3 for r in range(ROWS)]
        second = dec.generate_beam_indirect(head, SLOTS, SRC, first[0][2], 3, BEAMS, scores_in=first[2][2])
        B._same(tuple(torch.cat([x, y]) for x, y in zip(first, second)), want, "three and three")
    finally:
        head.close()
        dec.close()


def test_end_token_is_held(qg, oracle, device):
    eos = int(B._expected()[0][2, 0])          # as test_gpu_generate_beam.test_end_token_is_held
    want = B._expected(eos=eos)
    dec, head = _decoder(qg), B._head(qg, device)
    try:
        _start(dec, device)
        B._same(dec.generate_beam_indirect(head, SLOTS, SRC, B._tokens_in(device), N_NEW, BEAMS, eos=eos), want,
                "with an end token")
    finally:
        head.close()
        dec.close()


def test_one_beam_is_generate_and_the_prompt_slot_may_be_a_place(qg, oracle, device):
    """beams = 1 with slots[g] == src_slots[g]: every sequence goes on in its own slot, the table stays the identity,
    and the tokens are generate's."""
    dec, head = _decoder(qg, 3), B._head(qg, device)
    try:
        _start(dec, device, beams=1, slots=[0, 1, 2], src=[0, 1, 2])
        tok, par, sc = dec.generate_beam_indirect(head, [0, 1, 2], [0, 1, 2], B._tokens_in(device), N_NEW, 1)
        assert np.array_equal(tok.cpu().numpy(), G._expected(False)) and not par.cpu().numpy().any()
        B._same((tok, par, sc), B._expected(beams=1), "beams = 1 against the oracle")
        assert np.array_equal(dec.beam_table().cpu().numpy(), BI.identity(3, G.MAX_SEQ))
    finally:
        head.close()
        dec.close()


def test_first_place_is_the_prompt_slot(qg, oracle, device):
    """slots[g * beams] == src_slots[g]: the prompt's slot carries a beam itself."""
    src = [0, BEAMS, 2 * BEAMS]
    dec, head = _decoder(qg, ROWS), B._head(qg, device)
    try:
        _start(dec, device, slots=SLOTS, src=src)
        B._same(dec.generate_beam_indirect(head, SLOTS, src, B._tokens_in(device), N_NEW, BEAMS), B._expected(),
                "the prompt slot is place 0")
        dec.beam_begin(SLOTS, src, list(PRE), BEAMS)             # its prompt rows are still its own: the search again
        B._same(dec.generate_beam_indirect(head, SLOTS, src, B._tokens_in(device), N_NEW, BEAMS), B._expected(),
                "the search again after a second beam_begin")
    finally:
        head.close()
        dec.close()


def test_more_than_32_rows(qg, oracle, device):
    """5 groups x 7 beams = 35 rows on a 64-slot decoder, three new tokens: the case the copy path refuses.  Groups 3
    and 4 reuse the encoder inputs and prefixes of groups 0 and 1 with other start tokens."""
    beams, seqs, n_new = 7, (0, 1, 2, 0, 1), 3
    rows = beams * len(seqs)
    start = [G.TOK_IN[0], G.TOK_IN[1], G.TOK_IN[2], 5, 123]
    E, P, W, bias = B._model(G.VOCAB)
    want = BO.generate_beam_ref([G._seq(g)[0] for g in seqs], [G._seq(g)[1] for g in seqs],
                                np.repeat(np.array(start, np.int32), beams), n_new, beams, E, W, bias, P, B.DIMS, B.SEED)
    slots, src = list(range(rows)), list(range(rows, rows + 5))
    dec, head = _decoder(qg, 64), B._head(qg, device, max_rows=rows)
    try:
        _prompts(dec, device, src, seqs)
        dec.beam_begin(slots, src, None, beams)
        tin = torch.tensor(start, dtype=torch.int32, device=device)
        B._same(dec.generate_beam_indirect(head, slots, src, tin, n_new, beams), want, "35 rows")
        with pytest.raises(qg.QGemmError):                       # two sets of 35 do not fit 64 slots, and 35 > 32
            dec.generate_beam(head, slots[:rows], list(range(29, 64)), tin, n_new, beams)
    finally:
        head.close()
        dec.close()


def test_captured_search_replays(qg, oracle, device):
    """beam_begin + the generate call captured on a fresh stream and replayed twice: begin puts the table back to the
    search's start, so every replay gives the oracle's rows."""
    want = B._expected()
    L = qg.load()
    dec, head = _decoder(qg), B._head(qg, device)
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    try:
        tin = B._tokens_in(device).repeat_interleave(BEAMS).contiguous()
        out = (torch.full((N_NEW, ROWS), -1, dtype=torch.int32, device=device),
               torch.full((N_NEW, ROWS), -1, dtype=torch.int32, device=device),
               torch.full((N_NEW, ROWS), float("nan"), device=device))
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            _start(dec, device)
            eager = dec.generate_beam_indirect(head, SLOTS, SRC, tin, N_NEW, BEAMS, pos=list(PRE))   # also the warm-up
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                assert L.qgemm_decoder_beam_begin(dec._h, GROUPS, BEAMS, ints(SLOTS), ints(SRC), ints(list(PRE)),
                                                  s.cuda_stream) == 0
                assert L.qgemm_decoder_generate_beam_indirect(
                    dec._h, head._h, GROUPS, BEAMS, ints(SLOTS), ints(SRC), tin.data_ptr(), N_NEW, ints(list(PRE)), None,
                    -1, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), s.cuda_stream) == 0
        B._same(eager, want, "the eager call")
        for i in range(2):
            out[0].fill_(-1), out[1].fill_(-1), out[2].fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            B._same(out, want, f"replay {i}")
    finally:
        head.close()
        dec.close()


def test_refusals(qg, oracle, device):
    dec, plain, single = _decoder(qg), G._decoder(qg, 1, kv_cache=False), G._decoder(qg, 1)
    head, small = B._head(qg, device), B._head(qg, device, max_rows=ROWS - 1)
    try:
        _start(dec, device)                                      # slots 12 and 13 are never begun
        state = lambda: [dec.slot_filled(s) for s in range(N_SLOTS)]
        before = state()

        def refused(slots=SLOTS, src=SRC, n_new=N_NEW, beams=BEAMS, pos=None, d=dec, h=head):
            rows = len(slots)
            out = (torch.full((n_new, rows), -1, dtype=torch.int32, device=device),
                   torch.full((n_new, rows), -1, dtype=torch.int32, device=device),
                   torch.full((n_new, rows), 1.0, device=device))
            with pytest.raises(qg.QGemmError) as e:
                d.generate_beam_indirect(h, slots, src, B._tokens_in(device).repeat_interleave(BEAMS)[:rows].contiguous(),
                                         n_new, beams, pos=pos, out=out)
            assert e.value.code == INVALID
            torch.cuda.synchronize()
            assert (out[0].cpu().numpy() == -1).all() and (out[2].cpu().numpy() == 1).all(), "a refused call launched"

        refused(slots=SLOTS[:-1] + [12])                         # a slot not begun by beam_begin
        refused(slots=SLOTS[:-1] + [N_SLOTS])                    # a slot out of range
        refused(slots=SLOTS[:-1] + [0])                          # a slot named twice
        refused(src=SRC[:2] + [13])                              # a prompt slot not begun
        refused(src=[SRC[1], SRC[0], SRC[2]])                    # a prompt of another enc_seq than the group's slots
        refused(n_new=G.MAX_SEQ - PRE[0] + 1)                    # pos + n_new > max_seq
        refused(pos=[PRE[0] + 1, 0, 0])                          # a position past the filled length
        refused(pos=[-1, 0, 0])
        refused(h=small)                                         # more rows than the head's max_rows
        refused(d=plain)                                         # a decoder without caches
        refused(slots=[0], src=[0], beams=1, d=single)           # one slot: no table
        refused(slots=SLOTS[:8], src=SRC[:2], beams=4)           # groups that mix sequences
        refused(beams=ROWS, src=SRC[:1])                         # more than 8 beams
        assert state() == before, "no filled length moved"
        # the plain calls refuse a slot in this state, before any launch; begin_slot clears the flag
        x = torch.zeros((1, D), device=device)
        for call in (lambda: dec.step_slot(0, x, pos=0), lambda: dec.step_batch([SRC[0], 0], torch.zeros((2, D), device=device),
                                                                                pos=[0, 0]),
                     lambda: dec.copy_slot(12, 0),
                     lambda: dec.generate(head, [0], B._tokens_in(device)[:1].contiguous(), 1),
                     lambda: dec.gather_slots([SRC[0]], [0], torch.zeros(1, dtype=torch.int32, device=device), [0], 1)):
            with pytest.raises(qg.QGemmError) as e:
                call()
            assert e.value.code == INVALID
        assert state() == before
        dec.begin_slot(0, G._dev(G._seq(0)[1], device))
        dec.step_slot(0, x)
        assert dec.slot_filled(0) == 1
        with pytest.raises(qg.QGemmError):                       # ... and the slot no longer belongs to the search
            dec.generate_beam_indirect(head, SLOTS, SRC, B._tokens_in(device), 1, BEAMS)
        tok, par, sc = dec.generate_beam_indirect(head, SLOTS[BEAMS:], SRC[1:], B._tokens_in(device)[1:].contiguous(), 0,
                                                  BEAMS)
        assert tok.shape == (0, ROWS - BEAMS)
    finally:
        head.close()
        small.close()
        for d in (dec, plain, single):
            d.close()
