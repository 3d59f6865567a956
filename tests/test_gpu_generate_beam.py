"""GPU parity of Decoder.generate_beam on the model and sizes of tests/test_gpu_generate.py (d_model 64, 2 heads, d_ff
128, 2 blocks, three groups with enc_seq 33, 20 and 9 prefilled with 5, 0 and 2 rows, six new tokens), three beams per
group in two sets of nine cache slots, at vocabulary 1000 and once more at 8200 (the split plans).  Tokens, parents and
the bits of the scores are compared with beam_oracle.generate_beam_ref on whole prefixes and with the same loop driven
from Python through embed / step_batch / logits / the numpy beam step / copy_slot."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import beam_oracle as BO
import test_gpu_generate as G
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

N_NEW, PRE, TOK_IN, D, DIMS, SEED = G.N_NEW, G.PRE, G.TOK_IN, G.D, G.DIMS, G.SEED
BEAMS, GROUPS = 3, 3
ROWS = BEAMS * GROUPS
SLOTS_A, SLOTS_B = list(range(ROWS)), list(range(ROWS, 2 * ROWS))
INVALID = 1


@functools.lru_cache(maxsize=None)
def _model(vocab):
    """E, P, W (d_model x vocab) and a bias: test_gpu_generate's at its vocabulary, seeded alike at another."""
    if vocab == G.VOCAB:
        return G._model()
    arrs = (O.uniform((vocab, D), 611), O.uniform((G.MAX_POS, D), 612, -0.1, 0.1), O.uniform((D, vocab), 613),
            O.uniform((vocab,), 614, -0.05, 0.05))
    for a in arrs:
        a.flags.writeable = False
    return arrs


@functools.lru_cache(maxsize=None)
def _expected(vocab=G.VOCAB, beams=BEAMS, eos=-1):
    """generate_beam_ref over the three groups (computed once per setting): (tokens, parents, scores, final rows)."""
    E, P, W, bias = _model(vocab)
    tok_in = np.repeat(np.array(TOK_IN, np.int32), beams)
    out = BO.generate_beam_ref([G._seq(g)[0] for g in range(GROUPS)], [G._seq(g)[1] for g in range(GROUPS)], tok_in,
                               N_NEW, beams, E, W, bias, P, DIMS, SEED, eos=eos)
    for a in out[:3]:
        a.flags.writeable = False
    return out


def _decoder(qg, n_slots=2 * ROWS):
    return qg.Decoder(*DIMS, max_seq=G.MAX_SEQ, max_enc_seq=33, seed=SEED, causal=True, kv_cache=True, n_slots=n_slots)


def _head(qg, device, vocab=G.VOCAB, max_rows=ROWS):
    E, P, W, bias = _model(vocab)
    return qg.Head(qg.pack_b(G._dev(W, device)), vocab, G._dev(bias, device), G._dev(E, device), G._dev(P, device),
                   max_rows=max_rows)


def _prefill(dec, device, beams=BEAMS, slots_a=None, slots_b=None):
    """Group g's sequence into its first set-A slot, then forked into the group's other slots of both sets."""
    slots_a = list(range(GROUPS * beams)) if slots_a is None else slots_a
    slots_b = list(range(GROUPS * beams, 2 * GROUPS * beams)) if slots_b is None else slots_b
    for g in range(GROUPS):
        first = slots_a[g * beams]
        dec.begin_slot(first, G._dev(G._seq(g)[1], device))
        if PRE[g]:
            dec.step_slot(first, G._dev(G._seq(g)[0], device))
        dec.beam_fork(first, slots_a[g * beams:(g + 1) * beams], slots_b[g * beams:(g + 1) * beams])
    return slots_a, slots_b


def _tokens_in(device):
    return torch.tensor(TOK_IN, dtype=torch.int32, device=device)


def _same(got, want, what):
    tok, par, sc = (t.cpu().numpy() for t in got)
    assert np.array_equal(tok, want[0]), f"{what}: tokens\n{tok}\n{want[0]}"
    assert np.array_equal(par, want[1]), f"{what}: parents\n{par}\n{want[1]}"
    assert_bits_equal(sc, want[2], f"{what}: scores")


@pytest.mark.parametrize("vocab", [G.VOCAB, 8200])
def test_against_the_oracle_and_the_python_loop(qg, oracle, device, vocab):
    want = _expected(vocab)
    assert len({tuple(r) for r in want[1].tolist()}) > 1, "the parents are not one fixed permutation"
    if vocab == 8200:
        assert qg.beam_step_plan(GROUPS, BEAMS, vocab) == (2, 2)
    dec, loop, alone = _decoder(qg), _decoder(qg), _decoder(qg, 1)
    head = _head(qg, device, vocab)
    try:
        _prefill(dec, device)
        got = dec.generate_beam(head, SLOTS_A, SLOTS_B, _tokens_in(device), N_NEW, BEAMS)
        _same(got, want, "generate_beam against generate_beam_ref")
        assert [dec.slot_filled(s) for s in SLOTS_A + SLOTS_B] == [PRE[s % ROWS // BEAMS] + N_NEW for s in range(2 * ROWS)]
        if vocab == G.VOCAB:
            # the live set (A after six steps) holds the K and V rows of every final hypothesis replayed alone
            for r in range(ROWS):
                rows = want[3][r]
                if rows is None:
                    continue
                alone.begin_slot(0, G._dev(G._seq(r // BEAMS)[1], device))
                alone.step_slot(0, G._dev(rows, device))
                for b in range(2):
                    a, c = dec.read_slot(b, SLOTS_A[r])[0], alone.read_slot(b, 0)[0]
                    n = rows.shape[0]
                    assert torch.equal(a[:n, D:].view(torch.int32), c[:n, D:].view(torch.int32)), f"place {r} block {b}"
        # the same loop driven from Python: the numpy beam step on read-back logits, copy_slot into the other set
        cur, other = _prefill(loop, device)
        tok = _tokens_in(device).repeat_interleave(BEAMS).contiguous()
        sc, rows_t, rows_p, rows_s = None, [], [], []
        for t in range(N_NEW):
            pos = [PRE[r // BEAMS] + t for r in range(ROWS)]
            logits = head.logits(loop.step_batch(cur, head.embed(tok, pos), pos=pos)).cpu().numpy()
            par, ntok, nsc = BO.beam_step_ref(logits, BEAMS, sc, tok.cpu().numpy(), -1)
            for i in range(ROWS):
                loop.copy_slot(other[i], cur[i // BEAMS * BEAMS + int(par[i])])
            rows_t.append(ntok), rows_p.append(par), rows_s.append(nsc)
            tok, sc, cur, other = G._dev(ntok, device), nsc, other, cur
        _same(got, (np.stack(rows_t), np.stack(rows_p), np.stack(rows_s)), "the Python-driven loop")
        hyp = qg.beam_hypotheses(*got, beams=BEAMS)
        assert [h[0] for h in hyp if h[0]] and all(len(h[0]) == N_NEW for h in hyp if h[0])
    finally:
        head.close()
        for d in (dec, loop, alone):
            d.close()


def test_one_beam_is_generate(qg, oracle, device):
    dec, head = _decoder(qg, 6), _head(qg, device)
    try:
        a, b = _prefill(dec, device, beams=1)
        tok, par, sc = dec.generate_beam(head, a, b, _tokens_in(device), N_NEW, 1)
        assert np.array_equal(tok.cpu().numpy(), G._expected(False)) and not par.cpu().numpy().any()
        _same((tok, par, sc), _expected(beams=1), "beams = 1 against the oracle")
    finally:
        head.close()
        dec.close()


def test_two_calls_continue_one(qg, oracle, device):
    want = _expected()
    dec, head = _decoder(qg), _head(qg, device)
    try:
        _prefill(dec, device)
        first = dec.generate_beam(head, SLOTS_A, SLOTS_B, _tokens_in(device), 3, BEAMS)
        assert [dec.slot_filled(s) for s in SLOTS_B] == [PRE[r // BEAMS] + 3 for r in range(ROWS)]
        second = dec.generate_beam(head, SLOTS_B, SLOTS_A, first[0][2], 3, BEAMS, scores_in=first[2][2])   # B holds them
        _same(tuple(torch.cat([x, y]) for x, y in zip(first, second)), want, "three and three")
    finally:
        head.close()
        dec.close()


def test_end_token_is_held(qg, oracle, device):
    """eos = the best token of group 0 at step 2 of the free search.  A hypothesis that emits it is held from the next
    step on -- token eos, score frozen -- while it competes with the group's live beams; one of them finishes at step
    2, in the middle of the search, and survives."""
    eos = int(_expected()[0][2, 0])
    want = _expected(eos=eos)
    tok, par, sc = want[:3]
    src = lambda t, r: r // BEAMS * BEAMS + int(par[t, r])
    held = [(t, r) for t in range(1, N_NEW) for r in range(ROWS) if tok[t, r] == eos and tok[t - 1, src(t, r)] == eos]
    for t, r in held:
        assert sc[t, r] == sc[t - 1, src(t, r)], "a held hypothesis keeps its score"
    fresh = [(t, r) for t in range(2, N_NEW - 1) for r in range(ROWS) if tok[t, r] == eos and tok[t - 1, src(t, r)] != eos]
    assert any((t + 1, q) in held and src(t + 1, q) == r for t, r in fresh for q in range(ROWS)), \
        "a hypothesis finishes in the middle of the search and is held"
    dec, head = _decoder(qg), _head(qg, device)
    try:
        _prefill(dec, device)
        got = dec.generate_beam(head, SLOTS_A, SLOTS_B, _tokens_in(device), N_NEW, BEAMS, eos=eos)
        _same(got, want, "with an end token")
        hyp = qg.beam_hypotheses(*got, eos=eos, beams=BEAMS)
        for t, r in held:
            if t == N_NEW - 1:
                assert hyp[r][0][-1] == eos and eos not in hyp[r][0][:-1] and len(hyp[r][0]) < N_NEW
    finally:
        head.close()
        dec.close()


def test_captured_generate_beam_replays(qg, oracle, device):
    """The call allocates nothing and does not synchronize: captured as the first work of a fresh stream with explicit
    positions and replayed twice (a group's slots share their prefix rows, so every replay starts from the same state)."""
    want = _expected()
    L = qg.load()
    dec, head = _decoder(qg), _head(qg, device)
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    try:
        tin = _tokens_in(device).repeat_interleave(BEAMS).contiguous()
        out = (torch.full((N_NEW, ROWS), -1, dtype=torch.int32, device=device),
               torch.full((N_NEW, ROWS), -1, dtype=torch.int32, device=device),
               torch.full((N_NEW, ROWS), float("nan"), device=device))
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            _prefill(dec, device)
            eager = dec.generate_beam(head, SLOTS_A, SLOTS_B, tin, N_NEW, BEAMS, pos=list(PRE))     # also the warm-up
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = L.qgemm_decoder_generate_beam(dec._h, head._h, GROUPS, BEAMS, ints(SLOTS_A), ints(SLOTS_B),
                                                   tin.data_ptr(), N_NEW, ints(list(PRE)), None, -1, out[0].data_ptr(),
                                                   out[1].data_ptr(), out[2].data_ptr(), s.cuda_stream)
                assert rc == 0
        _same(eager, want, "the eager call")
        for i in range(2):
            out[0].fill_(-1), out[1].fill_(-1), out[2].fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            _same(out, want, f"replay {i}")
    finally:
        head.close()
        dec.close()


def test_refusals(qg, oracle, device):
    dec, plain = _decoder(qg, 2 * ROWS + 2), G._decoder(qg, 1, kv_cache=False)
    head, small = _head(qg, device), _head(qg, device, max_rows=ROWS - 1)
    try:
        _prefill(dec, device)                                    # slots 18 and 19 are never begun
        state = [dec.slot_filled(s) for s in range(2 * ROWS + 2)]

        def refused(a=SLOTS_A, b=SLOTS_B, n_new=N_NEW, beams=BEAMS, pos=None, d=dec, h=head):
            rows = len(a)
            out = (torch.full((n_new, rows), -1, dtype=torch.int32, device=device),
                   torch.full((n_new, rows), -1, dtype=torch.int32, device=device),
                   torch.full((n_new, rows), 1.0, device=device))
            with pytest.raises(qg.QGemmError) as e:
                d.generate_beam(h, a, b, _tokens_in(device).repeat_interleave(BEAMS)[:rows].contiguous(), n_new, beams,
                                pos=pos, out=out)
            assert e.value.code == INVALID
            torch.cuda.synchronize()
            assert (out[0].cpu().numpy() == -1).all() and (out[2].cpu().numpy() == 1).all(), "a refused call launches nothing"

        refused(b=SLOTS_B[:-1] + [18])                           # a slot not begun
        refused(b=SLOTS_B[:-1] + [20])                           # a slot out of range
        refused(a=SLOTS_A[:-1] + [0])                            # a slot twice in one set
        refused(b=SLOTS_B[:-1] + [0])                            # a slot in both sets
        refused(b=SLOTS_B[BEAMS:] + SLOTS_B[:BEAMS])             # set B's enc_seq differs from its set-A counterpart
        refused(n_new=G.MAX_SEQ - PRE[0] + 1)                    # pos + n_new > max_seq
        refused(pos=[PRE[0] + 1, 0, 0])                          # a position past the filled length
        refused(pos=[-1, 0, 0])
        refused(h=small)                                         # more rows than the head's max_rows
        refused(d=plain)                                         # a decoder without caches
        refused(a=SLOTS_A[:8], b=SLOTS_B[:8], beams=4)           # groups that mix sequences: enc_seq differs inside one
        refused(beams=ROWS)                                      # more than 8 beams
        assert [dec.slot_filled(s) for s in range(2 * ROWS + 2)] == state, "no filled length moved"
        tok, par, sc = dec.generate_beam(head, SLOTS_A, SLOTS_B, _tokens_in(device), 0, BEAMS)
        assert tok.shape == (0, ROWS) and [dec.slot_filled(s) for s in range(2 * ROWS + 2)] == state
    finally:
        head.close()
        small.close()
        dec.close()
        plain.close()
