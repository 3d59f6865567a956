"""GPU parity of Head.sample_tokens and Decoder.generate_sampled, on the model and sizes of tests/test_gpu_generate.py
(d_model 64, vocabulary 1000, three cache slots prefilled with 5, 0 and 2 rows, six new tokens; its helpers are used as
they are).  The tokens are compared with sample_oracle.generate_sampled_ref on every sequence's whole prefix, with the
same loop driven from Python through embed / step_batch / sample_tokens, and with every sequence generated alone on a
one-slot decoder under the same stream number."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import causal_oracle
import head_oracle
import sample_oracle as SO
import test_gpu_generate as G
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

N_NEW, PRE, TOK_IN, D = G.N_NEW, G.PRE, G.TOK_IN, G.D
TOP_K, TOP_P, TEMP, SAMPLE_SEED = 50, 0.9, 0.8, 31
STREAMS = (7, 1, 40)                              # a sequence's stream number goes with it, whatever its slot
INVALID = 1


@functools.lru_cache(maxsize=None)
def _expected(eos=None, top_k=TOP_K, temperature=TEMP):
    """generate_sampled_ref per sequence, as an N_NEW x 3 array (computed once per end token)."""
    E, P, W, bias = G._model()
    cols = [SO.generate_sampled_ref(G._seq(b)[0], G._seq(b)[1], TOK_IN[b], N_NEW, E, W, bias, P, G.DIMS, G.SEED, top_k,
                                    TOP_P, temperature, SAMPLE_SEED, STREAMS[b], eos) for b in range(3)]
    out = np.array(cols, np.int32).T.copy()
    out.flags.writeable = False
    return out


def _sampled(dec, head, slots, tokens_in, n_new, seqs=(0, 1, 2), **kw):
    kw.setdefault("streams", [STREAMS[b] for b in seqs])
    return dec.generate_sampled(head, slots, tokens_in, n_new, TOP_K, TOP_P, TEMP, SAMPLE_SEED, **kw)


def test_generate_sampled_against_three_references(qg, oracle, device):
    want = _expected()
    assert (want != G._expected(False)).any(), "the draws leave the greedy trajectory somewhere"
    dec, loop, alone = G._decoder(qg, 3), G._decoder(qg, 3), G._decoder(qg, 1)
    head = G._head(qg, device)
    try:
        G._prefill(dec, device)
        out = torch.full((N_NEW, 3), -1, dtype=torch.int32, device=device)
        assert _sampled(dec, head, [0, 1, 2], G._tokens_in(device), N_NEW, tokens_out=out) is out
        got = out.cpu().numpy()
        assert np.array_equal(got, want), f"generate_sampled against generate_sampled_ref:\n{got}\n{want}"
        assert [dec.slot_filled(b) for b in range(3)] == [PRE[b] + N_NEW for b in range(3)]
        # the caches hold the rows of exactly the tokens fed: one more row per slot, bit for bit, as the greedy test does
        E, P = G._model()[:2]
        probe = O.uniform((1, D), 650)
        for b in range(3):
            fed = [TOK_IN[b]] + want[:-1, b].tolist()
            rows = head_oracle.embed_rows_ref(E, fed, P, [PRE[b]], rows_per_seq=N_NEW)
            whole = np.concatenate([G._seq(b)[0], rows, probe])
            ref = causal_oracle.decoder_forward_causal_ref(whole, G._seq(b)[1], *G.DIMS, G.SEED)[-1:]
            assert_bits_equal(dec.step_slot(b, G._dev(probe, device)).cpu().numpy(), ref, f"slot {b} after generate")
        # the same loop driven from Python
        G._prefill(loop, device)
        tok, rows = G._tokens_in(device), []
        for t in range(N_NEW):
            pos = [PRE[b] + t for b in range(3)]
            H = loop.step_batch([0, 1, 2], head.embed(tok, pos), pos=pos)
            tok = head.sample_tokens(H, TOP_K, TOP_P, TEMP, SAMPLE_SEED,
                                     counters=[(STREAMS[b] << 32) + pos[b] for b in range(3)], prev=tok)
            rows.append(tok.cpu().numpy())
        assert np.array_equal(np.stack(rows), want), "the Python-driven loop"
        # every sequence alone on a one-slot decoder, under its own stream number
        for b in range(3):
            G._prefill(alone, device, seqs=(b,))
            one = _sampled(alone, head, [0], G._tokens_in(device, (b,)), N_NEW, seqs=(b,)).cpu().numpy()
            assert np.array_equal(one[:, 0], want[:, b]), f"sequence {b} alone"
    finally:
        head.close()
        for d in (dec, loop, alone):
            d.close()


def test_two_calls_and_a_permuted_batch(qg, oracle, device):
    """The counter is the position: six tokens as two calls of three, with the slots in another order."""
    want = _expected()
    dec, head = G._decoder(qg, 3), G._head(qg, device)
    try:
        G._prefill(dec, device)
        order = [2, 0, 1]
        a = _sampled(dec, head, order, G._tokens_in(device, order), 3, seqs=order)
        b = _sampled(dec, head, order, a[2], 3, seqs=order)
        assert np.array_equal(torch.cat([a, b]).cpu().numpy(), want[:, order])
        # a rewind repeats its draws
        again = _sampled(dec, head, order, a[2], 3, seqs=order, pos=[PRE[s] + 3 for s in order])
        assert torch.equal(again, b)
    finally:
        head.close()
        dec.close()


def test_default_streams_are_the_slots(qg, oracle, device):
    dec, head = G._decoder(qg, 3), G._head(qg, device)
    try:
        G._prefill(dec, device)
        a = dec.generate_sampled(head, [0, 1, 2], G._tokens_in(device), 2, TOP_K, TOP_P, TEMP, SAMPLE_SEED)
        b = dec.generate_sampled(head, [0, 1, 2], G._tokens_in(device), 2, TOP_K, TOP_P, TEMP, SAMPLE_SEED,
                                 streams=[0, 1, 2], pos=list(PRE))
        assert torch.equal(a, b)
    finally:
        head.close()
        dec.close()


@pytest.mark.parametrize("top_k,temperature", [(1, TEMP), (TOP_K, 0.0)])
def test_greedy_settings_give_generates_tokens(qg, oracle, device, top_k, temperature):
    want = G._expected(False)
    dec, head = G._decoder(qg, 3), G._head(qg, device)
    try:
        G._prefill(dec, device)
        got = dec.generate_sampled(head, [0, 1, 2], G._tokens_in(device), N_NEW, top_k, TOP_P, temperature, SAMPLE_SEED)
        assert np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(dec.generate(head, [0, 1, 2], G._tokens_in(device), N_NEW, pos=list(PRE)), got)
    finally:
        head.close()
        dec.close()


def test_end_token_is_held(qg, oracle, device):
    """eos = the token sequence 0 emits at step 2 of the free trajectory: from there on the sequence emits eos, its
    steps still run (fed with eos), and the other sequences go on."""
    free = _expected()
    eos = int(free[2, 0])
    assert eos not in free[:2, 0].tolist()
    want = _expected(eos)
    assert (want[2:, 0] == eos).all() and np.array_equal(want[:3], free[:3])
    dec, head = G._decoder(qg, 3), G._head(qg, device)
    try:
        G._prefill(dec, device)
        got = _sampled(dec, head, [0, 1, 2], G._tokens_in(device), N_NEW, eos=eos).cpu().numpy()
        assert np.array_equal(got, want), f"\n{got}\n{want}"
        assert [dec.slot_filled(b) for b in range(3)] == [PRE[b] + N_NEW for b in range(3)]
    finally:
        head.close()
        dec.close()


def test_captured_generate_sampled_replays(qg, oracle, device):
    """4 tokens of 2 slots captured once with explicit positions, so that every replay rewinds and repeats its draws."""
    want = _expected()[:4, :2]
    L = qg.load()
    dec, head = G._decoder(qg, 3), G._head(qg, device)
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    try:
        tin = G._tokens_in(device, (0, 1))
        out = torch.full((4, 2), -1, dtype=torch.int32, device=device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            G._prefill(dec, device)
            eager = _sampled(dec, head, [0, 1], tin, 4, seqs=(0, 1), pos=list(PRE[:2])).cpu().numpy()   # the warm-up
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = L.qgemm_decoder_generate_sampled(dec._h, head._h, 2, ints([0, 1]), tin.data_ptr(), 4,
                                                      ints(list(PRE[:2])), TOP_K, TOP_P, TEMP, SAMPLE_SEED,
                                                      (ctypes.c_uint32 * 2)(*STREAMS[:2]), -1, out.data_ptr(),
                                                      s.cuda_stream)
                assert rc == 0
        assert np.array_equal(eager, want)
        for i in range(2):
            out.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), f"replay {i}"
    finally:
        head.close()
        dec.close()


def test_refusals(qg, oracle, device):
    dec, plain = G._decoder(qg, 3), G._decoder(qg, 1, kv_cache=False)
    head, one_row = G._head(qg, device, max_rows=8), G._head(qg, device, max_rows=1)
    try:
        G._prefill(dec, device, seqs=(0, 1))                     # slot 2 is never begun

        def refused(d, h, slots, n_new=N_NEW, pos=None, top_k=TOP_K, top_p=TOP_P, temperature=TEMP):
            out = torch.full((n_new, len(slots)), -1, dtype=torch.int32, device=device)
            with pytest.raises(qg.QGemmError) as e:
                d.generate_sampled(h, slots, G._tokens_in(device)[:len(slots)].contiguous(), n_new, top_k, top_p,
                                   temperature, SAMPLE_SEED, pos=pos, tokens_out=out)
            assert e.value.code == INVALID
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == -1).all(), "a refused call launches nothing"

        refused(dec, head, [0, 2])                               # a slot not begun
        refused(dec, head, [0, 1], n_new=G.MAX_SEQ - PRE[0] + 1)  # pos + n_new > max_seq
        refused(dec, head, [0, 1], pos=[PRE[0] + 1, 0])          # a position past the filled length
        refused(dec, head, [0, 0])                               # a slot twice
        refused(dec, one_row, [0, 1])                            # more sequences than the head's max_rows
        refused(plain, head, [0])                                # a decoder without caches
        for bad in (dict(top_k=0), dict(top_k=1025), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
                    dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan"))):
            refused(dec, head, [0, 1], **bad)
        assert [dec.slot_filled(b) for b in range(3)] == [PRE[0], PRE[1], None]
        H = G._dev(O.uniform((2, D), 640), device)
        tok = torch.full((2,), -1, dtype=torch.int32, device=device)
        with pytest.raises(qg.QGemmError):
            head.sample_tokens(H, 0, tokens=tok)                 # refused before the logits are launched
        with pytest.raises(qg.QGemmError):
            one_row.sample_tokens(H, 4, tokens=tok)              # more rows than max_rows
        torch.cuda.synchronize()
        assert (tok.cpu().numpy() == -1).all()
        assert _sampled(dec, head, [0, 1], G._tokens_in(device)[:2].contiguous(), 0, seqs=(0, 1)).shape == (0, 2)
        assert [dec.slot_filled(b) for b in range(2)] == [PRE[0], PRE[1]]
    finally:
        head.close()
        one_row.close()
        dec.close()
        plain.close()
