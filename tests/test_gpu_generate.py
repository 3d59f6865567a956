"""GPU parity of the head object and of Decoder.generate.  Dimensions: those of causal_oracle.DECODER_FUSED (d_model 64,
2 heads, d_ff 128, 2 blocks), a vocabulary of 1000 (no multiple of the GEMM's tiles), three cache slots with enc_seq
33, 20 and 9 prefilled with 5, 0 and 2 rows, six new tokens.  generate's tokens are compared with three references: the
numpy oracle on every sequence's whole prefix, the same loop driven from Python through embed / step_batch /
next_tokens, and every sequence generated alone on a one-slot decoder."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import causal_oracle
import head_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

DIMS = causal_oracle.DECODER_FUSED[2:]
SEED = causal_oracle.DECODER_SEED
D = DIMS[0]
VOCAB, MAX_SEQ, MAX_POS = 1000, 40, 40
ENC, PRE, N_NEW = (33, 20, 9), (5, 0, 2), 6
TOK_IN = (17, 999, 0)
INVALID = 1


@functools.lru_cache(maxsize=None)
def _model():
    """E, P, an untied weight W (d_model x vocab) and a bias: read-only."""
    arrs = (O.uniform((VOCAB, D), 601), O.uniform((MAX_POS, D), 602, -0.1, 0.1), O.uniform((D, VOCAB), 603),
            O.uniform((VOCAB,), 604, -0.05, 0.05))
    for a in arrs:
        a.flags.writeable = False
    return arrs


@functools.lru_cache(maxsize=None)
def _seq(b):
    """Sequence b's prefill rows and encoder output (read-only)."""
    X, enc = O.uniform((PRE[b], D), 620 + b) if PRE[b] else np.zeros((0, D), np.float32), O.uniform((ENC[b], D), 630 + b)
    X.flags.writeable = enc.flags.writeable = False
    return X, enc


@functools.lru_cache(maxsize=None)
def _expected(tied: bool):
    """generate_ref per sequence, as an N_NEW x 3 array (computed once)."""
    E, P, W, bias = _model()
    Wt, bt = (np.ascontiguousarray(E.T), None) if tied else (W, bias)
    cols = [head_oracle.generate_ref(_seq(b)[0], _seq(b)[1], TOK_IN[b], N_NEW, E, Wt, bt, P, DIMS, SEED)
            for b in range(3)]
    out = np.array(cols, np.int32).T.copy()
    out.flags.writeable = False
    return out


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _decoder(qg, n_slots, kv_cache=True):
    return qg.Decoder(*DIMS, max_seq=MAX_SEQ, max_enc_seq=33, seed=SEED, causal=True, kv_cache=kv_cache,
                      n_slots=n_slots)


def _head(qg, device, tied=False, max_rows=8, positions=True):
    E, P, W, bias = _model()
    Ed, Pd = _dev(E, device), _dev(P, device) if positions else None
    if tied:
        return qg.Head(qg.pack_b(Ed.t()), VOCAB, None, Ed, Pd, max_rows=max_rows)
    return qg.Head(qg.pack_b(_dev(W, device)), VOCAB, _dev(bias, device), Ed, Pd, max_rows=max_rows)


def _prefill(dec, device, seqs=(0, 1, 2)):
    for slot, b in enumerate(seqs):
        dec.begin_slot(slot, _dev(_seq(b)[1], device))
        if PRE[b]:
            dec.step_slot(slot, _dev(_seq(b)[0], device))


def _tokens_in(device, seqs=(0, 1, 2)):
    return torch.tensor([TOK_IN[b] for b in seqs], dtype=torch.int32, device=device)


def test_logits_and_next_tokens(qg, oracle, device):
    E, P, W, bias = _model()
    H = O.uniform((5, D), 640)
    Hd, Wp, bd = _dev(H, device), qg.pack_b(_dev(W, device)), _dev(bias, device)
    head = qg.Head(Wp, VOCAB, bd, max_rows=8)
    try:
        want = qg.linear(Hd, Wp, bd)
        got = head.logits(Hd)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "logits() is linear(), bit for bit"
        assert_bits_equal(got.cpu().numpy(), O.linear(H, W, bias), "logits against the oracle")
        wide = torch.full((5, VOCAB + 7), float("nan"), device=device)           # a row-strided output
        head.logits(Hd, out=wide[:, :VOCAB])
        assert torch.equal(wide[:, :VOCAB].view(torch.int32), want.view(torch.int32)) and torch.isnan(wide[:, VOCAB:]).all()
        tok = torch.full((5,), -1, dtype=torch.int32, device=device)
        assert head.next_tokens(Hd, tok) is tok
        want_tok = head_oracle.argmax_rows_ref(O.linear(H, W, bias))[0]
        assert np.array_equal(tok.cpu().numpy(), want_tok)
        assert np.array_equal(head.next_tokens(Hd[1:2]).cpu().numpy(), want_tok[1:2])
        with pytest.raises(qg.QGemmError):
            head.next_tokens(_dev(O.uniform((9, D), 641), device))                # more rows than max_rows
        with pytest.raises(qg.QGemmError):
            head.embed(tok)                                                       # a head without E
    finally:
        head.close()


@pytest.mark.parametrize("tied", [False, True])
def test_generate_against_three_references(qg, oracle, device, tied):
    want = _expected(tied)
    dec, loop, alone = _decoder(qg, 3), _decoder(qg, 3), _decoder(qg, 1)
    head = _head(qg, device, tied)
    try:
        _prefill(dec, device)
        out = torch.full((N_NEW, 3), -1, dtype=torch.int32, device=device)
        assert dec.generate(head, [0, 1, 2], _tokens_in(device), N_NEW, tokens_out=out) is out
        got = out.cpu().numpy()
        assert np.array_equal(got, want), f"generate against generate_ref:\n{got}\n{want}"
        assert [dec.slot_filled(b) for b in range(3)] == [PRE[b] + N_NEW for b in range(3)]
        # the caches hold the rows of exactly the tokens fed, at their positions: one more row per slot, bit for bit
        # (the tokens alone say little about that: this decoder's output moves little with its own input)
        E, P = _model()[:2]
        probe = O.uniform((1, D), 650)
        for b in range(3):
            fed = [TOK_IN[b]] + want[:-1, b].tolist()
            rows = head_oracle.embed_rows_ref(E, fed, P, [PRE[b]], rows_per_seq=N_NEW)
            whole = np.concatenate([_seq(b)[0], rows, probe])
            ref = causal_oracle.decoder_forward_causal_ref(whole, _seq(b)[1], *DIMS, SEED)[-1:]
            assert_bits_equal(dec.step_slot(b, _dev(probe, device)).cpu().numpy(), ref, f"slot {b} after generate")
        # the same loop driven from Python
        _prefill(loop, device)
        tok, rows = _tokens_in(device), []
        for t in range(N_NEW):
            pos = [PRE[b] + t for b in range(3)]
            tok = head.next_tokens(loop.step_batch([0, 1, 2], head.embed(tok, pos), pos=pos))
            rows.append(tok.cpu().numpy())
        assert np.array_equal(np.stack(rows), want), "the Python-driven loop"
        # every sequence alone on a one-slot decoder
        for b in range(3):
            _prefill(alone, device, seqs=(b,))
            one = alone.generate(head, [0], _tokens_in(device, (b,)), N_NEW).cpu().numpy()
            assert np.array_equal(one[:, 0], want[:, b]), f"sequence {b} alone"
    finally:
        head.close()
        for d in (dec, loop, alone):
            d.close()


def test_generate_in_two_calls_and_a_permuted_batch(qg, oracle, device):
    """Slots in another order, and the six tokens as two calls of three: the second call continues from the first
    one's last row."""
    want = _expected(False)
    dec, head = _decoder(qg, 3), _head(qg, device)
    try:
        _prefill(dec, device)
        order = [2, 0, 1]
        a = dec.generate(head, order, _tokens_in(device, order), 3)
        b = dec.generate(head, order, a[2], 3)
        got = torch.cat([a, b]).cpu().numpy()
        assert np.array_equal(got, want[:, order])
    finally:
        head.close()
        dec.close()


def test_captured_generate_replays(qg, oracle, device):
    """generate allocates nothing and does not synchronize: 4 tokens of 2 slots captured once with explicit positions,
    so that every replay rewinds, and replayed twice."""
    want = _expected(False)[:4, :2]
    L = qg.load()
    dec, head = _decoder(qg, 3), _head(qg, device)
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    try:
        tin = _tokens_in(device, (0, 1))
        out = torch.full((4, 2), -1, dtype=torch.int32, device=device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            _prefill(dec, device)
            eager = dec.generate(head, [0, 1], tin, 4, pos=list(PRE[:2])).cpu().numpy()     # also the warm-up
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = L.qgemm_decoder_generate(dec._h, head._h, 2, ints([0, 1]), tin.data_ptr(), 4, ints(list(PRE[:2])),
                                              out.data_ptr(), s.cuda_stream)
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
    dec, plain = _decoder(qg, 3), _decoder(qg, 1, kv_cache=False)
    head, one_row = _head(qg, device, max_rows=8), _head(qg, device, max_rows=1)
    try:
        _prefill(dec, device, seqs=(0, 1))                       # slot 2 is never begun

        def refused(d, h, slots, n_new=N_NEW, pos=None):
            out = torch.full((n_new, len(slots)), -1, dtype=torch.int32, device=device)
            with pytest.raises(qg.QGemmError) as e:
                d.generate(h, slots, _tokens_in(device)[:len(slots)].contiguous(), n_new, pos=pos, tokens_out=out)
            assert e.value.code == INVALID
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == -1).all(), "a refused call launches nothing"

        refused(dec, head, [0, 2])                               # a slot not begun
        refused(dec, head, [0, 1], n_new=MAX_SEQ - PRE[0] + 1)   # pos + n_new > max_seq
        refused(dec, head, [0, 1], pos=[PRE[0] + 1, 0])          # a position past the filled length
        refused(dec, head, [0, 0])                               # a slot twice
        refused(dec, one_row, [0, 1])                            # more sequences than the head's max_rows
        refused(plain, head, [0])                                # a decoder without caches
        assert [dec.slot_filled(b) for b in range(3)] == [PRE[0], PRE[1], None]
        assert dec.generate(head, [0, 1], _tokens_in(device)[:2].contiguous(), 0).shape == (0, 2)   # nothing to do
        assert [dec.slot_filled(b) for b in range(2)] == [PRE[0], PRE[1]]
    finally:
        head.close()
        one_row.close()
        dec.close()
        plain.close()
