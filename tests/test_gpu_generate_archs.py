"""The four generation loops -- generate, generate_sampled, generate_beam and generate_beam_indirect -- on every stack
architecture of tests/stack_cases.py (post-LN with GELU, pre-LN with the final norm, RoPE, each with cross-attention or
decoder-only, and the decoder-only reference block), held to the whole-search oracles with the entry's own chain as
their `forward`: tokens and parents as integers, scores by bits, every output buffer pre-filled with a sentinel.  After
every search one more fixed row goes to every surviving place and must be, bit for bit, the chain's row on the place's
final input rows plus that row: the caches hold what the search fed, and on a RoPE entry K rotated by the ORIGINAL
positions through every gather and re-index.  A RoPE entry's chain runs on the tables read back from the model.
tests/test_generate_archs_host.py shows on the CPU that the cases are sensitive to a wrong rotation, that the beams
reorder and that the end tokens are held."""
import ctypes

import numpy as np
import pytest
import torch

import stack_cases as C
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

INVALID = 1
D, N_NEW, BEAMS, GROUPS, ROWS = C.D, C.N_NEW, C.BEAMS, C.GROUPS, C.ROWS


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _ints(shape, device):
    return torch.full(shape, -7, dtype=torch.int32, device=device)


def _make(qg, name, device, n_slots):
    """the entry's model with every tensor of its weight set loaded, and its tables (None without RoPE)"""
    m = qg.Decoder(C.D, C.H, C.DFF, C.BLOCKS, C.MAX_SEQ, C.max_enc_seq(name), seed=C.MODEL_SEED, causal=True,
                   kv_cache=True, n_slots=n_slots, **C.decoder_keywords(name))
    W = C.weights(not C.MODELS[name].only)
    for block, kind in C.loaded_kinds(name):
        m.set_weight(block, kind, _dev(W[block, kind], device))
    tables = tuple(t.cpu().numpy() for t in m.rope_tables()) if C.MODELS[name].rope else None
    return m, tables


def _head(qg, device):
    E, P, W, bias = C.head_tables()
    return qg.Head(qg.pack_b(_dev(W, device)), C.VOCAB, _dev(bias, device), _dev(E, device), _dev(P, device), max_rows=8)


def _enc(name, b, device):
    e = C.enc_rows(name, b)
    return None if e is None else _dev(e, device)


def _begin(dec, slot, enc, rows, device):
    dec.begin_slot(slot, enc)
    if len(rows):
        dec.step_slot(slot, _dev(rows, device))


def _prefill(dec, name, device, pre=C.PRE):
    for b, n in enumerate(pre):
        _begin(dec, b, _enc(name, b, device), C.prefix(name, b, n), device)


def _tin(name, device, n=3):
    return torch.tensor(C.tokens_in(name, n), dtype=torch.int32, device=device)


def _same(got, want, what):
    tok, par, sc = got   # numpy, read back
    assert np.array_equal(tok, want[0]), f"{what}: tokens\n{tok}\n{want[0]}"
    assert np.array_equal(par, want[1]), f"{what}: parents\n{par}\n{want[1]}"
    assert_bits_equal(sc, want[2], f"{what}: scores")


# ---- generate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_generate(qg, oracle, device, name):
    dec, tables = _make(qg, name, device, 3)
    head = _head(qg, device)
    try:
        _prefill(dec, name, device)
        out = _ints((N_NEW, 3), device)
        dec.generate(head, [0, 1, 2], _tin(name, device), N_NEW, tokens_out=out)
        got = out.cpu().numpy()
        assert [dec.slot_filled(b) for b in range(3)] == [p + N_NEW for p in C.PRE]
        probe = torch.cat([_dev(C.probe_row(b), device) for b in range(3)])
        after = dec.step_batch([0, 1, 2], probe, Y=_nan((3, D), device)).cpu().numpy()
    finally:
        head.close()
        dec.close()
    want = C.expected_generate(name, tables)
    assert np.array_equal(got, want), f"{name}: generate against generate_ref\n{got}\n{want}"
    fwd = C.forward(name, tables)
    for b in range(3):   # the caches hold the rows of exactly the tokens fed, at their positions
        whole = np.concatenate([C.prefix(name, b), C.fed_rows(name, b, want), C.probe_row(b)])
        assert_bits_equal(after[b:b + 1], fwd(whole, C.enc_rows(name, b))[-1:], f"{name}: slot {b} after generate")


@pytest.mark.parametrize("name", C.NAMES)
def test_generate_sampled(qg, oracle, device, name):
    dec, tables = _make(qg, name, device, 3)
    head = _head(qg, device)
    free = C.expected_sampled(name, tables)
    eos = C.end_token(free)
    try:
        _prefill(dec, name, device)
        got = []
        for e in (None, eos):   # the second call rewinds every slot to its prefix
            out = _ints((N_NEW, 3), device)
            dec.generate_sampled(head, [0, 1, 2], _tin(name, device), N_NEW, C.TOP_K, C.TOP_P, C.TEMPERATURE,
                                 seed=C.SAMPLE_SEED, streams=list(C.STREAMS), eos=e, pos=list(C.PRE), tokens_out=out)
            got.append(out.cpu().numpy())
            assert [dec.slot_filled(b) for b in range(3)] == [p + N_NEW for p in C.PRE]
    finally:
        head.close()
        dec.close()
    assert np.array_equal(got[0], free), f"{name}: generate_sampled against generate_sampled_ref\n{got[0]}\n{free}"
    held = C.expected_sampled(name, tables, eos)
    assert np.array_equal(got[1], held), f"{name}: with the end token {eos}\n{got[1]}\n{held}"


# ---- the beam searches --------------------------------------------------------------------------------------------------
def _beam_outputs(device):
    return _ints((N_NEW, ROWS), device), _ints((N_NEW, ROWS), device), _nan((N_NEW, ROWS), device)


def _beam_tin(name, device):
    return torch.tensor(C.beam_tokens_in(name), dtype=torch.int32, device=device)


def _probes(device):
    return torch.cat([_dev(C.probe_row(r), device) for r in range(ROWS)])


def _check_places(name, tables, want, after, what):
    """every surviving place's row after the search: the chain on the place's final input rows plus the probe row"""
    fwd = C.forward(name, tables)
    seen = 0
    for r in range(ROWS):
        if want[3][r] is None:
            continue
        whole = np.concatenate([want[3][r], C.probe_row(r)])
        assert_bits_equal(after[r:r + 1], fwd(whole, C.enc_rows(name, r // BEAMS))[-1:], f"{what}: place {r} after the search")
        seen += 1
    assert seen >= GROUPS


@pytest.mark.parametrize("name", C.NAMES)
def test_generate_beam_copy_path(qg, oracle, device, name):
    A, B = list(range(ROWS)), list(range(ROWS, 2 * ROWS))
    dec, tables = _make(qg, name, device, 2 * ROWS)
    head = _head(qg, device)
    eos = C.end_token(C.expected_beam(name, tables)[0])
    try:
        got, after = [], []
        for e in (-1, eos):
            for g in range(GROUPS):   # the group's prompt into its first slot of A, forked into its slots of both sets
                first = A[g * BEAMS]
                _begin(dec, first, _enc(name, g, device), C.beam_prefix(name, g), device)
                dec.beam_fork(first, A[g * BEAMS:(g + 1) * BEAMS], B[g * BEAMS:(g + 1) * BEAMS])
            out = dec.generate_beam(head, A, B, _beam_tin(name, device), N_NEW, BEAMS, eos=e, out=_beam_outputs(device))
            got.append(tuple(t.cpu().numpy() for t in out))
            assert [dec.slot_filled(s) for s in A + B] == [C.BEAM_PRE[s % ROWS // BEAMS] + N_NEW for s in range(2 * ROWS)]
            # N_NEW is even: the beams' caches are in A
            after.append(dec.step_batch(A, _probes(device), Y=_nan((ROWS, D), device)).cpu().numpy())
    finally:
        head.close()
        dec.close()
    for e, g, a in zip((-1, eos), got, after):
        want = C.expected_beam(name, tables, e)
        _same(g, want, f"{name}: generate_beam, eos {e}")
        _check_places(name, tables, want, a, f"{name}: generate_beam, eos {e}")


@pytest.mark.parametrize("name", C.NAMES)
def test_generate_beam_indirect(qg, oracle, device, name):
    slots, src = list(range(ROWS)), [ROWS, ROWS + 1]
    cross = [src[r // BEAMS] for r in range(ROWS)]
    dec, tables = _make(qg, name, device, ROWS + GROUPS)
    head = _head(qg, device)
    eos = C.end_token(C.expected_beam(name, tables)[0])
    try:
        for g in range(GROUPS):
            _begin(dec, src[g], _enc(name, g, device), C.beam_prefix(name, g), device)
        got, after = [], []
        for e in (-1, eos):
            dec.beam_begin(slots, src, None, BEAMS)   # (again: the table goes back to the search's start)
            out = dec.generate_beam_indirect(head, slots, src, _beam_tin(name, device), N_NEW, BEAMS, eos=e,
                                             out=_beam_outputs(device))
            got.append(tuple(t.cpu().numpy() for t in out))
            assert [dec.slot_filled(s) for s in slots] == [C.BEAM_PRE[r // BEAMS] + N_NEW for r in range(ROWS)]
            assert [dec.slot_filled(s) for s in src] == list(C.BEAM_PRE), "a prompt slot moved"
            after.append(dec.step_batch_indirect(slots, cross, _probes(device), Y=_nan((ROWS, D), device)).cpu().numpy())
    finally:
        head.close()
        dec.close()
    for e, g, a in zip((-1, eos), got, after):
        want = C.expected_beam(name, tables, e)
        _same(g, want, f"{name}: generate_beam_indirect, eos {e}")
        _check_places(name, tables, want, a, f"{name}: generate_beam_indirect, eos {e}")


# ---- the tables' end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.ROPE_NAMES)
def test_generate_up_to_the_tables_last_row(qg, oracle, device, name):
    """Prefixes of 12 and 11 rows, four new tokens: slot 0's last token is fed at position max_seq - 1 and reads the
    tables' last row.  One more token is refused with hipErrorInvalidValue (pos + n_new > max_seq) before any launch."""
    n = len(C.END_PRE)
    dec, tables = _make(qg, name, device, n)
    head = _head(qg, device)
    try:
        _prefill(dec, name, device, C.END_PRE)

        def refused():
            before = [dec.slot_filled(b) for b in range(n)]
            out = _ints((C.END_N_NEW + 1, n), device)
            with pytest.raises(qg.QGemmError) as e:
                dec.generate(head, list(range(n)), _tin(name, device, n), C.END_N_NEW + 1, pos=list(C.END_PRE), tokens_out=out)
            assert e.value.code == INVALID
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == -7).all(), "a refused call launched"
            assert [dec.slot_filled(b) for b in range(n)] == before, "a refused call moved a filled length"

        refused()
        out = _ints((C.END_N_NEW, n), device)
        dec.generate(head, list(range(n)), _tin(name, device, n), C.END_N_NEW, tokens_out=out)
        got = out.cpu().numpy()
        assert [dec.slot_filled(b) for b in range(n)] == [p + C.END_N_NEW for p in C.END_PRE] == [C.MAX_SEQ, C.MAX_SEQ - 1]
        refused()
        last = dec.step_slot(1, _dev(C.probe_row(1), device), Y=_nan((1, D), device)).cpu().numpy()   # position max_seq - 1
    finally:
        head.close()
        dec.close()
    want = C.expected_generate_end(name, tables)
    assert np.array_equal(got, want), f"{name}: generate at the tables' end\n{got}\n{want}"
    whole = np.concatenate([C.prefix(name, 1, C.END_PRE[1]), C.fed_rows(name, 1, want, C.END_PRE), C.probe_row(1)])
    assert whole.shape[0] == C.MAX_SEQ
    assert_bits_equal(last, C.forward(name, tables)(whole, C.enc_rows(name, 1))[-1:], f"{name}: slot 1's row at the last position")


# ---- one capture --------------------------------------------------------------------------------------------------------
def test_captured_generate_replays_on_a_rope_model(qg, oracle, device):
    name = "only-pre-rope"
    L = qg.load()
    ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    dec, tables = _make(qg, name, device, 3)
    head = _head(qg, device)
    try:
        tin = _tin(name, device)
        out = _ints((N_NEW, 3), device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):
            _prefill(dec, name, device)
            eager = dec.generate(head, [0, 1, 2], tin, N_NEW, pos=list(C.PRE)).cpu().numpy()   # also the warm-up
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = L.qgemm_decoder_generate(dec._h, head._h, 3, ints([0, 1, 2]), tin.data_ptr(), N_NEW,
                                              ints(list(C.PRE)), out.data_ptr(), s.cuda_stream)
                assert rc == 0
            for i in range(2):
                _prefill(dec, name, device)   # the slots as they were before the search
                out.fill_(-7)
                s.synchronize()
                g.replay()
                s.synchronize()
                assert np.array_equal(out.cpu().numpy(), eager), f"replay {i}"
                assert [dec.slot_filled(b) for b in range(3)] == list(C.PRE), "a replay moves no host-side length"
    finally:
        head.close()
        dec.close()
    assert np.array_equal(eager, C.expected_generate(name, tables)), "the eager call against generate_ref"


# ---- the admission guards -----------------------------------------------------------------------------------------------
def test_decoder_only_loops_refuse_unbegun_and_indirect_slots(qg, oracle, device):
    """A decoder-only slot has enc_seq 0 begun or not: the loops admit by the slot's begun flag.  Slots 0 (2 rows) and 1
    (no row) are begun, 2 and 3 never, 4 and 5 belong to a copy-free search.  Every refusal is hipErrorInvalidValue
    before any launch: the sentinel outputs stay, no filled length moves."""
    name = "only-post"
    dec, _ = _make(qg, name, device, 6)
    head = _head(qg, device)
    try:
        _begin(dec, 0, None, C.prefix(name, 2), device)
        dec.begin_slot(1)
        dec.beam_begin([4, 5], [0], None, 2)
        state = lambda: [dec.slot_filled(s) for s in range(6)]  # noqa: E731
        before = state()
        assert before == [2, 0, None, None, 2, 2]

        def tok(n):
            return torch.tensor([3, 11][:n], dtype=torch.int32, device=device)

        def refused(call, rows):
            outs = (_ints((2, rows), device), _ints((2, rows), device), torch.full((2, rows), 1.0, device=device))
            with pytest.raises(qg.QGemmError) as e:
                call(outs)
            assert e.value.code == INVALID
            torch.cuda.synchronize()
            assert all((o.cpu().numpy() == v).all() for o, v in zip(outs, (-7, -7, 1.0))), "a refused call launched"
            assert state() == before

        for bad in (2, 4):   # never begun; begun by beam_begin
            refused(lambda o: dec.generate(head, [0, bad], tok(2), 2, tokens_out=o[0]), 2)
            refused(lambda o: dec.generate_sampled(head, [0, bad], tok(2), 2, 4, tokens_out=o[0]), 2)
            refused(lambda o: dec.generate_beam(head, [1], [bad], tok(1), 2, 1, out=o), 1)
            refused(lambda o: dec.generate_beam(head, [bad], [1], tok(1), 2, 1, out=o), 1)
        refused(lambda o: dec.generate_beam_indirect(head, [4, 5], [3], tok(1), 2, 2, out=o), 2)    # the prompt slot
        refused(lambda o: dec.generate_beam_indirect(head, [4, 2], [0], tok(1), 2, 2, out=o), 2)    # a beam slot
        refused(lambda o: dec.generate_beam_indirect(head, [4, 1], [0], tok(1), 2, 2, out=o), 2)    # begun, but plainly
        # what the guards admit: a begun slot without a row, and the search's own slots
        assert dec.generate(head, [0, 1], tok(2), 2).shape == (2, 2)
        assert dec.generate_beam_indirect(head, [4, 5], [0], tok(1), 2, 2)[0].shape == (2, 2)
        assert state() == [4, 2, None, None, 4, 4]
    finally:
        head.close()
        dec.close()
