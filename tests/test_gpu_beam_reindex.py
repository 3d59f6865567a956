"""GPU parity of the row-table kernels of the copy-free beam search (beam.hip) against
tests/beam_indirect_oracle.py: qgemm_beam_reindex on any table, in place, and the decoder's beam_begin / beam_reindex /
beam_table.  The tables are filled with seeded bytes, so a byte moved from the wrong row or column shows, and every byte
the contract does not name must keep its value."""
import ctypes

import numpy as np
import pytest
import torch

import beam_indirect_oracle as BI
import test_gpu_generate as G

pytestmark = pytest.mark.gpu
INVALID = 1
N_ROWS = (0, 1, 15, 16, 17, 64)      # one group each: nothing, one byte, around the 16-column piece, the whole row


def _parents(beams, groups, seed, bad=()):
    par = np.random.default_rng(seed).integers(0, beams, groups * beams).astype(np.int32)
    if beams > 1:
        par[beams:2 * beams] = par[beams]                      # a group whose places all repeat one parent
    for at, v in bad:
        par[at] = v
    return par


@pytest.mark.parametrize("view", ["aligned", "offset"])
@pytest.mark.parametrize("beams", [1, 3, 8])
def test_reindex_in_place(qg, device, beams, view):
    """Six groups with 0, 1, 15, 16, 17 and 64 columns, their rows scattered over a 64-row table; repeated parents and two
    out-of-range ones (255 entries); the aligned table takes the 16-byte accesses, the view 1 byte past a 16-byte
    boundary with an odd row stride the byte ones.  Run twice on the same table: two steps of the model."""
    groups, width = len(N_ROWS), 64
    rows = groups * beams
    slots = [int(v) for v in np.random.default_rng(beams).permutation(64)[:rows]]
    host = np.random.default_rng(800 + beams).integers(0, 256, (64, width)).astype(np.uint8)
    if view == "aligned":
        table = torch.from_numpy(host.copy()).to(device)
        assert table.data_ptr() % 16 == 0 and table.stride(0) % 16 == 0
    else:
        wide = torch.full((65, 81), 99, dtype=torch.uint8, device=device)
        wide[:64, 1:65] = torch.from_numpy(host).to(device)
        table = wide[:64, 1:65]
        assert table.data_ptr() % 16 == 1 and table.stride(0) % 2 == 1
    want = host.copy()
    for step in range(2):
        bad = ((rows - 1, beams), (rows - beams, -1)) if step == 0 else ()     # in the 64-column group
        par = _parents(beams, groups, 810 + step, bad)
        assert qg.beam_reindex(table, slots, torch.from_numpy(par).to(device), N_ROWS, beams) is table
        before = want.copy()
        BI.reindex(want, slots, par, N_ROWS, beams)
        got = table.cpu().numpy()
        assert np.array_equal(got, want), f"step {step}: {np.argwhere(got != want)[:5].tolist()}"
        if step == 0:
            assert (want[slots[rows - 1]] == 255).all() and (want[slots[rows - beams]] == 255).all()
            if beams > 1:
                assert (want != before).any(), "the reorder moved nothing"
    untouched = [r for r in range(64) if r not in slots]
    assert np.array_equal(table.cpu().numpy()[untouched], host[untouched]), "rows of other slots were written"
    if view == "offset":
        w = wide.cpu().numpy()
        w[:64, 1:65] = 99
        assert (w == 99).all(), "bytes outside the view were written"


def test_reindex_refusals(qg, device):
    L = qg.load()
    table = torch.full((64, 32), 7, dtype=torch.uint8, device=device)
    par = torch.zeros(64, dtype=torch.int32, device=device)
    ints = lambda v: (ctypes.c_int * len(v))(*v)

    def call(t=table.data_ptr(), stride=32, groups=2, beams=2, slots=(0, 1, 2, 3), p=par.data_ptr(), n_rows=(32, 5)):
        return L.qgemm_beam_reindex(t, stride, groups, beams, None if slots is None else ints(list(slots)), p,
                                    None if n_rows is None else ints(list(n_rows)), None)

    for kw in (dict(t=None), dict(p=None), dict(slots=None), dict(n_rows=None), dict(stride=0), dict(groups=0),
               dict(beams=0), dict(beams=9, slots=tuple(range(18))), dict(groups=9, beams=8, slots=tuple(range(72)),
                                                                           n_rows=(1,) * 9),
               dict(slots=(0, 1, 2, 64)), dict(slots=(0, 1, 2, -1)), dict(slots=(0, 1, 2, 0)), dict(n_rows=(33, 5)),
               dict(n_rows=(32, -1))):
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert (table.cpu().numpy() == 7).all(), "a refused call wrote the table"
    assert call() == 0


# ---- the decoder's table ----------------------------------------------------------------------------------------------
PROMPT = (G.MAX_SEQ, 17, 0)          # prompt rows of the three groups: a full slab, past a 16-column piece, none
SRC = (24, 25, 26)          # the prompts' slots; slot 27 is never begun
N_SLOTS = 28


def _decoder(qg, device, n_slots=N_SLOTS):
    dec = G._decoder(qg, n_slots)
    for g, n in enumerate(PROMPT):
        dec.begin_slot(SRC[g], G._dev(G.O.uniform((9, G.D), 830 + g), device))
        if n:
            dec.step_slot(SRC[g], G._dev(G.O.uniform((n, G.D), 840 + g), device))
    return dec


@pytest.mark.parametrize("beams", [1, 3, 8])
def test_decoder_begin_reindex_and_table(qg, oracle, device, beams):
    """beam_table() is the identity at creation; beam_begin writes the prompts' slots into the first pos[g] entries of
    the groups' rows and nothing else; beam_reindex (n_rows = the whole prompts, then 15 / 16 / 0 columns) equals the
    model; the host state follows (enc_seq, filled, the plain calls refuse the slots, begin_slot frees them)."""
    dec = _decoder(qg, device)
    try:
        rows = 3 * beams
        slots = [int(v) for v in np.random.default_rng(beams).permutation(24)[:rows]]
        want = BI.identity(N_SLOTS, G.MAX_SEQ)
        assert np.array_equal(dec.beam_table().cpu().numpy(), want), "the table starts as the identity"
        dec.beam_begin(slots, SRC, None, beams)
        BI.begin(want, slots, SRC, PROMPT, beams)
        assert np.array_equal(dec.beam_table().cpu().numpy(), want), "beam_begin"
        assert [dec.slot_filled(s) for s in slots] == [PROMPT[i // beams] for i in range(rows)]
        for n_rows, seed, bad in ((list(PROMPT), 850, ((1, beams),) if beams > 1 else ()), ([15, 16, 0], 851, ())):
            par = _parents(beams, 3, seed, bad)
            dec.beam_reindex(slots, torch.from_numpy(par).to(device), n_rows, beams)
            BI.reindex(want, slots, par, n_rows, beams)
            got = dec.beam_table().cpu().numpy()
            assert np.array_equal(got, want), f"beam_reindex {n_rows}: {np.argwhere(got != want)[:5].tolist()}"
            assert [dec.slot_filled(s) for s in slots] == [n_rows[i // beams] for i in range(rows)]
            if bad:
                assert (want[slots[1], :PROMPT[0]] == 255).all(), "the out-of-range parent's entries"
        # the slots are flagged: the plain calls refuse them before any launch, begin_slot frees a slot
        x = torch.zeros((1, G.D), device=device)
        for bad_call in (lambda: dec.step_slot(slots[0], x, pos=0), lambda: dec.step_batch([slots[0]], x, pos=[0]),
                         lambda: dec.step_varlen([slots[0]], x, [1], pos=[0]), lambda: dec.copy_slot(27, slots[0])):
            with pytest.raises(qg.QGemmError) as e:
                bad_call()
            assert e.value.code == INVALID
        dec.begin_slot(slots[0], G._dev(G.O.uniform((9, G.D), 860), device))
        dec.step_slot(slots[0], x)
        assert dec.slot_filled(slots[0]) == 1
    finally:
        dec.close()


def test_decoder_table_refusals(qg, oracle, device):
    dec, single = _decoder(qg, device), G._decoder(qg, 1)
    try:
        L = qg.load()
        ints = lambda v: (ctypes.c_int * len(v))(*v)
        par = torch.zeros(8, dtype=torch.int32, device=device)
        begin = lambda slots, src, pos, beams=2, d=dec: L.qgemm_decoder_beam_begin(
            d._h, len(src), beams, ints(slots), ints(src), ints(pos), None)
        state = lambda: [dec.slot_filled(s) for s in range(N_SLOTS)]
        a, b, c = SRC
        before, table = state(), dec.beam_table().cpu().numpy()
        assert begin([0, 1], [a], [0], d=single) == INVALID                # one slot: no table
        assert begin([0, 1], [27], [0]) == INVALID                         # a prompt slot not begun
        assert begin([0, 1], [N_SLOTS], [0]) == INVALID and begin([0, N_SLOTS], [a], [0]) == INVALID
        assert begin([0, 1], [b], [18]) == INVALID                         # pos above the prompt's filled length
        assert begin([0, 1], [b], [-1]) == INVALID
        assert begin([0, 0], [b], [3]) == INVALID                          # a slot named twice
        assert begin([0, b], [b], [3]) == INVALID                          # the prompt slot at a place other than 0
        assert begin([0, 1, b, 2], [b, c], [3, 0]) == INVALID              # another group's prompt slot
        assert begin([b, 1, 2, 3], [b, b], [3, 3]) == INVALID              # a prompt that is a place and shared
        assert begin(list(range(9)), [b], [3], beams=9) == INVALID
        assert state() == before and np.array_equal(dec.beam_table().cpu().numpy(), table)
        assert begin([b, 1], [b], [17]) == 0                               # place 0 may be the prompt slot itself
        assert begin([b, 1], [b], [17]) == 0                               # ... and the same begin may come again:
        assert begin([b, 1], [b], [18]) == INVALID                         # the slot keeps 17 prompt rows, no more
        assert begin([b, 1], [b], [17]) == 0
        reindex = lambda slots, n_rows, beams=2, p=par.data_ptr(): L.qgemm_decoder_beam_reindex(
            dec._h, len(n_rows), beams, ints(slots), p, ints(n_rows), None)
        before, table = state(), dec.beam_table().cpu().numpy()
        assert reindex([b, 1], [18]) == INVALID                            # above the filled length
        assert reindex([b, 1], [-1]) == INVALID
        assert reindex([b, 2], [1]) == INVALID                             # slot 2 was not begun by beam_begin
        assert reindex([b, b], [1]) == INVALID and reindex([b, 1], [1], p=None) == INVALID
        assert L.qgemm_decoder_read_beam_table(dec._h, None, None) == INVALID
        assert L.qgemm_decoder_read_beam_table(single._h, par.data_ptr(), None) == INVALID
        assert state() == before and np.array_equal(dec.beam_table().cpu().numpy(), table)
        assert reindex([b, 1], [17]) == 0
    finally:
        dec.close()
        single.close()
