"""The row table of the copy-free beam search without a GPU: tests/beam_indirect_oracle.py's begin /
append / reindex against a numpy model that COPIES whole caches by the parents, which is gather_slots' semantics.  After
every step the rows every place sees through the table must be, bit for bit, the rows the copy model holds for it -- so
reading through the table is the copy, and an invalid parent poisons the same rows on both paths.  The argument checks
of the new entry points that need no GPU are exercised too."""
import ctypes

import numpy as np
import pytest

import beam_indirect_oracle as BI
from util import assert_bits_equal

MAX_SEQ, WIDTH, GROUPS, STEPS = 24, 3, 3, 12
START = (0, 5, 2)          # the groups' prompt lengths, one of them empty


def _parents(beams, steps, seed):
    """steps x (GROUPS * beams) parents: the identity, all from one parent and a permutation first, then seeded ones."""
    rng = np.random.default_rng(seed)
    rows = []
    for t in range(steps):
        if t == 0:
            par = np.tile(np.arange(beams), GROUPS)
        elif t == 1:
            par = np.repeat(rng.integers(0, beams, GROUPS), beams)
        elif t == 2:
            par = np.concatenate([rng.permutation(beams) for _ in range(GROUPS)])
        else:
            par = rng.integers(0, beams, GROUPS * beams)
        rows.append(par.astype(np.int32))
    return rows


def _run(beams, parents_of_step, own_src):
    """Both models over the steps; own_src: group g's first slot is its prompt slot.  Yields per step (place, n,
    effective rows, copy-model rows)."""
    rows = GROUPS * beams
    slots = [int(v) for v in np.random.default_rng(beams).permutation(rows + GROUPS)[:rows]]   # scattered over the table
    free = [s for s in range(rows + GROUPS) if s not in slots]
    src = [slots[g * beams] if own_src else free[g] for g in range(GROUPS)]
    n_slots = rows + GROUPS
    rng = np.random.default_rng(100 + beams)
    slabs = np.full((n_slots, MAX_SEQ, WIDTH), np.nan, np.float32)
    prompt = [rng.standard_normal((START[g], WIDTH)).astype(np.float32) for g in range(GROUPS)]
    for g in range(GROUPS):
        slabs[src[g], :START[g]] = prompt[g]
    own = BI.begin(BI.identity(n_slots, MAX_SEQ), slots, src, START, beams)
    copies = [np.full((MAX_SEQ, WIDTH), np.nan, np.float32) for _ in range(rows)]      # the copy model: a cache per place
    for i in range(rows):
        copies[i][:START[i // beams]] = prompt[i // beams]
    for t, par in enumerate(parents_of_step):
        pos = [START[i // beams] + t for i in range(rows)]
        new = rng.standard_normal((rows, WIDTH)).astype(np.float32)
        for i in range(rows):                                   # the step: every place writes its own new row
            slabs[slots[i], pos[i]] = new[i]
            copies[i][pos[i]] = new[i]
        BI.append(own, slots, pos)
        n_rows = [START[g] + t + 1 for g in range(GROUPS)]
        BI.reindex(own, slots, par, n_rows, beams)
        old = [c.copy() for c in copies]
        for i in range(rows):                                   # gather_slots: whole rows 0 .. n - 1 from the parent
            g, p, n = i // beams, int(par[i]), n_rows[i // beams]
            copies[i][:n] = old[g * beams + p][:n] if 0 <= p < beams else np.nan
        for i in range(rows):
            yield t, i, n_rows[i // beams], BI.effective(slabs, own[slots[i]], n_rows[i // beams]), copies[i], own, slots


@pytest.mark.parametrize("own_src", [False, True], ids=["separate_prompt_slots", "first_slot_is_the_prompt"])
@pytest.mark.parametrize("beams", [1, 3, 8])
def test_table_reads_what_the_copy_holds(beams, own_src):
    moved = False
    for t, i, n, eff, copy, own, slots in _run(beams, _parents(beams, STEPS, 7 * beams), own_src):
        assert_bits_equal(eff, copy[:n], f"beams {beams} step {t} place {i}")
        assert not np.isnan(eff).any()
        moved = moved or bool((own[slots[i], :n] != slots[i]).any())
    assert moved or beams == 1 and own_src, "the table never pointed away from a place's own slab"


@pytest.mark.parametrize("beams", [3, 8])
def test_invalid_parent_poisons_the_same_rows(beams):
    par = _parents(beams, 6, 11)
    par[3][beams + 1] = beams          # one past the range
    par[4][2 * beams] = -1
    seen_nan = 0
    for t, i, n, eff, copy, own, slots in _run(beams, par, False):
        assert_bits_equal(eff, copy[:n], f"beams {beams} step {t} place {i}")
        if t == 3 and i == beams + 1:
            assert (own[slots[i], :n] == BI.INVALID).all() and np.isnan(eff).all()
            assert (own[slots[i], n:] == slots[i]).all(), "entries at or past n_rows are not written"
            seen_nan += 1
        if t == 4 and i == 2 * beams:
            assert (own[slots[i], :n] == BI.INVALID).all() and np.isnan(eff).all()
            seen_nan += 1
    assert seen_nan == 2


def test_gather_builds_the_batched_calls_slabs():
    slabs = np.arange(3 * 4 * 2, dtype=np.float32).reshape(3, 4, 2)
    own = np.array([[0, 1, 2, 255], [2, 2, 3, 0]], np.uint8)
    got = BI.gather(slabs, own, [1, 0, 1], [2, 4, 3])
    assert_bits_equal(got[0, :2], np.stack([slabs[2, 0], slabs[2, 1]]), "two rows of table row 1")
    assert np.isnan(got[0, 2:]).all()
    assert_bits_equal(got[1, :3], np.stack([slabs[0, 0], slabs[1, 1], slabs[2, 2]]), "table row 0")
    assert np.isnan(got[1, 3]).all(), "255 names no slab"
    assert np.isnan(got[2, 2]).all(), "an entry equal to the number of slabs names none either"


def test_new_entry_points_refuse_without_a_gpu(qg):
    """Every check comes before the first launch, so the refusals need no device: null pointers and counts out of range."""
    L = qg.load()
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    bad = qg.HIP_ERROR_INVALID_VALUE
    for name in ("qgemm_attention_decode_indirect", "qgemm_beam_reindex", "qgemm_decoder_beam_begin",
                 "qgemm_decoder_step_batch_indirect", "qgemm_decoder_beam_reindex", "qgemm_decoder_read_beam_table",
                 "qgemm_decoder_generate_beam_indirect"):
        assert name in qg.EXPORTED_SYMBOLS and hasattr(L, name)
    p = 4096                                                                    # a non-null stand-in, never dereferenced
    assert L.qgemm_beam_reindex(None, 16, 1, 2, ints([0, 1]), p, ints([4]), None) == bad
    assert L.qgemm_beam_reindex(p, 16, 1, 2, ints([0, 1]), None, ints([4]), None) == bad
    assert L.qgemm_beam_reindex(p, 16, 0, 2, ints([0, 1]), p, ints([4]), None) == bad        # no group
    assert L.qgemm_beam_reindex(p, 16, 1, 9, ints(list(range(9))), p, ints([4]), None) == bad   # beams > 8
    assert L.qgemm_beam_reindex(p, 16, 9, 8, ints(list(range(72))), p, ints([4] * 9), None) == bad   # 72 places
    assert L.qgemm_beam_reindex(p, 16, 1, 2, ints([0, 0]), p, ints([4]), None) == bad        # a row named twice
    assert L.qgemm_beam_reindex(p, 16, 1, 2, ints([0, 64]), p, ints([4]), None) == bad       # past the 64 rows
    assert L.qgemm_beam_reindex(p, 16, 1, 2, ints([0, -1]), p, ints([4]), None) == bad
    assert L.qgemm_beam_reindex(p, 16, 1, 2, ints([0, 1]), p, ints([17]), None) == bad       # n_rows > the stride
    assert L.qgemm_beam_reindex(p, 16, 1, 2, ints([0, 1]), p, ints([-1]), None) == bad
    assert L.qgemm_beam_reindex(p, 16, 1, 2, ints([0, 1]), p, ints([0]), None) == 0          # nothing to move: no launch

    def attn(table=p, n_slabs=2, stride=8, tab_row=(0,), seq_kv=(8,), n_seqs=1, r=1, dk=8):
        return L.qgemm_attention_decode_indirect(p, 16, p, 16, 128, p, 16, 128, p, 16, n_seqs, r, table, stride, n_slabs,
                                                 ints(list(tab_row)), ints(list(seq_kv)), ints([0] * len(seq_kv)), 2, dk,
                                                 1.0, None)
    assert attn(table=None) == bad
    assert attn(n_slabs=0) == bad and attn(n_slabs=65) == bad
    assert attn(stride=7) == bad                                                # a stride below seq_kv
    assert attn(tab_row=(-1,)) == bad
    assert attn(seq_kv=(0,)) == bad and attn(seq_kv=(4097,), stride=4097) == bad
    assert attn(r=9) == bad and attn(dk=65) == bad and attn(n_seqs=65) == bad
    assert attn(n_seqs=0) == 0                                                  # no sequence: no launch
    for fn, args in ((L.qgemm_decoder_beam_begin, (None, 1, 1, ints([0]), ints([0]), ints([0]), None)),
                     (L.qgemm_decoder_step_batch_indirect, (None, 1, ints([0]), ints([0]), ints([0]), 1, p, p, None)),
                     (L.qgemm_decoder_beam_reindex, (None, 1, 1, ints([0]), p, ints([0]), None)),
                     (L.qgemm_decoder_read_beam_table, (None, p, None)),
                     (L.qgemm_decoder_generate_beam_indirect,
                      (None, None, 1, 1, ints([0]), ints([0]), p, 1, None, None, -1, p, p, p, None))):
        assert fn(*args) == bad
