"""GPU test of Decoder.gather_slots (qgemm_decoder_gather_slots): a pure copy, so every cache float is compared with a
snapshot taken before the call (Decoder.read_slot).  d_model 64 runs the 16-byte path, d_model 6 the dword path; two
blocks; two groups of three beams with their own row counts; a bystander slot that nobody names."""
import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

BEAMS, MAX_SEQ, ENC = 3, 12, (5, 7)                 # group g's slots have enc_seq ENC[g]
SRC, DST, BYSTANDER = [0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11], 12
FILLED = [9, 7, 8, 12, 12, 12]                      # of the source slots
QUIET_NAN = 0x7FC00000
INVALID = 1


def _decoder(qg, d):
    return qg.Decoder(d, 2, 2 * d, 2, max_seq=MAX_SEQ, max_enc_seq=8, seed=3, causal=True, kv_cache=True, n_slots=13)


def _fill(dec, d, device):
    """Every slot begun and stepped to its own length with its own rows, so that no two slabs hold the same floats."""
    for slot in range(13):
        g = 0 if slot in (0, 1, 2, 6, 7, 8, 12) else 1
        dec.begin_slot(slot, torch.from_numpy(O.uniform((ENC[g], d), 40 + slot)).to(device))
        n = FILLED[slot] if slot < 6 else MAX_SEQ
        dec.step_slot(slot, torch.from_numpy(O.uniform((n, d), 60 + slot)).to(device))


def _snapshot(dec):
    torch.cuda.synchronize()
    return {(b, s): tuple(t.cpu().numpy().view(np.uint32) for t in dec.read_slot(b, s)) for b in range(2)
            for s in range(13)}


def _check(dec, d, before, parents, n_rows):
    after = _snapshot(dec)
    for b in range(2):
        for s in SRC + [BYSTANDER]:
            assert np.array_equal(after[b, s][0], before[b, s][0]), f"block {b} slot {s}: sources and bystanders stay"
        for s in range(13):
            assert np.array_equal(after[b, s][1], before[b, s][1]), f"block {b} slot {s}: the cross caches stay"
        for i, s in enumerate(DST):
            g, n, par = i // BEAMS, n_rows[i // BEAMS], parents[i]
            got, old = after[b, s][0], before[b, s][0]
            assert np.array_equal(got[:, :d], old[:, :d]), f"block {b} slot {s}: the Q third stays"
            assert np.array_equal(got[n:], old[n:]), f"block {b} slot {s}: rows at and past n_rows stay"
            if 0 <= par < BEAMS:
                want = before[b, SRC[g * BEAMS + par]][0][:n, d:]
            else:
                want = np.full((n, 2 * d), QUIET_NAN, np.uint32)
            assert np.array_equal(got[:n, d:], want), f"block {b} slot {s}: [K | V] of parent {par}"


@pytest.mark.parametrize("d", [64, 6])
def test_gather(qg, oracle, device, d):
    dec = _decoder(qg, d)
    try:
        _fill(dec, d, device)
        cases = [([2, 0, 1, 1, 2, 0], [7, 12]),          # a permutation; n_rows = the smallest filled / max_seq
                 ([1, 1, 1, 0, 0, 0], [1, 5]),           # all equal
                 ([0, 1, 2, 0, 1, 2], [0, 12]),          # the identity; nothing to copy in group 0
                 ([0, -1, 3, 2, 1 << 30, 1], [7, 3]),    # out of range on both sides: rows of NaNs, the others right
                 ([0, 0, 0, 0, 0, 0], [0, 0])]           # nothing at all
        for parents, n_rows in cases:
            before = _snapshot(dec)
            dec.gather_slots(DST, SRC, torch.tensor(parents, dtype=torch.int32, device=device), n_rows, BEAMS)
            _check(dec, d, before, parents, n_rows)
            assert [dec.slot_filled(s) for s in DST] == [n_rows[0]] * 3 + [n_rows[1]] * 3
            assert [dec.slot_filled(s) for s in SRC] == FILLED and dec.slot_filled(BYSTANDER) == MAX_SEQ
    finally:
        dec.close()


def test_refusals(qg, oracle, device):
    d = 8
    dec = qg.Decoder(d, 2, 16, 2, max_seq=MAX_SEQ, max_enc_seq=8, seed=3, causal=True, kv_cache=True, n_slots=8)
    plain = qg.Decoder(d, 2, 16, 2, max_seq=MAX_SEQ, max_enc_seq=8, seed=3, causal=True, kv_cache=False)
    try:
        for slot, enc, n in ((0, 5, 6), (1, 5, 4), (2, 5, 0), (3, 5, 0), (4, 7, 6), (5, 7, 0)):   # 6 and 7: not begun
            dec.begin_slot(slot, torch.from_numpy(O.uniform((enc, d), 40 + slot)).to(device))
            if n:
                dec.step_slot(slot, torch.from_numpy(O.uniform((n, d), 60 + slot)).to(device))
        state = [dec.slot_filled(s) for s in range(8)]
        before = None
        par = torch.zeros(2, dtype=torch.int32, device=device)

        def refused(dst, src, n_rows, beams=2, decoder=dec, parents=par):
            with pytest.raises(qg.QGemmError) as e:
                decoder.gather_slots(dst, src, parents, n_rows, beams)
            assert e.value.code == INVALID

        dec.gather_slots([2, 3], [0, 1], par, [4], 2)                 # fine: the rest are variations of it
        assert dec.slot_filled(2) == dec.slot_filled(3) == 4
        state = [dec.slot_filled(s) for s in range(8)]
        torch.cuda.synchronize()
        before = {s: dec.read_slot(0, s)[0].cpu().numpy().view(np.uint32) for s in range(8)}
        refused([2, 3], [0, 1], [4], decoder=plain)                   # a decoder without slots
        refused([2, 8], [0, 1], [4])                                  # a slot out of range
        refused([2, 3], [0, -1], [4])
        refused([2, 6], [0, 1], [4])                                  # a slot not begun
        refused([2, 3], [0, 7], [4])
        refused([2, 2], [0, 1], [4])                                  # a destination named twice
        refused([2, 1], [0, 1], [4])                                  # a slot in both lists
        refused([2, 3], [0, 1], [5])                                  # n_rows above the filled of source 1
        refused([2, 3], [0, 0], [MAX_SEQ + 1])                        # n_rows above max_seq
        refused([2, 3], [0, 1], [-1])
        refused([2, 3], [0, 4], [4])                                  # enc_seq differs within the group
        refused([2, 5], [0, 1], [4])
        with pytest.raises(AssertionError):
            dec.gather_slots([2, 3, 5], [0, 1, 4], torch.zeros(3, dtype=torch.int32, device=device), [4, 4], 2)
        L = qg.load()
        ints = lambda v: (L.qgemm_decoder_gather_slots.argtypes[3]._type_ * len(v))(*v)
        assert L.qgemm_decoder_gather_slots(dec._h, 0, 2, ints([2, 3]), ints([0, 1]), par.data_ptr(), ints([4]),
                                            None) == INVALID          # n_groups out of range
        for beams in (0, 9):                                          # beams out of range
            assert L.qgemm_decoder_gather_slots(dec._h, 1, beams, ints([2, 3]), ints([0, 1]), par.data_ptr(), ints([4]),
                                                None) == INVALID
        assert L.qgemm_decoder_gather_slots(dec._h, 1, 2, ints([2, 3]), ints([0, 1]), None, ints([4]), None) == INVALID
        assert [dec.slot_filled(s) for s in range(8)] == state, "a refused call moves no filled length"
        torch.cuda.synchronize()
        for s in range(8):
            assert np.array_equal(dec.read_slot(0, s)[0].cpu().numpy().view(np.uint32), before[s]), "and launches nothing"
    finally:
        dec.close()
        plain.close()
