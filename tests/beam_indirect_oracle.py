"""A numpy restatement of the row table of the copy-free beam search (include/qgemm.h at
qgemm_decoder_beam_begin): own[s][j] is the slot whose slab holds, at row j, the K and V of position j of the sequence in
slot s.  begin, append and reindex change table bytes only; `effective` reads a place's rows through the table, which is
what the indirect decode attention sees.  255 marks an invalid entry; an entry that names no slab reads as NaN rows."""
import numpy as np

INVALID = 255


def identity(n_slots, max_seq):
    """The table a decoder is created with: own[s][j] = s."""
    return np.repeat(np.arange(n_slots, dtype=np.uint8)[:, None], max_seq, axis=1)


def begin(own, slots, src_slots, pos, beams):
    """Entries 0 .. pos[g] - 1 of every slot of group g name the group's prompt slot.  In place; returns own."""
    for g, src in enumerate(src_slots):
        for q in range(beams):
            own[slots[g * beams + q], :pos[g]] = src
    return own


def append(own, slots, pos, r=1):
    """A step of r rows at pos[b] on slot slots[b]: the slot's own slab holds them.  In place; returns own."""
    for b, s in enumerate(slots):
        own[s, pos[b]:pos[b] + r] = s
    return own


def reindex(own, slots, parents, n_rows, beams):
    """own[slots[g * beams + q]][j] = old own[slots[g * beams + parents[g * beams + q]]][j] for j < n_rows[g]; a parent
    outside [0, beams) gives 255.  In place (from a copy of the old rows); returns own."""
    old = own.copy()
    for g, n in enumerate(n_rows):
        for q in range(beams):
            p = int(parents[g * beams + q])
            dst = slots[g * beams + q]
            own[dst, :n] = old[slots[g * beams + p], :n] if 0 <= p < beams else INVALID
    return own


def effective(slabs, own_row, n):
    """Rows 0 .. n - 1 of a place: row j is row j of slab own_row[j], NaN where the entry names no slab.
    slabs: [n_slabs, rows, width], fp32 or their bits as int32 (then the quiet NaN's bits)."""
    nan = np.nan if np.issubdtype(slabs.dtype, np.floating) else 0x7fc00000
    out = np.full((n,) + slabs.shape[2:], nan, slabs.dtype)
    for j in range(n):
        if own_row[j] < slabs.shape[0]:
            out[j] = slabs[own_row[j], j]
    return out


def gather(slabs, own, tab_row, seq_kv):
    """Slabs for the plain batched call: slab b holds sequence b's effective rows (NaN past seq_kv[b])."""
    out = np.full((len(tab_row),) + slabs.shape[1:], np.nan, slabs.dtype)
    for b, (t, n) in enumerate(zip(tab_row, seq_kv)):
        out[b, :n] = effective(slabs, own[t], n)
    return out
