"""The six decode launches over a table of sequences without a GPU: every entry point refuses the same
bad argument sets with hipErrorInvalidValue, from the arguments alone and before any launch (the pointers are dummies),
and an empty batch is a success that launches nothing.  One table of bad sets serves all six; the return codes are the
ones the launches had before their checks and table fill became decode_table_from_host / decode_table_ok."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
PTR = 8      # a dummy device pointer: never dereferenced, every call here ends before a launch

# what every entry point takes; `heads` is (n_heads,) for the multi-head launches, (n_heads, n_kv_heads) for the others
BASE = dict(Q=PTR, K=PTR, V=PTR, O=PTR, n_seqs=1, rows=1, slot=None, seq_kv=(4,), q_pos0=None, dk=8,
            row_slab=PTR, stride=8, n_slabs=1)

# (name, overrides): each set is bad in ONE way
BAD = [
    ("null Q", dict(Q=None)), ("null K", dict(K=None)), ("null V", dict(V=None)), ("null O", dict(O=None)),
    ("null seq_kv", dict(seq_kv=None)),
    ("n_seqs -1", dict(n_seqs=-1)), ("n_seqs 65", dict(n_seqs=65, seq_kv=(4,) * 65)),
    ("rows 0", dict(rows=0)), ("rows 9", dict(rows=9)),
    ("d_k 0", dict(dk=0)), ("d_k 65", dict(dk=65)), ("d_k 80", dict(dk=80)), ("d_k 160", dict(dk=160)),
    ("seq_kv 0", dict(seq_kv=(0,))), ("seq_kv 4097", dict(seq_kv=(4097,), stride=8192)),
    ("second seq_kv 0", dict(n_seqs=2, seq_kv=(4, 0))),
    ("q_pos0 -1", dict(q_pos0=(-1,))), ("slot -1", dict(slot=(-1,))),
]
BAD_INDIRECT = [
    ("null table", dict(row_slab=None)), ("n_slabs 0", dict(n_slabs=0)), ("n_slabs 65", dict(n_slabs=65)),
    ("stride < seq_kv", dict(stride=3)), ("stride -1", dict(stride=-1)),
]
BAD_GROUPS = [("n_kv_heads 0", (4, 0)), ("not a divisor", (4, 3)), ("G 17", (34, 2)), ("n_heads 0", (0, 2))]

# entry point -> (indirect, the head counts it is tried with)
ENTRIES = {
    "qgemm_attention_decode_batched": (False, [(4,)]),
    "qgemm_attention_decode_indirect": (True, [(4,)]),
    "qgemm_attention_decode_batched_gqa": (False, [(4, 2), (4, 4)]),     # G = 1: the multi-head launch's checks
    "qgemm_attention_decode_indirect_gqa": (True, [(4, 2), (4, 4)]),
    "qgemm_attention_decode_batched_kv16": (False, [(4, 2), (4, 4)]),    # G = 1: the same kernel
    "qgemm_attention_decode_indirect_kv16": (True, [(4, 2), (4, 4)]),
}


def ints(v):
    return None if v is None else (ctypes.c_int * len(v))(*v)


def call(L, entry, heads, **over):
    a = dict(BASE, **over)
    indirect = ENTRIES[entry][0]
    args = [a["Q"], 8, a["K"], 8, 64, a["V"], 8, 64, a["O"], 8, a["n_seqs"], a["rows"]]
    if indirect:
        args += [a["row_slab"], a["stride"], a["n_slabs"]]
    args += [ints(a["slot"]), ints(a["seq_kv"]), ints(a["q_pos0"]), *heads, a["dk"], 0.5, None]
    return getattr(L, entry)(*args)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_table_launches_refuse_before_the_gpu(qg, entry):
    L = qg.load()
    indirect, head_sets = ENTRIES[entry]
    for heads in head_sets:
        for name, over in BAD + (BAD_INDIRECT if indirect else []):
            assert call(L, entry, heads, **over) == INVALID, (name, heads)
        # the bad sets stay refused under a mask and with explicit slots
        for name, over in (("seq_kv 0", dict(seq_kv=(0,))), ("rows 9", dict(rows=9))):
            assert call(L, entry, heads, q_pos0=(0,), slot=(0,), **over) == INVALID, (name, heads, "masked")
        assert call(L, entry, heads, n_seqs=0) == 0, heads   # no sequence: nothing launched
        assert call(L, entry, heads, n_seqs=0, dk=65) == INVALID, heads   # ... after the checks
    if len(head_sets[0]) == 2:
        for name, heads in BAD_GROUPS:
            assert call(L, entry, heads) == INVALID, name
            assert call(L, entry, heads, n_seqs=0) == INVALID, (name, "empty batch")
    else:
        assert call(L, entry, (0,)) == INVALID, "n_heads 0"
