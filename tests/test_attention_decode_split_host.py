"""Split-key decode attention without a GPU: the plan's kernel names, the default split_keys rule of
include/qgemm.h worked by hand, the workspace size, and the entry point's refusals -- all from the arguments alone, before
any launch (the pointers are dummies)."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
PTR = 8      # a dummy device pointer: never dereferenced, every call here ends before a launch


@pytest.mark.parametrize("dk,name", [(1, "attention_decode_split_kernel"), (64, "attention_decode_split_kernel"),
                                     (96, "attention_decode_split_wide_kernel"),
                                     (128, "attention_decode_split_wide_kernel")])
def test_plan_names_the_kernel_by_width(qg, dk, name):
    assert qg.attention_decode_split_plan(3, 2, 5000, 8, 2, dk, 256) == (256, name)


# (n_seqs, rows, max_seq_kv, n_heads, n_kv_heads) -> L.  W = n_seqs rows n_kv ceil(G / 4), want = ceil(512 / W),
# L = ceil(max_seq_kv / want) up to a multiple of 128, clamped to 128 .. 1024
DEFAULTS = [
    ((1, 1, 4096, 32, 8), 128),      # W 8, want 64, 64 keys -> 128
    ((1, 1, 131072, 32, 8), 1024),   # W 8, want 64, 2048 keys -> the upper clamp
    ((4, 1, 3000, 32, 8), 256),      # W 32, want 16, 188 keys -> 256
    ((8, 2, 5000, 14, 2), 640),      # G 7: two blocks; W 64, want 8, 625 keys -> 640
    ((3, 1, 9000, 8, 2), 128),       # W 6, want 86, 105 keys -> 128
    ((16, 1, 4096, 32, 8), 1024),    # W 128, want 4, 1024 keys
    ((64, 1, 4096, 64, 8), 1024),    # W 1024, want 1, 4096 keys -> the upper clamp
    ((2, 8, 700, 8, 8), 256),        # G 1; W 128, want 4, 175 keys -> 256
]


@pytest.mark.parametrize("args,want", DEFAULTS, ids=str)
def test_default_split_keys(qg, args, want):
    assert qg.attention_decode_split_plan(*args, 128)[0] == want
    assert qg.attention_decode_split_plan(*args, 128, split_keys=0)[0] == want
    assert qg.attention_decode_split_plan(*args, 128, split_keys=384)[0] == 384  # a given value comes back


@pytest.mark.parametrize("n_seqs,rows,max_kv,heads,dk,split", [(1, 1, 1, 1, 1, 128), (3, 8, 8200, 32, 128, 1024),
                                                               (64, 1, 131072, 8, 96, 128), (2, 3, 129, 6, 20, 128)])
def test_workspace_size(qg, n_seqs, rows, max_kv, heads, dk, split):
    assert qg.attention_decode_split_workspace_size(n_seqs, rows, max_kv, heads, dk, split) == \
        n_seqs * rows * heads * -(-max_kv // split) * (dk + 2) * 4


def test_workspace_size_for_the_default(qg):
    # no n_kv_heads here: the smallest L the rule gives for 32 heads (W = 8: L = 128), enough for every grouping
    assert qg.attention_decode_split_workspace_size(1, 1, 4096, 32, 128) == 32 * 32 * 130 * 4
    assert qg.attention_decode_split_workspace_size(1, 1, 4096, 32, 80) == 0      # outside the envelope
    assert qg.attention_decode_split_workspace_size(1, 1, 4096, 32, 128, 192) == 0


BASE = dict(Q=PTR, K=PTR, V=PTR, O=PTR, n_seqs=1, rows=1, seq_kv=(300,), heads=(8, 2), dk=64, split=128, ws=PTR,
            ws_bytes=8 * 3 * 66 * 4)
REFUSED = [
    ("L 64", dict(split=64)), ("L 191", dict(split=191)), ("L 1152", dict(split=1152)), ("L 2048", dict(split=2048)),
    ("131073 keys", dict(seq_kv=(131073,), ws_bytes=1 << 30)), ("9 rows", dict(rows=9, ws_bytes=1 << 30)),
    ("G 17", dict(heads=(34, 2), ws_bytes=1 << 30)), ("d_k 80", dict(dk=80, ws_bytes=1 << 30)),
    ("short workspace", dict(ws_bytes=8 * 3 * 66 * 4 - 1)), ("short workspace, default L", dict(split=0, ws_bytes=16)),
    ("null workspace", dict(ws=None)), ("null Q", dict(Q=None)), ("null K", dict(K=None)), ("null V", dict(V=None)),
    ("null O", dict(O=None)), ("null seq_kv", dict(seq_kv=None)),
]


def call(L, **over):
    a = dict(BASE, **over)
    kv = None if a["seq_kv"] is None else (ctypes.c_int * len(a["seq_kv"]))(*a["seq_kv"])
    return L.qgemm_attention_decode_split(a["Q"], 512, a["K"], 128, 1 << 20, a["V"], 128, 1 << 20, a["O"], 512,
                                          a["n_seqs"], a["rows"], None, kv, None, *a["heads"], a["dk"], 0.125, a["split"],
                                          a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("name,over", REFUSED, ids=[n for n, _ in REFUSED])
def test_entry_refuses_before_the_gpu(qg, name, over):
    L = qg.load()
    assert call(L, **over) == INVALID
    if "workspace" not in name and "keys" not in name:  # (an empty batch has no key count and needs no workspace)
        assert call(L, n_seqs=0, **over) == INVALID  # ... and is refused for every other reason


def test_empty_batch_and_default_split_are_accepted(qg):
    L = qg.load()
    for split in (0, 128, 640, 1024):
        assert call(L, n_seqs=0, split=split) == 0  # no sequence: nothing launched
    assert call(L, n_seqs=0, split=0, ws=None, ws_bytes=0) == 0
    assert qg.attention_decode_split_plan(1, 1, 131072, 8, 2, 64, 0)[0] == 512  # W 2, want 256
    with pytest.raises(qg.QGemmError):
        qg.attention_decode_split_plan(1, 1, 131073, 8, 2, 64)
