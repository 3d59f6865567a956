"""Tiled prefill attention over a bf16 K / V cache without a GPU: the plan names its two kernels and the
entry point refuses from the arguments alone, before any launch (the pointers are dummies)."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
PTR = 8      # a dummy device pointer: never dereferenced, every call here ends before a launch


@pytest.mark.parametrize("dk,name", [(1, "attention_tiled_kv16_kernel"), (64, "attention_tiled_kv16_kernel"),
                                     (96, "attention_tiled_kv16_wide_kernel"), (128, "attention_tiled_kv16_wide_kernel")])
def test_plan_names_the_kernel_by_width(qg, dk, name):
    assert qg.attention_varlen_tiled_kv16_plan((5, 0), (131072, 1), 4, 2, dk) == name


BASE = dict(K=PTR, seq_q=(4, 5), seq_kv=(6, 7), q_row0=(0, 4), kv_row0=(0, 6), heads=(4, 2), dk=64, q_pos0=None)
REFUSED = [
    ("d_k 65", dict(dk=65)), ("seq_kv 0", dict(seq_kv=(6, 0))), ("131073 keys", dict(seq_kv=(131073, 7))),
    ("KV heads 3 of 4", dict(heads=(4, 3))), ("65 sequences", dict(seq_q=(1,) * 65, seq_kv=(9,) * 65, q_row0=(0,) * 65,
                                                                  kv_row0=(0,) * 65)),
    ("negative kv_row0", dict(kv_row0=(0, -1))), ("negative q_pos0", dict(q_pos0=(0, -1))),
    ("null seq_kv", dict(seq_kv=None)), ("null K", dict(K=None)),
]


def call(L, **over):
    a = dict(BASE, **over)
    n = len(a["seq_q"])
    ints = lambda v: None if v is None else (ctypes.c_int * max(1, n))(*v)        # noqa: E731
    longs = lambda v: None if v is None else (ctypes.c_int64 * max(1, n))(*v)     # noqa: E731
    return L.qgemm_attention_varlen_tiled_kv16(PTR, 512, a["K"], 128, PTR, 128, PTR, 512, n, longs(a["q_row0"]),
                                               ints(a["seq_q"]), longs(a["kv_row0"]), ints(a["seq_kv"]),
                                               ints(a["q_pos0"]), *a["heads"], a["dk"], 0.125, None)


@pytest.mark.parametrize("name,over", REFUSED, ids=[n for n, _ in REFUSED])
def test_entry_refuses_before_the_gpu(qg, name, over):
    assert call(qg.load(), **over) == INVALID


def test_no_sequence_returns_zero(qg):
    assert call(qg.load(), seq_q=(), seq_kv=(), q_row0=(), kv_row0=()) == 0
