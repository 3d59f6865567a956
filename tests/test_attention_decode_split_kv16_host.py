"""Split-key decode attention over a bf16 cache without a GPU: the plan names its two kernels and returns
the fp32 plan's split_keys, and the entry point refuses from the arguments alone, before any launch (the pointers are
dummies)."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
PTR = 8      # a dummy device pointer: never dereferenced, every call here ends before a launch


@pytest.mark.parametrize("dk,name", [(1, "attention_decode_split_kv16_kernel"), (64, "attention_decode_split_kv16_kernel"),
                                     (96, "attention_decode_split_kv16_wide_kernel"),
                                     (128, "attention_decode_split_kv16_wide_kernel")])
def test_plan_names_the_kernel_by_width(qg, dk, name):
    assert qg.attention_decode_split_kv16_plan(3, 2, 5000, 8, 2, dk, 256) == (256, name)


@pytest.mark.parametrize("args", [(1, 1, 4096, 32, 8), (1, 1, 131072, 32, 8), (8, 2, 5000, 14, 2), (3, 1, 9000, 8, 2),
                                  (64, 1, 4096, 64, 8), (2, 8, 700, 8, 8)], ids=str)
@pytest.mark.parametrize("asked", [None, 0, 384])
def test_plan_returns_the_fp32_plans_split_keys(qg, args, asked):
    assert qg.attention_decode_split_kv16_plan(*args, 128, asked)[0] == qg.attention_decode_split_plan(*args, 128, asked)[0]


BASE = dict(K=PTR, n_seqs=1, seq_kv=(300,), heads=(8, 2), dk=64, split=128, ws=PTR, ws_bytes=8 * 3 * 66 * 4)
REFUSED = [
    ("L 192", dict(split=192)), ("L 2048", dict(split=2048)), ("131073 keys", dict(seq_kv=(131073,), ws_bytes=1 << 30)),
    ("d_k 80", dict(dk=80, ws_bytes=1 << 30)), ("G 17", dict(heads=(34, 2), ws_bytes=1 << 30)),
    ("short workspace", dict(ws_bytes=8 * 3 * 66 * 4 - 1)), ("short workspace, default L", dict(split=0, ws_bytes=16)),
    ("null workspace", dict(ws=None)), ("null K", dict(K=None)),
]


def call(L, **over):
    a = dict(BASE, **over)
    kv = (ctypes.c_int * len(a["seq_kv"]))(*a["seq_kv"])
    return L.qgemm_attention_decode_split_kv16(PTR, 512, a["K"], 128, 1 << 20, PTR, 128, 1 << 20, PTR, 512, a["n_seqs"], 1,
                                               None, kv, None, *a["heads"], a["dk"], 0.125, a["split"], a["ws"],
                                               a["ws_bytes"], None)


@pytest.mark.parametrize("name,over", REFUSED, ids=[n for n, _ in REFUSED])
def test_entry_refuses_before_the_gpu(qg, name, over):
    assert call(qg.load(), **over) == INVALID


def test_empty_batch_is_accepted_and_the_plan_refuses_with_the_call(qg):
    assert call(qg.load(), n_seqs=0) == 0  # no sequence: nothing launched
    for bad in ((1, 1, 131073, 8, 2, 64), (1, 1, 300, 8, 2, 80), (1, 1, 300, 34, 2, 64), (1, 9, 300, 8, 2, 64)):
        with pytest.raises(qg.QGemmError):
            qg.attention_decode_split_kv16_plan(*bad)
    with pytest.raises(qg.QGemmError):
        qg.attention_decode_split_kv16_plan(1, 1, 300, 8, 2, 64, 192)
