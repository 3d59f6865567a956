"""Tiled online-softmax prefill attention without a GPU: the plan's kernel names across the envelope's
edges and the entry point's refusals -- all from the arguments alone, before any launch (the pointers are dummies)."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
PTR = 8      # a dummy device pointer: never dereferenced, every call here ends before a launch
NARROW, WIDE = "attention_tiled_kernel", "attention_tiled_wide_kernel"


# (seq_q, seq_kv, heads, KV heads, d_k) -> the kernel, or None: refused
PLANS = [
    ((5,), (7,), 4, 2, 1, NARROW), ((5,), (7,), 4, 2, 64, NARROW), ((5,), (7,), 4, 2, 65, None),
    ((5,), (7,), 4, 2, 96, WIDE), ((5,), (7,), 4, 2, 128, WIDE), ((5,), (7,), 4, 2, 129, None),
    ((5,), (7,), 4, 2, 0, None), ((5,), (7,), 4, 3, 64, None), ((5,), (7,), 4, 8, 64, None), ((5,), (7,), 4, 0, 64, None),
    ((5,), (7,), 0, 0, 64, None), ((5,), (7,), 4, 4, 64, NARROW), ((5,), (7,), 34, 2, 128, WIDE),   # G 1, G 17
    ((5, 0), (131072, 1), 4, 2, 64, NARROW), ((5, 0), (131073, 1), 4, 2, 64, None), ((5, 0), (7, 0), 4, 2, 64, None),
    ((5, -1), (7, 7), 4, 2, 64, None),
    ((), (), 4, 2, 96, WIDE), ((), (), 4, 2, 100, None), ((1,) * 64, (9,) * 64, 4, 2, 8, NARROW),
    ((1,) * 65, (9,) * 65, 4, 2, 8, None),
]


def _call(qg, seq_q, seq_kv, H, n_kv, dk, **over):
    """qgemm_attention_varlen_tiled on dummy pointers; over: Q / K / V / O, the arrays, q_pos0"""
    n = len(seq_q)
    ints = lambda v: (ctypes.c_int * max(1, n))(*v)          # noqa: E731
    longs = lambda v: (ctypes.c_int64 * max(1, n))(*v)       # noqa: E731
    a = dict(Q=PTR, K=PTR, V=PTR, O=PTR, q_row0=longs([0] * n), seq_q=ints(seq_q), kv_row0=longs([0] * n),
             seq_kv=ints(seq_kv), q_pos0=None)
    for k, v in over.items():  # null_<array>: that array as NULL
        if k.startswith("null_"):
            a[k[5:]] = None
        else:
            a[k] = v if v is None or k in "QKVO" else (ints(v) if k == "q_pos0" else longs(v))
    return qg.load().qgemm_attention_varlen_tiled(a["Q"], 512, a["K"], 128, a["V"], 128, a["O"], 512, n, a["q_row0"],
                                                  a["seq_q"], a["kv_row0"], a["seq_kv"], a["q_pos0"], H, n_kv, dk, 0.125,
                                                  None)


@pytest.mark.parametrize("seq_q,seq_kv,H,n_kv,dk,kernel", PLANS, ids=str)
def test_plan_over_the_envelope(qg, seq_q, seq_kv, H, n_kv, dk, kernel):
    if kernel is None:
        with pytest.raises(qg.QGemmError):
            qg.attention_varlen_tiled_plan(seq_q, seq_kv, H, n_kv, dk)
        assert _call(qg, seq_q, seq_kv, H, n_kv, dk) == INVALID  # the call refuses what the plan refuses
    else:
        assert qg.attention_varlen_tiled_plan(seq_q, seq_kv, H, n_kv, dk) == kernel


@pytest.mark.parametrize("over", [dict(Q=None), dict(K=None), dict(V=None), dict(O=None), dict(q_row0=None),
                                  dict(kv_row0=None), dict(null_seq_q=1), dict(null_seq_kv=1), dict(q_row0=[0, -1]),
                                  dict(kv_row0=[-1, 0]), dict(q_pos0=[0, -1])], ids=str)
def test_entry_refuses_before_the_gpu(qg, over):
    assert _call(qg, (4, 5), (6, 7), 4, 2, 64, **over) == INVALID


def test_empty_calls_launch_nothing(qg):
    assert _call(qg, (), (), 4, 2, 64) == 0                 # no sequence
    assert _call(qg, (0, 0), (6, 131072), 4, 1, 128) == 0   # no query row: no work item, returns before the launch
    one = (ctypes.c_int * 1)(9)
    assert qg.load().qgemm_attention_varlen_tiled_plan(1, one, one, 4, 2, 8, None) == 0  # the name is optional
