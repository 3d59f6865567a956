"""Grouped-query prefill over packed sequences without a GPU: qgemm_attention_varlen_gqa_plan and
_workspace_size across the fused kernel's edges, G = 1 answering what the multi-head varlen entries answer, and the
refusals of the three new entry points."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
NARROW, WIDE, PER_SEQ = "attention_fused_gqa_kernel<many>", "attention_fused_gqa_wide_kernel<many>", "per_sequence"


def _ints(v):
    return (ctypes.c_int * max(1, len(v)))(*v)


def _ws(qg, seq_q, seq_kv, H, n_kv, dk):
    return qg.load().qgemm_attention_varlen_gqa_workspace_size(len(seq_q), _ints(seq_q), _ints(seq_kv), H, n_kv, dk)


# (seq_q, seq_kv, heads, kv heads, d_k) -> plan
@pytest.mark.parametrize("seq_q,seq_kv,H,n_kv,dk,plan", [
    ((33, 1, 40), (512, 512, 1), 8, 2, 64, NARROW), ((33, 1, 40), (512, 513, 1), 8, 2, 64, PER_SEQ),
    ((33, 9), (512, 7), 8, 2, 128, WIDE), ((33, 9), (513, 7), 8, 2, 128, PER_SEQ),
    ((40, 9), (40, 7), 4, 2, 65, PER_SEQ), ((40, 9), (40, 7), 4, 2, 96, WIDE), ((40, 9), (40, 7), 4, 2, 100, PER_SEQ),
    ((40, 9), (40, 7), 4, 2, 129, PER_SEQ), ((40, 2), (40, 7), 4, 2, 1, NARROW),
    ((40,), (40,), 14, 2, 64, NARROW), ((40,), (40,), 32, 1, 128, WIDE), ((1,), (4096,), 64, 2, 64, PER_SEQ),
    ((), (), 8, 2, 128, WIDE), ((), (), 8, 2, 100, PER_SEQ), ((0, 0), (40, 512), 8, 2, 64, NARROW),
    ((0, 0), (40, 513), 8, 2, 64, PER_SEQ),
], ids=str)
def test_plan_names_and_workspace(qg, seq_q, seq_kv, H, n_kv, dk, plan):
    """0 on the fused plans; per sequence the largest qgemm_attention_gqa_workspace_size over the sequences with rows"""
    assert qg.attention_varlen_gqa_plan(seq_q, seq_kv, H, n_kv, dk) == plan
    single = [qg.load().qgemm_attention_gqa_workspace_size(q, kv, H, n_kv, dk) for q, kv in zip(seq_q, seq_kv) if q]
    assert _ws(qg, seq_q, seq_kv, H, n_kv, dk) == (max(single, default=0) if plan == PER_SEQ else 0)
    if plan == PER_SEQ and any(q > 8 for q in seq_q):
        assert _ws(qg, seq_q, seq_kv, H, n_kv, dk) > 0    # a prefill-sized sequence brings the grouped path's scores


@pytest.mark.parametrize("seq_q,seq_kv,H,dk", [((33, 1), (512, 7), 4, 64), ((33, 9), (512, 513), 4, 64),
                                               ((33, 1), (40, 7), 2, 128), ((), (), 2, 24)], ids=str)
def test_one_head_per_group_is_the_mha_call(qg, seq_q, seq_kv, H, dk):
    assert qg.attention_varlen_gqa_plan(seq_q, seq_kv, H, H, dk) == qg.attention_varlen_plan(seq_q, seq_kv, H, dk)
    assert _ws(qg, seq_q, seq_kv, H, H, dk) == qg.load().qgemm_attention_varlen_workspace_size(
        len(seq_q), _ints(seq_q), _ints(seq_kv), H, dk)


def _call(qg, seq_q, seq_kv, H, n_kv, dk, q_row0=None, kv_row0=None, q_pos0=None):
    """qgemm_attention_varlen_gqa on dummy non-null pointers with a workspace that is large enough"""
    n = len(seq_q)
    longs = lambda v: (ctypes.c_int64 * max(1, n))(*(v or [0] * n))   # noqa: E731
    return qg.load().qgemm_attention_varlen_gqa(8, 8, 8, 8, 8, 8, 8, 8, n, longs(q_row0), _ints(seq_q), longs(kv_row0),
                                                _ints(seq_kv), None if q_pos0 is None else _ints(q_pos0), H, n_kv, dk,
                                                0.5, 8, 1 << 40, None)


@pytest.mark.parametrize("seq_q,seq_kv,H,n_kv,dk", [
    ((4, 5), (6, 7), 4, 3, 8), ((4, 5), (6, 7), 4, 8, 8), ((4, 5), (6, 7), 4, 0, 8),   # no whole number of groups
    ((4,) * 65, (6,) * 65, 4, 2, 8),
    ((4, 5), (6, 0), 4, 2, 8), ((4, 5), (4097, 7), 4, 2, 8), ((4, -1), (6, 7), 4, 2, 8),
    ((4, 5), (6, 7), 0, 0, 8), ((4, 5), (6, 7), 4, 2, 0),
], ids=str)
def test_refusals(qg, seq_q, seq_kv, H, n_kv, dk):
    """hipErrorInvalidValue from the plan and from the call, before any launch; 0 from the size query"""
    name = ctypes.c_char_p()
    n = len(seq_q)
    assert qg.load().qgemm_attention_varlen_gqa_plan(n, _ints(seq_q), _ints(seq_kv), H, n_kv, dk,
                                                     ctypes.byref(name)) == INVALID
    assert _ws(qg, seq_q, seq_kv, H, n_kv, dk) == 0
    assert _call(qg, seq_q, seq_kv, H, n_kv, dk) == INVALID
    with pytest.raises(qg.QGemmError):
        qg.attention_varlen_gqa_plan(seq_q, seq_kv, H, n_kv, dk)


def test_offsets_nulls_and_the_workspace(qg):
    L = qg.load()
    for dk in (8, 100):   # the fused route and the per-sequence one
        assert _call(qg, (4, 5), (6, 7), 4, 2, dk, q_row0=[0, -1]) == INVALID
        assert _call(qg, (4, 5), (6, 7), 4, 2, dk, kv_row0=[-1, 0]) == INVALID
        assert _call(qg, (4, 5), (6, 7), 4, 2, dk, q_pos0=[0, -1]) == INVALID
    assert _call(qg, (), (), 4, 2, 8) == 0    # no sequence: nothing launched
    one, zero = _ints([9]), (ctypes.c_int64 * 1)(0)
    assert L.qgemm_attention_varlen_gqa_plan(1, one, one, 4, 2, 8, None) == 0   # the name is optional
    assert L.qgemm_attention_varlen_gqa_plan(1, None, one, 4, 2, 8, None) == INVALID
    assert L.qgemm_attention_varlen_gqa_workspace_size(1, one, None, 4, 2, 8) == 0
    assert L.qgemm_attention_varlen_gqa(None, 8, 8, 8, 8, 8, 8, 8, 1, zero, one, zero, one, None, 4, 2, 8, 0.5, None, 0,
                                        None) == INVALID
    # 9 rows at d_k 100 take the grouped three launches: refused without their scores, and one byte short of them
    need = L.qgemm_attention_varlen_gqa_workspace_size(1, one, one, 4, 2, 100)
    assert need == 4 * 4 * 9 * 9
    for ws, size in ((None, 0), (8, need - 1)):
        assert L.qgemm_attention_varlen_gqa(8, 8, 8, 8, 8, 8, 8, 8, 1, zero, one, zero, one, None, 4, 2, 100, 0.5, ws,
                                            size, None) == INVALID
