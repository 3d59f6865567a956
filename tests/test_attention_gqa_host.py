"""Grouped-query attention without a GPU: the plan names across the envelope's edges, G = 1 answering
what qgemm_attention_plan answers, the workspace rule and the refusals of the five new entry points."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
NARROW, WIDE, GROUPED = "attention_decode_gqa_kernel", "attention_decode_gqa_wide_kernel", "grouped_three_launches"


# (seq_q, seq_kv, heads, kv heads, d_k) -> plan
@pytest.mark.parametrize("shape,plan", [
    ((8, 4096, 8, 2, 64), NARROW), ((9, 4096, 8, 2, 64), GROUPED), ((0, 40, 4, 2, 8), NARROW),
    ((1, 512, 32, 8, 96), WIDE), ((8, 4096, 32, 8, 128), WIDE), ((1, 512, 32, 8, 100), GROUPED),
    ((9, 40, 32, 8, 128), GROUPED), ((1, 40, 4, 2, 65), GROUPED), ((1, 40, 4, 2, 129), GROUPED),
    ((1, 40, 32, 2, 64), NARROW), ((1, 40, 34, 2, 64), GROUPED), ((1, 40, 16, 1, 128), WIDE), ((1, 40, 17, 1, 128), GROUPED),
], ids=str)
def test_plan_names(qg, shape, plan):
    assert qg.attention_gqa_plan(*shape) == plan
    seq_q, seq_kv, H, n_kv, dk = shape
    need = qg.load().qgemm_attention_gqa_workspace_size(*shape)
    assert need == (4 * H * seq_q * seq_kv if plan == GROUPED else 0)   # the MHA-sized scores on the grouped path alone


@pytest.mark.parametrize("shape", [(1, 4096, 16, 64), (8, 513, 2, 128), (9, 512, 1, 64), (33, 4096, 2, 128), (1, 40, 1, 65)],
                         ids=str)
def test_one_head_per_group_is_the_mha_call(qg, shape):
    seq_q, seq_kv, H, dk = shape
    L = qg.load()
    assert qg.attention_gqa_plan(seq_q, seq_kv, H, H, dk) == qg.attention_plan(*shape)
    assert L.qgemm_attention_gqa_workspace_size(seq_q, seq_kv, H, H, dk) == L.qgemm_attention_workspace_size(*shape)


def test_refusals(qg):
    L = qg.load()
    name = ctypes.c_char_p()
    # (seq_q, seq_kv, heads, kv heads, d_k): the MHA entry's refusals, n_kv_heads < 1, n_heads % n_kv_heads != 0
    for bad in ((1, 4097, 4, 2, 8), (1, 0, 4, 2, 8), (-1, 4, 4, 2, 8), (1, 4, 0, 1, 8), (1, 4, 4, 2, 0), (1, 4, 4, 0, 8),
                (1, 4, 4, -1, 8), (1, 4, 4, 3, 8), (1, 4, 4, 8, 8)):
        assert L.qgemm_attention_gqa_plan(*bad, ctypes.byref(name)) == INVALID, bad
        assert L.qgemm_attention_gqa_workspace_size(*bad) == 0, bad
        assert L.qgemm_attention_gqa(8, 8, 8, 8, 8, 8, 8, 8, *bad, 0.5, 0, 0, 8, 1 << 30, None) == INVALID, bad
        with pytest.raises(qg.QGemmError):
            qg.attention_gqa_plan(*bad)
    assert L.qgemm_attention_gqa_plan(1, 4, 4, 2, 8, None) == 0   # the name is optional
    assert L.qgemm_attention_gqa(None, 8, 8, 8, 8, 8, 8, 8, 1, 4, 4, 2, 8, 0.5, 0, 0, None, 0, None) == INVALID
    assert L.qgemm_attention_gqa(8, 8, 8, 8, 8, 8, 8, 8, 1, 4, 4, 2, 8, 0.5, 1, -1, None, 0, None) == INVALID   # q_pos0
    assert L.qgemm_attention_gqa(8, 8, 8, 8, 8, 8, 8, 8, 9, 4, 4, 2, 8, 0.5, 0, 0, None, 0, None) == INVALID    # workspace
    # the two table launches: n_kv_heads < 1, a partial group, G > 16, then what the MHA launches refuse
    one = (ctypes.c_int * 1)(4)
    for H, n_kv, dk, rows in ((4, 0, 8, 1), (4, 3, 8, 1), (34, 2, 8, 1), (4, 2, 65, 1), (4, 2, 8, 9), (4, 2, 8, 0)):
        assert L.qgemm_attention_decode_batched_gqa(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, rows, None, one, None, H, n_kv, dk,
                                                    0.5, None) == INVALID, (H, n_kv, dk, rows)
        assert L.qgemm_attention_decode_indirect_gqa(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, rows, 8, 8, 1, None, one, None, H,
                                                     n_kv, dk, 0.5, None) == INVALID, (H, n_kv, dk, rows)
    assert L.qgemm_attention_decode_indirect_gqa(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, 1, None, 8, 1, None, one, None, 4, 2, 8,
                                                 0.5, None) == INVALID   # no table
    assert L.qgemm_attention_decode_indirect_gqa(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, 1, 8, 3, 1, None, one, None, 4, 2, 8,
                                                 0.5, None) == INVALID   # a table row shorter than the sequence
    assert L.qgemm_attention_decode_batched_gqa(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 0, 1, None, one, None, 4, 2, 8, 0.5,
                                                None) == 0   # no sequence: nothing launched
