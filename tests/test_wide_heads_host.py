"""The wide decode envelope (d_k 96 and 128) without a GPU: what qgemm_attention_plan names, what the
batched and indirect decode launches accept and refuse before any launch, and the workspace rule that stays."""
import ctypes

import pytest

INVALID = 1  # hipErrorInvalidValue
WIDE = "attention_decode_wide_kernel"


@pytest.mark.parametrize("shape", [(1, 40, 1, 96), (8, 4096, 2, 128), (1, 513, 2, 128)], ids=str)
def test_plan_names_the_wide_kernel(qg, shape):
    assert qg.attention_plan(*shape) == WIDE


@pytest.mark.parametrize("shape", [(1, 40, 1, 65), (1, 40, 1, 112), (1, 40, 1, 160), (9, 40, 1, 128)], ids=str)
def test_plan_outside_the_wide_envelope(qg, shape):
    assert qg.attention_plan(*shape) != WIDE


@pytest.mark.parametrize("dk,want", [(96, 0), (128, 0), (65, INVALID), (112, INVALID), (160, INVALID)])
def test_batched_and_indirect_launches_with_no_sequence(qg, dk, want):
    """n_seqs = 0 launches nothing and reads no pointer: the return value is the envelope check's alone."""
    L = qg.load()
    none = (ctypes.c_int * 1)()
    assert L.qgemm_attention_decode_batched(8, dk, 8, dk, 8 * dk, 8, dk, 8 * dk, 8, dk, 0, 1, None, none, None, 1, dk,
                                            0.5, None) == want
    assert L.qgemm_attention_decode_indirect(8, dk, 8, dk, 8 * dk, 8, dk, 8 * dk, 8, dk, 0, 1, 8, 8, 1, None, none, None,
                                             1, dk, 0.5, None) == want


def test_workspace_size_is_left_alone(qg):
    assert qg.load().qgemm_attention_workspace_size(1, 513, 2, 128) == 4 * 2 * 1 * 513
