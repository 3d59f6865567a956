"""The bf16 K / V cache without a GPU: the five symbols in the header, the library, the symbol list and
the ctypes prototypes, the plan names across the envelope and the plan's refusals."""
import ctypes
import os

import pytest

INVALID = 1  # hipErrorInvalidValue
NARROW, WIDE = "attention_decode_kv16_kernel", "attention_decode_kv16_wide_kernel"
SYMBOLS = ("qgemm_attention_decode_batched_kv16", "qgemm_attention_decode_indirect_kv16",
           "qgemm_attention_decode_kv16_plan", "qgemm_kv_append_bf16")


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_declared_exported_listed_prototyped(qg, symbol):
    header = open(os.path.join(os.path.dirname(qg.PKG_DIR), "include", "qgemm.h")).read()
    assert f"QGEMM_API int {symbol}(" in header
    assert symbol in qg.EXPORTED_SYMBOLS
    fn = getattr(qg.load(), symbol)   # AttributeError: not exported
    assert fn.argtypes and fn.restype is ctypes.c_int


# (rows per sequence, heads, kv heads, d_k) -> plan
@pytest.mark.parametrize("shape,plan", [
    ((1, 1, 1, 1), NARROW), ((8, 32, 32, 64), NARROW), ((1, 32, 2, 64), NARROW), ((4, 6, 2, 20), NARROW),
    ((1, 32, 8, 96), WIDE), ((8, 32, 8, 128), WIDE), ((1, 16, 1, 128), WIDE), ((1, 32, 32, 128), WIDE),
], ids=str)
def test_plan_names(qg, shape, plan):
    assert qg.attention_decode_kv16_plan(*shape) == plan


@pytest.mark.parametrize("bad", [(1, 4, 2, 65), (1, 4, 2, 80), (1, 4, 2, 160), (1, 17, 1, 64), (0, 4, 2, 64), (9, 4, 2, 64),
                                 (1, 4, 3, 64), (1, 4, 0, 64), (1, 0, 1, 64), (1, 4, 2, 0)], ids=str)
def test_plan_refusals(qg, bad):
    assert qg.load().qgemm_attention_decode_kv16_plan(*bad, None) == INVALID
    with pytest.raises(qg.QGemmError):
        qg.attention_decode_kv16_plan(*bad)


def test_launches_refuse_before_the_gpu(qg):
    """Outside the envelope there is no other path: hipErrorInvalidValue, from arguments alone."""
    L = qg.load()
    one = (ctypes.c_int * 1)(4)
    for H, n_kv, dk, rows in ((4, 0, 8, 1), (4, 3, 8, 1), (34, 2, 8, 1), (4, 2, 65, 1), (4, 2, 8, 9), (4, 2, 8, 0)):
        assert L.qgemm_attention_decode_batched_kv16(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, rows, None, one, None, H, n_kv, dk,
                                                     0.5, None) == INVALID, (H, n_kv, dk, rows)
        assert L.qgemm_attention_decode_indirect_kv16(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, rows, 8, 8, 1, None, one, None, H,
                                                      n_kv, dk, 0.5, None) == INVALID, (H, n_kv, dk, rows)
    far = (ctypes.c_int * 1)(4097)
    assert L.qgemm_attention_decode_batched_kv16(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, 1, None, far, None, 4, 2, 8, 0.5,
                                                 None) == INVALID
    assert L.qgemm_attention_decode_batched_kv16(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 0, 1, None, one, None, 4, 2, 8, 0.5,
                                                 None) == 0   # no sequence: nothing launched
    neg = (ctypes.c_int * 1)(-1)
    # (n_seqs, rows_per_seq, kv_slot, pos, width)
    for bad in ((0, 1, None, one, 8), (65, 1, None, one, 8), (1, 0, None, one, 8), (1, 1, None, one, 0), (1, 1, None, neg, 8),
                (1, 1, neg, one, 8), (1, 1, None, None, 8)):
        assert L.qgemm_kv_append_bf16(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, *bad, None) == INVALID, bad
