"""The output end of the model without a GPU: the properties of the argmax oracle itself, the launch plan query of
qgemm_argmax_rows (qgemm_argmax_rows_plan needs no device) and the exported symbols."""
import ctypes

import numpy as np
import pytest

import head_oracle

NAN, INF = float("nan"), float("inf")


def _idx(row):
    idx, val = head_oracle.argmax_rows_ref(np.array([row], np.float32))
    return int(idx[0]), val[0]


def test_oracle_ties_take_the_lowest_index():
    assert _idx([1, 5, 5, 2, 5])[0] == 1
    assert _idx([7, 7])[0] == 0
    assert _idx([-INF, -INF, -INF])[0] == 0
    assert _idx([3])[0] == 0


def test_oracle_signed_zeros_are_equal():
    i, v = _idx([-1, -0.0, 0.0])
    assert i == 1 and np.signbit(v)          # -0 came first and +0 is not greater
    i, v = _idx([0.0, -0.0])
    assert i == 0 and not np.signbit(v)


def test_oracle_nan_rules():
    assert _idx([1, NAN, 0.5])[0] == 0        # a NaN past column 0 never wins
    assert _idx([1, NAN, 2, NAN])[0] == 2
    assert _idx([-INF, NAN])[0] == 0
    i, v = _idx([NAN, 9, INF])                # a NaN at column 0 is never beaten
    assert i == 0 and np.isnan(v)


def test_oracle_embed_rows():
    E = np.arange(12, dtype=np.float32).reshape(4, 3)
    P = np.full((5, 3), 0.5, np.float32)
    Y = head_oracle.embed_rows_ref(E, [3, 0, 4, -1], P, [1, 3], rows_per_seq=2)
    assert np.array_equal(Y[0], E[3] + 0.5) and np.array_equal(Y[1], E[0] + 0.5)
    assert (Y[2:].view(np.uint32) == head_oracle.QUIET_NAN).all()


def _plan(L, rows, w):
    parts = ctypes.c_int(-1)
    rc = L.qgemm_argmax_rows_plan(rows, w, ctypes.byref(parts))
    return rc, parts.value


def test_argmax_rows_plan(qg):
    L = qg.load()
    assert _plan(L, 64, 1000) == (0, 1)              # a narrow row: one workgroup per row
    assert _plan(L, 4096, 131072) == (0, 1)          # many rows fill the GPU by themselves
    rc, one_wide = _plan(L, 1, 131072)
    assert rc == 0 and one_wide > 1                  # one wide row is split
    assert _plan(L, 2, 70001)[1] > 1 and qg.argmax_rows_plan(2, 70001) == _plan(L, 2, 70001)[1]
    for rows in (1, 2, 3, 16, 64, 65, 255, 256, 257, 5000):
        for w in (1, 4095, 4096, 8191, 8192, 32768, 70001, 131072, 1 << 24):
            rc, parts = _plan(L, rows, w)
            assert rc == 0 and 1 <= parts <= 64, (rows, w, parts)
            assert parts == 1 or (rows < 256 and parts * rows < 768), (rows, w, parts)
            assert parts == 1 or w // parts >= 4096, (rows, w, parts)         # no row is cut finer than 4096 columns
            ws = L.qgemm_argmax_rows_workspace_size(rows, w)
            assert ws == (0 if parts == 1 else 8 * rows * parts)
    assert L.qgemm_argmax_rows_plan(0, 8, None) == 0
    for rows, w in ((1, 0), (1, -3), (-1, 8), (1, (1 << 24) + 1)):
        assert _plan(L, rows, w)[0] == qg.HIP_ERROR_INVALID_VALUE, (rows, w)
        assert L.qgemm_argmax_rows_workspace_size(rows, w) == 0
    with pytest.raises(qg.QGemmError):
        qg.argmax_rows_plan(1, 0)


def test_new_symbols_are_exported(qg):
    L = qg.load()
    for name in ("qgemm_argmax_rows_workspace_size", "qgemm_argmax_rows_plan", "qgemm_argmax_rows", "qgemm_embed_rows",
                 "qgemm_head_create", "qgemm_head_logits", "qgemm_head_next_tokens", "qgemm_head_embed",
                 "qgemm_head_destroy", "qgemm_decoder_generate"):
        assert name in qg.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    for name in ("argmax_rows", "argmax_rows_plan", "embed_rows", "Head"):
        assert hasattr(qg, name)
    assert hasattr(qg.Decoder, "generate")


def test_argument_checks_need_no_gpu(qg):
    """Null pointers and bad dimensions are refused before any device call."""
    L = qg.load()
    bad = qg.HIP_ERROR_INVALID_VALUE
    assert L.qgemm_argmax_rows(None, 8, 1, 8, 16, None, None, 0, None) == bad
    assert L.qgemm_argmax_rows(16, 8, 1, 8, None, None, None, 0, None) == bad
    assert L.qgemm_argmax_rows(16, 7, 1, 8, 16, None, None, 0, None) == bad      # a row stride below w
    assert L.qgemm_argmax_rows(16, 8, 1, 0, 16, None, None, 0, None) == bad
    assert L.qgemm_argmax_rows(16, 131072, 1, 131072, 16, None, None, 0, None) == bad   # split, no workspace
    assert L.qgemm_embed_rows(None, 4, 4, 4, 16, None, 0, 0, None, 1, 1, 16, 4, None) == bad
    assert L.qgemm_embed_rows(16, 4, 4, 4, 16, None, 0, 0, None, 65, 1, 16, 4, None) == bad  # more than 64 sequences
    h = ctypes.c_void_p(1)
    assert L.qgemm_head_create(None, 4, 4, None, None, 0, None, 0, 0, 1, ctypes.byref(h)) == bad and not h.value
    assert L.qgemm_head_logits(None, 16, 4, 1, 16, 4, None) == bad
    assert L.qgemm_head_next_tokens(None, 16, 4, 1, 16, None) == bad
    assert L.qgemm_head_embed(None, 16, None, 1, 1, 16, 4, None) == bad
    assert L.qgemm_decoder_generate(None, None, 1, None, None, 1, None, None, None) == bad
    assert L.qgemm_head_destroy(None) == 0
