"""Incremental decoding without a GPU: the new entry points are declared, exported and listed; qgemm_attention_plan
names the launch of every shape class and agrees with qgemm_attention_workspace_size; the step's and begin's argument
checks that need no decoder; and, on the oracle alone, the fact the step's expected values rest on -- row n - 1 of the
causal decoder's forward on the first n rows is row n - 1 of its forward on all of them."""
import ctypes
import inspect
import re
import subprocess

import pytest

import causal_oracle
from util import assert_bits_equal

INVALID = 1  # hipErrorInvalidValue
NEW_SYMBOLS = ("qgemm_attention_plan", "qgemm_decoder_begin", "qgemm_decoder_step")


def test_new_symbols_are_declared_exported_and_listed(qg):
    header = open(qg.HEADER_PATH).read()
    declared = re.findall(r"^QGEMM_API\s+[\w\s\*]+?\b((?:op_|qgemm_)\w+)\s*\(", header, flags=re.M)
    nm = subprocess.run(["nm", "-D", "--defined-only", qg.LIB_PATH], check=True, capture_output=True, text=True).stdout
    L = qg.load()
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} not declared in include/qgemm.h"
        assert sym in qg.EXPORTED_SYMBOLS, f"{sym} not in EXPORTED_SYMBOLS"
        assert re.search(rf" T {sym}$", nm, flags=re.M), f"{sym} not exported by libqgemm.so"
        assert getattr(L, sym).argtypes, f"{sym} has no ctypes prototype"
    m = re.search(r"QGEMM_DECODER_KV_CACHE\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == qg.QGEMM_DECODER_KV_CACHE
    # one bit of its own, beside the mask's
    v = qg.QGEMM_DECODER_KV_CACHE
    assert v > 0 and v & (v - 1) == 0 and v != qg.QGEMM_DECODER_CAUSAL


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 4096, 16, 64), (8, 513, 2, 8), (8, 512, 16, 64), (1, 77, 2, 24),
                                   (0, 40, 1, 4)], ids=str)
def test_plan_is_the_decode_kernel(qg, shape):
    assert qg.attention_plan(*shape).startswith("attention_decode")


@pytest.mark.parametrize("shape", [(9, 40, 2, 24), (9, 512, 1, 64), (1, 40, 1, 65), (8, 4096, 1, 65), (9, 513, 2, 8),
                                   (33, 4096, 1, 64), (512, 512, 1, 64)], ids=str)
def test_plan_outside_the_decode_envelope_agrees_with_the_workspace_size(qg, shape):
    """seq_q >= 9 or d_k > 64: the fused launch exactly where the workspace size is 0, else the three launches."""
    name = qg.attention_plan(*shape)
    assert not name.startswith("attention_decode")
    fused = qg.load().qgemm_attention_workspace_size(*shape) == 0
    assert name.startswith("attention_fused" if fused else "three_launches"), (shape, name)
    assert fused == (shape[1] <= 512 and shape[3] <= 64)


def test_plan_leaves_the_workspace_size_alone(qg):
    """Past the fused envelope a decode-shaped call still has to bring the three launches' workspace."""
    L = qg.load()
    assert L.qgemm_attention_workspace_size(1, 512, 2, 8) == 0
    assert L.qgemm_attention_workspace_size(1, 513, 2, 8) == 4 * 2 * 1 * 513
    assert L.qgemm_attention_workspace_size(8, 4096, 16, 64) == 4 * 16 * 8 * 4096
    assert qg.attention_plan(1, 513, 2, 8).startswith("attention_decode")
    # ... and a call without it is refused as before, before any launch
    assert L.qgemm_attention(8, 8, 8, 8, 8, 8, 8, 8, 1, 513, 2, 8, 0.5, None, 0, None) == INVALID
    assert L.qgemm_attention_causal(8, 8, 8, 8, 8, 8, 8, 8, 1, 513, 2, 8, 0.5, 512, None, 0, None) == INVALID


def test_plan_argument_checks(qg):
    L = qg.load()
    name = ctypes.c_char_p()
    for bad in ((1, 4097, 1, 4), (1, 0, 1, 4), (-1, 4, 1, 4), (1, 4, 0, 4), (1, 4, 1, 0)):
        assert L.qgemm_attention_plan(*bad, ctypes.byref(name)) == INVALID, bad
        with pytest.raises(qg.QGemmError):
            qg.attention_plan(*bad)
    assert L.qgemm_attention_plan(1, 4, 1, 4, None) == 0   # the name is optional


def test_create_ex_cache_flag_needs_the_mask(qg):
    f = qg.load().qgemm_decoder_create_ex
    h = ctypes.c_void_p(123)
    for flags in (qg.QGEMM_DECODER_KV_CACHE, qg.QGEMM_DECODER_KV_CACHE | 2, qg.QGEMM_DECODER_KV_CACHE | 16,
                  qg.QGEMM_DECODER_KV_CACHE | qg.QGEMM_DECODER_CAUSAL | 32):
        h.value = 123
        assert f(8, 4, 8, 1, 6, 6, 1, flags, ctypes.byref(h)) == INVALID, flags
        assert not h.value, "a refused create leaves a null handle"
    both = qg.QGEMM_DECODER_KV_CACHE | qg.QGEMM_DECODER_CAUSAL
    assert f(8, 4, 8, 1, 6, 6, 1, both, None) == INVALID
    assert f(8, 3, 8, 1, 6, 6, 1, both, ctypes.byref(h)) == INVALID   # the dimension checks come first


def test_begin_and_step_refuse_a_null_decoder(qg):
    L = qg.load()
    assert L.qgemm_decoder_begin(None, 8, 4, None) == INVALID
    assert L.qgemm_decoder_step(None, 8, 8, 0, 1, None) == INVALID


def test_python_keywords_default_to_todays_behaviour(qg):
    d = inspect.signature(qg.Decoder.__init__).parameters
    assert d["kv_cache"].default is False and d["causal"].default is False
    s = inspect.signature(qg.Decoder.step).parameters
    assert list(s) == ["self", "X_new", "pos", "Y"] and s["pos"].default is None and s["Y"].default is None
    assert list(inspect.signature(qg.Decoder.begin).parameters) == ["self", "enc_out"]
    assert list(inspect.signature(qg.attention_plan).parameters) == ["seq_q", "seq_kv", "n_heads", "d_k"]


@pytest.mark.parametrize("n", [1, 17, 40])
def test_last_row_of_a_prefix_forward_is_that_row_of_the_full_forward(oracle, n):
    """What a step's expected value rests on: decoder_expected(rows = n)[n - 1] == decoder_expected()[n - 1]."""
    shape = causal_oracle.DECODER_FUSED
    full = causal_oracle.decoder_expected(shape)
    part = causal_oracle.decoder_expected(shape, True, n)
    assert part.shape == (n, shape[2])
    assert_bits_equal(part[n - 1], full[n - 1], f"row {n - 1} of the forward on {n} rows")
