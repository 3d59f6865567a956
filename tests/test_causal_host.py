"""The causal mask without a GPU: properties of the expected values themselves (tests/causal_oracle.py), so the GPU
tests compare against a composition that is known to mask, and the new C entry points' presence and argument checks
through ctypes (every rejected call returns before any launch)."""
import ctypes
import re

import numpy as np
import pytest

import attn_oracle
import causal_oracle
from util import assert_bits_equal, bits

INVALID = 1  # hipErrorInvalidValue
NEW_SYMBOLS = ("qgemm_attention_causal", "qgemm_softmax_rows_causal", "qgemm_decoder_create_ex")


# ---- the composition alone ----

@pytest.mark.parametrize("shape", causal_oracle.SHAPES, ids=str)
def test_prefix_property_of_the_composition(oracle, shape):
    """Row i of the masked result is row 0 of the UNMASKED attention of query i against keys and values 0 .. L_i - 1:
    with finite V and no -0 accumulator the masked keys' fmaf(+0, v, acc) steps change nothing.  No output is -0."""
    seq_q, seq_kv, H, dk, q_pos0 = shape
    Q, K, V = causal_oracle.qkv(shape)
    got = causal_oracle.expected(shape)
    L = causal_oracle.limits(seq_q, seq_kv, q_pos0)
    assert L.min() >= 1 and L.max() <= seq_kv
    scale = attn_oracle.default_scale(dk)
    want = np.empty_like(got)
    for i in range(seq_q):
        want[i] = attn_oracle.attention_ref(Q[i:i + 1], K[:L[i]], V[:L[i]], H, scale)[0]
    assert_bits_equal(got, want, f"prefix property {shape}")
    assert not (bits(got) == 0x80000000).any(), "an output is -0"


@pytest.mark.parametrize("shape", causal_oracle.SHAPES, ids=str)
def test_masked_rows_differ_from_unmasked(oracle, shape):
    """Every row that does not see all keys differs from the unmasked result (in every head), the rows that see all of
    them are its bits: the GPU comparison against the composition cannot pass on an unmasked kernel."""
    seq_q, seq_kv, H, dk, q_pos0 = shape
    masked, plain = causal_oracle.expected(shape), causal_oracle.expected_unmasked(shape)
    L = causal_oracle.limits(seq_q, seq_kv, q_pos0)
    full = L == seq_kv
    assert_bits_equal(masked[full], plain[full], f"rows that see every key {shape}")
    differs = (bits(masked) != bits(plain)).reshape(seq_q, H, dk).any(axis=2)
    assert differs[~full].all(), "a masked row equals the unmasked result"
    if shape != (1, 1, 1, 1, 0):
        assert (~full).any(), "the shape masks nothing"


@pytest.mark.parametrize("shape", [(33, 33, 2, 24, 32), (33, 33, 2, 24, 1000), (20, 40, 1, 65, 39)], ids=str)
def test_mask_without_effect_is_the_unmasked_result(oracle, shape):
    """q_pos0 >= seq_kv - 1: every L_i is seq_kv."""
    Q, K, V = causal_oracle.qkv(shape)
    H, dk, q_pos0 = shape[2:]
    scale = attn_oracle.default_scale(dk)
    assert_bits_equal(causal_oracle.attention_causal_ref(Q, K, V, H, scale, q_pos0),
                      attn_oracle.attention_ref(Q, K, V, H, scale), f"no-op mask {shape}")


def test_softmax_rows_causal_ref_rows(oracle):
    """The stacked form: row r of a stack of 3 matrices uses query r % seq_q's limit; masked columns are +0 and are
    never read (NaN there changes nothing)."""
    seq_q, w, q_pos0 = 5, 9, 2
    S = oracle.uniform((3, seq_q, w), 7) * np.float32(4.0)
    P = causal_oracle.softmax_rows_causal(S, seq_q, q_pos0, 0.5)
    L = causal_oracle.limits(seq_q, w, q_pos0)
    assert list(L) == [3, 4, 5, 6, 7]
    for m in range(3):
        for i in range(seq_q):
            assert_bits_equal(P[m, i, :L[i]], oracle.softmax_rows(S[m, i:i + 1, :L[i]].copy(), 0.5)[0], f"row {m},{i}")
            assert (bits(P[m, i, L[i]:]) == 0).all()
    S2 = S.copy()
    for i in range(seq_q):
        S2[:, i, L[i]:] = np.nan
    assert_bits_equal(causal_oracle.softmax_rows_causal(S2, seq_q, q_pos0, 0.5), P, "NaN at masked scores")


def test_causal_decoder_ref_has_the_prefix_property_and_the_plain_one_does_not(oracle):
    shape = causal_oracle.DECODER_FUSED
    full, part = causal_oracle.decoder_expected(shape), causal_oracle.decoder_expected(shape, True, 17)
    assert_bits_equal(part, full[:17], "causal decoder reference: forward(X[:17]) vs forward(X)[:17]")
    pfull, ppart = causal_oracle.decoder_expected(shape, False), causal_oracle.decoder_expected(shape, False, 17)
    assert (bits(ppart) != bits(pfull[:17])).any(axis=1).all(), "the unmasked decoder has a prefix-stable row"
    assert (bits(full) != bits(pfull)).any()


# ---- the entry points: present, and every argument check before any launch ----

def test_new_symbols_are_declared_exported_and_listed(qg):
    import subprocess
    header = open(qg.HEADER_PATH).read()
    declared = re.findall(r"^QGEMM_API\s+[\w\s\*]+?\b((?:op_|qgemm_)\w+)\s*\(", header, flags=re.M)
    nm = subprocess.run(["nm", "-D", "--defined-only", qg.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} not declared in include/qgemm.h"
        assert sym in qg.EXPORTED_SYMBOLS, f"{sym} not in EXPORTED_SYMBOLS"
        assert re.search(rf" T {sym}$", nm, flags=re.M), f"{sym} not exported by libqgemm.so"
    assert re.search(r"QGEMM_DECODER_CAUSAL\s*=\s*1\b", header) and qg.QGEMM_DECODER_CAUSAL == 1


def _attn_causal(L, Q=8, K=8, V=8, O=8, seq_q=4, seq_kv=4, H=1, dk=4, q_pos0=0, ws=None, ws_bytes=0):
    return L.qgemm_attention_causal(Q, 4, K, 4, V, 4, O, 4, seq_q, seq_kv, H, dk, 0.5, q_pos0, ws, ws_bytes, None)


def test_attention_causal_argument_checks(qg):
    L = qg.load()
    assert _attn_causal(L, q_pos0=-1) == INVALID
    assert _attn_causal(L, q_pos0=-2) == INVALID
    for null in ("Q", "K", "V", "O"):
        assert _attn_causal(L, **{null: None}) == INVALID, null
    assert _attn_causal(L, seq_q=-1) == INVALID
    assert _attn_causal(L, seq_kv=0) == INVALID
    assert _attn_causal(L, seq_kv=4097) == INVALID
    assert _attn_causal(L, H=0) == INVALID
    assert _attn_causal(L, dk=0) == INVALID
    # outside the fused envelope the workspace is qgemm_attention's, and a missing or short one is refused
    need = L.qgemm_attention_workspace_size(4, 513, 1, 4)
    assert need == 4 * 4 * 513
    assert _attn_causal(L, seq_kv=513) == INVALID
    assert _attn_causal(L, seq_kv=513, ws=8, ws_bytes=need - 1) == INVALID
    # no queries: nothing to do, inside and outside the envelope, whatever q_pos0 >= 0
    assert _attn_causal(L, seq_q=0) == 0
    assert _attn_causal(L, seq_q=0, q_pos0=2 ** 31 - 1) == 0
    assert _attn_causal(L, seq_q=0, seq_kv=513) == 0
    assert _attn_causal(L, seq_q=0, q_pos0=-1) == INVALID


def test_softmax_rows_causal_argument_checks(qg):
    f = qg.load().qgemm_softmax_rows_causal
    assert f(None, 8, 4, 4, 1.0, 2, 0, None) == INVALID
    assert f(8, None, 4, 4, 1.0, 2, 0, None) == INVALID
    assert f(8, 8, 4, 4, 1.0, 0, 0, None) == INVALID      # seq_q < 1
    assert f(8, 8, 4, 4, 1.0, -3, 0, None) == INVALID
    assert f(8, 8, 4, 4, 1.0, 3, 0, None) == INVALID      # rows % seq_q != 0
    assert f(8, 8, 4, 4, 1.0, 2, -1, None) == INVALID     # q_pos0 < 0
    assert f(8, 8, 4, 0, 1.0, 2, 0, None) == INVALID      # w < 1
    assert f(8, 8, 4, 4097, 1.0, 2, 0, None) == INVALID   # w > 4096
    assert f(8, 8, -2, 4, 1.0, 2, 0, None) == INVALID     # rows < 0
    assert f(8, 8, 0, 4, 1.0, 2, 0, None) == 0            # no rows: nothing to do


def test_decoder_create_ex_argument_checks(qg):
    f = qg.load().qgemm_decoder_create_ex
    h = ctypes.c_void_p(123)
    for flags in (2, 3, 4, -1, 1 << 30):
        h.value = 123
        assert f(8, 4, 8, 1, 6, 6, 1, flags, ctypes.byref(h)) == INVALID, flags
        assert not h.value, "a refused create leaves a null handle"
    assert f(8, 4, 8, 1, 6, 6, 1, 0, None) == INVALID
    assert f(8, 4, 8, 1, 6, 6, 1, qg.QGEMM_DECODER_CAUSAL, None) == INVALID
    # qgemm_decoder_create's own dimension checks, with either flag value
    for flags in (0, qg.QGEMM_DECODER_CAUSAL):
        assert f(8, 3, 8, 1, 6, 6, 1, flags, ctypes.byref(h)) == INVALID   # d_model % n_heads != 0
        assert f(8, 4, 8, 1, 4097, 6, 1, flags, ctypes.byref(h)) == INVALID


def test_python_keywords_default_to_todays_behaviour(qg):
    import inspect
    a = inspect.signature(qg.attention).parameters
    assert a["causal"].default is False and a["q_pos0"].default is None
    s = inspect.signature(qg.softmax_rows_causal).parameters
    assert list(s) == ["S", "seq_q", "q_pos0", "scale", "P"] and s["q_pos0"].default == 0 and s["scale"].default == 1.0
    d = inspect.signature(qg.Decoder.__init__).parameters
    assert d["causal"].default is False and d["seed"].default == 0
