"""Batched incremental decoding without a GPU: the new entry points are declared, exported, listed and prototyped;
QGEMM_DECODE_MAX_BATCH agrees between the header and Python; every argument check that
qgemm_attention_decode_batched and qgemm_decoder_create_slots make before a launch or an allocation; the slot calls
refuse a null decoder; and the Python signatures that existing callers rely on are unchanged."""
import ctypes
import inspect
import re
import subprocess

import pytest

INVALID = 1  # hipErrorInvalidValue
NEW_SYMBOLS = ("qgemm_attention_decode_batched", "qgemm_decoder_create_slots", "qgemm_decoder_begin_slot",
               "qgemm_decoder_step_slot", "qgemm_decoder_step_batch", "qgemm_decoder_copy_slot",
               "qgemm_decoder_slot_state")


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_new_symbols_are_declared_exported_listed_and_prototyped(qg):
    header = open(qg.HEADER_PATH).read()
    declared = re.findall(r"^QGEMM_API\s+[\w\s\*]+?\b((?:op_|qgemm_)\w+)\s*\(", header, flags=re.M)
    nm = subprocess.run(["nm", "-D", "--defined-only", qg.LIB_PATH], check=True, capture_output=True, text=True).stdout
    L = qg.load()
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} not declared in include/qgemm.h"
        assert sym in qg.EXPORTED_SYMBOLS, f"{sym} not in EXPORTED_SYMBOLS"
        assert re.search(rf" T {sym}$", nm, flags=re.M), f"{sym} not exported by libqgemm.so"
        assert getattr(L, sym).argtypes, f"{sym} has no ctypes prototype"
        assert getattr(L, sym).restype is ctypes.c_int


def test_max_batch_is_64_in_header_and_python(qg):
    m = re.search(r"QGEMM_DECODE_MAX_BATCH\s*=\s*(\d+)", open(qg.HEADER_PATH).read())
    assert m and int(m.group(1)) == 64
    assert qg.QGEMM_DECODE_MAX_BATCH == 64


def _batched(qg, **kw):
    """qgemm_attention_decode_batched with dummy non-null pointers and valid arguments, one of them replaced."""
    a = dict(Q=8, qs=8, K=8, ks=8, kss=64, V=8, vs=8, vss=64, O=8, os=8, n_seqs=2, rows_per_seq=1,
             kv_slot=_ints(0, 1), seq_kv=_ints(4, 5), q_pos0=_ints(3, 4), n_heads=2, d_k=4, scale=0.5, stream=None)
    a.update(kw)
    return qg.load().qgemm_attention_decode_batched(*a.values())


@pytest.mark.parametrize("bad", [
    dict(Q=None), dict(K=None), dict(V=None), dict(O=None), dict(seq_kv=None),
    dict(n_seqs=-1), dict(n_seqs=65, kv_slot=None, q_pos0=None, seq_kv=_ints(*[4] * 65)),
    dict(rows_per_seq=0), dict(rows_per_seq=9), dict(rows_per_seq=-1),
    dict(d_k=0), dict(d_k=65), dict(n_heads=0), dict(n_heads=-2),
    dict(seq_kv=_ints(4, 0)), dict(seq_kv=_ints(-1, 4)), dict(seq_kv=_ints(4, 4097)),
    dict(q_pos0=_ints(3, -1)), dict(q_pos0=_ints(-5, 0)),
    dict(kv_slot=_ints(0, -1)), dict(kv_slot=_ints(-1, 0)),
    # the same per-sequence checks with the optional tables left out
    dict(kv_slot=None, q_pos0=None, seq_kv=_ints(0, 4)),
    dict(kv_slot=None, seq_kv=_ints(4, 4097)),
], ids=lambda d: ",".join(f"{k}" for k in d))
def test_attention_decode_batched_refuses_before_any_launch(qg, bad):
    """No GPU is needed: every one of these returns hipErrorInvalidValue without touching the device."""
    assert _batched(qg, **bad) == INVALID


def test_attention_decode_batched_with_no_sequence_returns_0(qg):
    assert _batched(qg, n_seqs=0) == 0
    assert _batched(qg, n_seqs=0, kv_slot=None, q_pos0=None) == 0
    # ... but only after the checks that do not depend on the sequences
    assert _batched(qg, n_seqs=0, Q=None) == INVALID
    assert _batched(qg, n_seqs=0, seq_kv=None) == INVALID
    assert _batched(qg, n_seqs=0, d_k=65) == INVALID


def test_create_slots_refusals_leave_a_null_handle(qg):
    f = qg.load().qgemm_decoder_create_slots
    both = qg.QGEMM_DECODER_CAUSAL | qg.QGEMM_DECODER_KV_CACHE
    h = ctypes.c_void_p(123)

    def create(flags=both, n_slots=2, heads=4, handle=h):
        h.value = 123
        return f(8, heads, 8, 1, 6, 6, 1, flags, n_slots, ctypes.byref(handle) if handle is not None else None)

    for kw in (dict(n_slots=0), dict(n_slots=65), dict(n_slots=-1),
               dict(flags=0), dict(flags=qg.QGEMM_DECODER_CAUSAL), dict(flags=qg.QGEMM_DECODER_KV_CACHE),
               dict(flags=both | 2), dict(flags=both | 4), dict(flags=both | 16),
               dict(heads=3)):                       # the dimension checks of every create
        assert create(**kw) == INVALID, kw
        assert not h.value, f"a refused create leaves a null handle ({kw})"
    assert create(handle=None) == INVALID


def test_slot_calls_refuse_a_null_decoder(qg):
    L = qg.load()
    one = _ints(0)
    assert L.qgemm_decoder_begin_slot(None, 0, 8, 4, None) == INVALID
    assert L.qgemm_decoder_step_slot(None, 0, 8, 8, 0, 1, None) == INVALID
    assert L.qgemm_decoder_step_batch(None, 1, one, one, 1, 8, 8, None) == INVALID
    assert L.qgemm_decoder_copy_slot(None, 1, 0, None) == INVALID
    e, n = ctypes.c_int(7), ctypes.c_int(7)
    assert L.qgemm_decoder_slot_state(None, 0, ctypes.byref(e), ctypes.byref(n)) == INVALID
    assert (e.value, n.value) == (7, 7)


def test_python_signatures(qg):
    d = inspect.signature(qg.Decoder.__init__).parameters
    assert list(d)[-1] == "n_slots" and d["n_slots"].default == 1
    assert d["kv_cache"].default is False and d["causal"].default is False
    s = inspect.signature(qg.Decoder.step).parameters
    assert list(s) == ["self", "X_new", "pos", "Y"] and s["pos"].default is None and s["Y"].default is None
    assert list(inspect.signature(qg.Decoder.begin).parameters) == ["self", "enc_out"]
    assert list(inspect.signature(qg.Decoder.begin_slot).parameters) == ["self", "slot", "enc_out"]
    assert list(inspect.signature(qg.Decoder.step_slot).parameters) == ["self", "slot", "X_new", "pos", "Y"]
    b = inspect.signature(qg.Decoder.step_batch).parameters
    assert list(b) == ["self", "slots", "X_new", "pos", "rows_per_seq", "Y"] and b["rows_per_seq"].default == 1
    assert list(inspect.signature(qg.Decoder.copy_slot).parameters) == ["self", "dst", "src"]
    assert list(inspect.signature(qg.Decoder.slot_filled).parameters) == ["self", "slot"]
    a = inspect.signature(qg.attention_decode_batched).parameters
    assert list(a) == ["Q", "K", "V", "n_heads", "seq_kv", "q_pos0", "kv_slot", "rows_per_seq", "scale", "O"]
    assert a["q_pos0"].default is None and a["kv_slot"].default is None and a["rows_per_seq"].default == 1
