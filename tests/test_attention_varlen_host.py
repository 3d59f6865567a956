"""The batched variable-length forward without a GPU: the new entry points are declared, exported, listed and
prototyped; QGEMM_VARLEN_MAX_SEQS agrees between the header and Python; qgemm_attention_varlen_plan at the edges of the
table launch's envelope; qgemm_attention_varlen_workspace_size is 0 exactly on the table launch and the largest
single-call size otherwise; every argument check qgemm_attention_varlen makes before a launch; the stack calls refuse
what they can refuse without a device; and the Python signatures."""
import ctypes
import inspect
import re
import subprocess

import pytest

INVALID = 1  # hipErrorInvalidValue
MANY, PER_SEQ = "attention_fused_kernel<many>", "per_sequence"
NEW_SYMBOLS = ("qgemm_attention_varlen", "qgemm_attention_varlen_workspace_size", "qgemm_attention_varlen_plan",
               "qgemm_encoder_create_rows", "qgemm_encoder_forward_batch", "qgemm_decoder_create_rows",
               "qgemm_decoder_step_varlen")


def _ints(*v):
    return (ctypes.c_int * max(1, len(v)))(*v)


def _longs(*v):
    return (ctypes.c_int64 * max(1, len(v)))(*v)


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
        want = ctypes.c_size_t if sym.endswith("workspace_size") else ctypes.c_int
        assert getattr(L, sym).restype is want


def test_max_seqs_is_64_in_header_and_python(qg):
    m = re.search(r"QGEMM_VARLEN_MAX_SEQS\s*=\s*(\d+)", open(qg.HEADER_PATH).read())
    assert m and int(m.group(1)) == 64
    assert qg.QGEMM_VARLEN_MAX_SEQS == 64


def _plan(qg, seq_q, seq_kv, n_heads=2, d_k=64):
    name = ctypes.c_char_p()
    n = len(seq_q)
    rc = qg.load().qgemm_attention_varlen_plan(n, _ints(*seq_q), _ints(*seq_kv), n_heads, d_k, ctypes.byref(name))
    return rc, (name.value.decode() if rc == 0 else None)


def _ws(qg, seq_q, seq_kv, n_heads=2, d_k=64):
    return qg.load().qgemm_attention_varlen_workspace_size(len(seq_q), _ints(*seq_q), _ints(*seq_kv), n_heads, d_k)


def test_plan_at_the_envelope_edges(qg):
    # every seq_kv = 512 against one at 513
    assert _plan(qg, [33, 1, 40], [512, 512, 512]) == (0, MANY)
    assert _plan(qg, [33, 1, 40], [512, 513, 512]) == (0, PER_SEQ)
    # d_k 64 against 65
    assert _plan(qg, [33, 1], [100, 7], d_k=64) == (0, MANY)
    assert _plan(qg, [33, 1], [100, 7], d_k=65) == (0, PER_SEQ)
    # n_seqs 0, 1, 64 and 65
    assert _plan(qg, [], []) == (0, MANY)
    assert _plan(qg, [5], [9]) == (0, MANY)
    assert _plan(qg, [5] * 64, [9] * 64) == (0, MANY)
    assert _plan(qg, [5] * 65, [9] * 65) == (INVALID, None)
    # an empty sequence in the table, and the wrapper
    assert _plan(qg, [5, 0, 7], [9, 3, 512]) == (0, MANY)
    assert qg.attention_varlen_plan([5, 0, 7], [9, 3, 512], 2, 24) == MANY
    assert qg.attention_varlen_plan([5, 0, 7], [9, 3, 4096], 2, 24) == PER_SEQ
    # what the call refuses, the query refuses
    for seq_q, seq_kv, kw in (([5, -1], [9, 9], {}), ([5, 5], [9, 0], {}), ([5, 5], [9, 4097], {}),
                              ([5], [9], dict(n_heads=0)), ([5], [9], dict(d_k=0))):
        assert _plan(qg, seq_q, seq_kv, **kw) == (INVALID, None), (seq_q, seq_kv, kw)
    L = qg.load()
    assert L.qgemm_attention_varlen_plan(1, None, _ints(9), 2, 24, None) == INVALID
    assert L.qgemm_attention_varlen_plan(1, _ints(5), None, 2, 24, None) == INVALID
    assert L.qgemm_attention_varlen_plan(1, _ints(5), _ints(9), 2, 24, None) == 0   # kernel may be NULL


@pytest.mark.parametrize("seq_q,seq_kv,d_k", [
    ([33, 1, 40], [512, 512, 512], 64),
    ([33, 1, 40], [512, 513, 512], 64),     # the 513-key sequence has one query row: the decode launch, yet a workspace
    ([33, 9, 40], [512, 513, 700], 24),
    ([33, 40], [100, 7], 65),
    ([0, 40], [513, 7], 24),                # no query row: that sequence needs no scores
    ([], [], 24),
    ([7] * 64, [512] * 64, 64),
])
def test_workspace_is_zero_exactly_on_the_table_launch(qg, seq_q, seq_kv, d_k):
    L = qg.load()
    H = 3
    single = [L.qgemm_attention_workspace_size(q, kv, H, d_k) for q, kv in zip(seq_q, seq_kv)]
    for q, kv, s in zip(seq_q, seq_kv, single):     # the single-call size, spelled out
        assert s == (0 if kv <= 512 and d_k <= 64 else 4 * H * q * kv)
    rc, plan = _plan(qg, seq_q, seq_kv, n_heads=H, d_k=d_k)
    assert rc == 0
    need = _ws(qg, seq_q, seq_kv, n_heads=H, d_k=d_k)
    assert need == max(single, default=0)
    if plan == MANY:
        assert need == 0
    else:
        assert any(kv > 512 or d_k > 64 for kv in seq_kv)
    if need:
        assert plan == PER_SEQ


def test_workspace_size_of_refused_arguments_is_zero(qg):
    L = qg.load()
    assert L.qgemm_attention_varlen_workspace_size(65, _ints(*[9] * 65), _ints(*[600] * 65), 2, 24) == 0
    assert L.qgemm_attention_varlen_workspace_size(-1, _ints(9), _ints(600), 2, 24) == 0
    assert L.qgemm_attention_varlen_workspace_size(1, None, _ints(600), 2, 24) == 0
    assert L.qgemm_attention_varlen_workspace_size(1, _ints(9), None, 2, 24) == 0


def _varlen(qg, **kw):
    """qgemm_attention_varlen with dummy non-null pointers and valid arguments, one of them replaced."""
    a = dict(Q=8, qs=8, K=8, ks=8, V=8, vs=8, O=8, os=8, n_seqs=2, q_row0=_longs(0, 4), seq_q=_ints(4, 5),
             kv_row0=_longs(0, 6), seq_kv=_ints(6, 7), q_pos0=_ints(2, 2), n_heads=2, d_k=4, scale=0.5, ws=None,
             ws_bytes=0, stream=None)
    a.update(kw)
    return qg.load().qgemm_attention_varlen(*a.values())


@pytest.mark.parametrize("bad", [
    dict(Q=None), dict(K=None), dict(V=None), dict(O=None),
    dict(q_row0=None), dict(seq_q=None), dict(kv_row0=None), dict(seq_kv=None),
    dict(n_seqs=-1),
    dict(n_seqs=65, q_row0=_longs(*[0] * 65), seq_q=_ints(*[4] * 65), kv_row0=_longs(*[0] * 65),
         seq_kv=_ints(*[6] * 65), q_pos0=None),
    dict(q_row0=_longs(0, -1)), dict(q_row0=_longs(-4, 0)), dict(kv_row0=_longs(0, -1)), dict(kv_row0=_longs(-1, 0)),
    dict(seq_q=_ints(4, -1)), dict(seq_q=_ints(-1, 4)),
    dict(seq_kv=_ints(6, 0)), dict(seq_kv=_ints(-1, 6)), dict(seq_kv=_ints(6, 4097)),
    dict(q_pos0=_ints(2, -1)), dict(q_pos0=_ints(-5, 0)),
    dict(n_heads=0), dict(n_heads=-2), dict(d_k=0), dict(d_k=-1),
    # the same per-sequence checks without a mask
    dict(q_pos0=None, seq_kv=_ints(0, 6)), dict(q_pos0=None, seq_q=_ints(4, -3)),
    # a workspace smaller than the size query's answer, or none: 513 keys x 9 rows x 2 heads of scores
    dict(seq_q=_ints(4, 9), seq_kv=_ints(6, 513), ws=None, ws_bytes=0),
    dict(seq_q=_ints(4, 9), seq_kv=_ints(6, 513), ws=8, ws_bytes=4 * 2 * 9 * 513 - 1),
    dict(seq_q=_ints(4, 9), seq_kv=_ints(6, 513), ws=None, ws_bytes=4 * 2 * 9 * 513),
    # outside the table launch and the second sequence wrong: refused before the first sequence is launched
    dict(seq_q=_ints(9, 9), seq_kv=_ints(513, 0), ws=8, ws_bytes=1 << 20),
    dict(seq_q=_ints(9, 9), seq_kv=_ints(513, 6), q_pos0=_ints(0, -1), ws=8, ws_bytes=1 << 20),
    dict(d_k=65, seq_q=_ints(9, -1), ws=8, ws_bytes=1 << 20),
], ids=lambda d: ",".join(f"{k}" for k in d))
def test_attention_varlen_refuses_before_any_launch(qg, bad):
    """No GPU is needed: every one of these returns hipErrorInvalidValue without touching the device."""
    assert _varlen(qg, **bad) == INVALID


def test_attention_varlen_with_no_sequence_returns_0(qg):
    assert _varlen(qg, n_seqs=0) == 0
    assert _varlen(qg, n_seqs=0, q_pos0=None) == 0
    # ... but only after the checks that do not depend on the sequences
    assert _varlen(qg, n_seqs=0, Q=None) == INVALID
    assert _varlen(qg, n_seqs=0, seq_kv=None) == INVALID
    assert _varlen(qg, n_seqs=0, d_k=0) == INVALID


def test_stack_calls_refuse_without_a_device(qg):
    L = qg.load()
    one = _ints(1)
    assert L.qgemm_encoder_forward_batch(None, 8, 8, 1, one, None) == INVALID
    assert L.qgemm_decoder_step_varlen(None, 1, _ints(0), _ints(0), one, 8, 8, None) == INVALID
    both = qg.QGEMM_DECODER_CAUSAL | qg.QGEMM_DECODER_KV_CACHE
    h = ctypes.c_void_p(123)

    def enc(max_rows, d_model=1024, d_ff=4096, handle=h):
        h.value = 123
        return L.qgemm_encoder_create_rows(d_model, 16, d_ff, 2, 512, max_rows, 1,
                                           ctypes.byref(handle) if handle is not None else None)

    def dec(max_rows, flags=both, n_slots=2, handle=h):
        h.value = 123
        return L.qgemm_decoder_create_rows(1024, 16, 4096, 2, 512, 512, 1, flags, n_slots, max_rows,
                                           ctypes.byref(handle) if handle is not None else None)

    # the row budget's bound: round_up(max_rows, 256) * round_up(max(3 d_model, d_ff), 128) <= 2^31 - 1; at d_model
    # 1024, d_ff 4096 the widest buffer has 4096 columns, so 524288 rows (2^31 elements) is the first budget refused
    for rc in (enc(-1), enc(524288), enc(524287), enc(2 ** 31 - 1), enc(2 ** 19, d_model=1366, d_ff=2),
               dec(-1), dec(524288), dec(2 ** 31 - 1)):
        assert rc == INVALID
        assert not h.value, "a refused create leaves a null handle"
    assert enc(0, handle=None) == INVALID and dec(0, handle=None) == INVALID
    for kw in (dict(flags=0), dict(flags=qg.QGEMM_DECODER_CAUSAL), dict(flags=both | 4), dict(n_slots=0),
               dict(n_slots=65)):
        assert dec(64, **kw) == INVALID, kw
        assert not h.value


def test_python_signatures(qg):
    a = inspect.signature(qg.attention_varlen).parameters
    assert list(a) == ["Q", "K", "V", "n_heads", "seq_q", "seq_kv", "q_row0", "kv_row0", "q_pos0", "scale", "O"]
    for name in ("q_row0", "kv_row0", "q_pos0", "scale", "O"):
        assert a[name].default is None
    assert list(inspect.signature(qg.attention_varlen_plan).parameters) == ["seq_q", "seq_kv", "n_heads", "d_k"]
    e = inspect.signature(qg.Encoder.__init__).parameters
    assert list(e)[-1] == "max_rows" and e["max_rows"].default is None and e["seed"].default == 0
    f = inspect.signature(qg.Encoder.forward_batch).parameters
    assert list(f) == ["self", "X", "seq_lens", "Y"] and f["Y"].default is None
    d = inspect.signature(qg.Decoder.__init__).parameters
    assert list(d)[-2:] == ["max_rows", "n_slots"] and d["max_rows"].default is None and d["n_slots"].default == 1
    s = inspect.signature(qg.Decoder.step_varlen).parameters
    assert list(s) == ["self", "slots", "X_new", "n_rows", "pos", "Y"] and s["pos"].default is None
    # what existing callers rely on is unchanged
    assert list(inspect.signature(qg.Encoder.forward).parameters) == ["self", "X", "Y"]
    b = inspect.signature(qg.Decoder.step_batch).parameters
    assert list(b) == ["self", "slots", "X_new", "pos", "rows_per_seq", "Y"]
