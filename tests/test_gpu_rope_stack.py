"""Rotary embeddings in the stack (rope=True, QGEMM_ARCH_ROPE) on the device, bit for bit against
tests/rope_oracle.py on three models: a pre-LN decoder-only model with the final norm, a post-LN encoder and a post-LN
decoder with cross-attention (7 encoder rows).  d_model 64, 4 heads (d_k 16), d_ff 200, 2 blocks, max_seq 16, 9 rows.
The oracle is fed the tables READ BACK from the model, so no bit-exact check rests on two libms agreeing; the tables
themselves are held to 1 ulp of rope_oracle.make_tables."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import prenorm_oracle as PO
import rope_oracle as RO
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

D, H, DFF, BLOCKS, MAX_SEQ, SEQ, ENC_SEQ = 64, 4, 200, 2, 16, 9, 7
DK = D // H
SEED = 404
INVALID = 1
F = np.float32
# model: (cross weights, the oracle's arch)
MODELS = {"only-pre": (False, 0x301), "enc-post": (False, 1), "dec-post": (True, 1)}


def _dev(a, device, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(device).to(dtype)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


@functools.lru_cache(maxsize=None)
def _weights(cross):
    return PO.prenorm_weights(D, H, DFF, BLOCKS, 23, cross=cross, final_norm=True)


@functools.lru_cache(maxsize=None)
def _x(seed=11, rows=SEQ):
    X = O.uniform((rows, D), seed)
    X.flags.writeable = False
    return X


def _make(qg, which, device, **kw):
    """the model with every tensor of its weight set loaded"""
    if which == "only-pre":
        m = qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, 0, seed=SEED, causal=True, kv_cache=True, decoder_only=True,
                       arch="standard", norm_first=True, final_norm=True, rope=True, **kw)
    elif which == "enc-post":
        m = qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ, seed=SEED, arch="standard", rope=True, **kw)
    else:
        m = qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, ENC_SEQ, seed=SEED, causal=True, kv_cache=True, arch="standard",
                       rope=True, **kw)
    for (block, kind), a in _weights(MODELS[which][0]).items():
        if kind < PO.GF or which == "only-pre":
            m.set_weight(block, kind, _dev(a, device))
    return m


def _tables(m):
    return tuple(t.cpu().numpy() for t in m.rope_tables())


def _oracle(which, X, tables, enc=None):
    cross, arch = MODELS[which]
    W = _weights(cross)
    if which == "enc-post":
        return RO.encoder_forward_rope(X, W, D, H, BLOCKS, tables, arch)
    if which == "dec-post":
        return RO.decoder_forward_rope(X, enc, W, D, H, BLOCKS, tables, arch, causal=True)
    return RO.decoder_only_forward(X, W, D, H, BLOCKS, arch, causal=True, rope=tables)


def _forward(m, which, X, enc, **kw):
    return m.forward(X, **kw) if which == "enc-post" else m.forward(X, enc, **kw)


# ---- the tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(MODELS))
def test_tables_at_creation(qg, oracle, device, which):
    m = _make(qg, which, device)
    try:
        cos, sin = _tables(m)
        assert m.weight_shape(qg.KIND_ROPE_COS) == (MAX_SEQ, DK // 2, 1) == m.weight_shape(qg.KIND_ROPE_SIN)
        assert m.info()["arch"] == MODELS[which][1] | 0x800 | (0x400 if which == "only-pre" else 0)
        p, n = ctypes.c_void_p(), ctypes.c_int()
        assert qg.load().qgemm_model_bias(m._h, 0, 28, ctypes.byref(p), ctypes.byref(n)) == INVALID
    finally:
        m.close()
    wc, ws = RO.make_tables(MAX_SEQ, DK)
    assert cos.shape == sin.shape == (MAX_SEQ, DK // 2)
    for got, want in ((cos, wc), (sin, ws)):   # two libms may round a double cos differently: 1 fp32 ulp
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
    assert (cos[0] == 1).all() and (sin[0] == 0).all()


# ---- forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(MODELS))
def test_forward_prefix_and_steps(qg, oracle, device, which):
    X = _dev(_x(), device)
    enc = _dev(_x(12, ENC_SEQ), device) if which == "dec-post" else None
    m = _make(qg, which, device)
    try:
        tables = _tables(m)
        got = _forward(m, which, X, enc, Y=_nan((SEQ, D), device)).cpu().numpy()
        assert_bits_equal(X.cpu().numpy(), _x(), "forward leaves X unchanged")
        if which != "enc-post":
            part = _forward(m, which, X[:4].contiguous(), enc).cpu().numpy()
            assert_bits_equal(part, got[:4], "forward(X[:4]) == forward(X)[:4]")
            m.begin(enc)
            rows = torch.cat([m.step(X[i:i + 1].contiguous(), Y=_nan((1, D), device)) for i in range(SEQ)]).cpu().numpy()
            m.begin(enc)
            chunks = torch.cat([m.step(X[0:5]), m.step(X[5:6]), m.step(X[6:9])]).cpu().numpy()
            again = m.step(X[3:9].contiguous(), pos=3).cpu().numpy()   # a rewind: the cache holds rotated K
            assert_bits_equal(rows, got, "steps row by row against forward")
            assert_bits_equal(chunks, got, "steps 5, 1, 3 against forward")
            assert_bits_equal(again, got[3:], "a rewind to position 3")
    finally:
        m.close()
    want = _oracle(which, _x(), tables, None if enc is None else _x(12, ENC_SEQ))
    assert_bits_equal(got, want, f"forward with RoPE, {which}")
    # the rotation is there (and only on the self-attention): the same chain without it is another function
    cross, arch = MODELS[which]
    plain = (RO.decoder_forward_rope(_x(), _x(12, ENC_SEQ), _weights(cross), D, H, BLOCKS, None, arch, causal=True)
             if which == "dec-post" else
             RO.decoder_only_forward(_x(), _weights(cross), D, H, BLOCKS, arch, causal=which != "enc-post"))
    assert np.abs(plain - want).max() > 1e-3


SLOT_PRE = (4, 0, 2)


@pytest.mark.parametrize("which", ["only-pre", "dec-post"])
def test_batched_steps_equal_each_sequences_forward(qg, oracle, device, which):
    """step_batch (one row each at positions 4, 0, 2), then step_varlen (rows 2, 1, 3 behind them), then the copy-free
    beam search's step on two beams of slot 0's sequence: every row is its own sequence's forward row."""
    enc = [_x(50 + b, (7, 5, 3)[b]) for b in range(3)] if which == "dec-post" else [None] * 3
    seq = [_x(40 + b) for b in range(3)]
    m = _make(qg, which, device, n_slots=4, max_rows=16)
    try:
        tables = _tables(m)
        for b in range(3):
            m.begin_slot(b, None if enc[b] is None else _dev(enc[b], device))
            if SLOT_PRE[b]:
                m.step_slot(b, _dev(seq[b][:SLOT_PRE[b]], device))
        new = torch.cat([_dev(seq[b][SLOT_PRE[b]:SLOT_PRE[b] + 1], device) for b in range(3)])
        one = m.step_batch([0, 1, 2], new, Y=_nan((3, D), device)).cpu().numpy()
        cnt = (2, 1, 3)
        more = torch.cat([_dev(seq[b][SLOT_PRE[b] + 1:SLOT_PRE[b] + 1 + cnt[b]], device) for b in range(3)])
        var = m.step_varlen([0, 1, 2], more, list(cnt), Y=_nan((6, D), device)).cpu().numpy()
        # slot 0 holds 7 rows: two beams on its first 6, each fed row 6 -- beam 1 through slot 3's slab
        m.beam_begin([0, 3], [0], [6], 2)
        row6 = _dev(np.concatenate([seq[0][6:7], seq[0][6:7]]), device)
        beam = m.step_batch_indirect([0, 3], [0, 0], row6, pos=[6, 6], Y=_nan((2, D), device)).cpu().numpy()
    finally:
        m.close()
    want = [_oracle(which, seq[b], tables, enc[b]) for b in range(3)]
    r0 = 0
    for b in range(3):
        p = SLOT_PRE[b]
        assert_bits_equal(one[b:b + 1], want[b][p:p + 1], f"step_batch, slot {b} at position {p}")
        assert_bits_equal(var[r0:r0 + cnt[b]], want[b][p + 1:p + 1 + cnt[b]], f"step_varlen, slot {b}")
        r0 += cnt[b]
    for q in range(2):
        assert_bits_equal(beam[q:q + 1], want[0][6:7], f"step_batch_indirect, beam {q}")


def test_forward_batch_restarts_the_position_per_sequence(qg, oracle, device):
    X = _x()
    m = _make(qg, "enc-post", device, max_rows=16)
    try:
        tables = _tables(m)
        got = m.forward_batch(_dev(np.concatenate([X, X[2:6], X[8:9]]), device), [9, 4, 1],
                              Y=_nan((14, D), device)).cpu().numpy()
        single = [m.forward(_dev(x, device)).cpu().numpy() for x in (X, X[2:6], X[8:9])]
    finally:
        m.close()
    for b, (lo, hi) in enumerate(((0, 9), (9, 13), (13, 14))):
        assert_bits_equal(got[lo:hi], single[b], f"sequence {b} against its own forward")
        assert_bits_equal(got[lo:hi], _oracle("enc-post", (X, X[2:6], X[8:9])[b], tables), f"sequence {b} against the oracle")


# ---- the tables as weights --------------------------------------------------------------------------------------------
def test_a_replaced_table_changes_the_output_and_resets_the_slots(qg, oracle, device):
    X = _dev(_x(), device)
    rng = np.random.default_rng(8)
    ang = rng.uniform(0.0, 6.0, (MAX_SEQ, DK // 2))
    cos, sin = np.cos(ang).astype(F), np.sin(ang).astype(F)   # another table altogether: every angle its own
    m = _make(qg, "only-pre", device, n_slots=2)
    try:
        before = m.forward(X).cpu().numpy()
        m.begin_slot(0)
        m.begin_slot(1)
        m.step_slot(0, X[:3].contiguous())
        assert [m.slot_filled(0), m.slot_filled(1)] == [3, 0]
        # cos from a strided bf16-free fp32 view (every second column of a wider parent), sin contiguous
        wide = torch.full((MAX_SEQ, DK), float("nan"), device=device)
        wide[:, ::2] = _dev(cos, device)
        m.set_weight(0, qg.KIND_ROPE_COS, wide[:, ::2])
        assert m.slot_filled(0) is None and m.slot_filled(1) is None
        with pytest.raises(qg.QGemmError) as ei:
            m.step_slot(0, X[3:4].contiguous(), pos=3)
        assert ei.value.code == INVALID
        m.set_weight(0, qg.KIND_ROPE_SIN, _dev(sin, device))
        tables = _tables(m)
        assert_bits_equal(tables[0], cos, "cos as loaded")
        assert_bits_equal(tables[1], sin, "sin as loaded")
        got = m.forward(X).cpu().numpy()
        m.begin_slot(1)
        steps = m.step_slot(1, X[:5].contiguous()).cpu().numpy()
        L, v, stream = qg.load(), torch.zeros(MAX_SEQ * DK, device=device), qg._stream(device)
        for kind in (28, 29):   # block 0, head 0 alone; kind 30 does not exist
            assert L.qgemm_model_set_weight(m._h, 1, kind, 0, v.data_ptr(), 0, DK // 2, 1, stream) == INVALID
            assert L.qgemm_model_set_weight(m._h, 0, kind, 1, v.data_ptr(), 0, DK // 2, 1, stream) == INVALID
        assert L.qgemm_model_set_weight(m._h, 0, 30, 0, v.data_ptr(), 0, DK // 2, 1, stream) == INVALID
    finally:
        m.close()
    want = _oracle("only-pre", _x(), (cos, sin))
    assert_bits_equal(got, want, "forward on the replaced tables")
    assert_bits_equal(steps, want[:5], "a step after the slot's next begin")
    assert np.abs(got - before).max() > 1e-3


def test_table_kinds_are_refused_without_rope(qg, oracle, device):
    L = qg.load()
    models = [qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ, arch="standard"), qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ),
              qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, 0, decoder_only=True, arch="standard", norm_first=True)]
    v, stream = torch.zeros(MAX_SEQ * DK, device=device), qg._stream(device)
    c, s, r, h = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
    try:
        for m in models:
            for kind in (28, 29):
                assert L.qgemm_model_set_weight(m._h, 0, kind, 0, v.data_ptr(), 0, DK // 2, 1, stream) == INVALID
                assert L.qgemm_model_weight_shape(m._h, kind, None, None, None) == INVALID
            assert L.qgemm_model_rope_tables(m._h, ctypes.byref(c), ctypes.byref(s), ctypes.byref(r),
                                             ctypes.byref(h)) == INVALID
            with pytest.raises(qg.QGemmError):
                m.rope_tables()
    finally:
        for m in models:
            m.close()


def test_captured_forward_replays_the_same_bits(qg, oracle, device):
    L = qg.load()
    X = _dev(_x(), device)
    m = _make(qg, "only-pre", device)
    try:
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        Y = _nan((SEQ, D), device)
        with torch.cuda.stream(s):
            eager = m.forward(X).cpu().numpy()   # also the warm-up
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                assert L.qgemm_decoder_forward(m._h, X.data_ptr(), None, Y.data_ptr(), SEQ, 0, s.cuda_stream) == 0
        for i in range(2):
            Y.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_bits_equal(Y.cpu().numpy(), eager, f"replay {i}")
    finally:
        m.close()
