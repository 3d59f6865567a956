"""Rotary embeddings in the stack at their edges, bit for bit against tests/rope_oracle.py.

Head sizes: inside a stack the rows rope.hip rotates are the QKV GEMM's, 3 d_model floats apart, so the kernel's pair
path runs only where d_k % 8 != 0 -- d_k 2, 6 and 12 here -- and its float4 path at d_k 8, 40 and 64; d_k 40 and 64
also cross attention_decode's d_k > 32 fork, and 64 is the batched step's limit.  The tables are loaded with a random
angle per entry, so a swapped cos / sin, a wrong pair partner or a wrong group stride shows at every size.

Full tables: 64 slots (kDecodeMaxBatch = kVarlenMaxSeqs, the whole position table of one rotation launch) at filled
lengths 0 .. 15, so the tables' first and last rows are both read, through step_varlen, step_batch and step_varlen
again; 64 sequences of 1 .. 16 rows through an encoder's forward_batch; three sequences through a cross-attention
decoder's step_varlen from position 0 and on to position max_seq - 1 (a decoder takes no forward_batch: the call is
refused, and its batched forward IS step_varlen at position 0).  Every row is compared with the same rows fed to one
slot alone, and a third of the sequences with the oracle on the tables read back from the model.

copy_slot: a fork after 5 rows and two diverging steps, each the oracle's row on its own 6 rows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import prenorm_oracle as PO
import rope_oracle as RO
import stack_cases as C
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

INVALID = 1
F = np.float32
D, H, DFF, BLOCKS, MAX_SEQ = C.D, C.H, C.DFF, C.BLOCKS, C.MAX_SEQ


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _tables(m):
    return tuple(t.cpu().numpy() for t in m.rope_tables())


# ---- head sizes -------------------------------------------------------------------------------------------------------
HS_HEADS, HS_DFF, HS_MAX_SEQ, HS_SEQ = 2, 72, 12, 9
HS_PRE = (4, 0, 2)


@functools.lru_cache(maxsize=None)
def _hs_weights(dk):
    return PO.prenorm_weights(HS_HEADS * dk, HS_HEADS, HS_DFF, 1, 31 + dk, cross=False, final_norm=False)


@functools.lru_cache(maxsize=None)
def _hs_tables(dk):
    """a random angle for every entry: no row is a rotation of its neighbour, no column a power of another"""
    ang = np.random.default_rng(900 + dk).uniform(0.0, 6.0, (HS_MAX_SEQ, dk // 2))
    return np.cos(ang).astype(F), np.sin(ang).astype(F)


def _hs_rows(dk, b):
    return O.uniform((HS_SEQ, HS_HEADS * dk), 2000 + 10 * dk + b)


def _hs_oracle(dk, X):
    return RO.decoder_only_forward(X, _hs_weights(dk), HS_HEADS * dk, HS_HEADS, 1, arch=1, causal=True, rope=_hs_tables(dk))


@pytest.mark.parametrize("dk", [2, 6, 12, 8, 40, 64])
def test_head_sizes(qg, oracle, device, dk):
    d = HS_HEADS * dk
    m = qg.Decoder(d, HS_HEADS, HS_DFF, 1, HS_MAX_SEQ, 0, seed=5, causal=True, kv_cache=True, n_slots=3,
                   decoder_only=True, arch="standard", rope=True)
    cos, sin = _hs_tables(dk)
    seqs = [np.ascontiguousarray(_hs_rows(dk, b)) for b in range(3)]
    try:
        for (block, kind), a in _hs_weights(dk).items():
            m.set_weight(block, kind, _dev(a, device))
        m.set_weight(0, qg.KIND_ROPE_COS, _dev(cos, device))
        m.set_weight(0, qg.KIND_ROPE_SIN, _dev(sin, device))
        got_c, got_s = _tables(m)
        assert_bits_equal(got_c, cos, "cos as loaded")
        assert_bits_equal(got_s, sin, "sin as loaded")
        X = _dev(seqs[0], device)
        fwd = m.forward(X, Y=_nan((HS_SEQ, d), device)).cpu().numpy()
        m.begin()
        chunks = torch.cat([m.step(X[0:5].contiguous(), Y=_nan((5, d), device)), m.step(X[5:6].contiguous(), Y=_nan((1, d), device)),
                            m.step(X[6:9].contiguous(), Y=_nan((3, d), device))]).cpu().numpy()
        again = m.step(X[3:9].contiguous(), pos=3, Y=_nan((6, d), device)).cpu().numpy()   # the cache holds rotated K
        for b in range(3):
            m.begin_slot(b)
            if HS_PRE[b]:
                m.step_slot(b, _dev(seqs[b][:HS_PRE[b]], device))
        new = torch.cat([_dev(seqs[b][HS_PRE[b]:HS_PRE[b] + 1], device) for b in range(3)])
        batch = m.step_batch([0, 1, 2], new, Y=_nan((3, d), device)).cpu().numpy()
    finally:
        m.close()
    assert_bits_equal(fwd, _hs_oracle(dk, seqs[0]), f"d_k {dk}: forward against the oracle")
    assert_bits_equal(chunks, fwd, f"d_k {dk}: steps 5, 1, 3 against forward")
    assert_bits_equal(again, fwd[3:], f"d_k {dk}: a rewind to position 3")
    for b in range(3):
        p = HS_PRE[b]
        assert_bits_equal(batch[b:b + 1], _hs_oracle(dk, seqs[b][:p + 1])[-1:], f"d_k {dk}: step_batch, slot {b} at {p}")


# ---- full tables ------------------------------------------------------------------------------------------------------
N_SLOTS = 64


def _load(m, name, device):
    W = C.weights(not C.MODELS[name].only)
    for block, kind in C.loaded_kinds(name):
        m.set_weight(block, kind, _dev(W[block, kind], device))


def _seq(b):
    return C.rows(2500 + b, MAX_SEQ)


def test_64_slots_from_position_0_to_the_last(qg, oracle, device):
    """Slot b is prefilled to length b % 16 by ONE step_varlen over the 60 non-empty slots in a permuted order, ONE
    step_batch appends a row to all 64 (a slot at 15 reads the tables' last row, a slot at 0 the first), ONE
    step_varlen appends 1 .. 3 more where they fit."""
    name = "only-pre-rope"
    kw = C.decoder_keywords(name)
    pre = [b % MAX_SEQ for b in range(N_SLOTS)]
    more = [min(1 + b % 3, MAX_SEQ - pre[b] - 1) for b in range(N_SLOTS)]
    total = [pre[b] + 1 + more[b] for b in range(N_SLOTS)]
    assert 0 in pre and MAX_SEQ - 1 in pre and max(total) == MAX_SEQ and {1, 2, 3} <= set(more)
    order = [b for b in np.random.default_rng(5).permutation(N_SLOTS).tolist() if pre[b]]
    late = [b for b in reversed(range(N_SLOTS)) if more[b]]
    m = qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, 0, seed=C.MODEL_SEED, causal=True, kv_cache=True, max_rows=512,
                   n_slots=N_SLOTS, **kw)
    one = qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, 0, seed=C.MODEL_SEED, causal=True, kv_cache=True, **kw)
    try:
        _load(m, name, device)
        _load(one, name, device)
        tables = _tables(m)
        for b in range(N_SLOTS):
            m.begin_slot(b)
        X1 = _dev(np.concatenate([_seq(b)[:pre[b]] for b in order]), device)
        Y1 = m.step_varlen(order, X1, [pre[b] for b in order], Y=_nan(tuple(X1.shape), device)).cpu().numpy()
        assert [m.slot_filled(b) for b in range(N_SLOTS)] == pre
        X2 = _dev(np.concatenate([_seq(b)[pre[b]:pre[b] + 1] for b in range(N_SLOTS)]), device)
        Y2 = m.step_batch(list(range(N_SLOTS)), X2, Y=_nan((N_SLOTS, D), device)).cpu().numpy()
        X3 = _dev(np.concatenate([_seq(b)[pre[b] + 1:total[b]] for b in late]), device)
        Y3 = m.step_varlen(late, X3, [more[b] for b in late], Y=_nan(tuple(X3.shape), device)).cpu().numpy()
        assert [m.slot_filled(b) for b in range(N_SLOTS)] == total
        alone = []
        for b in range(N_SLOTS):
            one.begin()
            alone.append(one.step(_dev(_seq(b)[:total[b]], device), Y=_nan((total[b], D), device)).cpu().numpy())
    finally:
        m.close()
        one.close()
    at1 = dict(zip(order, np.cumsum([0] + [pre[b] for b in order])))
    at3 = dict(zip(late, np.cumsum([0] + [more[b] for b in late])))
    fwd = C.forward(name, tables)
    for b in range(N_SLOTS):
        got = np.concatenate([Y1[at1[b]:at1[b] + pre[b]] if pre[b] else np.zeros((0, D), F), Y2[b:b + 1],
                              Y3[at3[b]:at3[b] + more[b]] if more[b] else np.zeros((0, D), F)])
        assert_bits_equal(got, alone[b], f"slot {b}: its rows against one slot alone")
        if b % 3 == 0:
            assert_bits_equal(got, fwd(_seq(b)[:total[b]], None), f"slot {b}: its rows against the oracle")


def test_encoder_forward_batch_of_64_sequences(qg, oracle, device):
    lens = [1 + 7 * b % MAX_SEQ for b in range(N_SLOTS)]
    assert {1, MAX_SEQ} <= set(lens)
    W = C.weights(False)
    enc = qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ, seed=C.MODEL_SEED, arch="standard", rope=True, max_rows=sum(lens))
    try:
        for (block, kind), a in W.items():
            if kind < PO.GF:
                enc.set_weight(block, kind, _dev(a, device))
        tables = _tables(enc)
        X = _dev(np.concatenate([_seq(b)[:lens[b]] for b in range(N_SLOTS)]), device)
        got = enc.forward_batch(X, lens, Y=_nan(tuple(X.shape), device)).cpu().numpy()
        single = [enc.forward(_dev(_seq(b)[:lens[b]], device), Y=_nan((lens[b], D), device)).cpu().numpy()
                  for b in range(N_SLOTS)]
    finally:
        enc.close()
    at = np.cumsum([0] + lens)
    for b in range(N_SLOTS):
        assert_bits_equal(got[at[b]:at[b + 1]], single[b], f"sequence {b} against its own forward")
        if b % 8 == 1 or lens[b] == MAX_SEQ:
            want = RO.encoder_forward_rope(_seq(b)[:lens[b]], W, D, H, BLOCKS, tables, 1)
            assert_bits_equal(got[at[b]:at[b + 1]], want, f"sequence {b} against the oracle")


def test_cross_decoder_varlen_pass_from_position_0_and_behind_it(qg, oracle, device):
    """The decoder's Varlen pass with its own positions (self_pos0): three sequences of 9, 4 and 1 rows from position 0
    in one step_varlen, then 7, 3 and 2 rows behind them, slot 0 up to position max_seq - 1.  Every sequence's rows are
    its own forward's and the oracle's."""
    name = "dec-post-rope"
    first, second = (9, 4, 1), (7, 3, 2)
    total = [a + b for a, b in zip(first, second)]
    m = qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, C.MAX_ENC, seed=C.MODEL_SEED, causal=True, kv_cache=True, max_rows=32,
                   n_slots=3, **C.decoder_keywords(name))
    try:
        _load(m, name, device)
        tables = _tables(m)
        encs = [_dev(C.enc_rows(name, b), device) for b in range(3)]
        X = _dev(np.concatenate([_seq(b)[:first[b]] for b in range(3)]), device)
        Y = _nan(tuple(X.shape), device)
        rc = qg.load().qgemm_encoder_forward_batch(m._h, X.data_ptr(), Y.data_ptr(), 3, (ctypes.c_int * 3)(*first),
                                                   qg._stream(device))
        assert rc == INVALID, "a decoder takes no forward_batch"
        torch.cuda.synchronize()
        assert torch.isnan(Y).all()
        for b in range(3):
            m.begin_slot(b, encs[b])
        Y1 = m.step_varlen([0, 1, 2], X, list(first), Y=Y).cpu().numpy()
        X2 = _dev(np.concatenate([_seq(b)[first[b]:total[b]] for b in (2, 0, 1)]), device)   # in another order
        Y2 = m.step_varlen([2, 0, 1], X2, [second[b] for b in (2, 0, 1)], Y=_nan(tuple(X2.shape), device)).cpu().numpy()
        assert [m.slot_filled(b) for b in range(3)] == total and total[0] == MAX_SEQ
        own = [m.forward(_dev(_seq(b)[:total[b]], device), encs[b]).cpu().numpy() for b in range(3)]
    finally:
        m.close()
    at1 = np.cumsum((0,) + first)
    at2 = dict(zip((2, 0, 1), np.cumsum([0] + [second[b] for b in (2, 0, 1)])))
    fwd = C.forward(name, tables)
    for b in range(3):
        got = np.concatenate([Y1[at1[b]:at1[b + 1]], Y2[at2[b]:at2[b] + second[b]]])
        assert_bits_equal(got, own[b], f"sequence {b} against its own forward")
        assert_bits_equal(got, fwd(_seq(b)[:total[b]], C.enc_rows(name, b)), f"sequence {b} against the oracle")


# ---- copy_slot --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.ROPE_NAMES)
def test_copy_slot_then_diverging_steps(qg, oracle, device, name):
    a, b = O.uniform((1, D), 81), O.uniform((1, D), 82)
    enc = C.enc_rows(name, 0)
    m = qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, C.max_enc_seq(name), seed=C.MODEL_SEED, causal=True, kv_cache=True,
                   n_slots=2, **C.decoder_keywords(name))
    try:
        _load(m, name, device)
        tables = _tables(m)
        m.begin_slot(0, None if enc is None else _dev(enc, device))
        m.step_slot(0, _dev(_seq(0)[:5], device))
        assert m.slot_filled(1) is None
        m.copy_slot(1, 0)
        assert m.slot_filled(1) == 5
        ya = m.step_slot(0, _dev(a, device), Y=_nan((1, D), device)).cpu().numpy()
        yb = m.step_slot(1, _dev(b, device), Y=_nan((1, D), device)).cpu().numpy()
    finally:
        m.close()
    fwd = C.forward(name, tables)
    for got, new in ((ya, a), (yb, b)):
        assert_bits_equal(got, fwd(np.concatenate([_seq(0)[:5], new]), enc)[-1:], f"{name}: a fork's own continuation")
    assert not np.array_equal(ya, yb)
