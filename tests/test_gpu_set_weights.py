"""GPU check of caller-supplied weights on Encoder and Decoder (qgemm_model_set_weight): a stack loaded
with another seed's draws IS that seed's stack, byte for byte; heavy-tailed weights against tests/weights_oracle.py bit
for bit; bf16 [out, in] sources equal the widened fp32 [in, out] load; the decoder's slots go back to "not begun"; one
tensor changes its own columns alone; every refusal.  d_model 48 / 3 heads (d_k 16: aligned windows) and d_model 40 / 5
heads (d_k 8: windows that share 16-row groups), d_ff 72, 2 blocks."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attn_oracle
import weights_oracle as WO_
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

CFGS = ((48, 3), (40, 5))
DFF, BLOCKS, SEQ, ENC_SEQ = 72, 2, 9, 7
SEED_A, SEED_B = 101, 202
INVALID = 1


def _dev(a, device, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).to(dtype)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _load(model, W, device, dtype=torch.float32, layout="kn"):
    """Every tensor of the weight set through set_weight; "nk": as [out, in] (the per-head kinds [n_heads, d_k, d])."""
    for (block, kind), a in W.items():
        t = _dev(a, device, dtype)
        if layout == "nk" and t.dim() >= 2:
            t = t.transpose(-1, -2).contiguous()
        model.set_weight(block, kind, t, layout=layout)


def _packed_bytes(model, cross):
    """(scale region, q region) of every packed weight of every block, and the biases."""
    out = []
    for i in range(BLOCKS):
        for which in range(7 if cross else 4):
            p = model.packed_weight(i, which)
            out += [p.scale.view(torch.int32).clone(), p.q_raw.clone()]
        out += [model.bias(i, 5).view(torch.int32), model.bias(i, 7).view(torch.int32)]
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _seed_draws(qg, d, H, seed, cross, device):
    """The draws of `seed` made on the device: qgemm_fill_uniform at encoder_weight_seed with the documented bounds."""
    dk = d // H
    bk, bd, bf = attn_oracle.init_bound(dk), attn_oracle.init_bound(d), attn_oracle.init_bound(DFF)
    bound = {3: 1.0, 11: 1.0, 4: bd, 5: bd, 6: bf, 7: bf}
    W = {}
    for i in range(BLOCKS):
        for kind in (WO_.DECODER_KINDS if cross else WO_.ENCODER_KINDS):
            shape = WO_.weight_shape(kind, d, H, DFF)
            t = torch.empty(shape, device=device)
            if kind in WO_.HEAD_KINDS:
                for h in range(H):
                    qg.fill_uniform(t[h], qg.encoder_weight_seed(seed, i, kind, h), -bk, bk)
            else:
                qg.fill_uniform(t, qg.encoder_weight_seed(seed, i, kind, 0), -bound[kind], bound[kind])
            W[i, kind] = t
    return W


@functools.lru_cache(maxsize=None)
def _inputs(d):
    return O.uniform((SEQ, d), 11), O.uniform((ENC_SEQ, d), 12)


@functools.lru_cache(maxsize=None)
def _heavy(d, H, cross):
    return WO_.heavy_tailed_weights(d, H, DFF, BLOCKS, 17, cross=cross)


@functools.lru_cache(maxsize=None)
def _expected(d, H, which):
    """The oracle on the heavy-tailed set, once per process: "enc", "dec" or "dec_causal"."""
    X, enc = _inputs(d)
    if which == "enc":
        out = WO_.encoder_forward_w(X, _heavy(d, H, False), d, H, BLOCKS)
    else:
        out = WO_.decoder_forward_w(X, enc, _heavy(d, H, True), d, H, BLOCKS, causal=which == "dec_causal")
    out.flags.writeable = False
    return out


# ---- twin: seed B loaded with seed A's draws is seed A's stack --------------------------------------------------------
@pytest.mark.parametrize("d,H", CFGS)
def test_encoder_twin(qg, oracle, device, d, H):
    X = _dev(_inputs(d)[0], device)
    a, b = qg.Encoder(d, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED_A), qg.Encoder(d, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED_B)
    try:
        assert not _same(_packed_bytes(a, False), _packed_bytes(b, False))
        b.load_weights(_seed_draws(qg, d, H, SEED_A, False, device))
        assert _same(_packed_bytes(a, False), _packed_bytes(b, False)), "packed weights and biases, byte for byte"
        ya, yb = a.forward(X, Y=_nan(X.shape, device)), b.forward(X, Y=_nan(X.shape, device))
        assert_bits_equal(yb.cpu().numpy(), ya.cpu().numpy(), "twin forward")
        assert_bits_equal(yb.cpu().numpy(), attn_oracle.encoder_forward_ref(_inputs(d)[0], d, H, DFF, BLOCKS, SEED_A),
                          "twin forward against the seeded oracle")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("d,H", CFGS)
def test_decoder_twin(qg, oracle, device, d, H):
    X, enc = (_dev(v, device) for v in _inputs(d))
    mk = lambda seed: qg.Decoder(d, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=seed)  # noqa: E731
    a, b = mk(SEED_A), mk(SEED_B)
    try:
        assert not _same(_packed_bytes(a, True), _packed_bytes(b, True))
        b.load_weights(_seed_draws(qg, d, H, SEED_A, True, device))
        assert _same(_packed_bytes(a, True), _packed_bytes(b, True)), "packed weights and biases, byte for byte"
        ya, yb = a.forward(X, enc, Y=_nan(X.shape, device)), b.forward(X, enc, Y=_nan(X.shape, device))
        assert_bits_equal(yb.cpu().numpy(), ya.cpu().numpy(), "twin forward")
    finally:
        a.close()
        b.close()


# ---- heavy-tailed weights against the weight-array oracle -----------------------------------------------------------
@pytest.mark.parametrize("d,H", CFGS)
def test_encoder_forward_on_heavy_tailed_weights(qg, oracle, device, d, H):
    X = _dev(_inputs(d)[0], device)
    enc = qg.Encoder(d, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED_B)
    try:
        _load(enc, _heavy(d, H, False), device)
        got = enc.forward(X, Y=_nan(X.shape, device)).cpu().numpy()
    finally:
        enc.close()
    assert_bits_equal(got, _expected(d, H, "enc"), "Encoder.forward")


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("d,H", CFGS)
def test_decoder_forward_on_heavy_tailed_weights(qg, oracle, device, d, H, causal):
    X, enc = (_dev(v, device) for v in _inputs(d))
    dec = qg.Decoder(d, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=SEED_B, causal=causal)
    try:
        _load(dec, _heavy(d, H, True), device)
        got = dec.forward(X, enc, Y=_nan(X.shape, device)).cpu().numpy()
    finally:
        dec.close()
    assert_bits_equal(got, _expected(d, H, "dec_causal" if causal else "dec"), "Decoder.forward")


@pytest.mark.parametrize("d,H", CFGS)
def test_decoder_steps_on_heavy_tailed_weights(qg, oracle, device, d, H):
    """begin, a prefill step of 5 rows, two one-row steps: rows 0 .. 6 of the causal forward (its prefix property)."""
    X, enc = (_dev(v, device) for v in _inputs(d))
    dec = qg.Decoder(d, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=SEED_B, causal=True, kv_cache=True)
    try:
        _load(dec, _heavy(d, H, True), device)
        dec.begin(enc)
        outs = [dec.step(X[0:5], Y=_nan((5, d), device)), dec.step(X[5:6], Y=_nan((1, d), device)),
                dec.step(X[6:7], Y=_nan((1, d), device))]
        got = torch.cat(outs).cpu().numpy()
        assert dec.filled == 7
    finally:
        dec.close()
    assert_bits_equal(got, _expected(d, H, "dec_causal")[:7], "begin + steps 5, 1, 1")


# ---- bf16 [out, in] sources ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", CFGS)
def test_bf16_out_in_sources_equal_the_widened_load(qg, oracle, device, d, H):
    W = {key: torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy() for key, a in _heavy(d, H, True).items()}
    X, enc = (_dev(v, device) for v in _inputs(d))
    mk = lambda: qg.Decoder(d, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=SEED_B)  # noqa: E731
    a, b = mk(), mk()
    try:
        _load(a, W, device)                                        # fp32 [in, out]
        _load(b, W, device, dtype=torch.bfloat16, layout="nk")     # bf16 [out, in]
        assert _same(_packed_bytes(a, True), _packed_bytes(b, True)), "packed weights and biases, byte for byte"
        ya, yb = a.forward(X, enc, Y=_nan(X.shape, device)), b.forward(X, enc, Y=_nan(X.shape, device))
        assert_bits_equal(yb.cpu().numpy(), ya.cpu().numpy(), "forward after the bf16 [out, in] load")
        assert_bits_equal(ya.cpu().numpy(), WO_.decoder_forward_w(*_inputs(d), W, d, H, BLOCKS), "against the oracle")
    finally:
        a.close()
        b.close()


# ---- a decoder with caches: every slot back to "not begun" ----------------------------------------------------------
def _slot_state(qg, dec, slot):
    e, f = ctypes.c_int(-1), ctypes.c_int(-1)
    assert qg.load().qgemm_decoder_slot_state(dec._h, slot, ctypes.byref(e), ctypes.byref(f)) == 0
    return e.value, f.value


@pytest.mark.parametrize("d,H", CFGS)
def test_set_weight_resets_every_slot(qg, oracle, device, d, H):
    X, enc = (_dev(v, device) for v in _inputs(d))
    W = _heavy(d, H, True)
    dec = qg.Decoder(d, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=SEED_B, causal=True, kv_cache=True,
                     n_slots=4)
    try:
        _load(dec, W, device)
        dec.begin_slot(0, enc)
        dec.begin_slot(1, enc)
        dec.step_slot(0, X[0:3])
        dec.step_slot(1, X[0:2])
        dec.beam_begin([2, 3], [0], [3], beams=2)   # slots 2 and 3 carry the beam search's flag
        assert [dec.slot_filled(s) for s in range(4)] == [3, 2, 3, 3]
        dec.set_weight(1, attn_oracle.WK, _dev(W[1, attn_oracle.WK][2], device), head=2)
        for s in range(4):
            assert _slot_state(qg, dec, s) == (0, 0) and dec.slot_filled(s) is None
        with pytest.raises(qg.QGemmError) as ei:
            dec.step_slot(0, X[3:4], pos=0)
        assert ei.value.code == INVALID
        with pytest.raises(qg.QGemmError):
            dec.step_batch([0, 1], X[0:2], pos=[0, 0])
        with pytest.raises(qg.QGemmError):
            dec.step_batch_indirect([2, 3], [0, 0], X[0:2], pos=[3, 3])
        with pytest.raises(qg.QGemmError):
            dec.beam_begin([2, 3], [0], [0], beams=2)   # the prompt slot is not begun either
        dec.begin_slot(1, enc)
        got = dec.step_slot(1, X[0:5], Y=_nan((5, d), device)).cpu().numpy()
        assert dec.slot_filled(1) == 5 and dec.slot_filled(0) is None
    finally:
        dec.close()
    assert_bits_equal(got, _expected(d, H, "dec_causal")[:5], "step after the slot's next begin")


# ---- one tensor changed: its columns alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype", [("kn", torch.float32), ("nk", torch.bfloat16)], ids=["f32-kn", "bf16-nk"])
@pytest.mark.parametrize("d,H", CFGS)
def test_one_tensor_changes_its_own_columns_alone(qg, oracle, device, d, H, layout, dtype):
    dk = d // H
    new = torch.from_numpy(_heavy(d, H, False)[0, attn_oracle.WK][1]).to(torch.bfloat16).to(torch.float32)
    enc = qg.Encoder(d, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED_A)
    try:
        before = enc.packed_weight(0, qg.WEIGHT_WQKV)
        scale0, q0 = before.scale.clone(), before.q.clone()
        others = _packed_bytes(enc, False)[2:]
        src = new.to(device).to(dtype)
        enc.set_weight(0, qg.KIND_WK, src.t().contiguous() if layout == "nk" else src, head=1, layout=layout)
        after = enc.packed_weight(0, qg.WEIGHT_WQKV)
        c0 = d + dk
        keep = torch.ones(after.rows_pad, dtype=torch.bool, device=device)
        keep[c0:c0 + dk] = False
        assert torch.equal(after.scale.view(torch.int32)[keep], scale0.view(torch.int32)[keep])
        assert torch.equal(after.q[keep], q0[keep]), "every other packed row of wqkv is unchanged"
        ref = qg.pack_b(new.to(device))   # the tensor packed alone: its columns' scales and rows
        assert torch.equal(after.scale.view(torch.int32)[c0:c0 + dk], ref.scale.view(torch.int32)[:dk])
        assert torch.equal(after.q[c0:c0 + dk], ref.q[:dk])
        assert _same(_packed_bytes(enc, False)[2:], others), "every other weight and bias is unchanged"
    finally:
        enc.close()


# ---- refusals, all before any launch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", CFGS)
def test_refusals(qg, oracle, device, d, H):
    L = qg.load()
    enc = qg.Encoder(d, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED_A)
    dec = qg.Decoder(d, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=SEED_A, causal=True, kv_cache=True)
    W = torch.zeros((d, d), device=device)
    try:
        def set_(model, block=0, kind=0, head=0, ptr=W.data_ptr(), dtype=0, sh=d, sw=1):
            return L.qgemm_model_set_weight(model._h, block, kind, head, ptr, dtype, sh, sw, _stream)

        _stream = qg._stream(device)
        assert set_(enc) == 0 and set_(dec) == 0   # the baseline of the refusals below is accepted
        before = _packed_bytes(enc, False) + _packed_bytes(dec, True)
        dec.begin(_dev(_inputs(d)[1], device))
        for kind in (8, 9, 10, 11, 12, -1):
            assert set_(enc, kind=kind) == INVALID, kind
        for kind in (12, -1):
            assert set_(dec, kind=kind) == INVALID, kind
        for model in (enc, dec):
            assert set_(model, block=BLOCKS) == INVALID and set_(model, block=-1) == INVALID
            assert set_(model, head=H) == INVALID and set_(model, head=-1) == INVALID
            assert set_(model, kind=3, head=1) == INVALID and set_(model, kind=5, head=1) == INVALID
            assert set_(model, ptr=None) == INVALID
            assert set_(model, dtype=2) == INVALID and set_(model, dtype=-1) == INVALID
            assert set_(model, sh=-1) == INVALID and set_(model, sw=-1) == INVALID
        assert set_(dec, kind=8, head=H) == INVALID
        assert dec.filled == 0, "a refused call leaves the slots alone"
        assert _same(_packed_bytes(enc, False) + _packed_bytes(dec, True), before), "and writes nothing"
        i, p = ctypes.c_int(), ctypes.c_void_p()
        assert L.qgemm_model_weight_shape(enc._h, 8, None, None, None) == INVALID
        assert L.qgemm_model_weight_shape(enc._h, -1, None, None, None) == INVALID
        assert L.qgemm_model_packed_weight(enc._h, 0, 4, ctypes.byref(p), None, None) == INVALID
        assert L.qgemm_model_packed_weight(dec._h, 0, 7, ctypes.byref(p), None, None) == INVALID
        assert L.qgemm_model_packed_weight(dec._h, BLOCKS, 0, ctypes.byref(p), None, None) == INVALID
        assert L.qgemm_model_packed_weight(dec._h, 0, 0, None, None, None) == INVALID
        assert L.qgemm_model_bias(enc._h, 0, 4, ctypes.byref(p), ctypes.byref(i)) == INVALID
        assert L.qgemm_model_bias(enc._h, -1, 5, ctypes.byref(p), ctypes.byref(i)) == INVALID
        assert enc.weight_shape(1) == (d, d // H, H) and enc.weight_shape(6) == (DFF, d, 1)
        assert dec.weight_shape(10) == (d, d // H, H) and dec.weight_shape(7) == (1, d, 1)
    finally:
        enc.close()
        dec.close()
