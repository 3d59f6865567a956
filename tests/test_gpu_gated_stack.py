"""RMSNorm and the gated FFN in the stack (norm="rms", gated_ffn=True) on the device, bit for bit against
tests/gated_oracle.py.  d_model 64, 4 heads, d_ff 200 (the W3 window then starts at column 200, no multiple of 16),
2 blocks, max_seq 16, 9 rows; one forward at d_ff 50 (k % 4 != 0: the scalar pack inside the stack).  A RoPE model's
oracle runs on the tables READ BACK from the model, so no bit-exact check rests on two libms agreeing."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gated_oracle as GO
import head_oracle
import prenorm_oracle as PO
import stack_cases as C
import standard_oracle as SO
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

D, H, DFF, BLOCKS, MAX_SEQ, SEQ, ENC_SEQ = 64, 4, 200, 2, 16, 9, 7
DK = D // H
SEED = 404
INVALID = 1
F = np.float32
BETAS = (SO.BE1, SO.BE2, SO.BE3, PO.BEF)
# model: (family, arch as the oracle reads it, activation); "llama" is 0x6F01 on the device
MODELS = {
    "enc-post-rms-reglu": ("encoder", 0x6001, "relu"),
    "dec-pre-rms-geglu": ("decoder", 0x6301, "gelu_tanh"),
    "llama": ("only", GO.LLAMA, "silu"),
    "enc-post-rms-gelu": ("encoder", 0x2001, "gelu_tanh"),      # RMSNORM alone
    "enc-post-ln-swiglu": ("encoder", 0x4001, "silu"),          # GATED_FFN alone
    "only-pre-ln-geglu": ("only", 0x4701, "gelu_tanh"),
}


def _dev(a, device, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(device).to(dtype)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


@functools.lru_cache(maxsize=None)
def _weights(cross, dff=DFF):
    return GO.gated_weights(D, H, dff, BLOCKS, 23, cross=cross)


@functools.lru_cache(maxsize=None)
def _x(seed=11, rows=SEQ):
    X = O.uniform((rows, D), seed)
    X.flags.writeable = False
    return X


def _has(arch, kind):
    """whether a model of `arch` has tensor `kind` of the weight set"""
    if kind in (GO.W3, GO.B3):
        return bool(arch & GO.GATED_FFN)
    if kind in BETAS and arch & GO.RMSNORM:
        return False
    return kind < PO.GF or bool(arch & GO.FINAL_NORM)


def _make(qg, which, device, dff=DFF, load=True, **kw):
    """the model, with every tensor of its weight set loaded"""
    family, arch, act = MODELS[which]
    keys = dict(seed=SEED, arch="standard", activation=act, norm_first=bool(arch & GO.NORM_FIRST),
                final_norm=bool(arch & GO.FINAL_NORM), rope=bool(arch & GO.ROPE),
                norm="rms" if arch & GO.RMSNORM else "layer", gated_ffn=bool(arch & GO.GATED_FFN), **kw)
    if family == "encoder":
        m = qg.Encoder(D, H, dff, BLOCKS, MAX_SEQ, **keys)
    elif family == "decoder":
        m = qg.Decoder(D, H, dff, BLOCKS, MAX_SEQ, ENC_SEQ, causal=True, kv_cache=True, **keys)
    else:
        m = qg.Decoder(D, H, dff, BLOCKS, MAX_SEQ, 0, causal=True, kv_cache=True, decoder_only=True, **keys)
    if load:
        for (block, kind), a in _weights(family == "decoder", dff).items():
            if _has(arch, kind):
                m.set_weight(block, kind, _dev(a, device))
    return m


def _tables(m, which):
    return tuple(t.cpu().numpy() for t in m.rope_tables()) if MODELS[which][1] & GO.ROPE else None


def _oracle(which, X, tables, enc=None, dff=DFF):
    family, arch, act = MODELS[which]
    return GO.forward(X, enc, _weights(family == "decoder", dff), D, H, BLOCKS, arch, family != "encoder", act, 1e-5, None,
                      tables)


def _forward(m, which, X, enc=None, **kw):
    return m.forward(X, **kw) if MODELS[which][0] == "encoder" else m.forward(X, enc, **kw)


# ---- (a), (b) forward on every combination --------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(MODELS))
def test_forward(qg, oracle, device, which):
    family, arch, act = MODELS[which]
    X = _dev(_x(), device)
    enc = _dev(_x(12, ENC_SEQ), device) if family == "decoder" else None
    m = _make(qg, which, device)
    try:
        tables = _tables(m, which)
        info = m.info()
        got = _forward(m, which, X, enc, Y=_nan((SEQ, D), device)).cpu().numpy()
        assert_bits_equal(X.cpu().numpy(), _x(), "forward leaves X unchanged")
        if family != "encoder":
            m.begin(enc)
            steps = torch.cat([m.step(X[0:5]), m.step(X[5:6]), m.step(X[6:9])]).cpu().numpy()
            assert_bits_equal(steps, got, "steps 5, 1, 3 against forward")
    finally:
        m.close()
    assert info["arch"] == arch and info["activation"] == qg.ACTIVATIONS[act]
    want = _oracle(which, _x(), tables, None if enc is None else _x(12, ENC_SEQ))
    assert_bits_equal(got, want, f"forward, {which}")
    # each bit is there: the same weights without it are another function
    for bit in (GO.RMSNORM, GO.GATED_FFN):
        if arch & bit:
            other = GO.forward(_x(), None if enc is None else _x(12, ENC_SEQ), _weights(family == "decoder"), D, H, BLOCKS,
                               arch & ~bit, family != "encoder", "relu" if act == "silu" else act, 1e-5, None, tables)
            assert np.abs(other - want).max() > 1e-3


def test_forward_with_the_scalar_pack(qg, oracle, device):
    """d_ff = 50: the up half starts at float 50 of a row of 100, so the gated pack goes float by float"""
    X = _dev(_x(), device)
    m = _make(qg, "llama", device, dff=50)
    try:
        tables = _tables(m, "llama")
        got = m.forward(X, None, Y=_nan((SEQ, D), device)).cpu().numpy()
        assert m.packed_weight(0, qg.WEIGHT_W1).rows == 100 and m.weight_shape(qg.KIND_W3) == (D, 50, 1)
    finally:
        m.close()
    assert_bits_equal(got, _oracle("llama", _x(), tables, dff=50), "forward at d_ff = 50")


# ---- (c) the cached, batched and generating calls on the Llama model -------------------------------------------------
SLOT_PRE = (4, 0, 2)


def test_llama_steps_equal_forward(qg, oracle, device):
    """step_slot row by row and in chunks, step_batch of 3 slots (one row each at positions 4, 0, 2), then step_varlen
    (rows 2, 1, 3 behind them), and a step_varlen prefill of three fresh slots: every row is its sequence's forward row."""
    seq = [_x(40 + b) for b in range(3)]
    m = _make(qg, "llama", device, n_slots=4, max_rows=16)
    try:
        tables = _tables(m, "llama")
        fwd = m.forward(_dev(seq[0], device)).cpu().numpy()
        m.begin_slot(3)
        rows = torch.cat([m.step_slot(3, _dev(seq[0][i:i + 1], device), Y=_nan((1, D), device)) for i in range(SEQ)]).cpu().numpy()
        again = m.step_slot(3, _dev(seq[0][3:9], device), pos=3).cpu().numpy()   # a rewind
        for b in range(3):
            m.begin_slot(b)
            if SLOT_PRE[b]:
                m.step_slot(b, _dev(seq[b][:SLOT_PRE[b]], device))
        new = torch.cat([_dev(seq[b][SLOT_PRE[b]:SLOT_PRE[b] + 1], device) for b in range(3)])
        one = m.step_batch([0, 1, 2], new, Y=_nan((3, D), device)).cpu().numpy()
        cnt = (2, 1, 3)
        more = torch.cat([_dev(seq[b][SLOT_PRE[b] + 1:SLOT_PRE[b] + 1 + cnt[b]], device) for b in range(3)])
        var = m.step_varlen([0, 1, 2], more, list(cnt), Y=_nan((6, D), device)).cpu().numpy()
        pre = (5, 2, 7)
        for b in range(3):
            m.begin_slot(b)
        prefill = m.step_varlen([0, 1, 2], torch.cat([_dev(seq[b][:pre[b]], device) for b in range(3)]), list(pre),
                                Y=_nan((sum(pre), D), device)).cpu().numpy()
        assert [m.slot_filled(b) for b in range(3)] == list(pre)
    finally:
        m.close()
    want = [_oracle("llama", seq[b], tables) for b in range(3)]
    assert_bits_equal(fwd, want[0], "forward")
    assert_bits_equal(rows, want[0], "step_slot row by row against forward")
    assert_bits_equal(again, want[0][3:], "a rewind to position 3")
    r0 = p0 = 0
    for b in range(3):
        p = SLOT_PRE[b]
        assert_bits_equal(one[b:b + 1], want[b][p:p + 1], f"step_batch, slot {b} at position {p}")
        assert_bits_equal(var[r0:r0 + cnt[b]], want[b][p + 1:p + 1 + cnt[b]], f"step_varlen, slot {b}")
        assert_bits_equal(prefill[p0:p0 + pre[b]], want[b][:pre[b]], f"step_varlen prefill, slot {b}")
        r0 += cnt[b]
        p0 += pre[b]


def test_llama_generate_against_the_greedy_chain(qg, oracle, device):
    E, P, Wh, bias = C.head_tables()
    pre, tin, n_new = (4, 0, 2), (7, 28, 49), 4
    m = _make(qg, "llama", device, n_slots=3)
    head = qg.Head(qg.pack_b(_dev(Wh, device)), C.VOCAB, _dev(bias, device), _dev(E, device), _dev(P, device), max_rows=8)
    try:
        tables = _tables(m, "llama")
        for b in range(3):
            m.begin_slot(b)
            if pre[b]:
                m.step_slot(b, _dev(_x(60 + b)[:pre[b]], device))
        out = torch.full((n_new, 3), -7, dtype=torch.int32, device=device)
        m.generate(head, [0, 1, 2], torch.tensor(tin, dtype=torch.int32, device=device), n_new, tokens_out=out)
        got = out.cpu().numpy()
        assert [m.slot_filled(b) for b in range(3)] == [p + n_new for p in pre]
    finally:
        head.close()
        m.close()
    fwd = lambda X, enc: _oracle("llama", X, tables)  # noqa: E731
    want = np.array([head_oracle.generate_ref(_x(60 + b)[:pre[b]], None, tin[b], n_new, E, Wh, bias, P, (D, H, DFF, BLOCKS),
                                              None, forward=fwd) for b in range(3)], np.int32).T
    assert np.array_equal(got, want), f"generate against generate_ref\n{got}\n{want}"


def test_captured_llama_forward_replays_the_same_bits(qg, oracle, device):
    L = qg.load()
    X = _dev(_x(), device)
    m = _make(qg, "llama", device)
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


# ---- (d) set_weight of the new layout -------------------------------------------------------------------------------
def _bytes(p):
    return p.scale.view(torch.int32).clone(), p.q_raw.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_set_weight_packs_the_gate_and_up_windows(qg, oracle, device):
    """W1 and W3 from fp32 "kn" and from bf16 "nk" sources: the block's packed [W1 | W3] equals pack_b of the assembled
    matrix byte for byte, the other half keeps its bytes, b3 and gamma are copied, and every slot is reset."""
    rng = np.random.default_rng(5)
    W = _weights(False)
    m = _make(qg, "llama", device, n_slots=2)
    try:
        assert m.weight_shape(qg.KIND_W1) == (D, DFF, 1) == m.weight_shape(qg.KIND_W3)
        assert m.weight_shape(qg.KIND_B3) == (1, DFF, 1)
        whole = lambda w1, w3: _bytes(qg.pack_b(torch.cat([w1, w3], dim=1).contiguous()))  # noqa: E731
        w1, w3 = _dev(W[1, GO.W1], device), _dev(W[1, GO.W3], device)
        assert _same(_bytes(m.packed_weight(1, qg.WEIGHT_W1)), whole(w1, w3)), "as loaded by _make"
        other = _bytes(m.packed_weight(0, qg.WEIGHT_W1))
        w2_before = _bytes(m.packed_weight(1, qg.WEIGHT_W2))
        for kind in (qg.KIND_W3, qg.KIND_W1):
            # fp32 [in, out], every second column of a wider parent
            wide = _nan((D, 2 * DFF), device)
            new = _dev((rng.standard_normal((D, DFF)) * 0.3).astype(F), device)
            wide[:, ::2] = new
            m.begin_slot(0)
            m.step_slot(0, _dev(_x()[:3], device))
            m.set_weight(1, kind, wide[:, ::2])
            assert m.slot_filled(0) is None and m.slot_filled(1) is None, "the slots are reset"
            w1, w3 = (new, w3) if kind == qg.KIND_W1 else (w1, new)
            assert _same(_bytes(m.packed_weight(1, qg.WEIGHT_W1)), whole(w1, w3)), f"kind {kind} from fp32 kn"
            # bf16 [out, in]: the packed window is that of the widened values
            src = _dev((rng.standard_normal((DFF, D)) * 0.3).astype(F), device).to(torch.bfloat16)
            m.set_weight(1, kind, src, layout="nk")
            new = src.float().t().contiguous()
            w1, w3 = (new, w3) if kind == qg.KIND_W1 else (w1, new)
            assert _same(_bytes(m.packed_weight(1, qg.WEIGHT_W1)), whole(w1, w3)), f"kind {kind} from bf16 nk"
        assert _same(_bytes(m.packed_weight(0, qg.WEIGHT_W1)), other), "block 0 keeps its bytes"
        assert _same(_bytes(m.packed_weight(1, qg.WEIGHT_W2)), w2_before), "W2 keeps its bytes"
        # b3 and a gamma: the copy path, fp32 and bf16
        b1_before = m.bias(1, qg.KIND_B1)
        b3 = _dev((rng.standard_normal(DFF) * 0.2).astype(F), device).to(torch.bfloat16)
        m.begin_slot(1)
        m.set_weight(1, qg.KIND_B3, b3)
        assert m.slot_filled(1) is None
        assert torch.equal(m.bias(1, qg.KIND_B3), b3.float()) and torch.equal(m.bias(1, qg.KIND_B1), b1_before)
        g3 = _dev((1.0 + rng.standard_normal(D) * 0.2).astype(F), device)
        m.set_weight(1, qg.KIND_G3, g3)
        assert torch.equal(m.bias(1, qg.KIND_G3), g3)
        # and the forward runs on what was loaded
        tables = _tables(m, "llama")
        got = m.forward(_dev(_x(), device)).cpu().numpy()
    finally:
        m.close()
    W2 = dict(W)
    W2[1, GO.W1], W2[1, GO.W3] = w1.cpu().numpy(), w3.cpu().numpy()
    W2[1, GO.B3], W2[1, SO.G3] = b3.float().cpu().numpy(), g3.cpu().numpy()
    want = GO.forward(_x(), None, W2, D, H, BLOCKS, GO.LLAMA, True, "silu", 1e-5, None, tables)
    assert_bits_equal(got, want, "forward on the replaced tensors")


def test_seeded_creation_draws_w3_with_w1s_bound(qg, oracle, device):
    """W3 is the stream encoder_weight_seed(seed, block, 30, 0) at W1's bound, b3 = +0, beside the unchanged W1 and b1"""
    m = _make(qg, "llama", device, load=False)
    plain = qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ, seed=SEED, arch="standard")
    try:
        bound = float(F(1.0 / np.sqrt(float(D))))
        for i in range(BLOCKS):
            w1, w3 = torch.empty((D, DFF), device=device), torch.empty((D, DFF), device=device)
            qg.fill_uniform(w1, qg.encoder_weight_seed(SEED, i, qg.KIND_W1, 0), -bound, bound)
            qg.fill_uniform(w3, qg.encoder_weight_seed(SEED, i, qg.KIND_W3, 0), -bound, bound)
            got = m.packed_weight(i, qg.WEIGHT_W1)
            assert (got.rows, got.k) == (2 * DFF, D)
            assert _same(_bytes(got), _bytes(qg.pack_b(torch.cat([w1, w3], dim=1).contiguous())))
            assert _same(_bytes(plain.packed_weight(i, qg.WEIGHT_W1)), _bytes(qg.pack_b(w1)))
            assert torch.equal(m.bias(i, qg.KIND_B1), plain.bias(i, qg.KIND_B1))
            b3 = m.bias(i, qg.KIND_B3)
            assert b3.shape == (DFF,) and not b3.any() and not torch.signbit(b3).any()
    finally:
        m.close()
        plain.close()


# ---- (e) the kinds a model has ---------------------------------------------------------------------------------------
def test_kinds_are_refused_where_the_model_lacks_them(qg, oracle, device):
    L = qg.load()
    v, stream = torch.zeros(4 * D * DFF, device=device), qg._stream(device)
    p, n = ctypes.c_void_p(), ctypes.c_int()

    def refused(m, kind, block=0):
        assert L.qgemm_model_set_weight(m._h, block, kind, 0, v.data_ptr(), 0, DFF, 1, stream) == INVALID
        assert L.qgemm_model_weight_shape(m._h, kind, None, None, None) == INVALID
        assert L.qgemm_model_bias(m._h, block, kind, ctypes.byref(p), ctypes.byref(n)) == INVALID

    ungated = [qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ), qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ, arch="standard"),
               _make(qg, "enc-post-rms-gelu", device, load=False)]
    rms = [_make(qg, "llama", device, load=False), _make(qg, "dec-pre-rms-geglu", device, load=False),
           _make(qg, "enc-post-rms-gelu", device, load=False)]
    ln = _make(qg, "only-pre-ln-geglu", device, load=False)
    try:
        for m in ungated:
            refused(m, 30)
            refused(m, 31)
            assert m.packed_weight(0, qg.WEIGHT_W1).rows == DFF
        for m in rms:
            for kind in (17, 19, 25, 27):
                refused(m, kind)
            for kind in (16, 18):   # the gammas stay
                assert m.weight_shape(kind) == (1, D, 1) and torch.equal(m.bias(0, kind), torch.ones(D, device=device))
        assert rms[0].weight_shape(26) == (1, D, 1) == rms[1].weight_shape(24)
        for m in (rms[0], rms[1], ln):
            assert m.packed_weight(1, qg.WEIGHT_W1).rows == 2 * DFF and m.packed_weight(1, qg.WEIGHT_W1).k == D
            assert m.packed_weight(1, qg.WEIGHT_W2).rows == D and m.packed_weight(1, qg.WEIGHT_W2).k == DFF
            refused(m, 32)
            assert L.qgemm_model_set_weight(m._h, 0, 30, 1, v.data_ptr(), 0, DFF, 1, stream) == INVALID   # head 1
            assert L.qgemm_model_set_weight(m._h, BLOCKS, 30, 0, v.data_ptr(), 0, DFF, 1, stream) == INVALID
            assert L.qgemm_model_set_weight(m._h, 1, 30, 0, v.data_ptr(), 0, DFF, 1, stream) == 0        # every block's
        assert ln.weight_shape(19) == (1, D, 1) and ln.weight_shape(27) == (1, D, 1)   # a LayerNorm model keeps its betas
        for m in (rms[0], ln):
            with pytest.raises(ValueError):
                m.load_torch_layer(0, torch.nn.TransformerEncoderLayer(D, H, DFF))
            with pytest.raises(ValueError):
                m.load_torch_final_norm(torch.nn.LayerNorm(D))
    finally:
        for m in ungated + rms + [ln]:
            m.close()


# ---- (f) the older architectures beside the new ones ---------------------------------------------------------------------
def test_older_architectures_in_the_same_process_keep_their_bits(qg, oracle, device):
    X = _dev(_x(), device)
    llama = _make(qg, "llama", device)
    ref = qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ, seed=5)
    pre = qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ, seed=SEED, arch="standard", norm_first=True, final_norm=True,
                     activation="gelu_tanh")
    try:
        W = _weights(False)
        for (block, kind), a in W.items():
            if kind not in (GO.W3, GO.B3):
                pre.set_weight(block, kind, _dev(a, device))
        llama.forward(X)
        got_ref = ref.forward(X, Y=_nan((SEQ, D), device)).cpu().numpy()
        got_pre = pre.forward(X, Y=_nan((SEQ, D), device)).cpu().numpy()
        llama.forward(X)
    finally:
        for m in (llama, ref, pre):
            m.close()
    assert_bits_equal(got_ref, O.encoder_forward(_x(), D, H, DFF, BLOCKS, 5), "the default architecture")
    assert_bits_equal(got_pre, PO.encoder_forward_pre(_x(), W, D, H, BLOCKS, "gelu_tanh", True), "arch 0x301")
