"""The standard post-LN architecture on the device (qgemm_model_create with QGEMM_ARCH_STANDARD), bit for
bit against tests/standard_oracle.py through every path of the stack: forward, forward_batch, begin + step, step_batch,
step_varlen, generate and its captured replay; the creator's reference architecture against the older creators; the new
weight kinds; load_torch_layer.  d_model 64, 4 heads, d_ff 200, 2 blocks, heavy-tailed weights plus random vectors."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attn_oracle
import standard_oracle as SO
import weights_oracle as WO_
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

D, H, DFF, BLOCKS, SEQ, ENC_SEQ = 64, 4, 200, 2, 9, 7
SEED = 303
INVALID = 1
F = np.float32


def _dev(a, device, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(device).to(dtype)   # (a copy: the cached inputs are read-only)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _load(model, W, device, vec_dtype=torch.float32):
    for (block, kind), a in W.items():
        model.set_weight(block, kind, _dev(a, device, vec_dtype if a.ndim == 1 else torch.float32))


@functools.lru_cache(maxsize=None)
def _weights(cross):
    return SO.standard_weights(D, H, DFF, BLOCKS, 17, cross=cross)


@functools.lru_cache(maxsize=None)
def _inputs():
    return O.uniform((SEQ, D), 11), O.uniform((ENC_SEQ, D), 12)


@functools.lru_cache(maxsize=None)
def _expected(which, activation="relu"):
    """The oracle chains on the weight set, once per process: "enc", "dec" or "dec_causal"."""
    X, enc = _inputs()
    if which == "enc":
        out = SO.encoder_forward_std(X, _weights(False), D, H, BLOCKS, activation)
    else:
        out = SO.decoder_forward_std(X, enc, _weights(True), D, H, BLOCKS, which == "dec_causal", activation)
    out.flags.writeable = False
    return out


def _encoder(qg, activation="relu", **kw):
    return qg.Encoder(D, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED, arch="standard", activation=activation, **kw)


def _decoder(qg, activation="relu", causal=True, kv_cache=True, **kw):
    return qg.Decoder(D, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=SEED, causal=causal, kv_cache=kv_cache,
                      arch="standard", activation=activation, **kw)


# ---- forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["relu", "gelu_tanh"])
def test_encoder_forward(qg, oracle, device, activation):
    enc = _encoder(qg, activation)
    try:
        _load(enc, _weights(False), device)
        got = enc.forward(_dev(_inputs()[0], device), Y=_nan((SEQ, D), device)).cpu().numpy()
    finally:
        enc.close()
    assert_bits_equal(got, _expected("enc", activation), f"Encoder.forward {activation}")


def test_fresh_standard_stack_has_the_documented_vectors(qg, oracle, device):
    """At creation: the matrices and b1, b2 of the seed as on the reference architecture, b = +0, gamma = 1, beta = +0."""
    W = WO_.seeded_weights(D, H, DFF, BLOCKS, SEED)
    for i in range(BLOCKS):
        for kind in SO.ENCODER_VECTOR_KINDS:
            W[i, kind] = np.ones(D, F) if kind in SO.GAMMA_KINDS else np.zeros(D, F)
    enc = _encoder(qg)
    try:
        for kind in SO.ENCODER_VECTOR_KINDS:
            assert_bits_equal(enc.bias(1, kind).cpu().numpy(), W[1, kind], f"kind {kind} at creation")
        got = enc.forward(_dev(_inputs()[0], device)).cpu().numpy()
        info = enc.info()
    finally:
        enc.close()
    assert_bits_equal(got, SO.encoder_forward_std(_inputs()[0], W, D, H, BLOCKS), "forward of a fresh standard stack")
    assert (info["arch"], info["activation"], info["cross"], info["d_ff"], info["seed"]) == (1, 0, 0, DFF, SEED)
    assert info["ln_eps"] == float(F(1e-5)) and info["size"] == ctypes.sizeof(qg.ModelDesc)


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
def test_decoder_forward(qg, oracle, device, causal):
    X, enc = (_dev(v, device) for v in _inputs())
    dec = _decoder(qg, causal=causal, kv_cache=False)
    try:
        _load(dec, _weights(True), device)
        got = dec.forward(X, enc, Y=_nan(X.shape, device)).cpu().numpy()
    finally:
        dec.close()
    assert_bits_equal(got, _expected("dec_causal" if causal else "dec"), "Decoder.forward")


# ---- cached steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["relu", "gelu_tanh"])
def test_begin_and_steps_equal_the_causal_forward(qg, oracle, device, activation):
    X, enc = (_dev(v, device) for v in _inputs())
    dec = _decoder(qg, activation)
    try:
        _load(dec, _weights(True), device)
        dec.begin(enc)
        outs = [dec.step(X[0:5], Y=_nan((5, D), device)), dec.step(X[5:6], Y=_nan((1, D), device)),
                dec.step(X[6:7], Y=_nan((1, D), device))]
        got = torch.cat(outs).cpu().numpy()
        assert dec.filled == 7
        # forward on the cached decoder: the prefix property on the device, forward(X[:n]) == forward(X)[:n]
        part = dec.forward(X[:4].contiguous(), enc).cpu().numpy()
    finally:
        dec.close()
    want = _expected("dec_causal", activation)
    assert_bits_equal(got, want[:7], "begin + steps 5, 1, 1")
    assert_bits_equal(part, want[:4], "forward(X[:4])")


SLOT_ENC, SLOT_PRE = (7, 5, 3), (4, 0, 2)


@functools.lru_cache(maxsize=None)
def _slot_seq(b):
    X, enc = O.uniform((6, D), 40 + b), O.uniform((SLOT_ENC[b], D), 50 + b)
    X.flags.writeable = enc.flags.writeable = False
    return X, enc


@functools.lru_cache(maxsize=None)
def _slot_expected(b, rows):
    """The causal forward of sequence b's first `rows` rows."""
    X, enc = _slot_seq(b)
    return SO.decoder_forward_std(X[:rows], enc, _weights(True), D, H, BLOCKS, True)


def test_step_batch_equals_every_slots_own_step(qg, oracle, device):
    dec = _decoder(qg, n_slots=3)
    try:
        _load(dec, _weights(True), device)
        alone = []
        for b in range(3):
            X, enc = (_dev(v, device) for v in _slot_seq(b))
            dec.begin_slot(b, enc)
            if SLOT_PRE[b]:
                dec.step_slot(b, X[:SLOT_PRE[b]].contiguous())
            alone.append(dec.step_slot(b, X[SLOT_PRE[b]:SLOT_PRE[b] + 1].contiguous()))
        new = torch.cat([_dev(_slot_seq(b)[0][SLOT_PRE[b]:SLOT_PRE[b] + 1], device) for b in range(3)])
        got = dec.step_batch([0, 1, 2], new, pos=list(SLOT_PRE), Y=_nan((3, D), device))   # the same rows again
        assert torch.equal(got.view(torch.int32), torch.cat(alone).view(torch.int32)), "step_batch against step_slot"
        got = got.cpu().numpy()
    finally:
        dec.close()
    for b in range(3):
        assert_bits_equal(got[b:b + 1], _slot_expected(b, SLOT_PRE[b] + 1)[-1:], f"slot {b} against the oracle")


def test_step_varlen_mixes_a_prefill_and_a_decoding_row(qg, oracle, device):
    dec = _decoder(qg, n_slots=2, max_rows=16)
    try:
        _load(dec, _weights(True), device)
        X0, enc0 = (_dev(v, device) for v in _slot_seq(0))
        X2, enc2 = (_dev(v, device) for v in _slot_seq(2))
        dec.begin_slot(0, enc0)
        dec.begin_slot(1, enc2)
        dec.step_slot(1, X2[:3].contiguous())
        got = dec.step_varlen([0, 1], torch.cat([X0[:4], X2[3:4]]), [4, 1], Y=_nan((5, D), device)).cpu().numpy()
        assert [dec.slot_filled(0), dec.slot_filled(1)] == [4, 4]
    finally:
        dec.close()
    assert_bits_equal(got[:4], _slot_expected(0, 4), "the prefill's rows")
    assert_bits_equal(got[4:], _slot_expected(2, 4)[-1:], "the decoding row")


def test_indirect_beam_steps_equal_each_beams_own_forward(qg, oracle, device):
    """The copy-free beam search's calls on a post-LN GELU stack: a 2-row prompt in slot 0, beam_begin of two beams on
    it, step_batch_indirect, beam_reindex (both beams continue beam 1), step_batch_indirect again.  Every output row is
    the last row of the causal forward on that beam's own prefix."""
    X, enc = _slot_seq(0)
    new1, new2 = O.uniform((2, D), 71), O.uniform((2, D), 72)
    dec = _decoder(qg, "gelu_tanh", n_slots=3)
    try:
        _load(dec, _weights(True), device)
        dec.begin_slot(0, _dev(enc, device))
        dec.step_slot(0, _dev(X[:2], device))
        dec.beam_begin([0, 1], [0], [2], 2)
        y1 = dec.step_batch_indirect([0, 1], [0, 0], _dev(new1, device), pos=[2, 2], Y=_nan((2, D), device)).cpu().numpy()
        dec.beam_reindex([0, 1], torch.tensor([1, 1], dtype=torch.int32, device=device), [3], 2)
        y2 = dec.step_batch_indirect([0, 1], [0, 0], _dev(new2, device), pos=[3, 3], Y=_nan((2, D), device)).cpu().numpy()
    finally:
        dec.close()
    for q in range(2):
        for got, prefix in ((y1, [X[:2], new1[q:q + 1]]), (y2, [X[:2], new1[1:2], new2[q:q + 1]])):
            want = SO.decoder_forward_std(np.concatenate(prefix), enc, _weights(True), D, H, BLOCKS, True, "gelu_tanh")
            assert_bits_equal(got[q:q + 1], want[-1:], f"beam {q} at position {len(want) - 1}")


def test_forward_batch_of_two_lengths(qg, oracle, device):
    X = _inputs()[0]
    enc = _encoder(qg, "gelu_tanh", max_rows=16)
    try:
        _load(enc, _weights(False), device)
        got = enc.forward_batch(_dev(np.concatenate([X, X[2:7]]), device), [9, 5], Y=_nan((14, D), device)).cpu().numpy()
    finally:
        enc.close()
    assert_bits_equal(got[:9], _expected("enc", "gelu_tanh"), "sequence 0")
    assert_bits_equal(got[9:], SO.encoder_forward_std(X[2:7], _weights(False), D, H, BLOCKS, "gelu_tanh"), "sequence 1")


# ---- generate ---------------------------------------------------------------------------------------------------------
VOCAB, N_NEW = 50, 3


def _head(qg, device):
    E, P = O.uniform((VOCAB, D), 601), O.uniform((SEQ, D), 602, -0.1, 0.1)
    Wv, bias = O.uniform((D, VOCAB), 603), O.uniform((VOCAB,), 604, -0.05, 0.05)
    return qg.Head(qg.pack_b(_dev(Wv, device)), VOCAB, _dev(bias, device), _dev(E, device), _dev(P, device), max_rows=8)


def _prefill(dec, device):
    for b in range(3):
        X, enc = (_dev(v, device) for v in _slot_seq(b))
        dec.begin_slot(b, enc)
        if SLOT_PRE[b]:
            dec.step_slot(b, X[:SLOT_PRE[b]].contiguous())


def test_generate_equals_the_python_loop_and_replays(qg, oracle, device):
    L = qg.load()
    dec, loop, head = _decoder(qg, "gelu_tanh", n_slots=3), _decoder(qg, "gelu_tanh", n_slots=3), _head(qg, device)
    ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    try:
        _load(dec, _weights(True), device)
        _load(loop, _weights(True), device)
        tin = torch.tensor([7, 49, 0], dtype=torch.int32, device=device)
        _prefill(loop, device)
        tok, rows, hidden = tin, [], None
        for t in range(N_NEW):
            pos = [SLOT_PRE[b] + t for b in range(3)]
            emb = head.embed(tok, pos)
            hidden = loop.step_batch([0, 1, 2], emb, pos=pos)
            if t == 0:
                first_emb, first_hidden = emb.cpu().numpy(), hidden.cpu().numpy()
            tok = head.next_tokens(hidden)
            rows.append(tok.cpu().numpy())
        want = np.stack(rows)
        # the loop's first step against the oracle: the hidden row of each sequence's prefix + its embedded token
        for b in range(3):
            whole = np.concatenate([_slot_seq(b)[0][:SLOT_PRE[b]], first_emb[b:b + 1]])
            ref = SO.decoder_forward_std(whole, _slot_seq(b)[1], _weights(True), D, H, BLOCKS, True, "gelu_tanh")[-1:]
            assert_bits_equal(first_hidden[b:b + 1], ref, f"step 0 of slot {b} against the oracle")
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        out = torch.full((N_NEW, 3), -1, dtype=torch.int32, device=device)
        with torch.cuda.stream(s):
            _prefill(dec, device)
            eager = dec.generate(head, [0, 1, 2], tin, N_NEW, pos=list(SLOT_PRE)).cpu().numpy()   # also the warm-up
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = L.qgemm_decoder_generate(dec._h, head._h, 3, ints([0, 1, 2]), tin.data_ptr(), N_NEW,
                                              ints(list(SLOT_PRE)), out.data_ptr(), s.cuda_stream)
                assert rc == 0
        assert np.array_equal(eager, want), f"generate against the Python-driven loop:\n{eager}\n{want}"
        for i in range(2):
            out.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), f"replay {i}"
    finally:
        head.close()
        dec.close()
        loop.close()


# ---- the creator's reference architecture is the older creators' --------------------------------------------------------
def _model(qg, cls, **kw):
    """A handle from qgemm_model_create with arch = REFERENCE, wrapped as an Encoder / Decoder object."""
    d = dict(size=ctypes.sizeof(qg.ModelDesc), cross=int(cls is qg.Decoder), d_model=D, n_heads=H, d_ff=DFF,
             n_blocks=BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ if cls is qg.Decoder else 0, seed=SEED, flags=0, n_slots=0,
             max_rows=0, arch=qg.QGEMM_ARCH_REFERENCE, activation=qg.QGEMM_ACT_RELU, ln_eps=0.0)
    d.update(kw)
    desc, h = qg.ModelDesc(**d), ctypes.c_void_p()
    assert qg.load().qgemm_model_create(ctypes.byref(desc), ctypes.byref(h)) == 0
    m = object.__new__(cls)
    m._h, m.d_model, m.n_heads, m.d_ff, m.n_blocks, m.max_seq, m.arch = h, D, H, DFF, BLOCKS, SEQ, "reference"
    m.n_slots = max(1, d["n_slots"])
    return m


def _packed_bytes(model, cross):
    out = []
    for i in range(BLOCKS):
        for which in range(7 if cross else 4):
            p = model.packed_weight(i, which)
            out += [p.scale.view(torch.int32).clone(), p.q_raw.clone()]
        out += [model.bias(i, 5).view(torch.int32), model.bias(i, 7).view(torch.int32)]
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_reference_arch_encoder_is_the_old_creators(qg, oracle, device):
    X = _dev(_inputs()[0], device)
    old, new = qg.Encoder(D, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED), _model(qg, qg.Encoder)
    try:
        assert _same(_packed_bytes(old, False), _packed_bytes(new, False)), "the same seeded weights, byte for byte"
        ya, yb = old.forward(X).cpu().numpy(), new.forward(X).cpu().numpy()
        assert new.info()["arch"] == 0 and old.info()["arch"] == 0 and old.info()["seed"] == SEED
    finally:
        old.close()
        new.close()
    assert_bits_equal(yb, ya, "forward")
    assert_bits_equal(yb, attn_oracle.encoder_forward_ref(_inputs()[0], D, H, DFF, BLOCKS, SEED), "the seeded oracle")


@pytest.mark.parametrize("flags,n_slots", [(0, 0), (1, 0), (9, 1), (9, 3)])
def test_reference_arch_decoder_is_the_old_creators(qg, oracle, device, flags, n_slots):
    X, enc = (_dev(v, device) for v in _inputs())
    old = qg.Decoder(D, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=SEED, causal=bool(flags & 1),
                     kv_cache=bool(flags & 8), n_slots=max(1, n_slots))
    new = _model(qg, qg.Decoder, flags=flags, n_slots=n_slots)
    try:
        assert _same(_packed_bytes(old, True), _packed_bytes(new, True)), "the same seeded weights, byte for byte"
        assert_bits_equal(new.forward(X, enc).cpu().numpy(), old.forward(X, enc).cpu().numpy(), "forward")
        info = new.info()
        assert (info["flags"], info["n_slots"], info["cross"], info["max_enc_seq"]) == (flags, max(1, n_slots), 1, ENC_SEQ)
        if flags & 8:
            for m in (old, new):
                m.begin_slot(n_slots - 1 if n_slots else 0, enc)
            a = old.step_slot(max(1, n_slots) - 1, X[:3].contiguous(), pos=0)
            b = new.step_slot(max(1, n_slots) - 1, X[:3].contiguous(), pos=0)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a cached step"
    finally:
        old.close()
        new.close()


# ---- the new kinds ------------------------------------------------------------------------------------------------------
def test_bf16_sources_for_the_new_kinds(qg, oracle, device):
    W = dict(_weights(True))
    for key, a in W.items():
        if a.ndim == 1:
            W[key] = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    X, enc = (_dev(v, device) for v in _inputs())
    a, b = _decoder(qg, kv_cache=False), _decoder(qg, kv_cache=False)
    try:
        _load(a, W, device)
        _load(b, W, device, vec_dtype=torch.bfloat16)
        for i in range(BLOCKS):
            for kind in SO.DECODER_VECTOR_KINDS + (5, 7):
                assert torch.equal(a.bias(i, kind).view(torch.int32), b.bias(i, kind).view(torch.int32)), (i, kind)
                assert_bits_equal(a.bias(i, kind).cpu().numpy(), W[i, kind], f"block {i} kind {kind} as loaded")
        ya, yb = a.forward(X, enc).cpu().numpy(), b.forward(X, enc).cpu().numpy()
        assert a.weight_shape(qg.KIND_BK) == (1, D, 1) and a.weight_shape(qg.KIND_BE2) == (1, D, 1)
    finally:
        a.close()
        b.close()
    assert_bits_equal(yb, ya, "forward after the bf16 load")
    assert_bits_equal(ya, SO.decoder_forward_std(*_inputs(), W, D, H, BLOCKS, True), "against the oracle")


def test_setting_a_gamma_resets_every_slot(qg, oracle, device):
    X, enc = (_dev(v, device) for v in _inputs())
    W = _weights(True)
    dec = _decoder(qg, n_slots=2)
    try:
        _load(dec, W, device)
        dec.begin_slot(0, enc)
        dec.begin_slot(1, enc)
        dec.step_slot(0, X[0:3].contiguous())
        assert [dec.slot_filled(0), dec.slot_filled(1)] == [3, 0]
        dec.set_weight(1, qg.KIND_G2, _dev(W[1, SO.G2], device))
        assert dec.slot_filled(0) is None and dec.slot_filled(1) is None
        with pytest.raises(qg.QGemmError) as ei:
            dec.step_slot(0, X[3:4].contiguous(), pos=0)
        assert ei.value.code == INVALID
        dec.begin_slot(1, enc)
        got = dec.step_slot(1, X[0:5].contiguous(), Y=_nan((5, D), device)).cpu().numpy()
    finally:
        dec.close()
    assert_bits_equal(got, _expected("dec_causal")[:5], "a step after the slot's next begin")


def test_new_kinds_are_refused_where_the_model_lacks_them(qg, oracle, device):
    L = qg.load()
    ref_enc = qg.Encoder(D, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED)
    ref_dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=SEED)
    std_enc, std_dec = _encoder(qg), _decoder(qg)
    v = torch.zeros(D, device=device)
    stream = qg._stream(device)
    p, n = ctypes.c_void_p(), ctypes.c_int()

    def set_(model, kind, head=0):
        return L.qgemm_model_set_weight(model._h, 0, kind, head, v.data_ptr(), 0, D, 1, stream)

    try:
        for model in (ref_enc, ref_dec):
            for kind in range(12, 27):
                assert set_(model, kind) == INVALID, kind
                assert L.qgemm_model_weight_shape(model._h, kind, None, None, None) == INVALID, kind
                assert L.qgemm_model_bias(model._h, 0, kind, ctypes.byref(p), ctypes.byref(n)) == INVALID, kind
        for kind in range(12, 20):
            assert set_(std_enc, kind) == 0 and set_(std_dec, kind) == 0, kind
            assert set_(std_enc, kind, head=1) == INVALID, kind
        for kind in range(20, 26):
            assert set_(std_enc, kind) == INVALID and set_(std_dec, kind) == 0, kind
            assert L.qgemm_model_bias(std_enc._h, 0, kind, ctypes.byref(p), ctypes.byref(n)) == INVALID, kind
        for model in (std_enc, std_dec):
            assert set_(model, 26) == INVALID and set_(model, -1) == INVALID
        assert L.qgemm_model_bias(std_dec._h, 0, 3, ctypes.byref(p), ctypes.byref(n)) == INVALID   # a matrix
        for model in (ref_enc, std_enc):
            with pytest.raises(ValueError):
                model.load_torch_layer(0, torch.nn.TransformerDecoderLayer(D, H, DFF))
    finally:
        for m in (ref_enc, ref_dec, std_enc, std_dec):
            m.close()


# ---- torch layers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder,activation", [(False, "gelu_tanh"), (True, "relu")], ids=["encoder-gelu", "decoder-relu"])
def test_load_torch_layer(qg, oracle, device, decoder, activation):
    """The layers, inputs and the recorded quantization bound of tests/test_standard_host.py (d_ff 128): forward after
    load_torch_layer is the oracle chain on the layers' tensors bit for bit, and torch's own output within the bound;
    on the decoder the cached steps give the same rows."""
    import test_standard_host as TH
    layers = TH._torch_layers(decoder, activation)
    W = SO.torch_layer_weights(layers, H)
    X = TH._rows(TH.SEQ, D, 21) / F(3.0)
    enc = TH._rows(TH.ENC_SEQ, D, 22) / F(3.0) if decoder else None
    mk = dict(arch="standard", activation=activation, seed=SEED)
    model = (qg.Decoder(D, H, TH.DFF, TH.LAYERS, max_seq=TH.SEQ, max_enc_seq=TH.ENC_SEQ, causal=True, kv_cache=True, **mk)
             if decoder else qg.Encoder(D, H, TH.DFF, TH.LAYERS, max_seq=TH.SEQ, **mk))
    try:
        for i, layer in enumerate(layers):
            model.load_torch_layer(i, layer)
        Xd = _dev(X, device)
        if decoder:
            encd = _dev(enc, device)
            got = model.forward(Xd, encd).cpu().numpy()
            model.begin(encd)
            steps = torch.cat([model.step(Xd[:5].contiguous()), model.step(Xd[5:6].contiguous()),
                               model.step(Xd[6:].contiguous())]).cpu().numpy()
            assert_bits_equal(steps, got, "begin + steps 5, 1, 3 against forward")
        else:
            got = model.forward(Xd).cpu().numpy()
        bad = type(layers[0])(D, H, dim_feedforward=TH.DFF, norm_first=True)
        with pytest.raises(ValueError):
            model.load_torch_layer(0, bad)
        with pytest.raises(ValueError):
            model.load_torch_layer(0, type(layers[0])(D, H, dim_feedforward=TH.DFF + 8))
        with pytest.raises(ValueError):
            model.load_torch_layer(0, type(layers[0])(2 * D, H, dim_feedforward=TH.DFF))
    finally:
        model.close()
    assert_bits_equal(got, TH._chain(W, X, enc, activation, None), "forward against the oracle chain")
    err = TH._rel_fro(got, TH._torch_forward(layers, X, enc))
    assert err <= 2 * TH.QUANT_MEASURED[decoder, activation], f"relative Frobenius error against torch {err:.3e}"
