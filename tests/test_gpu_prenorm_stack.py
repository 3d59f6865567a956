"""The pre-LN architecture on the device (arch="standard", norm_first=True [, final_norm=True]), bit for bit
against tests/prenorm_oracle.py through every path of the stack: forward, forward_batch, begin + step, step_batch,
step_varlen, generate, a captured forward; the final norm's kinds; load_torch_layer / load_torch_final_norm.  d_model
64, 4 heads, d_ff 200, 2 blocks, heavy-tailed weights plus random vectors for every kind, 26 / 27 included."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import prenorm_oracle as PO
import standard_oracle as SO
import weights_oracle as WO_
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

D, H, DFF, BLOCKS, SEQ, ENC_SEQ = 64, 4, 200, 2, 9, 7
SEED = 404
INVALID = 1
F = np.float32


def _dev(a, device, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(device).to(dtype)   # (a copy: the cached inputs are read-only)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _load(model, W, device):
    """Every tensor of W the model has: a model without a final norm is not given kinds 26 / 27."""
    for (block, kind), a in W.items():
        if kind < PO.GF or model.final_norm:
            model.set_weight(block, kind, _dev(a, device))


@functools.lru_cache(maxsize=None)
def _weights(cross):
    return PO.prenorm_weights(D, H, DFF, BLOCKS, 23, cross=cross, final_norm=True)


@functools.lru_cache(maxsize=None)
def _inputs():
    return O.uniform((SEQ, D), 11), O.uniform((ENC_SEQ, D), 12)


@functools.lru_cache(maxsize=None)
def _expected(which, activation="relu", final_norm=True):
    """The oracle chains on the weight set, once per process: "enc", "dec" or "dec_causal"."""
    X, enc = _inputs()
    if which == "enc":
        out = PO.encoder_forward_pre(X, _weights(False), D, H, BLOCKS, activation, final_norm)
    else:
        out = PO.decoder_forward_pre(X, enc, _weights(True), D, H, BLOCKS, which == "dec_causal", activation, final_norm)
    out.flags.writeable = False
    return out


def _encoder(qg, activation="relu", final_norm=True, **kw):
    return qg.Encoder(D, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED, arch="standard", activation=activation,
                      norm_first=True, final_norm=final_norm, **kw)


def _decoder(qg, activation="relu", final_norm=True, causal=True, kv_cache=True, **kw):
    return qg.Decoder(D, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=SEED, causal=causal, kv_cache=kv_cache,
                      arch="standard", activation=activation, norm_first=True, final_norm=final_norm, **kw)


# ---- forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("final_norm", [True, False], ids=["lnf", "nolnf"])
@pytest.mark.parametrize("activation", ["relu", "gelu_tanh"])
def test_encoder_forward(qg, oracle, device, activation, final_norm):
    enc = _encoder(qg, activation, final_norm)
    try:
        _load(enc, _weights(False), device)
        X = _dev(_inputs()[0], device)
        got = enc.forward(X, Y=_nan((SEQ, D), device)).cpu().numpy()
        assert_bits_equal(X.cpu().numpy(), _inputs()[0], "forward leaves X unchanged")
    finally:
        enc.close()
    assert_bits_equal(got, _expected("enc", activation, final_norm), f"Encoder.forward {activation} lnf={final_norm}")


@pytest.mark.parametrize("final_norm", [True, False], ids=["lnf", "nolnf"])
@pytest.mark.parametrize("activation", ["relu", "gelu_tanh"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
def test_decoder_forward(qg, oracle, device, causal, activation, final_norm):
    X, enc = (_dev(v, device) for v in _inputs())
    dec = _decoder(qg, activation, final_norm, causal=causal, kv_cache=False)
    try:
        _load(dec, _weights(True), device)
        got = dec.forward(X, enc, Y=_nan(X.shape, device)).cpu().numpy()
        assert_bits_equal(X.cpu().numpy(), _inputs()[0], "forward leaves X unchanged")
        assert_bits_equal(enc.cpu().numpy(), _inputs()[1], "forward leaves enc_out unchanged")
        if causal:  # the prefix property on the device
            part = dec.forward(X[:4].contiguous(), enc).cpu().numpy()
            assert_bits_equal(part, got[:4], "forward(X[:4]) == forward(X)[:4]")
    finally:
        dec.close()
    assert_bits_equal(got, _expected("dec_causal" if causal else "dec", activation, final_norm), "Decoder.forward")


def test_fresh_model_has_the_documented_final_norm(qg, oracle, device):
    """At creation gamma_f = 1, beta_f = +0 and every other tensor is the post-LN creator's; arch reads back as given."""
    W = WO_.seeded_weights(D, H, DFF, BLOCKS, SEED)
    for i in range(BLOCKS):
        for kind in SO.ENCODER_VECTOR_KINDS:
            W[i, kind] = np.ones(D, F) if kind in SO.GAMMA_KINDS else np.zeros(D, F)
    W[0, PO.GF], W[0, PO.BEF] = np.ones(D, F), np.zeros(D, F)
    enc, plain = _encoder(qg), _encoder(qg, final_norm=False)
    try:
        assert_bits_equal(enc.bias(0, qg.KIND_GF).cpu().numpy(), W[0, PO.GF], "gamma_f at creation")
        assert_bits_equal(enc.bias(0, qg.KIND_BEF).cpu().numpy(), W[0, PO.BEF], "beta_f at creation")
        assert enc.weight_shape(qg.KIND_GF) == (1, D, 1) and enc.weight_shape(qg.KIND_BEF) == (1, D, 1)
        got = enc.forward(_dev(_inputs()[0], device)).cpu().numpy()
        info, info_plain = enc.info(), plain.info()
    finally:
        enc.close()
        plain.close()
    assert_bits_equal(got, PO.encoder_forward_pre(_inputs()[0], W, D, H, BLOCKS), "forward of a fresh pre-LN stack")
    assert (info["arch"], info_plain["arch"], info["activation"], info["cross"]) == (0x301, 0x101, 0, 0)
    assert info["size"] == ctypes.sizeof(qg.ModelDesc)


# ---- cached steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,final_norm", [("relu", True), ("gelu_tanh", False)])
def test_steps_equal_the_causal_forward(qg, oracle, device, activation, final_norm):
    X, enc = (_dev(v, device) for v in _inputs())
    want = _expected("dec_causal", activation, final_norm)
    dec = _decoder(qg, activation, final_norm)
    try:
        _load(dec, _weights(True), device)
        dec.begin(enc)
        rows = torch.cat([dec.step(X[i:i + 1].contiguous(), Y=_nan((1, D), device)) for i in range(SEQ)]).cpu().numpy()
        assert dec.filled == SEQ
        dec.begin(enc)
        chunks = torch.cat([dec.step(X[0:5], Y=_nan((5, D), device)), dec.step(X[5:6], Y=_nan((1, D), device)),
                            dec.step(X[6:9], Y=_nan((3, D), device))]).cpu().numpy()
        assert_bits_equal(X.cpu().numpy(), _inputs()[0], "steps leave X unchanged")
    finally:
        dec.close()
    assert_bits_equal(rows, want, "begin + steps row by row")
    assert_bits_equal(chunks, want, "begin + steps 5, 1, 3")


SLOT_ENC, SLOT_PRE = (7, 5, 3), (4, 0, 2)


@functools.lru_cache(maxsize=None)
def _slot_seq(b):
    X, enc = O.uniform((6, D), 40 + b), O.uniform((SLOT_ENC[b], D), 50 + b)
    X.flags.writeable = enc.flags.writeable = False
    return X, enc


@functools.lru_cache(maxsize=None)
def _slot_expected(b, rows, activation="relu"):
    """The causal forward of sequence b's first `rows` rows."""
    X, enc = _slot_seq(b)
    return PO.decoder_forward_pre(X[:rows], enc, _weights(True), D, H, BLOCKS, True, activation)


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
    """The copy-free beam search's calls on a pre-LN stack with the final norm: a 2-row prompt in slot 0, beam_begin of
    two beams on it, step_batch_indirect, beam_reindex (both beams continue beam 1), step_batch_indirect again.  Every
    output row is the last row of the causal forward on that beam's own prefix."""
    X, enc = _slot_seq(0)
    new1, new2 = O.uniform((2, D), 71), O.uniform((2, D), 72)
    dec = _decoder(qg, n_slots=3)
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
            want = PO.decoder_forward_pre(np.concatenate(prefix), enc, _weights(True), D, H, BLOCKS, True)
            assert_bits_equal(got[q:q + 1], want[-1:], f"beam {q} at position {len(want) - 1}")


def test_forward_batch_of_three_lengths(qg, oracle, device):
    X = _inputs()[0]
    W = _weights(False)
    enc = _encoder(qg, "gelu_tanh", max_rows=16)
    try:
        _load(enc, W, device)
        got = enc.forward_batch(_dev(np.concatenate([X, X[2:6], X[8:9]]), device), [9, 4, 1],
                                Y=_nan((14, D), device)).cpu().numpy()
    finally:
        enc.close()
    assert_bits_equal(got[:9], _expected("enc", "gelu_tanh"), "sequence 0")
    assert_bits_equal(got[9:13], PO.encoder_forward_pre(X[2:6], W, D, H, BLOCKS, "gelu_tanh"), "sequence 1")
    assert_bits_equal(got[13:], PO.encoder_forward_pre(X[8:9], W, D, H, BLOCKS, "gelu_tanh"), "sequence 2")


# ---- generate ---------------------------------------------------------------------------------------------------------
VOCAB, N_NEW = 50, 4


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


def test_generate_equals_the_python_loop(qg, oracle, device):
    dec, loop, head = _decoder(qg, "gelu_tanh", n_slots=3), _decoder(qg, "gelu_tanh", n_slots=3), _head(qg, device)
    try:
        _load(dec, _weights(True), device)
        _load(loop, _weights(True), device)
        tin = torch.tensor([7, 49, 0], dtype=torch.int32, device=device)
        _prefill(loop, device)
        tok, rows = tin, []
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
            ref = PO.decoder_forward_pre(whole, _slot_seq(b)[1], _weights(True), D, H, BLOCKS, True, "gelu_tanh")[-1:]
            assert_bits_equal(first_hidden[b:b + 1], ref, f"step 0 of slot {b} against the oracle")
        _prefill(dec, device)
        got = dec.generate(head, [0, 1, 2], tin, N_NEW, pos=list(SLOT_PRE)).cpu().numpy()
    finally:
        head.close()
        dec.close()
        loop.close()
    assert np.array_equal(got, want), f"generate against the Python-driven loop:\n{got}\n{want}"


def test_captured_forward_replays_the_same_bits(qg, oracle, device):
    L = qg.load()
    X, enc = (_dev(v, device) for v in _inputs())
    dec = _decoder(qg, "gelu_tanh", kv_cache=False)
    try:
        _load(dec, _weights(True), device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        Y = _nan((SEQ, D), device)
        with torch.cuda.stream(s):
            eager = dec.forward(X, enc).cpu().numpy()   # also the warm-up
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = L.qgemm_decoder_forward(dec._h, X.data_ptr(), enc.data_ptr(), Y.data_ptr(), SEQ, ENC_SEQ,
                                             s.cuda_stream)
                assert rc == 0
        assert_bits_equal(eager, _expected("dec_causal", "gelu_tanh"), "the eager forward")
        for i in range(2):
            Y.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_bits_equal(Y.cpu().numpy(), eager, f"replay {i}")
    finally:
        dec.close()


# ---- the final norm's kinds ---------------------------------------------------------------------------------------------
def test_setting_gamma_f_resets_every_slot(qg, oracle, device):
    X, enc = (_dev(v, device) for v in _inputs())
    W = _weights(True)
    dec = _decoder(qg, n_slots=2)
    try:
        _load(dec, W, device)
        dec.begin_slot(0, enc)
        dec.begin_slot(1, enc)
        dec.step_slot(0, X[0:3].contiguous())
        assert [dec.slot_filled(0), dec.slot_filled(1)] == [3, 0]
        dec.set_weight(0, qg.KIND_GF, _dev(W[0, PO.GF], device))
        assert dec.slot_filled(0) is None and dec.slot_filled(1) is None
        with pytest.raises(qg.QGemmError) as ei:
            dec.step_slot(0, X[3:4].contiguous(), pos=0)
        assert ei.value.code == INVALID
        dec.begin_slot(1, enc)
        got = dec.step_slot(1, X[0:5].contiguous(), Y=_nan((5, D), device)).cpu().numpy()
        assert_bits_equal(dec.bias(0, qg.KIND_GF).cpu().numpy(), W[0, PO.GF], "gamma_f as loaded")
        assert_bits_equal(dec.bias(0, qg.KIND_BEF).cpu().numpy(), W[0, PO.BEF], "beta_f as loaded")
    finally:
        dec.close()
    assert_bits_equal(got, _expected("dec_causal")[:5], "a step after the slot's next begin")


def test_final_norm_kinds_are_refused_where_the_model_lacks_them(qg, oracle, device):
    L = qg.load()
    no_lnf_enc, no_lnf_dec = _encoder(qg, final_norm=False), _decoder(qg, final_norm=False)
    lnf_enc, lnf_dec = _encoder(qg), _decoder(qg)
    post = qg.Encoder(D, H, DFF, BLOCKS, max_seq=SEQ, seed=SEED, arch="standard")
    v = torch.zeros(D, device=device)
    stream = qg._stream(device)
    p, n = ctypes.c_void_p(), ctypes.c_int()

    def set_(model, kind, block=0, head=0):
        return L.qgemm_model_set_weight(model._h, block, kind, head, v.data_ptr(), 0, D, 1, stream)

    try:
        for model in (no_lnf_enc, no_lnf_dec, post):
            for kind in (26, 27, 28):
                assert set_(model, kind) == INVALID, kind
                assert L.qgemm_model_weight_shape(model._h, kind, None, None, None) == INVALID, kind
                assert L.qgemm_model_bias(model._h, 0, kind, ctypes.byref(p), ctypes.byref(n)) == INVALID, kind
        for model in (lnf_enc, lnf_dec):
            for kind in (26, 27):
                assert set_(model, kind) == 0, kind
                assert set_(model, kind, block=1) == INVALID and set_(model, kind, head=1) == INVALID, kind
                assert L.qgemm_model_bias(model._h, 1, kind, ctypes.byref(p), ctypes.byref(n)) == INVALID, kind
                assert L.qgemm_model_bias(model._h, 0, kind, ctypes.byref(p), ctypes.byref(n)) == 0 and n.value == D
            assert set_(model, 28) == INVALID
        for kind in range(20, 26):   # an encoder still lacks the cross-attention's vectors
            assert set_(lnf_enc, kind) == INVALID and set_(lnf_dec, kind) == 0, kind
        with pytest.raises(ValueError):
            no_lnf_enc.load_torch_final_norm(torch.nn.LayerNorm(D))
        with pytest.raises(ValueError):
            post.load_torch_final_norm(torch.nn.LayerNorm(D))
        with pytest.raises(ValueError):
            lnf_enc.load_torch_final_norm(torch.nn.Linear(D, D))
        with pytest.raises(ValueError):
            lnf_enc.load_torch_final_norm(torch.nn.LayerNorm(D, eps=1e-6))
        with pytest.raises(ValueError):
            lnf_enc.load_torch_final_norm(torch.nn.LayerNorm(D, elementwise_affine=False))
        with pytest.raises(ValueError):
            lnf_enc.load_torch_final_norm(torch.nn.LayerNorm(2 * D))
    finally:
        for m in (no_lnf_enc, no_lnf_dec, lnf_enc, lnf_dec, post):
            m.close()


# ---- torch layers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder,activation,final_norm", [(False, "gelu_tanh", True), (True, "relu", True),
                                                           (True, "gelu_tanh", False)],
                         ids=["encoder-gelu-lnf", "decoder-relu-lnf", "decoder-gelu-nolnf"])
def test_load_torch_layers(qg, oracle, device, decoder, activation, final_norm):
    """The layers, inputs and the recorded quantization bound of tests/test_prenorm_host.py (d_ff 128): forward after
    load_torch_layer + load_torch_final_norm is the oracle chain on the layers' tensors bit for bit, and torch's own
    output within the bound; on the decoder the cached steps give the same rows."""
    import test_prenorm_host as TH
    layers, norm = TH.torch_model(decoder, activation, final_norm)
    W = PO.torch_model_weights(layers, H, norm)
    X, enc = TH.inputs(decoder)
    mk = dict(arch="standard", activation=activation, seed=SEED, norm_first=True, final_norm=final_norm)
    model = (qg.Decoder(D, H, TH.DFF, TH.LAYERS, max_seq=TH.SEQ, max_enc_seq=TH.ENC_SEQ, causal=True, kv_cache=True, **mk)
             if decoder else qg.Encoder(D, H, TH.DFF, TH.LAYERS, max_seq=TH.SEQ, **mk))
    post = qg.Encoder(D, H, TH.DFF, TH.LAYERS, max_seq=TH.SEQ, arch="standard", activation=activation)
    try:
        for i, layer in enumerate(layers):
            model.load_torch_layer(i, layer)
        if final_norm:
            model.load_torch_final_norm(norm)
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
        # a mismatched norm_first raises, both ways; so do the post-LN loader's other refusals
        with pytest.raises(ValueError):
            model.load_torch_layer(0, type(layers[0])(D, H, dim_feedforward=TH.DFF, norm_first=False))
        with pytest.raises(ValueError):
            post.load_torch_layer(0, torch.nn.TransformerEncoderLayer(D, H, dim_feedforward=TH.DFF, norm_first=True))
        with pytest.raises(ValueError):
            model.load_torch_layer(0, type(layers[0])(D, H, dim_feedforward=TH.DFF + 8, norm_first=True))
    finally:
        model.close()
        post.close()
    assert_bits_equal(got, TH.chain(W, X, enc, activation, final_norm, None), "forward against the oracle chain")
    err = TH.rel_fro(got, TH.torch_forward(layers, norm, X, enc))
    print(f"pre-LN {decoder, activation, final_norm}: relative Frobenius error against torch {err:.3e}")
    assert err <= 2 * TH.QUANT_MEASURED[decoder, activation, final_norm]
