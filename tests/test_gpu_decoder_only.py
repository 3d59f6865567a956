"""Decoder-only stacks on the device (Decoder(..., 0, decoder_only=True), QGEMM_ARCH_DECODER_ONLY): the
encoder's blocks under the decoder's mask and caches, bit for bit against tests/rope_oracle.py's decoder_only_forward
through every call of the decoder family.  d_model 64, 4 heads, d_ff 200, 2 blocks, max_seq 16, 9 rows, heavy-tailed
weights plus random vectors for every kind the base architecture has."""
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

D, H, DFF, BLOCKS, MAX_SEQ, SEQ = 64, 4, 200, 2, 16, 9
SEED = 404
INVALID = 1
F = np.float32
# base: the keywords of the class call and the oracle's arch
BASES = {"reference": (dict(), 0), "post": (dict(arch="standard"), 1),
         "pre": (dict(arch="standard", norm_first=True, final_norm=True), 0x301)}


def _dev(a, device, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(device).to(dtype)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


@functools.lru_cache(maxsize=None)
def _weights():
    return PO.prenorm_weights(D, H, DFF, BLOCKS, 23, cross=False, final_norm=True)


def _load(model, base, device):
    """every tensor of the weight set that the base architecture has"""
    for (block, kind), a in _weights().items():
        if kind < 12 or (base != "reference" and (kind < PO.GF or base == "pre")):
            model.set_weight(block, kind, _dev(a, device))


@functools.lru_cache(maxsize=None)
def _x(seed=11, rows=SEQ):
    X = O.uniform((rows, D), seed)
    X.flags.writeable = False
    return X


@functools.lru_cache(maxsize=None)
def _expected(base, seed=11, rows=SEQ, causal=True):
    out = RO.decoder_only_forward(_x(seed)[:rows], _weights(), D, H, BLOCKS, arch=BASES[base][1], causal=causal)
    out.flags.writeable = False
    return out


def _decoder(qg, base, causal=True, kv_cache=True, **kw):
    return qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, 0, seed=SEED, causal=causal, kv_cache=kv_cache, decoder_only=True,
                      **BASES[base][0], **kw)


# ---- forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", sorted(BASES))
def test_unmasked_forward_is_the_encoders(qg, oracle, device, base):
    """flags = 0 and the default seed: the weights are drawn as the encoder's, so forward is Encoder.forward bit for bit."""
    dec = qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, 0, decoder_only=True, **BASES[base][0])
    enc = qg.Encoder(D, H, DFF, BLOCKS, MAX_SEQ, **BASES[base][0])
    try:
        X = _dev(_x(), device)
        got, want = dec.forward(X, Y=_nan((SEQ, D), device)), enc.forward(X)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not torch.isnan(got).any()
        info = dec.info()
        assert (info["cross"], info["max_enc_seq"], info["arch"]) == (1, 0, BASES[base][1] | 0x400)
    finally:
        dec.close()
        enc.close()


@pytest.mark.parametrize("base", sorted(BASES))
def test_causal_forward(qg, oracle, device, base):
    dec = _decoder(qg, base, kv_cache=False)
    try:
        _load(dec, base, device)
        X = _dev(_x(), device)
        got = dec.forward(X, Y=_nan((SEQ, D), device)).cpu().numpy()
        assert_bits_equal(X.cpu().numpy(), _x(), "forward leaves X unchanged")
        part = dec.forward(X[:4].contiguous()).cpu().numpy()
        assert_bits_equal(part, got[:4], "forward(X[:4]) == forward(X)[:4]")
    finally:
        dec.close()
    assert_bits_equal(got, _expected(base), f"Decoder.forward, decoder-only, {base}")


# ---- cached steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", sorted(BASES))
def test_steps_equal_the_causal_forward(qg, oracle, device, base):
    want = _expected(base)
    dec = _decoder(qg, base)
    try:
        _load(dec, base, device)
        X = _dev(_x(), device)
        assert dec.filled is None
        dec.begin()
        assert dec.filled == 0
        rows = torch.cat([dec.step(X[i:i + 1].contiguous(), Y=_nan((1, D), device)) for i in range(SEQ)]).cpu().numpy()
        assert dec.filled == SEQ
        dec.begin()
        chunks = torch.cat([dec.step(X[0:5], Y=_nan((5, D), device)), dec.step(X[5:6], Y=_nan((1, D), device)),
                            dec.step(X[6:9], Y=_nan((3, D), device))]).cpu().numpy()
        # a rewind: rows 3 .. 8 again over what the longer sequence left in the cache
        again = dec.step(X[3:9].contiguous(), pos=3, Y=_nan((6, D), device)).cpu().numpy()
        assert dec.filled == SEQ
    finally:
        dec.close()
    assert_bits_equal(rows, want, "begin + steps row by row")
    assert_bits_equal(chunks, want, "begin + steps 5, 1, 3")
    assert_bits_equal(again, want[3:], "a rewind to position 3")


SLOT_PRE = (4, 0, 2)


def _slot_rows(b, device, lo, hi):
    return _dev(_x(40 + b)[lo:hi], device)


def _prefill(dec, device, slots=(0, 1, 2)):
    for b, sl in enumerate(slots):
        dec.begin_slot(sl)
        if SLOT_PRE[b]:
            dec.step_slot(sl, _slot_rows(b, device, 0, SLOT_PRE[b]))


@pytest.mark.parametrize("base", ["post", "pre"])
def test_step_batch_on_three_slots(qg, oracle, device, base):
    dec = _decoder(qg, base, n_slots=3)
    try:
        _load(dec, base, device)
        _prefill(dec, device)
        new = torch.cat([_slot_rows(b, device, SLOT_PRE[b], SLOT_PRE[b] + 1) for b in range(3)])
        got = dec.step_batch([0, 1, 2], new, Y=_nan((3, D), device)).cpu().numpy()
        assert [dec.slot_filled(b) for b in range(3)] == [p + 1 for p in SLOT_PRE]
    finally:
        dec.close()
    for b in range(3):
        assert_bits_equal(got[b:b + 1], _expected(base, 40 + b, SLOT_PRE[b] + 1)[-1:], f"slot {b}")


@pytest.mark.parametrize("base", ["reference", "pre"])
def test_step_varlen_rows_4_1_3(qg, oracle, device, base):
    """a prefill of 4 rows, one decoding row behind a 2-row prefix and 3 rows behind a 4-row prefix, in one call"""
    dec = _decoder(qg, base, n_slots=3, max_rows=16)
    try:
        _load(dec, base, device)
        for sl in range(3):
            dec.begin_slot(sl)
        dec.step_slot(1, _slot_rows(1, device, 0, 2))
        dec.step_slot(2, _slot_rows(2, device, 0, 4))
        X = torch.cat([_slot_rows(0, device, 0, 4), _slot_rows(1, device, 2, 3), _slot_rows(2, device, 4, 7)])
        got = dec.step_varlen([0, 1, 2], X, [4, 1, 3], Y=_nan((8, D), device)).cpu().numpy()
        assert [dec.slot_filled(b) for b in range(3)] == [4, 3, 7]
    finally:
        dec.close()
    assert_bits_equal(got[:4], _expected(base, 40, 4), "the prefill's rows")
    assert_bits_equal(got[4:5], _expected(base, 41, 3)[-1:], "the decoding row")
    assert_bits_equal(got[5:], _expected(base, 42, 7)[4:], "three rows behind four")


def test_copy_slot_then_diverging_steps(qg, oracle, device):
    base = "post"
    dec = _decoder(qg, base, n_slots=2)
    a, b = O.uniform((1, D), 81), O.uniform((1, D), 82)
    try:
        _load(dec, base, device)
        dec.begin_slot(0)
        dec.step_slot(0, _dev(_x()[:5], device))
        assert dec.slot_filled(1) is None
        dec.copy_slot(1, 0)
        assert dec.slot_filled(1) == 5
        ya = dec.step_slot(0, _dev(a, device)).cpu().numpy()
        yb = dec.step_slot(1, _dev(b, device)).cpu().numpy()
        assert dec.read_slot(0, 0)[1].numel() == 0   # no cross slab
    finally:
        dec.close()
    for got, new in ((ya, a), (yb, b)):
        want = RO.decoder_only_forward(np.concatenate([_x()[:5], new]), _weights(), D, H, BLOCKS, arch=1)
        assert_bits_equal(got, want[-1:], "a fork's own continuation")


# ---- generate ---------------------------------------------------------------------------------------------------------
VOCAB, N_NEW = 50, 4


def _head(qg, device, max_rows=8):
    E, P = O.uniform((VOCAB, D), 601), O.uniform((MAX_SEQ, D), 602, -0.1, 0.1)
    Wv, bias = O.uniform((D, VOCAB), 603), O.uniform((VOCAB,), 604, -0.05, 0.05)
    return qg.Head(qg.pack_b(_dev(Wv, device)), VOCAB, _dev(bias, device), _dev(E, device), _dev(P, device),
                   max_rows=max_rows)


def test_generate_equals_the_python_loop(qg, oracle, device):
    base = "pre"
    dec, loop, head = _decoder(qg, base, n_slots=3), _decoder(qg, base, n_slots=3), _head(qg, device)
    try:
        _load(dec, base, device)
        _load(loop, base, device)
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
        for b in range(3):   # the loop's first step against the oracle
            whole = np.concatenate([_x(40 + b)[:SLOT_PRE[b]], first_emb[b:b + 1]])
            ref = RO.decoder_only_forward(whole, _weights(), D, H, BLOCKS, arch=0x301)[-1:]
            assert_bits_equal(first_hidden[b:b + 1], ref, f"step 0 of slot {b} against the oracle")
        _prefill(dec, device)
        got = dec.generate(head, [0, 1, 2], tin, N_NEW, pos=list(SLOT_PRE)).cpu().numpy()
    finally:
        head.close()
        dec.close()
        loop.close()
    assert np.array_equal(got, want), f"generate against the Python-driven loop:\n{got}\n{want}"


def test_beam_search_copy_free_equals_the_copy_path(qg, oracle, device):
    """2 groups x 2 beams: generate_beam_indirect on one slot set against generate_beam on two, token for token, parent
    for parent and score for score."""
    base, beams, pre = "post", 2, (3, 1)
    ind, old, head = _decoder(qg, base, n_slots=6), _decoder(qg, base, n_slots=8), _head(qg, device)
    tin = torch.tensor([5, 31], dtype=torch.int32, device=device)
    try:
        for dec in (ind, old):
            _load(dec, base, device)
        # the copy-free search: prompts in slots 4 and 5, the beams in slots 0 .. 3
        for g, sl in enumerate((4, 5)):
            ind.begin_slot(sl)
            ind.step_slot(sl, _slot_rows(g, device, 0, pre[g]))
        ind.beam_begin([0, 1, 2, 3], [4, 5], None, beams)
        got = ind.generate_beam_indirect(head, [0, 1, 2, 3], [4, 5], tin, N_NEW, beams)
        assert [ind.slot_filled(s) for s in range(4)] == [pre[0] + N_NEW] * 2 + [pre[1] + N_NEW] * 2
        # the copy path: the prompts in slots 0 and 2, forked into sets A = 0 .. 3 and B = 4 .. 7
        A, B = [0, 1, 2, 3], [4, 5, 6, 7]
        for g in range(2):
            old.begin_slot(2 * g)
            old.step_slot(2 * g, _slot_rows(g, device, 0, pre[g]))
            old.beam_fork(2 * g, A[2 * g:2 * g + 2], B[2 * g:2 * g + 2])
        want = old.generate_beam(head, A, B, tin, N_NEW, beams)
        for x, y, what in zip(got, want, ("tokens", "parents", "scores")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what
        assert torch.isfinite(got[2]).any()
    finally:
        head.close()
        ind.close()
        old.close()


# ---- what the handle refuses ------------------------------------------------------------------------------------------
def test_cross_kinds_and_cross_arguments_are_refused(qg, oracle, device):
    L = qg.load()
    v = torch.zeros(D * D, device=device)
    stream = qg._stream(device)
    X, enc = _dev(_x(), device), _dev(_x(12, 7), device)
    models = [_decoder(qg, "reference", n_slots=2), _decoder(qg, "post", n_slots=2), _decoder(qg, "pre", n_slots=2)]
    try:
        for m in models:
            for kind in list(range(8, 12)) + list(range(20, 26)):
                assert L.qgemm_model_set_weight(m._h, 0, kind, 0, v.data_ptr(), 0, D, 1, stream) == INVALID, kind
                assert L.qgemm_model_weight_shape(m._h, kind, None, None, None) == INVALID, kind
            p, n, k = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
            assert L.qgemm_model_packed_weight(m._h, 0, 4, ctypes.byref(p), ctypes.byref(n), ctypes.byref(k)) == INVALID
            with pytest.raises(AssertionError):
                m.forward(X, enc)
            with pytest.raises(AssertionError):
                m.begin_slot(0, enc)
            Y = torch.empty_like(X)
            assert L.qgemm_decoder_forward(m._h, X.data_ptr(), enc.data_ptr(), Y.data_ptr(), SEQ, 7, stream) == INVALID
            assert L.qgemm_decoder_forward(m._h, X.data_ptr(), None, Y.data_ptr(), SEQ, 7, stream) == INVALID
            assert L.qgemm_decoder_forward(m._h, X.data_ptr(), enc.data_ptr(), Y.data_ptr(), SEQ, 0, stream) == INVALID
            assert L.qgemm_decoder_begin_slot(m._h, 0, enc.data_ptr(), 7, stream) == INVALID
            assert L.qgemm_decoder_begin_slot(m._h, 0, None, 1, stream) == INVALID
            assert L.qgemm_decoder_begin_slot(m._h, 2, None, 0, stream) == INVALID
            assert m.slot_filled(0) is None, "a refused begin begins nothing"
            assert L.qgemm_decoder_step_slot(m._h, 0, X.data_ptr(), Y.data_ptr(), 0, 1, stream) == INVALID   # not begun
            assert L.qgemm_encoder_forward(m._h, X.data_ptr(), Y.data_ptr(), SEQ, stream) == INVALID   # the other family
            cross = torch.empty(4, device=device)
            assert L.qgemm_decoder_read_slot(m._h, 0, 0, None, cross.data_ptr(), stream) == INVALID
        torch.cuda.synchronize()
    finally:
        for m in models:
            m.close()


# ---- torch layers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_first", [False, True], ids=["post", "pre"])
def test_load_torch_encoder_layers(qg, oracle, device, norm_first):
    """The layers, inputs and recorded quantization bound of tests/test_rope_host.py: a TransformerEncoderLayer under a
    causal mask is this block.  forward after load_torch_layer is the oracle chain on the layers' tensors bit for bit,
    torch's own masked forward within the bound, and the cached steps give the same rows."""
    import test_rope_host as TH
    layers, norm = TH.torch_model(norm_first)
    W = PO.torch_model_weights(layers, H, norm)
    X = TH.inputs()
    model = qg.Decoder(D, H, TH.DFF, TH.LAYERS, MAX_SEQ, 0, causal=True, kv_cache=True, decoder_only=True,
                       arch="standard", norm_first=norm_first, final_norm=norm_first)
    cross = qg.Decoder(D, H, TH.DFF, TH.LAYERS, MAX_SEQ, 4, arch="standard", norm_first=norm_first)
    try:
        for i, layer in enumerate(layers):
            model.load_torch_layer(i, layer)
        if norm_first:
            model.load_torch_final_norm(norm)
        Xd = _dev(X, device)
        got = model.forward(Xd).cpu().numpy()
        model.begin()
        steps = torch.cat([model.step(Xd[:5].contiguous()), model.step(Xd[5:].contiguous())]).cpu().numpy()
        with pytest.raises(ValueError):   # a decoder layer has a cross-attention this model lacks
            model.load_torch_layer(0, torch.nn.TransformerDecoderLayer(D, H, dim_feedforward=TH.DFF, norm_first=norm_first))
        with pytest.raises(ValueError):   # and a model with cross-attention still takes no encoder layer
            cross.load_torch_layer(0, layers[0])
    finally:
        model.close()
        cross.close()
    assert_bits_equal(steps, got, "begin + steps 5, 4 against forward")
    assert_bits_equal(got, TH.chain(W, X, norm_first, None, None), "forward against the oracle chain")
    err = TH.rel_fro(got, TH.torch_own_forward(layers, norm, X))
    print(f"decoder-only norm_first={norm_first}: relative Frobenius error against torch {err:.3e}")
    assert err <= 2 * TH.QUANT_MEASURED[norm_first, False]


# ---- a captured step --------------------------------------------------------------------------------------------------
def test_captured_step_replays_the_same_bits(qg, oracle, device):
    """begin launches nothing, so the captured graph is the step alone: replayed on a rewound slot it gives its rows."""
    L = qg.load()
    base = "pre"
    dec = _decoder(qg, base)
    try:
        _load(dec, base, device)
        X = _dev(_x(), device)
        dec.begin()
        dec.step(X[:5].contiguous())
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device)
        new, Y = X[5:7].contiguous(), _nan((2, D), device)
        with torch.cuda.stream(s):
            eager = dec.step(new, pos=5).cpu().numpy()   # also the warm-up
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                assert L.qgemm_decoder_step(dec._h, new.data_ptr(), Y.data_ptr(), 5, 2, s.cuda_stream) == 0
        assert_bits_equal(eager, _expected(base)[5:7], "the eager step")
        for i in range(2):
            Y.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_bits_equal(Y.cpu().numpy(), eager, f"replay {i}")
        assert dec.filled == 7
    finally:
        dec.close()
