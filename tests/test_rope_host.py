"""Rotary embeddings and decoder-only stacks without a GPU: tests/rope_oracle.py against its own
definition's properties and against a torch model chained by hand, and the refusals of the new architecture bits,
keywords and entry points.

Every bound is a multiple of an error MEASURED on the CPU with these fixed, seeded inputs (the table in DESIGN.md s27
records the same figures), as tests/test_prenorm_host.py does: 4x for the fp32 wiring against torch -- the margin covers
another machine's libm and BLAS summation order, nothing else -- and 2x for the quantized chain, whose error is the int8
quantization's."""
import ctypes

import numpy as np
import pytest

import prenorm_oracle as PO
import rope_oracle as RO
import standard_oracle as SO

F = np.float32
D, H, DFF, SEQ, LAYERS = 64, 4, 128, 9, 2
DK = D // H

# relative Frobenius errors of the causal decoder-only chain against torch, measured on the CPU, keyed (norm_first,
# rope): the fp32 wiring and the quantized chain.  norm_first=True has the final LayerNorm
WIRING_MEASURED = {(False, False): 2.930e-7, (False, True): 2.824e-7, (True, False): 3.292e-7, (True, True): 3.208e-7}
QUANT_MEASURED = {(False, False): 3.216e-2, (False, True): 3.086e-2, (True, False): 2.946e-2, (True, True): 3.049e-2}
# (the same chain with the rotation the other way, in the order of the entries above: 0.745, 0.736, 0.711, 0.706 -- at
# least 11.6x the bound it must clear by 10x)
# the relative-position property: |rope(q, m) . rope(k, n) - rope(q, m + s) . rope(k, n + s)| / (|q| |k|), the largest
# over the draws of test_relative_position_property, measured on the CPU; the test allows 4x
RELATIVE_MEASURED = 8.940e-8


def _rows(rows, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, w)) * 3.0 + 0.5).astype(F)


# ---- the oracle against its own definition ----------------------------------------------------------------------------
def test_position_zero_is_the_identity():
    cos, sin = RO.make_tables(16, DK)
    assert (cos[0].view(np.uint32) == F(1).view(np.uint32)).all() and (sin[0].view(np.uint32) == 0).all()
    X = _rows(1, 3 * DK, 1)
    assert np.array_equal(RO.rope_rows(X, 3, DK, cos, sin, 0).view(np.uint32), X.view(np.uint32))


def test_pair_norms_are_preserved_within_rounding():
    """|(y_i, y_{i+h})|^2 = (c^2 + s^2) |(x_i, x_{i+h})|^2 and fl(c)^2 + fl(s)^2 = 1 +- 2^-23; five roundings on each
    output of relative size 2^-24 each: 2^-21 covers the squared norm's relative error."""
    cos, sin = RO.make_tables(32, DK)
    X = _rows(32, 2 * DK, 2)
    Y = RO.rope_rows(X, 2, DK, cos, sin, 0).astype(np.float64).reshape(32, 2, 2, DK // 2)
    X = X.astype(np.float64).reshape(32, 2, 2, DK // 2)
    nx, ny = (X ** 2).sum(axis=2), (Y ** 2).sum(axis=2)
    assert (np.abs(ny - nx) <= 2.0 ** -21 * nx).all()


def _relative_error():
    cos, sin = RO.make_tables(64, DK)
    rng = np.random.default_rng(4)
    worst = 0.0
    for _ in range(50):
        q, k = (rng.standard_normal((1, DK)).astype(F) for _ in range(2))
        m, n, s = int(rng.integers(0, 20)), int(rng.integers(0, 20)), int(rng.integers(1, 40))
        dot = lambda a, b: float((RO.rope_rows(q, 1, DK, cos, sin, a).astype(np.float64) @
                                  RO.rope_rows(k, 1, DK, cos, sin, b).astype(np.float64).T)[0, 0])
        scale = float(np.linalg.norm(q.astype(np.float64)) * np.linalg.norm(k.astype(np.float64)))
        worst = max(worst, abs(dot(m, n) - dot(m + s, n + s)) / scale)
    return worst


def test_relative_position_property():
    err = _relative_error()
    print(f"relative-position property: worst |difference| / (|q| |k|) {err:.3e}")
    assert err <= 4 * RELATIVE_MEASURED


def test_half_split_pairing_is_rotate_half():
    """x cos + rotate_half(x) sin with the tables repeated over both halves (Hugging Face Llama, GPT-NeoX), in torch
    fp32: within 1 ulp per element (torch may fuse nothing here, but its order of the two products is its own)."""
    import torch
    cos, sin = RO.make_tables(16, DK)
    X = _rows(9, 3 * DK, 3)
    x = torch.from_numpy(X).view(9, 3, DK)
    c = torch.from_numpy(np.concatenate([cos[2:11], cos[2:11]], axis=1))[:, None, :]
    s = torch.from_numpy(np.concatenate([sin[2:11], sin[2:11]], axis=1))[:, None, :]
    rot = torch.cat([-x[..., DK // 2:], x[..., :DK // 2]], dim=-1)
    want = (x * c + rot * s).reshape(9, 3 * DK).numpy()
    got = RO.rope_rows(X, 3, DK, cos, sin, 2)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got.astype(np.float64) - want) <= ulp).all()
    # the interleaved pairing is another function: the oracle must be far from it
    xi = X.reshape(9, 3, DK // 2, 2)
    ci, si = cos[2:11][:, None, :], sin[2:11][:, None, :]
    inter = np.stack([xi[..., 0] * ci - xi[..., 1] * si, xi[..., 1] * ci + xi[..., 0] * si], axis=-1).reshape(9, 3 * DK)
    assert np.abs(got - inter).max() > 0.1


def test_chains_without_rope_are_the_older_oracles(oracle):
    """rope_oracle's chains with rope=None restate nothing: bit for bit the post-LN and pre-LN encoder chains."""
    W = PO.prenorm_weights(D, H, DFF, LAYERS, 23, cross=False, final_norm=True)
    X = _rows(SEQ, D, 21) / F(3.0)
    got = RO.decoder_only_forward(X, W, D, H, LAYERS, arch=1, causal=False)
    assert np.array_equal(got.view(np.uint32), SO.encoder_forward_std(X, W, D, H, LAYERS).view(np.uint32))
    got = RO.decoder_only_forward(X, W, D, H, LAYERS, arch=0x301, causal=False)
    assert np.array_equal(got.view(np.uint32), PO.encoder_forward_pre(X, W, D, H, LAYERS).view(np.uint32))


# ---- the wiring against torch -----------------------------------------------------------------------------------------
def torch_model(norm_first: bool):
    """LAYERS torch.nn.TransformerEncoderLayer (relu) with every gamma != 1 and every bias and beta != 0, and with
    norm_first the LayerNorm behind them (else None).  The query and key projections are scaled by 2 and the value
    projection by 4, so that the attention pattern matters to the output: with torch's initial weights the softmax over
    at most nine keys is close to uniform and the output hardly depends on where Q and K point, rotated or not."""
    import torch
    torch.manual_seed(57 + (1 if norm_first else 0))
    layers = [torch.nn.TransformerEncoderLayer(D, H, dim_feedforward=DFF, dropout=0.0, norm_first=norm_first)
              for _ in range(LAYERS)]
    norm = torch.nn.LayerNorm(D, eps=1e-5) if norm_first else None
    with torch.no_grad():
        for m in layers + ([norm] if norm_first else []):
            m.eval()
            for name, p in m.named_parameters():
                if name.endswith("bias"):
                    p.copy_(0.2 * torch.randn_like(p))
                elif "norm" in name or m is norm:
                    p.copy_(1.0 + 0.2 * torch.randn_like(p))
        for layer in layers:
            layer.self_attn.in_proj_weight[:2 * D] *= 2.0
            layer.self_attn.in_proj_weight[2 * D:] *= 4.0
    return layers, norm


def wiring_tables():
    """The tables of the wiring tests: theta = 1, every pair turns by one radian per position (a caller's table, as
    qgemm_model_set_weight takes one).  At theta = 10000 half of the eight pairs turn by less than 0.1 rad over the
    nine positions, and the rotated and the unrotated model then differ by about three times the quantization error
    (measured: 4.8e-2 against 1.4e-2): no bound could tell the wirings apart."""
    ang = np.arange(16, dtype=np.float64)[:, None] * np.ones(DK // 2)[None, :]
    return np.cos(ang).astype(F), np.sin(ang).astype(F)


def torch_forward(layers, norm, X, rope):
    """The causal decoder-only model chained by hand on the layers' parameters: the projections, rotate_half on q and k
    (rope = (cos, sin) or None), scaled_dot_product_attention(is_causal=True), the layer's own norms and FFN."""
    import torch
    import torch.nn.functional as Fn

    def rot(t, c, s):  # t: [H, seq, d_k]
        half = torch.cat([-t[..., DK // 2:], t[..., :DK // 2]], dim=-1)
        return t * c + half * s

    def attn(layer, x):
        a = layer.self_attn
        q, k, v = Fn.linear(x, a.in_proj_weight, a.in_proj_bias).chunk(3, dim=-1)
        q, k, v = (t.view(-1, H, DK).transpose(0, 1) for t in (q, k, v))
        if rope is not None:
            c, s = (torch.from_numpy(np.concatenate([t[:x.shape[0]]] * 2, axis=1)) for t in rope)
            q, k = rot(q, c, s), rot(k, c, s)
        o = Fn.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(0, 1).reshape(-1, D)
        return a.out_proj(o)

    def ffn(layer, x):
        return layer.linear2(Fn.relu(layer.linear1(x)))

    with torch.no_grad():
        x = torch.from_numpy(X)
        for layer in layers:
            if layer.norm_first:
                x = x + attn(layer, layer.norm1(x))
                x = x + ffn(layer, layer.norm2(x))
            else:
                x = layer.norm1(x + attn(layer, x))
                x = layer.norm2(x + ffn(layer, x))
        return (x if norm is None else norm(x)).numpy()


def torch_own_forward(layers, norm, X):
    """torch's own forward of the layers under a causal mask (no rotation exists there)."""
    import torch
    with torch.no_grad():
        x = torch.from_numpy(X)
        mask = torch.nn.Transformer.generate_square_subsequent_mask(x.shape[0])
        for layer in layers:
            x = layer(x, src_mask=mask)
        return (x if norm is None else norm(x)).numpy()


def rel_fro(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want.astype(np.float64)))


def inputs():
    return _rows(SEQ, D, 21) / F(3.0)


def chain(W, X, norm_first, rope, mm):
    return RO.decoder_only_forward(X, W, D, H, LAYERS, arch=0x301 if norm_first else 1, causal=True, rope=rope, mm=mm)


@pytest.fixture(scope="module", params=sorted(WIRING_MEASURED), ids=lambda k: f"{'pre' if k[0] else 'post'}-{'rope' if k[1] else 'plain'}")
def torch_case(request, oracle):
    norm_first, rope = request.param
    layers, norm = torch_model(norm_first)
    tables = wiring_tables() if rope else None
    X = inputs()
    return request.param, PO.torch_model_weights(layers, H, norm), X, tables, torch_forward(layers, norm, X, tables)


def test_hand_chain_is_torchs_own_forward():
    """Without the rotation the hand-written chain must be the layers' own forward under a causal mask: the chain the
    rotation is tested in is torch's."""
    for norm_first in (False, True):
        layers, norm = torch_model(norm_first)
        X = inputs()
        assert rel_fro(torch_forward(layers, norm, X, None), torch_own_forward(layers, norm, X)) < 1e-6


def test_wiring_against_torch_fp32(torch_case):
    key, W, X, tables, want = torch_case
    err = rel_fro(chain(W, X, key[0], tables, lambda x, w: np.matmul(x, w, dtype=F)), want)
    print(f"decoder-only wiring {key}: relative Frobenius error {err:.3e}")
    assert err <= 4 * WIRING_MEASURED[key]


def test_quantized_chain_against_torch(torch_case):
    key, W, X, tables, want = torch_case
    err = rel_fro(chain(W, X, key[0], tables, None), want)
    # the same chain with the rotation the other way (without it where the torch model has one, with it where it has
    # none): the test must be able to tell the wirings apart
    err_other = rel_fro(chain(W, X, key[0], None if key[1] else wiring_tables(), None), want)
    print(f"decoder-only quantized {key}: relative Frobenius error {err:.3e}; the other rotation {err_other:.3e}")
    bound = 2 * QUANT_MEASURED[key]
    assert err <= bound
    assert err_other > 10 * bound


# ---- refusals before any GPU call -------------------------------------------------------------------------------------
def _desc(qg, **kw):
    d = dict(size=ctypes.sizeof(qg.ModelDesc), cross=1, d_model=8, n_heads=2, d_ff=8, n_blocks=1, max_seq=4,
             max_enc_seq=0, seed=1, flags=0, n_slots=0, max_rows=0, arch=0x401, activation=qg.QGEMM_ACT_RELU, ln_eps=1e-5)
    d.update(kw)
    return qg.ModelDesc(**d)


@pytest.mark.parametrize("kw", [
    dict(cross=0, arch=0x401),               # DECODER_ONLY on an encoder descriptor
    dict(cross=0, arch=0xC01),
    dict(arch=0x400 | 0x201),                # a good bit on FINAL_NORM without NORM_FIRST
    dict(arch=0x800), dict(arch=0xC00),      # ROPE on the reference base
    dict(cross=0, arch=0x800),
    dict(arch=0x801, d_model=6),             # d_k = 3
    dict(cross=0, arch=0x801, d_model=6),
    dict(arch=0x401, max_enc_seq=4),         # a decoder-only model has no encoder output to size anything by
    dict(arch=0x1001), dict(arch=0x1401), dict(cross=0, arch=0x1001),
    dict(arch=0x401, flags=8),               # KV_CACHE without CAUSAL, as on every decoder
    dict(arch=0x401, flags=2),
    dict(arch=0x401, flags=1, n_slots=2),    # slots need CAUSAL | KV_CACHE
    dict(arch=0x401, flags=9, n_slots=65),
    dict(arch=0x401, max_rows=-1),
    dict(arch=0x401, size=60),
], ids=lambda kw: ",".join(f"{k}={v:#x}" if k == "arch" else f"{k}={v}" for k, v in kw.items()))
def test_model_create_refusals(qg, kw):
    L = qg.load()
    h = ctypes.c_void_p(5)
    d = _desc(qg, **kw)
    assert L.qgemm_model_create(ctypes.byref(d), ctypes.byref(h)) == qg.HIP_ERROR_INVALID_VALUE
    assert not h.value


def test_python_keyword_refusals(qg):
    with pytest.raises(AssertionError):
        qg.Decoder(8, 2, 8, 1, 4, 4, decoder_only=True)                              # max_enc_seq != 0
    with pytest.raises(AssertionError):
        qg.Decoder(8, 2, 8, 1, 4, max_enc_seq=3, arch="standard", decoder_only=True)
    with pytest.raises(AssertionError):
        qg.Encoder(8, 2, 8, 1, 4, decoder_only=True)                                 # the keyword on Encoder
    with pytest.raises(AssertionError):
        qg.Encoder(8, 2, 8, 1, 4, rope=True)                                         # arch="reference"
    with pytest.raises(AssertionError):
        qg.Decoder(8, 2, 8, 1, 4, 0, decoder_only=True, rope=True)
    assert (qg.KIND_ROPE_COS, qg.KIND_ROPE_SIN) == (28, 29)
    assert (qg.QGEMM_ARCH_DECODER_ONLY, qg.QGEMM_ARCH_ROPE) == (0x400, 0x800)
    for name in ("qgemm_rope_rows", "qgemm_rope_rows_varlen", "qgemm_model_rope_tables", "qgemm_decoder_slot_begun"):
        assert name in qg.EXPORTED_SYMBOLS
    for name in ("rope_rows", "rope_rows_varlen"):
        assert callable(getattr(qg, name))
    assert callable(qg.Decoder.rope_tables) and callable(qg.Encoder.rope_tables)


P = 4096  # a non-null pointer that a refused call never reads


def test_rope_entry_point_refusals(qg):
    L, bad = qg.load(), qg.HIP_ERROR_INVALID_VALUE
    rr = L.qgemm_rope_rows
    #            X  stride rows groups d_k cos sin table pos0
    assert rr(0, 64, 1, 4, 16, P, P, 8, 0, None) == bad
    assert rr(P, 64, 1, 4, 16, 0, P, 8, 0, None) == bad
    assert rr(P, 64, 1, 4, 16, P, 0, 8, 0, None) == bad
    assert rr(P, 60, 1, 4, 15, P, P, 8, 0, None) == bad     # odd d_k
    assert rr(P, 64, 1, 4, 0, P, P, 8, 0, None) == bad
    assert rr(P, 64, 1, 4, 1, P, P, 8, 0, None) == bad
    assert rr(P, 64, 1, 0, 16, P, P, 8, 0, None) == bad
    assert rr(P, 63, 1, 4, 16, P, P, 8, 0, None) == bad     # stride < groups d_k
    assert rr(P, -64, 1, 4, 16, P, P, 8, 0, None) == bad
    assert rr(P, 64, -1, 4, 16, P, P, 8, 0, None) == bad
    assert rr(P, 64, 1, 4, 16, P, P, 8, -1, None) == bad
    assert rr(P, 64, 1, 4, 16, P, P, 8, 8, None) == bad     # position 8 of 8 rows
    assert rr(P, 64, 3, 4, 16, P, P, 8, 6, None) == bad     # the last row's position
    assert rr(P, 64, 9, 4, 16, P, P, 8, 0, None) == bad
    assert rr(P, 64, 1, 4, 16, P, P, 0, 0, None) == bad
    assert rr(P, 64, 0, 4, 16, P, P, 8, 3, None) == 0       # rows == 0
    rv = L.qgemm_rope_rows_varlen
    i64, i32 = ctypes.c_int64 * 65, ctypes.c_int * 65

    def call(X=P, stride=64, groups=4, d_k=16, cos=P, sin=P, table=8, n=2, row0=(0, 5), n_rows=(2, 3), pos0=(1, 5)):
        arr = lambda t, v: None if v is None else t(*v)
        return rv(X, stride, groups, d_k, cos, sin, table, n, arr(i64, row0), arr(i32, n_rows), arr(i32, pos0), None)

    for kw in (dict(X=0), dict(cos=0), dict(sin=0), dict(row0=None), dict(n_rows=None), dict(pos0=None), dict(d_k=6 + 1),
               dict(d_k=0), dict(groups=0), dict(stride=63), dict(stride=-64), dict(n=0), dict(n=65),
               dict(n_rows=(2, -1)), dict(pos0=(1, -1)), dict(pos0=(1, 8)), dict(pos0=(1, 6)), dict(pos0=(7, 5)),
               dict(row0=(0, -1)), dict(table=0)):
        assert call(**kw) == bad, kw
    assert call(n_rows=(0, 0)) == 0                         # nothing to do
