"""Host-only checks for the attention entry point and the decoder counterpart (no GPU).

* tests/attn_oracle.py's Python composition is held against the committed C restatement of the encoder bit for
  bit: that pins its weight layout, seeds and step order, which decoder_forward_ref shares.
* decoder_forward_ref is not two stacked encoder blocks.
* qgemm_attention / qgemm_decoder_create refuse bad arguments before any device work, and
  qgemm_attention_workspace_size is 0 exactly inside the fused launch's envelope.
"""
import ctypes

import numpy as np
import pytest

import attn_cases
import attn_oracle
from util import assert_bits_equal, bits


@pytest.mark.parametrize("seq,d,H,dff,blocks", [(6, 8, 4, 8, 2), (33, 64, 2, 96, 2)])
def test_encoder_ref_matches_the_c_oracle(oracle, seq, d, H, dff, blocks):
    X = oracle.uniform((seq, d), 11)
    got = attn_oracle.encoder_forward_ref(X, d, H, dff, blocks, 13)
    assert_bits_equal(got, oracle.encoder_forward(X, d, H, dff, blocks, 13), f"encoder_forward_ref seq={seq} d={d}")


def test_decoder_ref_is_not_a_stacked_encoder(oracle):
    """With enc_out = X the decoder still differs from the encoder: another attention with its own weights sits
    between the self-attention and the FFN, and the FFN's residual is that attention's output."""
    seq, d, H, dff, blocks = 6, 8, 4, 8, 2
    X = oracle.uniform((seq, d), 11)
    dec = attn_oracle.decoder_forward_ref(X, X, d, H, dff, blocks, 13)
    enc = oracle.encoder_forward(X, d, H, dff, blocks, 13)
    assert dec.shape == enc.shape and np.isfinite(dec).all()
    assert (bits(dec) != bits(enc)).mean() > 0.9


def test_attention_ref_one_key_is_v(oracle):
    """One key: P is exactly 1, so every output row is V's row (a -0 in V comes out as +0: the chain starts at +0)."""
    Q, K, V = oracle.uniform((5, 32), 1), oracle.uniform((1, 32), 2), oracle.uniform((1, 32), 3)
    V[0, 3] = -0.0
    got = attn_oracle.attention_ref(Q, K, V, 2, 0.25)
    want = np.repeat(V, 5, axis=0)
    want[:, 3] = 0.0
    assert_bits_equal(got, want, "attention_ref, one key")


def _attention(L, Q=8, K=8, V=8, O=8, seq_q=4, seq_kv=4, H=2, dk=8, ws=None, ws_bytes=0):
    return L.qgemm_attention(Q, dk * H, K, dk * H, V, dk * H, O, dk * H, seq_q, seq_kv, H, dk, 0.5, ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [
    dict(Q=None), dict(K=None), dict(V=None), dict(O=None),
    dict(seq_q=-1), dict(seq_kv=0), dict(H=0), dict(dk=0),
    dict(seq_kv=4097),                                             # the softmax row limit
    dict(seq_q=20, seq_kv=513, H=2, dk=8),                         # fallback without a workspace
    dict(seq_q=20, seq_kv=513, H=2, dk=8, ws=8, ws_bytes=4 * 2 * 20 * 513 - 1),   # one byte short
    dict(seq_q=20, seq_kv=40, H=1, dk=65, ws=8, ws_bytes=0),
])
def test_attention_invalid_arguments(qg, kw):
    assert _attention(qg.load(), **kw) == qg.HIP_ERROR_INVALID_VALUE


def test_attention_no_queries_returns_success(qg):
    L = qg.load()
    assert _attention(L, seq_q=0) == 0
    assert _attention(L, seq_q=0, seq_kv=513) == 0  # no scores: no workspace needed


def test_attention_workspace_size(qg):
    L = qg.load()
    size = L.qgemm_attention_workspace_size
    assert size(32, 512, 4, 64) == 0                     # the fused envelope's corner
    assert size(100000, 512, 4, 64) == 0                 # any seq_q
    assert size(20, 513, 2, 8) == 4 * 2 * 20 * 513       # just past seq_kv
    assert size(20, 40, 1, 65) == 4 * 1 * 20 * 40        # just past d_k
    for bad in [(-1, 4, 1, 8), (4, 0, 1, 8), (4, 4, 0, 8), (4, 4, 1, 0), (4, 4097, 1, 8)]:
        assert size(*bad) == 0, bad


@pytest.mark.parametrize("args", [
    (10, 4, 8, 1, 6, 6),       # d_model % n_heads != 0
    (8, 4, 8, 1, 6, 4097),     # max_enc_seq > 4096
    (8, 4, 8, 1, 4097, 6),     # max_seq > 4096
    (8, 0, 8, 1, 6, 6),
    (8, 4, 8, 0, 6, 6),
    (8, 4, 8, 1, 6, 0),
])
def test_decoder_create_invalid_arguments(qg, args):
    L = qg.load()
    h = ctypes.c_void_p(1)
    assert L.qgemm_decoder_create(*args, 0, ctypes.byref(h)) == qg.HIP_ERROR_INVALID_VALUE
    assert not h.value, "no handle on failure"
    assert L.qgemm_decoder_create(8, 4, 8, 1, 6, 6, 0, None) == qg.HIP_ERROR_INVALID_VALUE


def test_decoder_weight_kinds_extend_the_encoders(qg, oracle):
    assert qg.DECODER_WEIGHT_KINDS[:8] == qg.ENCODER_WEIGHT_KINDS
    assert qg.DECODER_WEIGHT_KINDS[8:] == ("Wq2", "Wk2", "Wv2", "Wo2")
    for kind in (8, 11):
        assert qg.encoder_weight_seed(13, 1, kind, 2) == oracle.encoder_weight_seed(13, 1, kind, 2)


# ---- the special-value sets of tests/attn_cases.py: each produces, in the oracle's result alone, the condition the
# GPU tests rely on it for (floors, not exact counts) ----

_TINY = np.float32(1.1754944e-38)  # the smallest normal fp32


def _subnormal(a):
    return (a != 0) & (np.abs(a) < _TINY)


def _softmax_row(name, row):
    return attn_cases.softmax_expected(name)[attn_cases.SOFTMAX_ROWS.index(row)]


def test_softmax_sets_shapes(oracle):
    sets = attn_cases.softmax_sets()
    assert set(sets) == {"scale_1", "scale_0", "scale_neg1", "overflow"}
    for name, ((S, scale), what) in sets.items():
        assert S.dtype == np.float32 and S.shape[1] == attn_cases.SOFTMAX_W and what
        assert S.shape[0] == (1 if name == "overflow" else len(attn_cases.SOFTMAX_ROWS))
    S = sets["scale_1"][0][0]
    assert np.signbit(S[2, 0]) and S[2, 0] == 0 and not np.signbit(S[2, 7]) and S[2, 7] == 0 and (S[2] <= 0).all()
    assert np.signbit(S[2, 3::3]).all() and (S[2, 3::3] == 0).all()
    assert np.isnan(S[3, 0]) and np.isnan(S[4, 100]) and np.isposinf(S[5, 150])
    assert np.isneginf(np.delete(S[1], 77)).all() and np.isfinite(S[1, 77])


def test_softmax_set_scale_1(oracle):
    a = _softmax_row("scale_1", "a")
    assert np.isfinite(a).all() and _subnormal(a).sum() >= 20 and (a == 0).sum() >= 5 and not np.signbit(a).any()
    b = _softmax_row("scale_1", "b")
    assert b[77] == 1.0 and (np.delete(b, 77) == 0).all() and not np.signbit(b).any()
    c = _softmax_row("scale_1", "c")
    assert np.isfinite(c).all() and c[0] == c[7] and c[0] == c.max()
    for row in "def":
        assert np.isnan(_softmax_row("scale_1", row)).all(), row


@pytest.mark.parametrize("name", ["scale_0", "scale_neg1"])
def test_softmax_sets_scale_0_and_minus_1(oracle, name):
    """Scale 0 turns every infinity into NaN (rows b and f) and every finite row into the uniform 1 / w; scale -1 turns
    row b's -inf into +inf (inf - inf: NaN) and row f's +inf into a -inf whose exp is +0, so f comes out finite."""
    a, c = _softmax_row(name, "a"), _softmax_row(name, "c")
    assert np.isfinite(a).all() and np.isfinite(c).all()
    for row in "bde":
        assert np.isnan(_softmax_row(name, row)).all(), row
    f = _softmax_row(name, "f")
    if name == "scale_0":
        assert np.isnan(f).all()
        assert (a == a[0]).all() and (c == c[0]).all() and a[0] > 0
    else:
        assert np.isfinite(f).all() and f[150] == 0 and (np.delete(f, 150) > 0).all()
        assert _subnormal(a).sum() >= 20 and (a == 0).sum() >= 5   # row a reversed: the same exps, from the far end


def test_softmax_set_overflow(oracle):
    (S, scale), _ = attn_cases.softmax_sets()["overflow"]
    with np.errstate(over="ignore"):
        prod = S * np.float32(scale)
    assert prod[0, 0] == 0 and np.isneginf(prod[0, 1:]).all()
    p = attn_cases.softmax_expected("overflow")[0]
    assert not np.isnan(p).any() and p[0] == 1.0 and (p == 0).sum() >= attn_cases.SOFTMAX_W - 1


@pytest.mark.parametrize("shape", [attn_cases.ATTN_BASE, attn_cases.ATTN_FALLBACK], ids=["fused", "fallback"])
def test_attention_sets_produce_their_conditions(qg, oracle, shape):
    seq_q, seq_kv, H, dk = shape
    sets = attn_cases.attention_sets(shape)
    assert tuple(sets) == attn_cases.ATTENTION_NAMES
    fused = qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk) == 0
    assert fused == (shape == attn_cases.ATTN_BASE)
    want = {n: attn_cases.attention_expected(n, shape) for n in sets}
    for n, ((Q, K, V), what) in sets.items():
        assert Q.shape == (seq_q, H * dk) and K.shape == V.shape == (seq_kv, H * dk) and what
        assert want[n].shape == Q.shape

    plain = attn_oracle.attention_ref(*(oracle.uniform(s, attn_cases.ATTN_SEED + i) for i, s in enumerate(
        [(seq_q, H * dk), (seq_kv, H * dk), (seq_kv, H * dk)])), H, attn_oracle.default_scale(dk))
    w = want["nan_in_k"]
    assert np.isnan(w[:, :dk]).all() and np.isfinite(w[:, dk:]).all()
    assert_bits_equal(w[:, dk:], plain[:, dk:], "head 1 beside a NaN head")
    w = want["inf_in_v"]
    assert np.isposinf(w[:, 30]).all() and np.isfinite(np.delete(w, 30, axis=1)).all()
    w = want["inf_in_v_peaked"]
    assert np.isposinf(w[:, 30]).sum() >= 1 and np.isnan(w[:, 30]).sum() >= 1
    assert np.isfinite(np.delete(w, 30, axis=1)).all()
    w = want["zero_q_row"]
    assert np.isfinite(w).all()
    V = sets["zero_q_row"][0][2]
    P = np.full((1, seq_kv), np.float32(1.0) / np.float32(seq_kv), np.float32)  # exp(0) / fl(sum of seq_kv ones)
    assert_bits_equal(w[4:5], oracle.mm_fp32(P, V), "row 4 is the uniform average of V")
    w = want["overflowing_scores"]
    assert np.isnan(w[5, :dk]).all() and np.isfinite(np.delete(w, 5, axis=0)).all() and np.isfinite(w[5, dk:]).all()
    assert (bits(want["neg_zero_v"]) == 0).all()
    w = want["tiny_v"]
    assert _subnormal(w).sum() >= 1000 and (w != 0).all()


def test_zero_row_decoder_inputs_stay_finite(oracle):
    """A zero row of X or enc_out has absmax 0 and scale inf; 0 * inf is NaN and the pack stores it as 0.  The
    oracle's result for these inputs is finite everywhere, and differs from the plain inputs' in nearly every bit."""
    X, enc = attn_cases.zero_row_decoder_inputs()
    assert not X[3].any() and not enc[7].any() and X[2].any() and enc[6].any()
    Y = attn_oracle.decoder_forward_ref(X, enc, 64, 2, 96, 2, 13)
    assert np.isfinite(Y).all()
    plain = attn_oracle.decoder_forward_ref(oracle.uniform((33, 64), 11), oracle.uniform((100, 64), 12), 64, 2, 96, 2,
                                            13)
    assert (bits(Y) != bits(plain)).mean() > 0.9, "the zero rows reach every output through both attentions"
