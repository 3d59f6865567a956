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
