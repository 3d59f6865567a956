"""GPU parity of the causal Decoder (qgemm_decoder_create_ex, QGEMM_DECODER_CAUSAL) against
tests/causal_oracle.decoder_forward_causal_ref, bit for bit, and the property the mask is for: forward(X[:n]) equals
forward(X)[:n].  The same comparison on a decoder without the mask differs, which is asserted too."""
import ctypes

import numpy as np
import pytest
import torch

import causal_oracle
from util import assert_bits_equal, bits

pytestmark = pytest.mark.gpu

SHAPES = [causal_oracle.DECODER_FUSED, causal_oracle.DECODER_FALLBACK]
IDS = ["fused", "self_attention_fallback"]


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _decoder(qg, shape, causal):
    seq, enc_seq, d, H, dff, blocks = shape
    return qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=enc_seq, seed=causal_oracle.DECODER_SEED,
                      causal=causal)


def _forward(dec, X, enc, device):
    Y = _nan(X.shape, device)
    dec.forward(_dev(X, device), _dev(enc, device), Y=Y)
    return Y.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_causal_decoder_bit_exact_and_prefix_stable(qg, oracle, device, shape):
    """One object: the full forward against the reference, then the first 17 rows alone -- the reference's bits for
    that input and, bit for bit, the first 17 rows of the full forward."""
    seq, _, d, H = shape[:4]
    assert (qg.load().qgemm_attention_workspace_size(seq, seq, H, d // H) == 0) == (shape is SHAPES[0])
    X, enc = causal_oracle.decoder_inputs(shape)
    dec = _decoder(qg, shape, True)
    try:
        full = _forward(dec, X, enc, device)
        part = _forward(dec, X[:17], enc, device)
    finally:
        dec.close()
    assert_bits_equal(full, causal_oracle.decoder_expected(shape), f"causal decoder {shape}")
    assert_bits_equal(part, causal_oracle.decoder_expected(shape, True, 17), f"causal decoder {shape}, 17 rows")
    assert_bits_equal(part, full[:17], "forward(X[:17]) against forward(X)[:17]")


def test_decoder_without_the_mask_is_not_prefix_stable(qg, oracle, device):
    """The teeth of the test above: without the mask the first 17 rows depend on the rows after them."""
    shape = causal_oracle.DECODER_FUSED
    X, enc = causal_oracle.decoder_inputs(shape)
    dec = _decoder(qg, shape, False)
    try:
        full = _forward(dec, X, enc, device)
        part = _forward(dec, X[:17], enc, device)
    finally:
        dec.close()
    assert_bits_equal(full, causal_oracle.decoder_expected(shape, False), "decoder without a mask")
    assert (bits(part) != bits(full[:17])).any(axis=1).all(), "an unmasked row did not depend on later rows"
    assert (bits(full) != bits(causal_oracle.decoder_expected(shape))).any(), "the mask changes nothing"


def _create_ex(qg, shape, flags):
    seq, enc_seq, d, H, dff, blocks = shape
    h = ctypes.c_void_p()
    rc = qg.load().qgemm_decoder_create_ex(d, H, dff, blocks, seq, enc_seq, causal_oracle.DECODER_SEED, flags,
                                           ctypes.byref(h))
    return rc, h


def _raw_forward(qg, h, X, enc, device):
    Xd, Ed, Y = _dev(X, device), _dev(enc, device), _nan(X.shape, device)
    rc = qg.load().qgemm_decoder_forward(h, Xd.data_ptr(), Ed.data_ptr(), Y.data_ptr(), X.shape[0], enc.shape[0],
                                         torch.cuda.current_stream(device).cuda_stream)
    assert rc == 0
    return Y.cpu().numpy()


def test_create_ex_flags(qg, oracle, device):
    """flags = 0 is qgemm_decoder_create; QGEMM_DECODER_CAUSAL masks; an unknown bit is refused with a null handle."""
    shape = causal_oracle.DECODER_FUSED
    X, enc = causal_oracle.decoder_inputs(shape)
    rc, h0 = _create_ex(qg, shape, 0)
    assert rc == 0 and h0.value
    try:
        assert_bits_equal(_raw_forward(qg, h0, X, enc, device), causal_oracle.decoder_expected(shape, False),
                          "create_ex(flags = 0)")
    finally:
        qg.load().qgemm_decoder_destroy(h0)
    rc, h1 = _create_ex(qg, shape, qg.QGEMM_DECODER_CAUSAL)
    assert rc == 0 and h1.value
    try:
        assert_bits_equal(_raw_forward(qg, h1, X, enc, device), causal_oracle.decoder_expected(shape),
                          "create_ex(QGEMM_DECODER_CAUSAL)")
    finally:
        qg.load().qgemm_decoder_destroy(h1)
    for flags in (2, 1 | 4):
        rc, h = _create_ex(qg, shape, flags)
        assert rc == qg.HIP_ERROR_INVALID_VALUE and not h.value
