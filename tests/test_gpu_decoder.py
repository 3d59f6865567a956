"""GPU parity of the decoder counterpart (transformer.cu:79-168 with quantized linears) against
tests/attn_oracle.decoder_forward_ref, bit for bit."""
import numpy as np
import pytest
import torch

import attn_oracle
from util import assert_bits_equal

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.mark.parametrize("seq,enc_seq,d,H,dff,blocks", [
    (6, 6, 8, 4, 8, 2),            # the reference main()'s shape
    (33, 100, 64, 2, 96, 2),       # tails in both sequence lengths
    (100, 40, 128, 4, 256, 1),     # enc_seq < seq
    (8, 520, 32, 2, 32, 1),        # cross-attention on the three-launch fallback (self-attention fused)
])
def test_decoder_forward_bit_exact(qg, oracle, device, seq, enc_seq, d, H, dff, blocks):
    X, enc = oracle.uniform((seq, d), 11), oracle.uniform((enc_seq, d), 12)
    dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=enc_seq, seed=13)
    try:
        Y = dec.forward(_dev(X, device), _dev(enc, device))
        torch.cuda.synchronize()
        want = attn_oracle.decoder_forward_ref(X, enc, d, H, dff, blocks, 13)
        assert_bits_equal(Y.cpu().numpy(), want,
                          f"decoder seq={seq} enc_seq={enc_seq} d={d} H={H} dff={dff} blocks={blocks}")
    finally:
        dec.close()


def test_decoder_second_forward_with_smaller_lengths(qg, oracle, device):
    """A second forward on the same object with a smaller seq and enc_seq: nothing of the first call (buffers,
    packed activations, split-K tickets) leaks into it; then the first shape again."""
    d, H, dff, blocks = 64, 2, 96, 2
    dec = qg.Decoder(d, H, dff, blocks, max_seq=33, max_enc_seq=100, seed=17)
    try:
        for seq, enc_seq in [(33, 100), (7, 21), (33, 100)]:
            X, enc = oracle.uniform((seq, d), 19), oracle.uniform((enc_seq, d), 20)
            Y = dec.forward(_dev(X, device), _dev(enc, device)).cpu().numpy()
            assert_bits_equal(Y, attn_oracle.decoder_forward_ref(X, enc, d, H, dff, blocks, 17),
                              f"decoder forward seq={seq} enc_seq={enc_seq} on a max_seq 33 / 100 object")
    finally:
        dec.close()


def test_decoder_rejects_lengths_past_its_limits(qg, device):
    dec = qg.Decoder(8, 4, 8, 1, max_seq=6, max_enc_seq=5, seed=1)
    try:
        ok = torch.zeros((6, 8), device=device)
        for seq, enc_seq in [(7, 5), (6, 6)]:
            with pytest.raises(qg.QGemmError) as ei:
                dec.forward(torch.zeros((seq, 8), device=device), torch.zeros((enc_seq, 8), device=device))
            assert ei.value.code == qg.HIP_ERROR_INVALID_VALUE
        with pytest.raises(qg.QGemmError):
            dec.forward(ok, torch.zeros((0, 8), device=device))
    finally:
        dec.close()
