"""GPU parity of qgemm_attention (self- and cross-attention) against tests/attn_oracle.attention_ref, bit for bit.

Cases are (seq_q, seq_kv, heads, d_k): the fused launch (d_k <= 64, seq_kv <= 512) on every path its code takes --
query-tile tails, a key count that is no multiple of 32 (the fl(res + 0) step) or is one, a second key chunk, d_k on
the scalar load path -- and the three-launch fallback just past either edge of the envelope; then strided views.
"""
import numpy as np
import pytest
import torch

import attn_oracle
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _qkv(oracle, seq_q, seq_kv, d, seed):
    return (oracle.uniform((seq_q, d), seed), oracle.uniform((seq_kv, d), seed + 1),
            oracle.uniform((seq_kv, d), seed + 2))


@pytest.mark.parametrize("seq_q,seq_kv,H,dk", [
    (6, 6, 4, 2),         # the reference main()'s shape
    (33, 100, 2, 24),     # query-tile tail; seq_kv % 32 != 0; d_k no multiple of 16
    (40, 257, 3, 7),      # a second key chunk holding one key; odd d_k: the scalar load path
    (100, 32, 2, 64),     # seq_kv < seq_q; seq_kv % 32 == 0: no fl(res + 0) step; full d_k
    (1, 512, 1, 64),      # a single query at the envelope's edge
    (5, 1, 2, 16),        # one key: P is exactly 1
    (20, 513, 2, 8),      # fallback: just past seq_kv
    (20, 40, 1, 65),      # fallback: just past d_k
])
def test_attention_bit_exact(qg, oracle, device, seq_q, seq_kv, H, dk):
    d = H * dk
    Q, K, V = _qkv(oracle, seq_q, seq_kv, d, 41)
    fused = qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk) == 0
    assert fused == (seq_kv <= 512 and dk <= 64)
    got = qg.attention(_dev(Q, device), _dev(K, device), _dev(V, device), H)
    want = attn_oracle.attention_ref(Q, K, V, H, attn_oracle.default_scale(dk))
    assert_bits_equal(got.cpu().numpy(), want, f"attention {seq_q}x{seq_kv} H={H} d_k={dk}")


def test_attention_explicit_scale_and_output(qg, oracle, device):
    seq_q, seq_kv, H, dk = 33, 100, 2, 24
    Q, K, V = _qkv(oracle, seq_q, seq_kv, H * dk, 43)
    out = torch.empty((seq_q, H * dk), device=device)
    got = qg.attention(_dev(Q, device), _dev(K, device), _dev(V, device), H, scale=0.375, O=out)
    assert got is out
    assert_bits_equal(out.cpu().numpy(), attn_oracle.attention_ref(Q, K, V, H, 0.375), "attention, scale 0.375")


def test_attention_qkv_column_slices(qg, oracle, device):
    """Q, K and V as the thirds of one [seq x 3d] buffer: the encoder's layout."""
    seq, H, dk = 100, 2, 24
    d = H * dk
    qkv = oracle.uniform((seq, 3 * d), 47)
    buf = _dev(qkv, device)
    got = qg.attention(buf[:, :d], buf[:, d:2 * d], buf[:, 2 * d:], H)
    want = attn_oracle.attention_ref(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], H, attn_oracle.default_scale(dk))
    assert_bits_equal(got.cpu().numpy(), want, "attention on column slices of [Q | K | V]")


@pytest.mark.parametrize("seq_q,seq_kv,H,dk", [(33, 100, 2, 24), (20, 513, 2, 8)])
def test_attention_misaligned_kv_rows(qg, oracle, device, seq_q, seq_kv, H, dk):
    """K and V with row stride d + 1: most rows are 4-byte aligned only (the per-row alignment test's scalar path;
    the fallback's general GEMM)."""
    d = H * dk
    Q, K, V = _qkv(oracle, seq_q, seq_kv, d, 53)
    Kw, Vw = (torch.zeros((seq_kv, d + 1), device=device) for _ in range(2))
    Kw[:, :d] = _dev(K, device)
    Vw[:, :d] = _dev(V, device)
    assert Kw[:, :d].stride(0) == d + 1
    got = qg.attention(_dev(Q, device), Kw[:, :d], Vw[:, :d], H)
    want = attn_oracle.attention_ref(Q, K, V, H, attn_oracle.default_scale(dk))
    assert_bits_equal(got.cpu().numpy(), want, f"attention, K / V row stride d + 1, seq_kv={seq_kv}")


@pytest.mark.parametrize("seq_q,seq_kv,H,dk", [(33, 100, 2, 24), (20, 40, 1, 65)])
def test_attention_output_slice_leaves_the_rest_untouched(qg, oracle, device, seq_q, seq_kv, H, dk):
    """O is a column slice of a wider sentinel-filled buffer with spare rows: nothing outside the slice is written."""
    d = H * dk
    Q, K, V = _qkv(oracle, seq_q, seq_kv, d, 59)
    wide = torch.full((seq_q + 3, d + 11), SENTINEL, device=device)
    out = wide[:seq_q, 5:5 + d]
    qg.attention(_dev(Q, device), _dev(K, device), _dev(V, device), H, O=out)
    w = wide.cpu().numpy()
    want = attn_oracle.attention_ref(Q, K, V, H, attn_oracle.default_scale(dk))
    assert_bits_equal(w[:seq_q, 5:5 + d], want, "attention into a column slice")
    mask = np.ones(w.shape, bool)
    mask[:seq_q, 5:5 + d] = False
    assert (w[mask] == np.float32(SENTINEL)).all(), "elements outside the output slice were written"


def test_attention_peaked_softmax(qg, oracle, device):
    """Q scaled by 60: most exps of a score row underflow to +0 and the row sums run over long runs of zeros and a
    few large terms."""
    seq_q, seq_kv, H, dk = 33, 100, 2, 24
    Q, K, V = _qkv(oracle, seq_q, seq_kv, H * dk, 61)
    Q = Q * np.float32(60.0)
    got = qg.attention(_dev(Q, device), _dev(K, device), _dev(V, device), H)
    want = attn_oracle.attention_ref(Q, K, V, H, attn_oracle.default_scale(dk))
    assert np.isfinite(want).all()
    assert_bits_equal(got.cpu().numpy(), want, "attention, Q x 60")
