"""GPU parity of qgemm_attention (self- and cross-attention) against tests/attn_oracle.attention_ref, bit for bit.

Cases are (seq_q, seq_kv, heads, d_k): the fused launch (d_k <= 64, seq_kv <= 512) on every path its code takes --
query-tile tails, a key count that is no multiple of 32 (the fl(res + 0) step) or is one, a second key chunk, d_k on
the scalar load path -- and the three-launch fallback just past either edge of the envelope; then strided views.  Further down: special values
(tests/attn_cases.py) on both paths, a seeded shape fuzz, a repeat screen, graph capture and replay, two streams.
"""
import numpy as np
import pytest
import torch

import attn_cases
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
    # d_k in 33 .. 63: 16 k-steps over a partly padded head, a third, partly masked P V column tile
    (17, 96, 2, 33),      # 31 padded columns; the last float4 of a row holds one real column; head 1 starts 33 floats
                          # in (every K / V piece on the scalar load path); the third column tile has one live column
    (31, 255, 1, 63),     # one chunk minus a key; one head column short of full
    (32, 256, 2, 48),     # exactly one full query tile and one full chunk; three full P V column tiles
    (65, 511, 1, 40),     # three query tiles, a one-row tail; the second chunk has 255 keys; the last lane of the sum
                          # chain is one element short
    (64, 512, 3, 1),      # d_k = 1
    (2, 17, 1, 64),       # two lanes carry the row sum
])
def test_attention_bit_exact(qg, oracle, device, seq_q, seq_kv, H, dk):
    d = H * dk
    Q, K, V = _qkv(oracle, seq_q, seq_kv, d, 41)
    fused = qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk) == 0
    assert fused == (seq_kv <= 512 and dk <= 64)
    out = torch.full((seq_q, d), float("nan"), device=device)
    got = qg.attention(_dev(Q, device), _dev(K, device), _dev(V, device), H, O=out)
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


# ---- special values, a seeded shape fuzz, repeats, graphs and streams.  These go through the C entry: the output is
# pre-filled with NaN and a fallback's workspace with 0xFF bytes, so no stale buffer can pass ----

def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _workspace(qg, device, seq_q, seq_kv, H, dk):
    """The fallback's scores, every byte 0xFF (a NaN pattern); None inside the fused envelope."""
    need = qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk)
    return torch.full((need,), 0xFF, dtype=torch.uint8, device=device) if need else None


def _raw(qg, Q, K, V, O, H, ws, stream, scale=None):
    """qgemm_attention on `stream` (a raw handle), nothing allocated here."""
    dk = Q.shape[1] // H
    rc = qg.load().qgemm_attention(Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0),
                                   O.data_ptr(), O.stride(0), Q.shape[0], K.shape[0], H, dk,
                                   attn_oracle.default_scale(dk) if scale is None else scale,
                                   ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                   stream)
    assert rc == 0, f"qgemm_attention returned {rc}"


def _run(qg, device, Q, K, V, H):
    seq_q, d = Q.shape
    out = _nan((seq_q, d), device)
    ws = _workspace(qg, device, seq_q, K.shape[0], H, d // H)
    _raw(qg, _dev(Q, device), _dev(K, device), _dev(V, device), out, H, ws,
         torch.cuda.current_stream(device).cuda_stream)
    return out.cpu().numpy()


def _want(Q, K, V, H):
    return attn_oracle.attention_ref(Q, K, V, H, attn_oracle.default_scale(Q.shape[1] // H))


def _attn_fuzz_shapes(count=24, seed=20261019):
    """Seeded (seq_q, seq_kv, H, d_k) inside the fused envelope: seq_q in [1, 70], seq_kv in [1, 512], d_k in [1, 64],
    H in [1, 3]; every other one log-uniform (small, ragged), the rest uniform."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        if i % 2:
            sq, skv, dk = (int(round(np.exp(rng.uniform(0.0, np.log(hi))))) for hi in (70, 512, 64))
        else:
            sq, skv, dk = (int(rng.integers(1, hi + 1)) for hi in (70, 512, 64))
        out.append((max(1, sq), max(1, skv), int(rng.integers(1, 4)), max(1, dk)))
    return out


@pytest.mark.parametrize("seq_q,seq_kv,H,dk", _attn_fuzz_shapes())
def test_attention_seeded_shape_fuzz(qg, oracle, device, seq_q, seq_kv, H, dk):
    """The fused kernel at shapes drawn from a fixed seed, not hand-picked: query-tile tails, chunk tails, k-step
    counts, load paths and live P V column tiles in whatever combination the draw gives."""
    assert qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk) == 0
    Q, K, V = _qkv(oracle, seq_q, seq_kv, H * dk, 71 + seq_q + seq_kv + H + dk)
    assert_bits_equal(_run(qg, device, Q, K, V, H), _want(Q, K, V, H),
                      f"attention fuzz {seq_q}x{seq_kv} H={H} d_k={dk}")


@pytest.mark.parametrize("name", attn_cases.ATTENTION_NAMES)
@pytest.mark.parametrize("shape", [attn_cases.ATTN_BASE, attn_cases.ATTN_FALLBACK], ids=["fused", "fallback"])
def test_attention_special_values(qg, device, shape, name):
    """NaN, +inf, 0 * inf, an all-zero query, overflowing scores, -0 and subnormal values (tests/attn_cases.py; each
    set's condition is asserted on the oracle by tests/test_attn_oracle_host.py) through the fused kernel's MFMA chains,
    lane-reduced max and lane-hop sum, and through the fallback's gemm_f32 + softmax_rows_kernel + gemm_f32: the same
    bits and the same NaN positions as the oracle on both."""
    seq_q, seq_kv, H, dk = shape
    assert (qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk) == 0) == (shape == attn_cases.ATTN_BASE)
    (Q, K, V), what = attn_cases.attention_sets(shape)[name]
    assert_bits_equal(_run(qg, device, Q, K, V, H), attn_cases.attention_expected(name, shape),
                      f"attention {seq_q}x{seq_kv}, {what}")


def test_attention_repeat_screen(qg, oracle, device):
    """20 calls of the fused kernel on one set of inputs at 128 x 300, 8 heads of 64 (32 workgroups, two key chunks,
    full d_k), each into its own NaN-filled output: a race between the phases that share S and the K / V stage (the
    wave-level waits before the sum chain, the chunk barriers) would not give the oracle's bits 20 times."""
    seq_q, seq_kv, H, dk = 128, 300, 8, 64
    Q, K, V = _qkv(oracle, seq_q, seq_kv, H * dk, 67)
    want = _want(Q, K, V, H)
    Qd, Kd, Vd = (_dev(a, device) for a in (Q, K, V))
    outs = _nan((20, seq_q, H * dk), device)
    s = torch.cuda.current_stream(device).cuda_stream
    for i in range(20):
        _raw(qg, Qd, Kd, Vd, outs[i], H, None, s)
    got = outs.cpu().numpy()
    for i in range(20):
        assert_bits_equal(got[i], want, f"attention repeat {i}")


@pytest.mark.parametrize("seq_q,seq_kv,H,dk", [(33, 100, 2, 24), (20, 513, 2, 8)], ids=["fused", "fallback"])
def test_attention_graph_capture_and_replay(qg, oracle, device, seq_q, seq_kv, H, dk):
    """qgemm_attention allocates nothing and does not synchronize on either path: after a warm-up on the side stream
    one call is captured into static buffers (the fallback's workspace allocated before the capture) and replayed three
    times on new inputs; every replay gives the oracle's bits for the inputs then in the buffers."""
    d = H * dk
    Qs, Ks, Vs = (torch.zeros(sh, device=device) for sh in ((seq_q, d), (seq_kv, d), (seq_kv, d)))
    out = _nan((seq_q, d), device)
    ws = _workspace(qg, device, seq_q, seq_kv, H, dk)
    assert (ws is None) == (seq_kv <= 512)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        _raw(qg, Qs, Ks, Vs, out, H, ws, s.cuda_stream)   # warm-up: module load, first launch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _raw(qg, Qs, Ks, Vs, out, H, ws, s.cuda_stream)
    for i in range(3):
        Q, K, V = _qkv(oracle, seq_q, seq_kv, d, 101 + 3 * i)
        for dst, src in ((Qs, Q), (Ks, K), (Vs, V)):
            dst.copy_(_dev(src, device))
        out.fill_(float("nan"))
        if ws is not None:
            ws.fill_(0xFF)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), _want(Q, K, V, H), f"attention graph replay {i}, seq_kv={seq_kv}")


def test_attention_concurrent_streams(qg, oracle, device):
    """The fallback on stream A (its own workspace) and the fused kernel on stream B, five interleaved rounds with
    different inputs and one synchronize at the end: nothing is shared between calls but what the caller passes."""
    shapes = [(20, 513, 2, 8), (33, 100, 2, 24)]
    lanes = []
    for li, (seq_q, seq_kv, H, dk) in enumerate(shapes):
        d = H * dk
        rounds = []
        for r in range(5):
            Q, K, V = _qkv(oracle, seq_q, seq_kv, d, 131 + 10 * li + 3 * r)
            rounds.append((_dev(Q, device), _dev(K, device), _dev(V, device), _nan((seq_q, d), device),
                           _want(Q, K, V, H)))
        lanes.append((H, _workspace(qg, device, seq_q, seq_kv, H, dk), torch.cuda.Stream(device), rounds))
    assert lanes[0][1] is not None and lanes[1][1] is None
    torch.cuda.synchronize()
    for r in range(5):
        for H, ws, s, rounds in lanes:
            Qd, Kd, Vd, out, _ = rounds[r]
            _raw(qg, Qd, Kd, Vd, out, H, ws, s.cuda_stream)
    torch.cuda.synchronize()
    for li, (_, _, _, rounds) in enumerate(lanes):
        for r, (_, _, _, out, want) in enumerate(rounds):
            assert_bits_equal(out.cpu().numpy(), want, f"attention stream {li} round {r}")
