"""GPU parity of qgemm_attention_causal and qgemm_softmax_rows_causal against tests/causal_oracle.py, bit for bit, on
the fused launch and on the three-launch fallback.  Every call goes into a NaN-filled output, a fallback's workspace is
filled with 0xFF bytes first.  tests/test_causal_host.py shows on the CPU that the expected values really mask (every
masked row differs from the unmasked result), so none of these passes on an unmasked kernel."""
import numpy as np
import pytest
import torch

import attn_oracle
import causal_oracle
from util import assert_bits_equal, bits

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _workspace(qg, device, seq_q, seq_kv, H, dk):
    need = qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk)
    return torch.full((need,), 0xFF, dtype=torch.uint8, device=device) if need else None


def _raw(qg, Q, K, V, O, H, q_pos0, ws, stream):
    """qgemm_attention_causal on `stream` (a raw handle), nothing allocated here."""
    dk = Q.shape[1] // H
    rc = qg.load().qgemm_attention_causal(Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(),
                                          V.stride(0), O.data_ptr(), O.stride(0), Q.shape[0], K.shape[0], H, dk,
                                          attn_oracle.default_scale(dk), q_pos0,
                                          ws.data_ptr() if ws is not None else None,
                                          ws.numel() if ws is not None else 0, stream)
    assert rc == 0, f"qgemm_attention_causal returned {rc}"


def _run(qg, device, Q, K, V, H, q_pos0):
    seq_q, d = Q.shape
    out = _nan((seq_q, d), device)
    ws = _workspace(qg, device, seq_q, K.shape[0], H, d // H)
    _raw(qg, _dev(Q, device), _dev(K, device), _dev(V, device), out, H, q_pos0, ws,
         torch.cuda.current_stream(device).cuda_stream)
    return out.cpu().numpy()


def _want(Q, K, V, H, q_pos0):
    return causal_oracle.attention_causal_ref(Q, K, V, H, attn_oracle.default_scale(Q.shape[1] // H), q_pos0)


def _fused(qg, shape):
    return qg.load().qgemm_attention_workspace_size(*shape[:4]) == 0


@pytest.mark.parametrize("shape", causal_oracle.SHAPES, ids=str)
def test_attention_causal_bit_exact(qg, oracle, device, shape):
    seq_q, seq_kv, H, dk, q_pos0 = shape
    assert _fused(qg, shape) == (seq_kv <= 512 and dk <= 64)
    Q, K, V = causal_oracle.qkv(shape)
    assert_bits_equal(_run(qg, device, Q, K, V, H, q_pos0), causal_oracle.expected(shape), f"causal attention {shape}")


@pytest.mark.parametrize("shape", [(33, 100, 2, 24), (20, 513, 2, 8)], ids=["fused", "fallback"])
def test_mask_without_effect_equals_attention(qg, oracle, device, shape):
    """q_pos0 = seq_kv - 1 and far past it: qgemm_attention's bits, from the GPU and from the oracle."""
    seq_q, seq_kv, H, dk = shape
    Q, K, V = causal_oracle.qkv(shape + (0,), 231)
    Qd, Kd, Vd = (_dev(a, device) for a in (Q, K, V))
    plain = qg.attention(Qd, Kd, Vd, H).cpu().numpy()
    assert_bits_equal(plain, attn_oracle.attention_ref(Q, K, V, H, attn_oracle.default_scale(dk)), "attention")
    for q_pos0 in (seq_kv - 1, seq_kv, 2 ** 31 - 1):
        got = qg.attention(Qd, Kd, Vd, H, O=_nan((seq_q, H * dk), device), causal=True, q_pos0=q_pos0)
        assert_bits_equal(got.cpu().numpy(), plain, f"causal attention with q_pos0 = {q_pos0}")


def test_python_default_q_pos0_aligns_queries_to_the_end_of_the_keys(qg, oracle, device):
    shape = (40, 289, 2, 24, 249)   # 249 = 289 - 40
    Q, K, V = causal_oracle.qkv(shape)
    got = qg.attention(_dev(Q, device), _dev(K, device), _dev(V, device), 2, causal=True)
    assert_bits_equal(got.cpu().numpy(), causal_oracle.expected(shape), "attention(causal=True), default q_pos0")
    with pytest.raises(AssertionError):
        qg.attention(_dev(K, device), _dev(Q, device), _dev(Q, device), 2, causal=True)   # seq_kv < seq_q


def test_attention_causal_qkv_column_slices(qg, oracle, device):
    """Q, K and V as the thirds of one [seq x 3d] buffer: the decoder's self-attention layout."""
    seq, H, dk = 70, 2, 24
    d = H * dk
    qkv = oracle.uniform((seq, 3 * d), 233)
    buf = _dev(qkv, device)
    got = qg.attention(buf[:, :d], buf[:, d:2 * d], buf[:, 2 * d:], H, O=_nan((seq, d), device), causal=True)
    assert_bits_equal(got.cpu().numpy(), _want(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], H, 0),
                      "causal attention on column slices of [Q | K | V]")


@pytest.mark.parametrize("shape", [(33, 33, 2, 24, 0), (20, 40, 1, 65, 20)], ids=["fused", "fallback"])
def test_attention_causal_output_slice_leaves_the_rest_untouched(qg, oracle, device, shape):
    seq_q, seq_kv, H, dk, q_pos0 = shape
    d = H * dk
    Q, K, V = causal_oracle.qkv(shape)
    wide = torch.full((seq_q + 3, d + 11), SENTINEL, device=device)
    out = wide[:seq_q, 5:5 + d]
    qg.attention(_dev(Q, device), _dev(K, device), _dev(V, device), H, O=out, causal=True, q_pos0=q_pos0)
    w = wide.cpu().numpy()
    assert_bits_equal(w[:seq_q, 5:5 + d], causal_oracle.expected(shape), "causal attention into a column slice")
    mask = np.ones(w.shape, bool)
    mask[:seq_q, 5:5 + d] = False
    assert (w[mask] == np.float32(SENTINEL)).all(), "elements outside the output slice were written"


@pytest.mark.parametrize("shape", [
    (33, 100, 2, 24, 10),     # fused: limits 11 .. 43; columns 43 .. 47 are computed (raw NaN scores), 48 .. never
    (40, 289, 2, 24, 100),    # fused: limits 101 .. 140; the second key chunk is never staged
    (20, 513, 2, 8, 100),     # fallback: every score is computed, the softmax reads none past its limit
], ids=str)
def test_nan_in_unseen_k_rows_changes_nothing(qg, oracle, device, shape):
    """K rows that no query of the call sees hold NaN: the output is the composition's, which is the clean input's --
    a masked score that reached the max, the sum or P V (raw, or stale LDS never zeroed) would show as NaN."""
    seq_q, seq_kv, H, dk, q_pos0 = shape
    Q, K, V = causal_oracle.qkv(shape, 241)
    lmax = int(causal_oracle.limits(seq_q, seq_kv, q_pos0).max())
    assert lmax < seq_kv
    Kn = K.copy()
    Kn[lmax:] = np.nan
    clean = _want(Q, K, V, H, q_pos0)
    assert np.isfinite(clean).all()
    assert_bits_equal(_want(Q, Kn, V, H, q_pos0), clean, "the composition itself")
    assert_bits_equal(_run(qg, device, Q, Kn, V, H, q_pos0), clean, f"NaN in K rows {lmax} .. of {shape}")


@pytest.mark.parametrize("shape,key,col", [((33, 33, 2, 24, 0), 20, 5), ((20, 513, 2, 8, 493), 505, 11)],
                         ids=["fused", "fallback"])
def test_inf_in_v_at_a_partly_masked_key(qg, oracle, device, shape, key, col):
    """+inf in V at a key that some rows see and some do not: +inf where P > 0, NaN (fmaf(+0, inf, acc)) where the key
    is masked -- the composition's bits on both paths."""
    seq_q, seq_kv, H, dk, q_pos0 = shape
    Q, K, V = causal_oracle.qkv(shape, 251)
    V[key, col] = np.inf
    want = _want(Q, K, V, H, q_pos0)
    sees = causal_oracle.limits(seq_q, seq_kv, q_pos0) > key
    assert sees.any() and (~sees).any()
    assert np.isposinf(want[sees, col]).all() and np.isnan(want[~sees, col]).all()
    assert np.isfinite(np.delete(want, col, axis=1)).all()
    assert_bits_equal(_run(qg, device, Q, K, V, H, q_pos0), want, f"inf at V[{key}, {col}] of {shape}")


def test_two_calls_back_to_back_with_different_q_pos0(qg, oracle, device):
    """The same inputs with q_pos0 = 0 and then 5 on one stream, no synchronize between: q_pos0 is per call."""
    shape = (33, 40, 2, 24)
    Q, K, V = causal_oracle.qkv(shape + (0,), 257)
    Qd, Kd, Vd = (_dev(a, device) for a in (Q, K, V))
    outs = _nan((2, 33, 48), device)
    s = torch.cuda.current_stream(device).cuda_stream
    _raw(qg, Qd, Kd, Vd, outs[0], 2, 0, None, s)
    _raw(qg, Qd, Kd, Vd, outs[1], 2, 5, None, s)
    got = outs.cpu().numpy()
    want = [_want(Q, K, V, 2, p) for p in (0, 5)]
    assert (bits(want[0]) != bits(want[1])).any()
    assert_bits_equal(got[0], want[0], "q_pos0 = 0")
    assert_bits_equal(got[1], want[1], "q_pos0 = 5")


def test_attention_causal_repeat_screen(qg, oracle, device):
    """20 calls of the fused kernel at 96 x 300, 4 heads of 64, q_pos0 = 204 (12 workgroups; the second key chunk runs
    in some tiles only; skipped column tiles beside live ones), each into its own NaN-filled output."""
    seq_q, seq_kv, H, dk, q_pos0 = 96, 300, 4, 64, 204
    Q, K, V = causal_oracle.qkv((seq_q, seq_kv, H, dk, q_pos0), 263)
    want = _want(Q, K, V, H, q_pos0)
    Qd, Kd, Vd = (_dev(a, device) for a in (Q, K, V))
    outs = _nan((20, seq_q, H * dk), device)
    s = torch.cuda.current_stream(device).cuda_stream
    for i in range(20):
        _raw(qg, Qd, Kd, Vd, outs[i], H, q_pos0, None, s)
    got = outs.cpu().numpy()
    for i in range(20):
        assert_bits_equal(got[i], want, f"causal attention repeat {i}")


@pytest.mark.parametrize("shape", [(33, 100, 2, 24, 67), (20, 513, 2, 8, 493)], ids=["fused", "fallback"])
def test_attention_causal_graph_capture_and_replay(qg, oracle, device, shape):
    """qgemm_attention_causal allocates nothing and does not synchronize on either path: one call is captured into
    static buffers and replayed three times on new inputs."""
    seq_q, seq_kv, H, dk, q_pos0 = shape
    d = H * dk
    Qs, Ks, Vs = (torch.zeros(sh, device=device) for sh in ((seq_q, d), (seq_kv, d), (seq_kv, d)))
    out = _nan((seq_q, d), device)
    ws = _workspace(qg, device, seq_q, seq_kv, H, dk)
    assert (ws is None) == (seq_kv <= 512)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        _raw(qg, Qs, Ks, Vs, out, H, q_pos0, ws, s.cuda_stream)   # warm-up: module load, first launch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _raw(qg, Qs, Ks, Vs, out, H, q_pos0, ws, s.cuda_stream)
    for i in range(3):
        Q, K, V = causal_oracle.qkv(shape, 271 + 3 * i)
        for dst, src in ((Qs, Q), (Ks, K), (Vs, V)):
            dst.copy_(_dev(src, device))
        out.fill_(float("nan"))
        if ws is not None:
            ws.fill_(0xFF)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), _want(Q, K, V, H, q_pos0), f"causal attention graph replay {i} {shape}")


@pytest.mark.parametrize("seq_q,w,q_pos0,scale", [(5, 9, 2, 0.5), (33, 200, 0, 1.0), (7, 1, 0, 1.0),
                                                  (20, 513, 493, 0.35355338), (4, 70, 500, 2.0)])
def test_softmax_rows_causal_in_place_and_out_of_place(qg, oracle, device, seq_q, w, q_pos0, scale):
    """A stack of 3 matrices of seq_q rows; the masked scores hold NaN, which the kernel must not read; out of place
    into a NaN-filled P, then in place."""
    S = oracle.uniform((3, seq_q, w), 281) * np.float32(6.0)
    L = causal_oracle.limits(seq_q, w, q_pos0)
    for i in range(seq_q):
        S[:, i, L[i]:] = np.nan
    want = causal_oracle.softmax_rows_causal(S, seq_q, q_pos0, scale)
    assert np.isfinite(want).all()
    Sd = _dev(S, device)
    P = _nan((3, seq_q, w), device)
    got = qg.softmax_rows_causal(Sd, seq_q, q_pos0, scale, P=P)
    assert got is P
    assert_bits_equal(P.cpu().numpy(), want, "softmax_rows_causal out of place")
    assert_bits_equal(Sd.cpu().numpy(), S, "the input of an out-of-place call")
    qg.softmax_rows_causal(Sd, seq_q, q_pos0, scale, P=Sd)
    assert_bits_equal(Sd.cpu().numpy(), want, "softmax_rows_causal in place")
