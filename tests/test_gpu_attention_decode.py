"""GPU parity of attention_decode_kernel -- the launch qgemm_attention and qgemm_attention_causal take for seq_q <= 8,
d_k <= 64 -- against tests/causal_oracle.py and tests/attn_oracle.py, bit for bit.  Every shape asserts through
qgemm_attention_plan that it really lands on that kernel.  Outputs are pre-filled with NaN; past the fused envelope
the call still has to bring qgemm_attention's workspace, which is filled with 0xFF bytes (the kernel leaves it alone).

The kernel stages K and V in chunks of 128 keys, walks the row sum in passes of 1024 elements (16 per lane) and takes
32 or 64 steps per score chain: the shapes are the smallest on both sides of each of these edges."""
import functools

import numpy as np
import pytest
import torch

import attn_cases
import attn_oracle
import causal_oracle
from util import assert_bits_equal, bits

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5

# (seq_q, seq_kv, heads, d_k, q_pos0)
CAUSAL_SHAPES = (
    (1, 1, 1, 1, 0),            # the smallest call
    (1, 2, 1, 1, 1),            # two keys
    (1, 33, 2, 24, 32),         # one past a 32-pad
    (1, 129, 2, 24, 128),       # one past the kernel's own 128-key chunk
    (1, 257, 2, 24, 256),       # one past a 256-key chunk
    (1, 513, 2, 8, 512),        # first shape past the fused envelope
    (1, 1025, 1, 16, 1024),     # one past a 1024-element pass of the sum chain
    (1, 4095, 2, 33, 4094),     # odd d_k, key count not a multiple of 32
    (1, 4096, 1, 64, 4095),     # the limit
    (3, 40, 1, 33, 37),         # several query rows
    (8, 8, 1, 4, 0),            # limits 1 .. 8
    (8, 600, 2, 16, 592),       # eight rows past 512 keys
    (4, 100, 2, 8, 10),         # every row hides most keys, q_pos0 < seq_kv - seq_q
)
UNMASKED_SHAPES = (
    (1, 77, 2, 24),             # cross-attention
    (5, 513, 1, 64),            # cross-attention past 512 keys
)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _nan(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _workspace(qg, device, seq_q, seq_kv, H, dk):
    need = qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk)
    return torch.full((need,), 0xFF, dtype=torch.uint8, device=device) if need else None


def _raw(qg, Q, K, V, O, H, q_pos0, ws, stream):
    """qgemm_attention_causal (q_pos0 >= 0) or qgemm_attention (q_pos0 None) on `stream`, nothing allocated here."""
    dk = Q.shape[1] // H
    assert qg.attention_plan(Q.shape[0], K.shape[0], H, dk).startswith("attention_decode")
    L = qg.load()
    tail = (ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, stream)
    head = (Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0), O.data_ptr(), O.stride(0),
            Q.shape[0], K.shape[0], H, dk, attn_oracle.default_scale(dk))
    rc = L.qgemm_attention(*head, *tail) if q_pos0 is None else L.qgemm_attention_causal(*head, q_pos0, *tail)
    assert rc == 0, f"the attention call returned {rc}"


def _run(qg, device, Q, K, V, H, q_pos0):
    seq_q, d = Q.shape
    out = _nan((seq_q, d), device)
    ws = _workspace(qg, device, seq_q, K.shape[0], H, d // H)
    _raw(qg, _dev(Q, device), _dev(K, device), _dev(V, device), out, H, q_pos0, ws,
         torch.cuda.current_stream(device).cuda_stream)
    if ws is not None:
        assert bool((ws == 0xFF).all()), "the decode launch wrote into the workspace"
    return out.cpu().numpy()


def _want(Q, K, V, H, q_pos0):
    scale = attn_oracle.default_scale(Q.shape[1] // H)
    if q_pos0 is None:
        return attn_oracle.attention_ref(Q, K, V, H, scale)
    return causal_oracle.attention_causal_ref(Q, K, V, H, scale, q_pos0)


@functools.lru_cache(maxsize=None)
def _expected(shape):
    Q, K, V = causal_oracle.qkv(shape)
    want = causal_oracle.attention_causal_ref(Q, K, V, shape[2], attn_oracle.default_scale(shape[3]), shape[4])
    want.flags.writeable = False
    return want


@pytest.mark.parametrize("shape", CAUSAL_SHAPES, ids=str)
def test_decode_causal_bit_exact(qg, oracle, device, shape):
    seq_q, seq_kv, H, dk, q_pos0 = shape
    Q, K, V = causal_oracle.qkv(shape)
    assert_bits_equal(_run(qg, device, Q, K, V, H, q_pos0), _expected(shape), f"decode attention {shape}")


@pytest.mark.parametrize("shape", UNMASKED_SHAPES, ids=str)
def test_decode_unmasked_bit_exact(qg, oracle, device, shape):
    seq_q, seq_kv, H, dk = shape
    Q, K, V = causal_oracle.qkv(shape + (0,), 307)
    assert_bits_equal(_run(qg, device, Q, K, V, H, None), _want(Q, K, V, H, None), f"decode attention {shape}, no mask")


@pytest.mark.parametrize("shape", [(3, 100, 2, 24), (2, 513, 2, 8)], ids=str)
def test_mask_without_effect_equals_the_unmasked_call(qg, oracle, device, shape):
    """q_pos0 = seq_kv - 1 and far past it: qgemm_attention's bits, from the GPU and from the oracle."""
    seq_q, seq_kv, H, dk = shape
    Q, K, V = causal_oracle.qkv(shape + (0,), 311)
    plain = _run(qg, device, Q, K, V, H, None)
    assert_bits_equal(plain, _want(Q, K, V, H, None), "attention")
    for q_pos0 in (seq_kv - 1, seq_kv, 2 ** 31 - 1):
        assert_bits_equal(_run(qg, device, Q, K, V, H, q_pos0), plain, f"causal attention with q_pos0 = {q_pos0}")


@pytest.mark.parametrize("pos,n", [(0, 1), (37, 1), (130, 3), (192, 8)], ids=str)
def test_queries_are_rows_of_the_cache_they_attend_to(qg, oracle, device, pos, n):
    """The decoder cache's layout: one [Q | K | V] buffer of max_seq rows; the queries are its rows pos .. pos + n - 1
    (first third), the keys and values its rows 0 .. pos + n - 1 (second and third).  The rows past pos + n hold NaN."""
    H, dk, max_seq = 2, 24, 200
    d = H * dk
    qkv = oracle.uniform((max_seq, 3 * d), 313)
    qkv[pos + n:] = np.nan
    buf = _dev(qkv, device)
    kv = pos + n
    out = _nan((n, d), device)
    _raw(qg, buf[pos:kv, :d], buf[:kv, d:2 * d], buf[:kv, 2 * d:], out, H, pos, None,
         torch.cuda.current_stream(device).cuda_stream)
    want = _want(qkv[pos:kv, :d], qkv[:kv, d:2 * d], qkv[:kv, 2 * d:], H, pos)
    assert np.isfinite(want).all()
    assert_bits_equal(out.cpu().numpy(), want, f"rows {pos} .. {kv - 1} of a [Q | K | V] cache")


def test_misaligned_column_slices_and_a_guarded_output_slice(qg, oracle, device):
    """K and V as column slices that start 4 and 12 bytes past a 16-byte boundary, with an odd row stride (the scalar
    path of the staging), Q likewise; the output a slice of a wider sentinel-filled buffer."""
    shape = (3, 140, 2, 24, 135)
    seq_q, seq_kv, H, dk, q_pos0 = shape
    d = H * dk
    Q, K, V = causal_oracle.qkv(shape)
    wq, wk, wv = (torch.zeros((r, d + 7), device=device) for r in (seq_q, seq_kv, seq_kv))
    wq[:, 3:3 + d], wk[:, 1:1 + d], wv[:, 3:3 + d] = _dev(Q, device), _dev(K, device), _dev(V, device)
    wide = torch.full((seq_q + 3, d + 11), SENTINEL, device=device)
    out = wide[1:1 + seq_q, 5:5 + d]
    _raw(qg, wq[:, 3:3 + d], wk[:, 1:1 + d], wv[:, 3:3 + d], out, H, q_pos0, None,
         torch.cuda.current_stream(device).cuda_stream)
    w = wide.cpu().numpy()
    assert_bits_equal(w[1:1 + seq_q, 5:5 + d], _expected(shape), "decode attention on misaligned slices")
    mask = np.ones(w.shape, bool)
    mask[1:1 + seq_q, 5:5 + d] = False
    assert (w[mask] == np.float32(SENTINEL)).all(), "elements outside the output slice were written"


@pytest.mark.parametrize("shape", [
    (4, 100, 2, 24, 10),     # limits 11 .. 14: keys 14 .. 99 are staged with the first chunk but never scored
    (2, 300, 2, 24, 100),    # limits 101, 102: the second and third K chunks are never staged
    (8, 600, 2, 16, 200),    # past the fused envelope
], ids=str)
def test_nan_in_unseen_k_rows_changes_nothing(qg, oracle, device, shape):
    """K rows that no query of the call sees hold NaN -- the keys a row's own chunk stages but its limit hides, and
    the rows past the last limit: the output is the composition's, which is the clean input's."""
    seq_q, seq_kv, H, dk, q_pos0 = shape
    Q, K, V = causal_oracle.qkv(shape, 317)
    lmax = int(causal_oracle.limits(seq_q, seq_kv, q_pos0).max())
    assert lmax < seq_kv
    Kn = K.copy()
    Kn[lmax:] = np.nan
    clean = _want(Q, K, V, H, q_pos0)
    assert np.isfinite(clean).all()
    assert_bits_equal(_want(Q, Kn, V, H, q_pos0), clean, "the composition itself")
    assert_bits_equal(_run(qg, device, Q, Kn, V, H, q_pos0), clean, f"NaN in K rows {lmax} .. of {shape}")


def test_nan_in_k_rows_masked_for_some_rows_only(qg, oracle, device):
    """NaN in the K row that only the last query sees: the other rows computed nothing from it."""
    shape = (4, 20, 1, 8, 16)
    seq_q, seq_kv, H, dk, q_pos0 = shape
    Q, K, V = causal_oracle.qkv(shape, 331)
    K[19] = np.nan
    want = _want(Q, K, V, H, q_pos0)
    assert np.isfinite(want[:3]).all() and np.isnan(want[3]).all()
    assert_bits_equal(_run(qg, device, Q, K, V, H, q_pos0), want, "NaN in the last key")


@pytest.mark.parametrize("shape,key,col", [((8, 33, 2, 24, 20), 24, 5), ((8, 600, 2, 16, 592), 596, 11)], ids=str)
def test_inf_in_v_at_a_partly_masked_key(qg, oracle, device, shape, key, col):
    """+inf in V at a key that some rows see and some do not: +inf where P > 0, NaN (fmaf(+0, inf, acc)) where the key
    is masked -- the masked tail of P V is not skipped."""
    seq_q, seq_kv, H, dk, q_pos0 = shape
    Q, K, V = causal_oracle.qkv(shape, 337)
    V[key, col] = np.inf
    want = _want(Q, K, V, H, q_pos0)
    sees = causal_oracle.limits(seq_q, seq_kv, q_pos0) > key
    assert sees.any() and (~sees).any()
    assert np.isposinf(want[sees, col]).all() and np.isnan(want[~sees, col]).all()
    assert np.isfinite(np.delete(want, col, axis=1)).all()
    assert_bits_equal(_run(qg, device, Q, K, V, H, q_pos0), want, f"inf at V[{key}, {col}] of {shape}")


DECODE_SPECIAL = (8, 100, 2, 24)   # attn_cases' sets (they touch Q rows 4 and 5, key 37) with 8 query rows


@functools.lru_cache(maxsize=None)
def _special_expected(name):
    Q, K, V = attn_cases.attention_sets(DECODE_SPECIAL)[name][0]
    return attn_oracle.attention_ref(Q, K, V, DECODE_SPECIAL[2], attn_oracle.default_scale(DECODE_SPECIAL[3]))


@pytest.mark.parametrize("name", attn_cases.ATTENTION_NAMES)
def test_special_values(qg, oracle, device, name):
    (Q, K, V), what = attn_cases.attention_sets(DECODE_SPECIAL)[name]
    want = _special_expected(name)
    if name in ("nan_in_k", "inf_in_v_peaked", "overflowing_scores"):
        assert np.isnan(want).any(), what
    if name == "inf_in_v":
        assert np.isposinf(want[:, 30]).all(), what
    if name == "neg_zero_v":
        assert (bits(want) == 0).all(), what
    assert_bits_equal(_run(qg, device, Q, K, V, DECODE_SPECIAL[2], None), want, f"{name}: {what}")


def test_two_calls_back_to_back_with_different_q_pos0(qg, oracle, device):
    """The same inputs with q_pos0 = 0 and then 5 on one stream, no synchronize between: q_pos0 is per call."""
    shape = (8, 40, 2, 24)
    Q, K, V = causal_oracle.qkv(shape + (0,), 347)
    Qd, Kd, Vd = (_dev(a, device) for a in (Q, K, V))
    outs = _nan((2, 8, 48), device)
    s = torch.cuda.current_stream(device).cuda_stream
    _raw(qg, Qd, Kd, Vd, outs[0], 2, 0, None, s)
    _raw(qg, Qd, Kd, Vd, outs[1], 2, 5, None, s)
    got = outs.cpu().numpy()
    want = [_want(Q, K, V, 2, p) for p in (0, 5)]
    assert (bits(want[0]) != bits(want[1])).any()
    assert_bits_equal(got[0], want[0], "q_pos0 = 0")
    assert_bits_equal(got[1], want[1], "q_pos0 = 5")


def test_decode_repeat_screen(qg, oracle, device):
    """20 calls at 8 x 1300, 4 heads of 64, q_pos0 = 1275 (32 workgroups, eleven key chunks, two passes of the sum
    chain, limits on both sides of a chunk edge), each into its own NaN-filled output."""
    seq_q, seq_kv, H, dk, q_pos0 = 8, 1300, 4, 64, 1275
    Q, K, V = causal_oracle.qkv((seq_q, seq_kv, H, dk, q_pos0), 349)
    want = _want(Q, K, V, H, q_pos0)
    Qd, Kd, Vd = (_dev(a, device) for a in (Q, K, V))
    outs = _nan((20, seq_q, H * dk), device)
    ws = _workspace(qg, device, seq_q, seq_kv, H, dk)
    s = torch.cuda.current_stream(device).cuda_stream
    for i in range(20):
        _raw(qg, Qd, Kd, Vd, outs[i], H, q_pos0, ws, s)
    got = outs.cpu().numpy()
    for i in range(20):
        assert_bits_equal(got[i], want, f"decode attention repeat {i}")


@pytest.mark.parametrize("shape", [(1, 100, 2, 24, 99), (8, 600, 2, 16, 592)], ids=str)
def test_decode_graph_capture_and_replay(qg, oracle, device, shape):
    """The call allocates nothing and does not synchronize: captured into static buffers, replayed on new inputs."""
    seq_q, seq_kv, H, dk, q_pos0 = shape
    d = H * dk
    Qs, Ks, Vs = (torch.zeros(sh, device=device) for sh in ((seq_q, d), (seq_kv, d), (seq_kv, d)))
    out = _nan((seq_q, d), device)
    ws = _workspace(qg, device, seq_q, seq_kv, H, dk)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        _raw(qg, Qs, Ks, Vs, out, H, q_pos0, ws, s.cuda_stream)   # warm-up: module load, first launch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _raw(qg, Qs, Ks, Vs, out, H, q_pos0, ws, s.cuda_stream)
    for i in range(3):
        Q, K, V = causal_oracle.qkv(shape, 353 + 3 * i)
        for dst, src in ((Qs, Q), (Ks, K), (Vs, V)):
            dst.copy_(_dev(src, device))
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), _want(Q, K, V, H, q_pos0), f"decode attention graph replay {i} {shape}")
