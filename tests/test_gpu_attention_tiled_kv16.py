"""Tiled prefill attention over a bf16 K / V cache on the GPU (qgemm_attention_varlen_tiled_kv16).  Inputs
are N(0, 1) from a fixed seed, K / V rounded to bf16 once on the host: the bf16 tensors go to the new call, their
.float() to the references.  Two references: attention_varlen_tiled of the same build on the widened K / V, bit for bit
(the sharp half), and float64 numpy softmax attention with the yardstick e32 = max |the same formula in numpy fp32 -
float64| and the project's bound 8 e32.  Figures of one run (e32, error per case): DESIGN.md s37."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_attention_tiled import _attend, _layout
from util import assert_bits_equal

pytestmark = pytest.mark.gpu
FACTOR = 8
BF16_INF, BF16_NAN = 0x7F80, 0x7FC0

# (heads, KV heads, d_k, seq_q, seq_kv, q_pos0: None / "zero" / "tail" (seq_kv - seq_q) / values, K / V views one element
#  past 16 bytes with an odd stride)
CASES = [
    (6, 2, 20, (1, 17, 65), (1, 63, 129), None, True),              # element loads, d_k % 4 != 0, a one-key sequence
    (14, 2, 64, (33, 130, 15), (33, 130, 15), "zero", False),       # square causal: partial tiles, waves pass over chunks
    (8, 8, 96, (64, 65, 3), (513, 600, 4097), "tail", False),       # G 1, 3/4 of the column tiles, many chunks
    (32, 2, 128, (70, 1, 16), (8200, 5000, 1025), (3000, 4999, 0), False),  # G 16, wide, mid-cache
    (4, 1, 128, (130, 0, 2), (257, 40, 64), "zero", False),         # an empty sequence; a chunk exactly full
    (4, 2, 64, (5, 5, 5, 5, 5), (64, 65, 128, 129, 193), None, False),   # one, two, three, four chunks: both buffers
    (2, 1, 128, (5, 5, 5, 5, 5), (64, 65, 128, 129, 193), "tail", False),  # ... of the wide kernel
    (2, 1, 64, (3,), (131072,), "tail", False),                     # the key cap
]


@functools.lru_cache(maxsize=None)
def _case(i):
    """The inputs of case i, its float64 reference on the widened inputs and e32 -- computed once, never changed."""
    H, n_kv, dk, seq_q, seq_kv, mask, _ = CASES[i]
    pos, q0, k0, nq, nk = _layout(seq_q, seq_kv, mask, None)
    rng = np.random.default_rng(3700 + i)
    Q = rng.standard_normal((nq + 2, H * dk), dtype=np.float32)
    K, V = (torch.from_numpy(rng.standard_normal((nk + 1, n_kv * dk), dtype=np.float32)).bfloat16() for _ in range(2))
    Kw, Vw = K.float().numpy(), V.float().numpy()
    ref, e32 = np.full(Q.shape, np.nan), 0.0
    for b, (q, n) in enumerate(zip(seq_q, seq_kv)):
        lims = [n if pos is None else min(n, pos[b] + r + 1) for r in range(q)]
        rs, ks = slice(q0[b], q0[b] + q), slice(k0[b], k0[b] + n)
        ref[rs] = _attend(Q[rs], Kw[ks], Vw[ks], H, n_kv, lims, np.float64)
        if q:
            e32 = max(e32, float(np.abs(_attend(Q[rs], Kw[ks], Vw[ks], H, n_kv, lims, np.float32) - ref[rs]).max()))
    Q.setflags(write=False)
    return Q, K, V, pos, q0, k0, ref, e32


def _dev(a, device, odd=False):
    """a on the device: contiguous, or a view that starts one element past a 16-byte boundary with an odd row stride."""
    if not odd:
        return a.to(device)
    n, w = a.shape
    flat = torch.full((1 + n * (w + 1),), float("nan"), dtype=a.dtype, device=device)
    view = flat[1:].as_strided((n, w), (w + 1, 1))
    view.copy_(a)
    return view


def _run(call, device, Q, Kd, Vd, H, n_kv, seq_q, seq_kv, pos, q0, k0):
    """One call (the new one, or attention_varlen_tiled on widened K / V) into a NaN-filled O of Q's rows; as numpy"""
    O = torch.full(Q.shape, float("nan"), device=device)
    call(torch.tensor(Q, device=device), Kd, Vd, H, n_kv, seq_q, seq_kv, q_row0=q0, kv_row0=k0, q_pos0=pos, O=O)
    torch.cuda.synchronize()
    return O.cpu().numpy()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[str(c[:5]) for c in CASES])
def test_against_the_fp32_tiled_bits_and_float64(qg, device, i):
    H, n_kv, dk, seq_q, seq_kv, _, odd = CASES[i]
    Q, K, V, pos, q0, k0, ref, e32 = _case(i)
    got = _run(qg.attention_varlen_tiled_kv16, device, Q, _dev(K, device, odd), _dev(V, device, odd), H, n_kv, seq_q,
               seq_kv, pos, q0, k0)
    want = _run(qg.attention_varlen_tiled, device, Q, _dev(K.float(), device, odd), _dev(V.float(), device, odd), H, n_kv,
                seq_q, seq_kv, pos, q0, k0)
    assert_bits_equal(got, want, "attention_varlen_tiled on the widened K / V")  # (NaN where no row is written, in both)
    inside = ~np.isnan(ref)
    assert np.isnan(got[~inside]).all(), "rows of O outside the call's sequences were written"
    err = float(np.abs(got[inside] - ref[inside]).max())
    print(f"case {CASES[i][:5]}: e32 {e32:.3e}  bf16 tiled {err:.3e} ({err / e32:.2f} e32)")
    assert err <= FACTOR * e32


def test_poisoned_hidden_keys_do_not_reach_the_output(qg, device):
    """bf16 inf / NaN at keys >= each sequence's largest limit and in the rows >= seq_kv: the same bits, and finite."""
    H, n_kv, dk, seq_q, seq_kv, pos = 8, 2, 64, (70, 5, 33), (300, 140, 700), [100, 130, 500]
    q0, k0 = [0, 70, 75], [0, 320, 480]
    rng = np.random.default_rng(3710)
    Q = rng.standard_normal((108, H * dk), dtype=np.float32)
    K, V = (torch.from_numpy(rng.standard_normal((1200, n_kv * dk), dtype=np.float32)).bfloat16() for _ in range(2))
    clean = _run(qg.attention_varlen_tiled_kv16, device, Q, _dev(K, device), _dev(V, device, True), H, n_kv, seq_q, seq_kv,
                 pos, q0, k0)
    assert np.isfinite(clean).all()
    Kb, Vb = K.view(torch.int16), V.view(torch.int16)
    for b, n in enumerate(seq_kv):
        lo, hi = k0[b] + min(n, pos[b] + seq_q[b]), (k0 + [1200])[b + 1]  # from the largest limit to the next sequence
        Kb[lo:hi:2], Kb[lo + 1:hi:2], Vb[lo:hi:2], Vb[lo + 1:hi:2] = BF16_INF, BF16_NAN, BF16_NAN, BF16_INF
    dirty = _run(qg.attention_varlen_tiled_kv16, device, Q, _dev(K, device), _dev(V, device, True), H, n_kv, seq_q, seq_kv,
                 pos, q0, k0)
    assert_bits_equal(dirty, clean, "poisoned hidden keys")


def test_a_sequence_alone_equals_its_rows_in_a_batch_of_64(qg, device):
    H, n_kv, dk = 4, 2, 64
    seq_q = tuple(1 + (7 * b) % 70 for b in range(64))
    seq_kv = tuple(q + (37 * b) % 600 for b, q in enumerate(seq_q))
    pos, q0, k0, nq, nk = _layout(seq_q, seq_kv, "tail", None)
    rng = np.random.default_rng(3711)
    Q = rng.standard_normal((nq, H * dk), dtype=np.float32)
    Kd, Vd = (torch.from_numpy(rng.standard_normal((nk, n_kv * dk), dtype=np.float32)).bfloat16().to(device)
              for _ in range(2))
    batch = _run(qg.attention_varlen_tiled_kv16, device, Q, Kd, Vd, H, n_kv, seq_q, seq_kv, pos, q0, k0)
    for b in (0, 17, 63):
        rs = slice(q0[b], q0[b] + seq_q[b])
        one = _run(qg.attention_varlen_tiled_kv16, device, Q, Kd, Vd, H, n_kv, [seq_q[b]], [seq_kv[b]], [pos[b]], [q0[b]],
                   [k0[b]])
        assert_bits_equal(one[rs], batch[rs], f"sequence {b} alone")


def test_cache_round_trip_through_kv_append_bf16(qg, device):
    """kv_append_bf16 fills [slabs, rows, width] caches in shuffled slots; the new call reads them through kv_row0 = slot
    x rows as a 512-key prefix plus a 70-row chunk, and equals attention_varlen_tiled on the caches' .float()."""
    H, n_kv, dk, slots, rows, prefix, chunk = 8, 2, 128, [2, 0, 3], 600, 512, 70
    n, width = prefix + chunk, n_kv * dk
    rng = np.random.default_rng(3712)
    Q = rng.standard_normal((3 * chunk, H * dk), dtype=np.float32)
    Kn, Vn = (torch.from_numpy(rng.standard_normal((3 * n, width), dtype=np.float32)).to(device) for _ in range(2))
    Kc, Vc = (torch.zeros((4, rows, width), dtype=torch.bfloat16, device=device) for _ in range(2))
    qg.kv_append_bf16(Kn, Vn, Kc, Vc, [0, 0, 0], kv_slot=slots, rows_per_seq=n)
    args = (H, n_kv, (chunk,) * 3, (n,) * 3, [prefix] * 3, [0, chunk, 2 * chunk], [s * rows for s in slots])
    got = _run(qg.attention_varlen_tiled_kv16, device, Q, Kc.view(-1, width), Vc.view(-1, width), *args)
    want = _run(qg.attention_varlen_tiled, device, Q, Kc.float().view(-1, width), Vc.float().view(-1, width), *args)
    assert np.isfinite(got).all()
    assert_bits_equal(got, want, "attention_varlen_tiled on the widened caches")


def test_fp32_k_is_refused_and_a_captured_graph_replays_the_eager_bits(qg, device):
    H, n_kv, dk, seq_q, seq_kv = 6, 2, 128, (70, 3, 129), (700, 129, 4100)
    rng = np.random.default_rng(3713)
    Q = torch.from_numpy(rng.standard_normal((sum(seq_q), H * dk), dtype=np.float32)).to(device)
    Kd, Vd = (torch.from_numpy(rng.standard_normal((sum(seq_kv), n_kv * dk), dtype=np.float32)).bfloat16().to(device)
              for _ in range(2))
    with pytest.raises(AssertionError, match="bfloat16"):
        qg.attention_varlen_tiled_kv16(Q, Kd.float(), Vd, H, n_kv, seq_q, seq_kv)
    out = torch.empty_like(Q)

    def call():
        qg.attention_varlen_tiled_kv16(Q, Kd, Vd, H, n_kv, seq_q, seq_kv, q_pos0=[n - q for q, n in zip(seq_q, seq_kv)],
                                       O=out)

    call()
    torch.cuda.synchronize()
    eager = out.cpu().numpy()
    assert np.isfinite(eager).all()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
    for i in range(3):
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), eager, f"graph replay {i}")
