"""Tiled online-softmax prefill attention on the GPU (qgemm_attention_varlen_tiled).  Its contract is its
own, so the reference is float64 numpy softmax attention on the same fp32 inputs (K / V head h // G for query head h, keys
>= lim dropped) and the yardstick e32 is computed here, on the CPU: e32 = max |the same formula in numpy fp32 - the
float64 reference|.  The kernel must stay within 8 e32 (its own summation order and a 1-ulp exp); one dropped or doubled
key moves a row by about |v| / n.  Where every sequence has <= 4096 keys attention_varlen_gqa of the same build goes
through the same assertion.  Figures of one run: DESIGN.md s35."""
import functools

import numpy as np
import pytest
import torch

from util import assert_bits_equal

pytestmark = pytest.mark.gpu
FACTOR = 8

# (heads, KV heads, d_k, seq_q, seq_kv, q_pos0: None / "zero" / "tail" (seq_kv - seq_q) / values, odd K / V views,
#  (q_row0, kv_row0) or None: packed)
CASES = [
    (6, 2, 20, (1, 17, 65), (1, 63, 129), None, True, None),           # G 3, d_k % 4 != 0, a one-key sequence
    (14, 2, 64, (33, 130, 15), (33, 130, 15), "zero", False, None),    # G 7, square causal
    (8, 8, 96, (64, 65, 3), (513, 600, 4097), "tail", False, None),    # G 1, tail chunks of a long cache
    (32, 2, 128, (70, 1, 16), (8200, 5000, 1025), (3000, 4999, 0), False, None),  # G 16, wide, mid-cache
    (4, 1, 128, (130, 0, 2), (257, 40, 64), "zero", False, None),      # an empty sequence inside the table
    (2, 1, 64, (3,), (131072,), "tail", False, None),                  # the key cap
    (8, 2, 64, (200, 40), (200, 4097), None, False, ((5, 210), (4100, 2))),  # rows between and around the sequences
]


def _attend(Q, K, V, H, n_kv, lims, dt):
    """Softmax attention in dtype dt: row r of Q over keys 0 .. lims[r] - 1, query head h on K / V head h // G."""
    dk, G = Q.shape[1] // H, H // n_kv
    scale = dt(np.float32(1.0 / np.sqrt(np.float64(dk))))
    Q, K, V = Q.astype(dt), K[:max(lims, default=0)].astype(dt), V[:max(lims, default=0)].astype(dt)
    out = np.empty(Q.shape, dtype=dt)
    for h in range(H):
        qc, kc = slice(h * dk, (h + 1) * dk), slice(h // G * dk, (h // G + 1) * dk)
        S = (Q[:, qc] @ K[:, kc].T) * scale
        for r, lim in enumerate(lims):
            p = np.exp(S[r, :lim] - S[r, :lim].max())
            out[r, qc] = (p @ V[:lim, kc]) / p.sum()
    return out


def _layout(seq_q, seq_kv, mask, rows0):
    pos = {None: None, "zero": [0] * len(seq_q), "tail": [n - q for q, n in zip(seq_q, seq_kv)]}.get(mask, mask)
    q0, k0 = rows0 or (np.cumsum((0,) + seq_q[:-1]).tolist(), np.cumsum((0,) + seq_kv[:-1]).tolist())
    return pos, list(q0), list(k0), max(a + n for a, n in zip(q0, seq_q)), max(a + n for a, n in zip(k0, seq_kv))


@functools.lru_cache(maxsize=None)
def _case(i):
    """The inputs of case i (N(0, 1), fixed seed), its float64 reference and e32 -- computed once, never changed."""
    H, n_kv, dk, seq_q, seq_kv, mask, _, rows0 = CASES[i]
    pos, q0, k0, nq, nk = _layout(seq_q, seq_kv, mask, rows0)
    rng = np.random.default_rng(3500 + i)
    Q = rng.standard_normal((nq + 2, H * dk), dtype=np.float32)
    K, V = (rng.standard_normal((nk + 1, n_kv * dk), dtype=np.float32) for _ in range(2))
    ref, e32 = np.full(Q.shape, np.nan), 0.0
    for b, (q, n) in enumerate(zip(seq_q, seq_kv)):
        lims = [n if pos is None else min(n, pos[b] + r + 1) for r in range(q)]
        rs, ks = slice(q0[b], q0[b] + q), slice(k0[b], k0[b] + n)
        ref[rs] = _attend(Q[rs], K[ks], V[ks], H, n_kv, lims, np.float64)
        if q:
            e32 = max(e32, float(np.abs(_attend(Q[rs], K[ks], V[ks], H, n_kv, lims, np.float32) - ref[rs]).max()))
    for a in (Q, K, V, ref):
        a.setflags(write=False)
    return Q, K, V, pos, q0, k0, ref, e32


def _dev(a, device, odd=False):
    """a on the device: contiguous, or a view that starts one element past a 16-byte boundary with an odd row stride."""
    if not odd:
        return torch.tensor(a, device=device)
    n, w = a.shape
    flat = torch.full((1 + n * (w + 1),), float("nan"), device=device)
    view = flat[1:].as_strided((n, w), (w + 1, 1))
    view.copy_(torch.tensor(a))
    return view


def _tiled(qg, device, Q, Kd, Vd, H, n_kv, seq_q, seq_kv, pos, q0, k0):
    """One call into a NaN-filled O of Q's rows; as numpy"""
    O = torch.full(Q.shape, float("nan"), device=device)
    qg.attention_varlen_tiled(torch.tensor(Q, device=device), Kd, Vd, H, n_kv, seq_q, seq_kv, q_row0=q0, kv_row0=k0,
                              q_pos0=pos, O=O)
    torch.cuda.synchronize()
    return O.cpu().numpy()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[str(c[:5]) for c in CASES])
def test_tiled_against_float64(qg, device, i):
    H, n_kv, dk, seq_q, seq_kv, _, odd, _ = CASES[i]
    Q, K, V, pos, q0, k0, ref, e32 = _case(i)
    Kd, Vd = _dev(K, device, odd), _dev(V, device, odd)
    got = _tiled(qg, device, Q, Kd, Vd, H, n_kv, seq_q, seq_kv, pos, q0, k0)
    inside = ~np.isnan(ref)
    assert np.isnan(got[~inside]).all(), "rows of O outside the call's sequences were written"
    err = float(np.abs(got[inside] - ref[inside]).max())
    print(f"case {CASES[i][:5]}: e32 {e32:.3e}  tiled {err:.3e} ({err / e32:.2f} e32)")
    assert err <= FACTOR * e32
    if max(seq_kv) <= 4096:  # the margin itself: the existing paths of the same build through the same assertion
        old = qg.attention_varlen_gqa(torch.tensor(Q, device=device), Kd, Vd, H, n_kv, seq_q, seq_kv, q_row0=q0,
                                      kv_row0=k0, q_pos0=pos).cpu().numpy()
        err_old = float(np.abs(old[inside] - ref[inside]).max())
        print(f"    attention_varlen_gqa {err_old:.3e} ({err_old / e32:.2f} e32)")
        assert err_old <= FACTOR * e32, "the margin is wrong, not the kernel"
    if max(seq_kv) == 131072:  # one key past the cap is refused
        with pytest.raises(qg.QGemmError):
            qg.attention_varlen_tiled(torch.tensor(Q, device=device), Kd, Vd, H, n_kv, seq_q, (131073,), q_pos0=pos)


def test_poisoned_hidden_keys_do_not_reach_the_output(qg, device):
    """inf and NaN in K and V at keys >= each sequence's largest limit and in the slab rows >= seq_kv: the same bits."""
    H, n_kv, dk, seq_q, seq_kv, pos = 8, 2, 64, (70, 5, 33), (300, 140, 700), [100, 130, 500]
    q0, k0 = [0, 70, 75], [0, 320, 480]
    rng = np.random.default_rng(3510)
    Q = rng.standard_normal((108, H * dk), dtype=np.float32)
    K, V = (rng.standard_normal((1200, n_kv * dk), dtype=np.float32) for _ in range(2))
    clean = _tiled(qg, device, Q, _dev(K, device), _dev(V, device, True), H, n_kv, seq_q, seq_kv, pos, q0, k0)
    assert np.isfinite(clean).all()
    for b, n in enumerate(seq_kv):
        lo, hi = k0[b] + min(n, pos[b] + seq_q[b]), (k0 + [1200])[b + 1]  # from the largest limit to the next sequence
        K[lo:hi:2], K[lo + 1:hi:2], V[lo:hi:2], V[lo + 1:hi:2] = np.inf, np.nan, np.nan, -np.inf
    dirty = _tiled(qg, device, Q, _dev(K, device), _dev(V, device, True), H, n_kv, seq_q, seq_kv, pos, q0, k0)
    assert_bits_equal(dirty, clean, "poisoned hidden keys")


@pytest.mark.parametrize("which", ["one of three", "one of 64"])
def test_a_sequence_alone_equals_its_rows_in_the_batch(qg, device, which):
    if which == "one of three":  # sequence 1 of the 8 / 8 x 96 case
        H, n_kv, dk, seq_q, seq_kv, _, _, _ = CASES[2]
        Q, K, V, pos, q0, k0, _, _ = _case(2)
        alone = [1]
    else:  # 64 sequences of their own lengths, each the tail of its cache
        H, n_kv, dk = 4, 2, 64
        seq_q = tuple(1 + (7 * b) % 70 for b in range(64))
        seq_kv = tuple(q + (37 * b) % 600 for b, q in enumerate(seq_q))
        pos, q0, k0, nq, nk = _layout(seq_q, seq_kv, "tail", None)
        rng = np.random.default_rng(3511)
        Q = rng.standard_normal((nq, H * dk), dtype=np.float32)
        K, V = (rng.standard_normal((nk, n_kv * dk), dtype=np.float32) for _ in range(2))
        alone = [0, 17, 63]
    Kd, Vd = _dev(K, device), _dev(V, device)
    batch = _tiled(qg, device, Q, Kd, Vd, H, n_kv, seq_q, seq_kv, pos, q0, k0)
    for b in alone:
        rs = slice(q0[b], q0[b] + seq_q[b])
        one = _tiled(qg, device, Q, Kd, Vd, H, n_kv, [seq_q[b]], [seq_kv[b]], [pos[b]], [q0[b]], [k0[b]])
        assert_bits_equal(one[rs], batch[rs], f"sequence {b} alone")


def test_graph_capture_and_replay(qg, device):
    """The call allocates nothing, copies nothing and does not synchronize: captured once, every replay gives the eager
    call's bits."""
    H, n_kv, dk, seq_q, seq_kv = 6, 2, 128, (70, 3, 129), (700, 129, 4100)
    rng = np.random.default_rng(3512)
    Q = torch.from_numpy(rng.standard_normal((sum(seq_q), H * dk), dtype=np.float32)).to(device)
    Kd, Vd = (torch.from_numpy(rng.standard_normal((sum(seq_kv), n_kv * dk), dtype=np.float32)).to(device)
              for _ in range(2))
    out = torch.empty_like(Q)

    def call():
        qg.attention_varlen_tiled(Q, Kd, Vd, H, n_kv, seq_q, seq_kv, q_pos0=[n - q for q, n in zip(seq_q, seq_kv)], O=out)

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
