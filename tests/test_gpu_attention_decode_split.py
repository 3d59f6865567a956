"""Split-key decode attention on the GPU (qgemm_attention_decode_split).  Its contract is its own, not
the sequential kernels' bits, so the reference is float64 numpy softmax attention on the same fp32 inputs (K / V head
h // G for query head h, keys >= lim dropped) and the yardstick e32 is computed here, on the CPU, from neither kernel:
e32 = max |the same formula in numpy fp32, unsplit - the float64 reference|.  The new path must stay within 8 e32 (a
different summation order and a 1-ulp exp); one dropped or doubled key moves a row by about |v| / n >= 6e-5.
Figures of one run (e32, error of the split path, error of the sequential launch where it applies): DESIGN.md s34."""
import functools

import numpy as np
import pytest
import torch

from util import assert_bits_equal

pytestmark = pytest.mark.gpu
FACTOR = 8

# (heads, KV heads, d_k, split_keys, keys per sequence, rows, mask, K / V one element past 16 bytes with an odd stride)
# mask: None; "tail": q_pos0 = seq_kv - rows (the rows are the sequence's last positions); "zero": q_pos0 = 0
CASES = [
    (6, 2, 20, 128, (1, 128, 129), 3, "tail", True),          # G 3; a one-key split; the boundary +- 1
    (14, 2, 64, 256, (255, 257, 600), 1, None, True),         # G 7: a partial last block of heads
    (8, 8, 96, 512, (513, 4096, 4097), 3, "tail", False),     # G 1
    (32, 2, 128, 1024, (1025, 5000, 8200), 8, "tail", False),  # G 16
    (4, 1, 128, 128, (16384, 300, 2), 8, "zero", True),       # rows see 1 .. 8 keys: every split but the first returns
    (8, 2, 64, 0, (9000, 40, 4097), 1, "tail", False),        # the default split_keys
]


def _attend(Q, K, V, H, n_kv, lims, dt):
    """Softmax attention in dtype dt: row r of Q over keys 0 .. lims[r] - 1, query head h on K / V head h // G."""
    dk, G = Q.shape[1] // H, H // n_kv
    scale = dt(np.float32(1.0 / np.sqrt(np.float64(dk))))
    Q, K, V = Q.astype(dt), K[:max(lims)].astype(dt), V[:max(lims)].astype(dt)
    out = np.empty(Q.shape, dtype=dt)
    for h in range(H):
        qc, kc = slice(h * dk, (h + 1) * dk), slice(h // G * dk, (h // G + 1) * dk)
        S = (Q[:, qc] @ K[:, kc].T) * scale
        for r, lim in enumerate(lims):
            p = np.exp(S[r, :lim] - S[r, :lim].max())
            out[r, qc] = (p @ V[:lim, kc]) / p.sum()
    return out


def _limits(n, rows, q_pos0):
    return [n if q_pos0 is None else min(n, q_pos0 + r + 1) for r in range(rows)]


@functools.lru_cache(maxsize=None)
def _case(i):
    """The inputs of case i (N(0, 1), fixed seed), its float64 reference and e32 -- computed once, never changed."""
    H, n_kv, dk, _, keys, rows, mask, _ = CASES[i]
    rng = np.random.default_rng(3400 + i)
    Q = rng.standard_normal((len(keys) * rows, H * dk), dtype=np.float32)
    K = rng.standard_normal((len(keys), max(keys), n_kv * dk), dtype=np.float32)
    V = rng.standard_normal((len(keys), max(keys), n_kv * dk), dtype=np.float32)
    pos = None if mask is None else [max(0, n - rows) if mask == "tail" else 0 for n in keys]
    ref, e32 = np.empty(Q.shape, dtype=np.float64), 0.0
    for b, n in enumerate(keys):
        lims, rs = _limits(n, rows, None if pos is None else pos[b]), slice(b * rows, (b + 1) * rows)
        ref[rs] = _attend(Q[rs], K[b], V[b], H, n_kv, lims, np.float64)
        e32 = max(e32, float(np.abs(_attend(Q[rs], K[b], V[b], H, n_kv, lims, np.float32) - ref[rs]).max()))
    for a in (Q, K, V, ref):
        a.setflags(write=False)
    return Q, K, V, pos, ref, e32


def _slabs(a, device, odd):
    """a on the device: contiguous, or a view that starts one element past a 16-byte boundary with an odd row stride."""
    if not odd:
        return torch.tensor(a, device=device)
    slabs, n, w = a.shape
    flat = torch.full((1 + slabs * n * (w + 1),), float("nan"), device=device)
    view = flat[1:].as_strided((slabs, n, w), (n * (w + 1), w + 1, 1))
    view.copy_(torch.tensor(a))
    return view


def _split(qg, device, Q, Kd, Vd, H, n_kv, keys, pos, rows, split, slots=None):
    """One call into a NaN-filled workspace and a NaN-filled parent of O; the parent's other rows must stay NaN."""
    dk = Q.shape[1] // H
    L = split or qg.attention_decode_split_plan(len(keys), rows, max(keys), H, n_kv, dk)[0]
    need = qg.attention_decode_split_workspace_size(len(keys), rows, max(keys), H, dk, L)
    ws = torch.full((need // 4,), float("nan"), device=device)
    parent = torch.full((len(Q) + 2, Q.shape[1]), float("nan"), device=device)
    qg.attention_decode_split(torch.tensor(Q, device=device), Kd, Vd, H, n_kv, slots, list(keys),
                              q_pos0=pos, rows_per_seq=rows, split_keys=split or None, workspace=ws, out=parent[1:-1])
    torch.cuda.synchronize()
    got = parent.cpu().numpy()
    assert np.isnan(got[0]).all() and np.isnan(got[-1]).all(), "rows of O's parent outside the call were written"
    return got[1:-1]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[str(c[:5]) for c in CASES])
def test_split_against_float64(qg, device, i):
    H, n_kv, dk, split, keys, rows, _, odd = CASES[i]
    Q, K, V, pos, ref, e32 = _case(i)
    Kd, Vd = _slabs(K, device, odd), _slabs(V, device, odd)
    got = _split(qg, device, Q, Kd, Vd, H, n_kv, keys, pos, rows, split)
    err = float(np.abs(got - ref).max())
    print(f"case {CASES[i][:5]}: e32 {e32:.3e}  split path {err:.3e} ({err / e32:.2f} e32)")
    assert err <= FACTOR * e32
    if split == 0:  # the call resolved split_keys as the plan does: the result is a function of the arguments and L
        L = qg.attention_decode_split_plan(len(keys), rows, max(keys), H, n_kv, dk)[0]
        assert_bits_equal(got, _split(qg, device, Q, Kd, Vd, H, n_kv, keys, pos, rows, L), f"default L = {L}")
    if max(keys) <= 4096:  # the margin itself: the sequential launch of the same build through the same assertion
        old = qg.attention_decode_batched_gqa(torch.tensor(Q, device=device), Kd, Vd, H, n_kv, list(keys), q_pos0=pos,
                                              rows_per_seq=rows).cpu().numpy()
        err_old = float(np.abs(old - ref).max())
        print(f"    sequential launch {err_old:.3e} ({err_old / e32:.2f} e32)")
        assert err_old <= FACTOR * e32, "the margin is wrong, not the kernel"


def test_masked_and_unused_values_do_not_reach_the_output(qg, device):
    """inf and NaN in K and V at keys >= every row's lim, NaN in the slab rows >= seq_kv: the same bits as without."""
    H, n_kv, dk, rows, keys, pos = 8, 2, 64, 3, (300, 140, 700), [100, 130, 500]
    rng = np.random.default_rng(3410)
    Q = rng.standard_normal((3 * rows, H * dk), dtype=np.float32)
    K, V = (rng.standard_normal((3, 704, n_kv * dk), dtype=np.float32) for _ in range(2))
    clean = _split(qg, device, Q, _slabs(K, device, False), _slabs(V, device, True), H, n_kv, keys, pos, rows, 128)
    assert np.isfinite(clean).all()
    for b, n in enumerate(keys):
        hidden = pos[b] + rows  # the last row's lim
        K[b, hidden:n:2], K[b, hidden + 1:n:2], V[b, hidden:n:2], V[b, hidden + 1:n:2] = np.inf, np.nan, np.nan, -np.inf
        K[b, n:], V[b, n:] = np.nan, np.nan
    dirty = _split(qg, device, Q, _slabs(K, device, False), _slabs(V, device, True), H, n_kv, keys, pos, rows, 128)
    assert_bits_equal(dirty, clean, "poisoned masked keys")


@pytest.mark.parametrize("which", ["one of three", "one of 64"])
def test_a_sequence_alone_equals_its_rows_in_the_batch(qg, device, which):
    if which == "one of three":  # sequence 1 of the 8 / 8 x 96 case
        H, n_kv, dk, split, keys, rows, _, _ = CASES[2]
        Q, K, V, pos, _, _ = _case(2)
        slots, alone = [0, 1, 2], [1]
    else:  # 64 sequences of their own lengths over three slabs
        H, n_kv, dk, split, rows = 4, 2, 64, 128, 1
        rng = np.random.default_rng(3411)
        keys, slots = tuple(1 + (37 * b) % 600 for b in range(64)), [b % 3 for b in range(64)]
        Q = rng.standard_normal((64, H * dk), dtype=np.float32)
        K, V = (rng.standard_normal((3, 600, n_kv * dk), dtype=np.float32) for _ in range(2))
        pos, alone = None, [0, 17, 63]
    Kd, Vd = _slabs(K, device, False), _slabs(V, device, False)
    batch = _split(qg, device, Q, Kd, Vd, H, n_kv, keys, pos, rows, split, slots)
    for b in alone:
        rs = slice(b * rows, (b + 1) * rows)
        one = _split(qg, device, Q[rs], Kd, Vd, H, n_kv, (keys[b],), None if pos is None else [pos[b]], rows, split,
                     [slots[b]])
        assert_bits_equal(one, batch[rs], f"sequence {b} alone")


def test_graph_capture_and_replay(qg, device):
    """The call allocates nothing, copies nothing and does not synchronize: captured once, every replay gives the eager
    call's bits."""
    H, n_kv, dk, rows, keys, split = 6, 2, 128, 2, (700, 129, 4100), 256
    rng = np.random.default_rng(3412)
    Q = torch.from_numpy(rng.standard_normal((3 * rows, H * dk), dtype=np.float32)).to(device)
    Kd, Vd = (torch.from_numpy(rng.standard_normal((3, 4100, n_kv * dk), dtype=np.float32)).to(device) for _ in range(2))
    ws = torch.empty(qg.attention_decode_split_workspace_size(3, rows, 4100, H, dk, split), dtype=torch.uint8,
                     device=device)
    out = torch.empty_like(Q)

    def call():
        qg.attention_decode_split(Q, Kd, Vd, H, n_kv, [2, 0, 1], list(keys), q_pos0=[n - rows for n in keys],
                                  rows_per_seq=rows, split_keys=split, workspace=ws, out=out)

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
        ws.fill_(255)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), eager, f"graph replay {i}")
