"""Split-key decode attention over a bf16 cache on the GPU (qgemm_attention_decode_split_kv16).  Inputs
are N(0, 1) from a fixed seed, rounded to bf16 once on the host: the bf16 tensors go to the new call, their .float() to
the references.  Two references: float64 numpy softmax attention (K / V head h // G, keys >= lim dropped) with the
yardstick e32 = max |the same formula in numpy fp32 - float64| and the project's bound 8 e32; and, the sharp half,
attention_decode_split of the same build on the widened slabs at the same L, bit for bit.
Figures of one run (e32, error per case): DESIGN.md s36."""
import functools

import numpy as np
import pytest
import torch

from util import assert_bits_equal

pytestmark = pytest.mark.gpu
FACTOR = 8
BF16_INF, BF16_NAN = 0x7F80, 0x7FC0

# (heads, KV heads, d_k, split_keys, keys per sequence, rows, mask, K / V one element past 16 bytes with an odd stride)
# mask: None; "tail": q_pos0 = seq_kv - rows (the rows are the sequence's last positions); "zero": q_pos0 = 0
CASES = [
    (6, 2, 20, 128, (1, 128, 129), 3, "tail", True),           # element-wise reads, a one-key split, the boundary +- 1
    (14, 2, 64, 256, (255, 257, 600), 1, None, True),          # a partial last head block; the kW 64 chunk tail
    (8, 8, 96, 512, (513, 4096, 4097), 3, "tail", False),      # G 1; the first key past the sequential envelope
    (32, 2, 128, 1024, (1025, 5000, 8200), 8, "tail", False),  # G 16; several chunks per split at the longest L
    (4, 1, 128, 128, (16384, 300, 2), 8, "zero", False),       # rows see 1 .. 8 keys: every split but the first returns
    (8, 2, 64, 0, (9000, 40, 4097), 1, "tail", False),         # the default split_keys
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


def _inputs(seed, n_rows, H, n_kv, dk, slabs, n):
    """Q fp32, K / V as bf16 torch tensors (rounded once, here)."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n_rows, H * dk), dtype=np.float32)
    K, V = (torch.from_numpy(rng.standard_normal((slabs, n, n_kv * dk), dtype=np.float32)).bfloat16() for _ in range(2))
    return Q, K, V


@functools.lru_cache(maxsize=None)
def _case(i):
    """The inputs of case i, its float64 reference on the widened inputs and e32 -- computed once, never changed."""
    H, n_kv, dk, _, keys, rows, mask, _ = CASES[i]
    Q, K, V = _inputs(3600 + i, len(keys) * rows, H, n_kv, dk, len(keys), max(keys))
    Kw, Vw = K.float().numpy(), V.float().numpy()
    pos = None if mask is None else [max(0, n - rows) if mask == "tail" else 0 for n in keys]
    ref, e32 = np.empty(Q.shape, dtype=np.float64), 0.0
    for b, n in enumerate(keys):
        lims = [n if pos is None else min(n, pos[b] + r + 1) for r in range(rows)]
        rs = slice(b * rows, (b + 1) * rows)
        ref[rs] = _attend(Q[rs], Kw[b], Vw[b], H, n_kv, lims, np.float64)
        e32 = max(e32, float(np.abs(_attend(Q[rs], Kw[b], Vw[b], H, n_kv, lims, np.float32) - ref[rs]).max()))
    Q.setflags(write=False)
    return Q, K, V, pos, ref, e32


def _slabs(a, device, odd=False):
    """a on the device: contiguous, or a view that starts one element past a 16-byte boundary with an odd row stride."""
    if not odd:
        return a.to(device)
    slabs, n, w = a.shape
    flat = torch.full((1 + slabs * n * (w + 1),), float("nan"), dtype=a.dtype, device=device)
    view = flat[1:].as_strided((slabs, n, w), (n * (w + 1), w + 1, 1))
    view.copy_(a)
    return view


def _run(call, device, Q, Kd, Vd, H, n_kv, keys, pos, rows, L, slots=None):
    """One split-key call (the new one, or attention_decode_split on widened slabs) into a NaN-filled workspace."""
    O = call(torch.tensor(Q, device=device), Kd, Vd, H, n_kv, slots, list(keys), q_pos0=pos, rows_per_seq=rows,
             split_keys=L, workspace=torch.full((1 << 22,), float("nan"), device=device))
    torch.cuda.synchronize()
    return O.cpu().numpy()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[str(c[:5]) for c in CASES])
def test_against_float64_and_the_fp32_split_bits(qg, device, i):
    H, n_kv, dk, split, keys, rows, _, odd = CASES[i]
    Q, K, V, pos, ref, e32 = _case(i)
    Kd, Vd = _slabs(K, device, odd), _slabs(V, device, odd)
    got = _run(qg.attention_decode_split_kv16, device, Q, Kd, Vd, H, n_kv, keys, pos, rows, split or None)
    err = float(np.abs(got - ref).max())
    print(f"case {CASES[i][:5]}: e32 {e32:.3e}  bf16 split path {err:.3e} ({err / e32:.2f} e32)")
    assert err <= FACTOR * e32
    L = split or qg.attention_decode_split_kv16_plan(len(keys), rows, max(keys), H, n_kv, dk)[0]
    assert L == qg.attention_decode_split_plan(len(keys), rows, max(keys), H, n_kv, dk, split or None)[0]
    want = _run(qg.attention_decode_split, device, Q, _slabs(K.float(), device, odd), _slabs(V.float(), device, odd),
                H, n_kv, keys, pos, rows, L)
    assert_bits_equal(got, want, f"attention_decode_split on the widened cache, L = {L}")
    if split == 0:  # ... and the default resolved as the plan says
        assert_bits_equal(got, _run(qg.attention_decode_split_kv16, device, Q, Kd, Vd, H, n_kv, keys, pos, rows, L),
                          f"default L = {L} given explicitly")


def test_poisoned_hidden_keys_do_not_reach_the_output(qg, device):
    """bf16 inf / NaN at keys >= every row's lim and in the slab rows >= seq_kv: the same bits as without them."""
    H, n_kv, dk, rows, keys, pos = 8, 2, 64, 3, (300, 140, 700), [100, 130, 500]
    Q, K, V = _inputs(3610, 3 * rows, H, n_kv, dk, 3, 704)
    clean = _run(qg.attention_decode_split_kv16, device, Q, _slabs(K, device), _slabs(V, device, True), H, n_kv, keys,
                 pos, rows, 128)
    assert np.isfinite(clean).all()
    Kb, Vb = K.view(torch.int16), V.view(torch.int16)
    for b in range(3):
        hidden = pos[b] + rows  # the last row's lim
        Kb[b, hidden::2], Kb[b, hidden + 1::2], Vb[b, hidden::2], Vb[b, hidden + 1::2] = BF16_INF, BF16_NAN, BF16_NAN, BF16_INF
    dirty = _run(qg.attention_decode_split_kv16, device, Q, _slabs(K, device), _slabs(V, device, True), H, n_kv, keys,
                 pos, rows, 128)
    assert_bits_equal(dirty, clean, "poisoned hidden keys")


def test_a_sequence_alone_equals_its_rows_in_a_batch_of_64(qg, device):
    H, n_kv, dk = 4, 2, 64
    keys, slots = tuple(1 + (37 * b) % 600 for b in range(64)), [b % 3 for b in range(64)]
    Q, K, V = _inputs(3611, 64, H, n_kv, dk, 3, 600)
    Kd, Vd = _slabs(K, device), _slabs(V, device)
    batch = _run(qg.attention_decode_split_kv16, device, Q, Kd, Vd, H, n_kv, keys, None, 1, 128, slots)
    for b in (0, 17, 63):
        one = _run(qg.attention_decode_split_kv16, device, Q[b:b + 1], Kd, Vd, H, n_kv, (keys[b],), None, 1, 128,
                   [slots[b]])
        assert_bits_equal(one, batch[b:b + 1], f"sequence {b} alone")


def test_fp32_slabs_are_refused(qg, device):
    """(Here, not with the host tests: the check needs device tensors to get as far as the dtype.)"""
    Q, K, V = _inputs(3613, 1, 4, 2, 64, 1, 8)
    with pytest.raises(AssertionError, match="bfloat16"):
        qg.attention_decode_split_kv16(torch.tensor(Q, device=device), K.float().to(device), V.to(device), 4, 2, None, [8])


def test_graph_capture_and_replay(qg, device):
    """The call allocates nothing, copies nothing and does not synchronize: captured once, every replay gives the eager
    call's bits."""
    H, n_kv, dk, rows, keys, split = 6, 2, 128, 2, (700, 129, 4100), 256
    Q, K, V = _inputs(3612, 3 * rows, H, n_kv, dk, 3, 4100)
    Q, Kd, Vd = torch.tensor(Q, device=device), K.to(device), V.to(device)
    ws = torch.empty(qg.attention_decode_split_workspace_size(3, rows, 4100, H, dk, split), dtype=torch.uint8,
                     device=device)
    out = torch.empty_like(Q)

    def call():
        qg.attention_decode_split_kv16(Q, Kd, Vd, H, n_kv, [2, 0, 1], list(keys), q_pos0=[n - rows for n in keys],
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
