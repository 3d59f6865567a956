"""The unmasked (q_pos0 left out) table launches of decode attention, one check for the multi-head, grouped-query and
bf16-cache test files: the non-causal DecodeMany and DecodeIndirect instantiations of the three decode kernels, which
the masked cases of those files do not reach (DESIGN.md s33 has the list).

Two or more sequences read prefixes of ONE K / V history (beam search's situation): the batched launch with every
sequence on the same slab, the indirect launch with key j in slab j & 1 through one table row per sequence, and the
entry 2 of 2 slabs at the last visible key of the last sequence, whose rows must then be NaN while the others stay
finite.  Outputs are pre-filled with NaN; every row is compared bit for bit."""
import numpy as np
import torch

from oracle import oracle as O
from util import assert_bits_equal


def check_unmasked_tables(device, rows, seq_kv, H, n_kv, dk, sliced, dtype, batched, indirect, want, seed):
    """batched(Q, K, V, seq_kv, kv_slot, out) / indirect(Q, K, V, table, seq_kv, out): the calls under test, without a
    mask; want(Q, K, V): the unmasked oracle on one sequence's views.  sliced: K and V start one element past a 16-byte
    boundary and have an odd row stride (the element loads)."""
    n, w, B = max(seq_kv), n_kv * dk, len(seq_kv)
    K, V = O.uniform((n, w), seed + 1), O.uniform((n, w), seed + 2)
    Qs = [O.uniform((rows, H * dk), seed + 10 * (b + 1)) for b in range(B)]
    Qd = torch.from_numpy(np.concatenate(Qs)).to(device)

    def cache(a):
        t = torch.from_numpy(a).to(dtype).to(device)
        if not sliced:
            return t
        wide = torch.zeros(a.shape[:2] + (w + 7,), dtype=dtype, device=device)
        wide[:, :, 1:1 + w] = t
        return wide[:, :, 1:1 + w]

    def run(call, what, Kb, Vb):
        out = torch.full((B * rows, H * dk), float("nan"), device=device)
        call(out)
        got = out.cpu().numpy()
        for b in range(B):
            assert_bits_equal(got[b * rows:(b + 1) * rows], want(Qs[b], Kb(b), Vb(b)), f"{what}: sequence {b}")
        return got

    slabs = [np.full((2, n + 3, w), np.nan, np.float32) for _ in range(2)]
    slabs[0][1, :n], slabs[1][1, :n] = K, V
    Kd, Vd = cache(slabs[0]), cache(slabs[1])
    got = run(lambda out: batched(Qd, Kd, Vd, list(seq_kv), [1] * B, out), "batched, unmasked",
              lambda b: K[:seq_kv[b]], lambda b: V[:seq_kv[b]])
    assert np.isfinite(got).all()

    j = np.arange(n)
    slabs = [np.full((2, n + 3, w), np.nan, np.float32) for _ in range(2)]
    slabs[0][j & 1, j], slabs[1][j & 1, j] = K, V
    own = np.full((B, n + 3), 255, np.uint8)
    own[:, :n] = j & 1
    bad = seq_kv[-1] - 1
    own[B - 1, bad] = 2   # names no slab: a row of NaNs, visible to every row of the last sequence
    Kn, Vn = K.copy(), V.copy()
    Kn[bad], Vn[bad] = np.nan, np.nan
    Kd, Vd, table = cache(slabs[0]), cache(slabs[1]), torch.from_numpy(own).to(device)
    got = run(lambda out: indirect(Qd, Kd, Vd, table, list(seq_kv), out), "indirect, unmasked",
              lambda b: (Kn if b == B - 1 else K)[:seq_kv[b]], lambda b: (Vn if b == B - 1 else V)[:seq_kv[b]])
    assert np.isfinite(got[:-rows]).all() and np.isnan(got[-rows:]).all()
