"""GPU test of the bf16 cache append (kv_append_bf16_kernel) through qgemm_kv_append_bf16: the rows it
writes carry the bit patterns of the CPU's rounding to bf16 -- nearest even, +-inf past the bf16 maximum, subnormals
and -0 kept, NaN stays NaN -- and every other element of the NaN-poisoned slabs keeps its bits."""
import numpy as np
import pytest
import torch

import attn_oracle
import causal_oracle
from oracle import oracle as O
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

POISON = 0x7FC1  # a NaN pattern the kernel never writes
# 1 + 2^-8 ties to 1 (even), 1 + 3 * 2^-8 ties to 1 + 2^-6; 3.3961775e38 lies above the bf16 maximum
PLANTED = np.array([np.inf, -np.inf, -0.0, 1e-40, 3.3961775e38, 1.00390625, 1.01171875], np.float32)


def _bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("case", [(1, 1, 8, "aligned"), (3, 2, 1024, "aligned"), (2, 8, 100, "aligned"),
                                  (2, 1, 129, "odd"), (2, 3, 256, "qkv")], ids=str)
def test_append_rounds_and_writes_only_its_rows(qg, device, case):
    """how "odd": the destination one element past alignment with an odd row stride; how "qkv": the sources are the K
    and V thirds of a [Q | K | V] buffer."""
    n_seqs, rps, width, how = case
    rows, slab_rows = n_seqs * rps, 12
    src = [O.uniform((rows, width), 901 + i) for i in range(2)]
    for a in src:
        flat = a.reshape(-1)
        flat[:len(PLANTED)] = PLANTED[:flat.size]
        flat[-1] = np.nan
    if how == "qkv":
        buf = torch.zeros((rows, 3 * width), device=device)
        buf[:, width:2 * width], buf[:, 2 * width:] = (torch.from_numpy(a).to(device) for a in src)
        Kd, Vd = buf[:, width:2 * width], buf[:, 2 * width:]
    else:
        Kd, Vd = (torch.from_numpy(a).to(device) for a in src)
    pad = 3 + width % 2 if how == "odd" else 0   # an odd row stride
    store = [torch.full((n_seqs + 1, slab_rows, width + pad), POISON, dtype=torch.int16, device=device).view(torch.bfloat16)
             for _ in range(2)]
    Kc, Vc = (s[:, :, 1:1 + width] if pad else s for s in store)
    kv_slot, pos = [n_seqs - b for b in range(n_seqs)], [(3 * b + 1) % (slab_rows - rps + 1) for b in range(n_seqs)]
    qg.kv_append_bf16(Kd, Vd, Kc, Vc, pos, kv_slot=kv_slot, rows_per_seq=rps)
    for a, s in zip(src, store):
        want = np.full(tuple(s.shape), POISON, np.uint16)
        rounded = _bits(torch.from_numpy(a).to(torch.bfloat16))
        for b in range(n_seqs):
            want[kv_slot[b], pos[b]:pos[b] + rps, (1 if pad else 0):(1 if pad else 0) + width] = rounded[b * rps:(b + 1) * rps]
        got = _bits(s)
        nan = (want & 0x7FFF) > 0x7F80   # the planted NaN reads back as a NaN, the poison keeps its bits
        assert ((got[nan] & 0x7FFF) > 0x7F80).all() and (got[want == POISON] == POISON).all()
        assert np.array_equal(got[~nan], want[~nan]), f"{case}: {(got[~nan] != want[~nan]).sum()} elements differ"


def test_append_then_decode(qg, oracle, device):
    """Rows 0 .. n - 1 appended in two calls, then attention_decode_batched_kv16 equals the oracle on the rounded values."""
    H, n_kv, dk, n = 4, 2, 64, 37
    Q, K, V = O.uniform((1, H * dk), 951), O.uniform((n, n_kv * dk), 952), O.uniform((n, n_kv * dk), 953)
    Kc, Vc = (torch.zeros((1, n + 2, n_kv * dk), dtype=torch.bfloat16, device=device) for _ in range(2))
    Kd, Vd = torch.from_numpy(K).to(device), torch.from_numpy(V).to(device)
    qg.kv_append_bf16(Kd[:30], Vd[:30], Kc, Vc, [0], rows_per_seq=30)
    qg.kv_append_bf16(Kd[30:], Vd[30:], Kc, Vc, [30], rows_per_seq=n - 30)
    out = torch.full((1, H * dk), float("nan"), device=device)
    qg.attention_decode_batched_kv16(torch.from_numpy(Q).to(device), Kc, Vc, H, n_kv, [n], q_pos0=[n - 1], O=out)
    Kr, Vr = (np.repeat(torch.from_numpy(a).to(torch.bfloat16).float().numpy().reshape(n, n_kv, dk), H // n_kv,
                        axis=1).reshape(n, -1) for a in (K, V))
    want = causal_oracle.attention_causal_ref(Q, Kr, Vr, H, attn_oracle.default_scale(dk), n - 1)
    assert_bits_equal(out.cpu().numpy(), want, "append + decode")
