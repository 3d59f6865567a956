#!/usr/bin/env python3
"""First measurements of the tiled prefill attention over a bf16 K / V cache.  (diagnostic, GPU box)

qgemm_attention_varlen_tiled_kv16 beside what a holder of a bf16 cache has today, all of the SAME build, causal, at
32 / 8 x 128, 32 / 8 x 64 and 32 / 32 x 128 (heads / KV heads x d_k):
  fp32     qgemm_attention_varlen_tiled on K / V widened beforehand (the kernel against the kernel);
  widen    that call plus the widening of the visible rows (.float() of seq_kv rows of K and of V) inside the timed call.
Shapes (s35's): one sequence of 512, 2048 and 4096 rows against as many keys; a 512-row chunk at q_pos0 3584 (4096 keys);
a 512-row chunk against 65536 keys.  Before anything is timed the kv16 output is compared BIT FOR BIT with both fp32 sides.

One process; the sides alternate inside every round; one JSON line per shape with the median of ROUNDS rounds of CALLS
back-to-back calls between two device events and the round-to-round spread (max - min), in us per call.  "**slower**"
marks a row where the new call's median exceeds the fp32 call's by more than both spreads.  First measurements, not bars:
no routing rule follows from them.
"""
import argparse
import ctypes
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from llama_probe import _ints, _ratios  # noqa: E402 - the verdict rule of s28's probe
from standard_probe import measure  # noqa: E402 - the protocol of s25's probe, unchanged

HEADS = ((32, 8, 128), (32, 8, 64), (32, 32, 128))
# (tag, seq_q, seq_kv, q_pos0)
SHAPES = [("square", n, n, 0) for n in (512, 2048, 4096)] + [("chunk", 512, 4096, 3584), ("chunk", 512, 65536, 65024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attention_tiled_kv16_probe.log"))
    args = ap.parse_args()

    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    st = qg._stream(dev)
    lines = [json.dumps(dict(what="library", version=qg.version()))]
    print(lines[0], flush=True)

    for H, n_kv, dk in HEADS:
        for tag, seq_q, seq_kv, pos in SHAPES:
            d, dkv = H * dk, n_kv * dk
            Q = torch.randn((seq_q, d), device=dev)
            K16, V16 = (torch.randn((seq_kv, dkv), device=dev).bfloat16() for _ in range(2))
            K32, V32 = K16.float(), V16.float()
            out = {k: torch.full((seq_q, d), float("nan"), device=dev) for k in ("kv16", "fp32", "widen")}
            sq, skv, p0 = _ints([seq_q]), _ints([seq_kv]), _ints([pos])
            zero = (ctypes.c_int64 * 1)(0)
            tail = (1, zero, sq, zero, skv, p0, H, n_kv, dk, ctypes.c_float(1.0 / math.sqrt(dk)).value, st)

            def kv16():
                rc = L.qgemm_attention_varlen_tiled_kv16(Q.data_ptr(), d, K16.data_ptr(), dkv, V16.data_ptr(), dkv,
                                                         out["kv16"].data_ptr(), d, *tail)
                assert rc == 0, rc

            def fp32(K=K32, V=V32, O=out["fp32"]):
                rc = L.qgemm_attention_varlen_tiled(Q.data_ptr(), d, K.data_ptr(), dkv, V.data_ptr(), dkv, O.data_ptr(), d,
                                                    *tail)
                assert rc == 0, rc

            def widen():
                fp32(K16[:seq_kv].float(), V16[:seq_kv].float(), out["widen"])

            variants = {"kv16": kv16, "fp32": fp32, "widen": widen}
            for fn in variants.values():
                fn()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out["kv16"]).all())
            for side in ("fp32", "widen"):  # bit for bit before anything is timed
                assert torch.equal(out["kv16"].view(torch.int32), out[side].view(torch.int32)), f"kv16 != {side}"
            rec = dict(what=tag, n_heads=H, n_kv_heads=n_kv, d_k=dk, seq_q=seq_q, seq_kv=seq_kv, bits_equal=True,
                       plan=qg.attention_varlen_tiled_kv16_plan([seq_q], [seq_kv], H, n_kv, dk))
            rec.update(measure(variants, args))
            _ratios(rec, (("kv16_over_fp32", "kv16", "fp32"), ("kv16_over_widen", "kv16", "widen")))
            # visible (row, key) pairs -> fp32 multiply-adds of both products, for a rate
            pairs = sum(min(seq_kv, pos + r + 1) for r in range(seq_q))
            rec.update(kv16_tflops=round(4.0 * pairs * dk * H / rec["kv16"]["us"] * 1e-6, 2), calls=args.calls,
                       rounds=args.rounds)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del Q, K16, V16, K32, V32, out

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/attention_tiled_kv16_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
