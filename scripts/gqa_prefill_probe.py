#!/usr/bin/env python3
"""First measurements of the fused grouped-query prefill kernel.  (diagnostic, GPU box)

Three sides per shape, all of this build:
  fused      qgemm_attention_varlen_gqa: ONE launch of attention_fused_gqa_kernel;
  grouped    qgemm_attention_gqa sequence by sequence, the grouped three launches (2 G + 1 launches each) -- what the
             call would otherwise run; attention_launch's code for it and gemm_f32.o are the parent commit's;
  repeated   qgemm_attention_varlen on K / V repeated to n_heads heads, the workaround: the multi-head fused kernel at
             d_k 64, three launches per sequence at d_k 128 (attention.o is byte-identical to the parent's).
Shapes: one 512 x 512 causal sequence at 32 / 8 x 128 (s30's 108.0 against 85.3 us), at 32 / 8 x 64 and at 28 / 4 x 128,
and 16 causal sequences of 64 .. 512 rows at 32 / 8 x 128 in one call.

The outputs must agree bit for bit before anything is timed.  One process; the sides alternate inside every round; one
JSON line per shape with the median of ROUNDS rounds of CALLS back-to-back calls between two device events and the
round-to-round spread (max - min), in us per call; "**slower**" where the fused side is slower than another by more
than both spreads, "faster" where it is faster by more than both.  First measurements, not bars.
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

from standard_probe import measure  # noqa: E402 - the protocol of s25's probe, unchanged
from varlen_probe import _ints, _longs, _prefix  # noqa: E402

# (name, heads, KV heads, d_k, sequence lengths)
SHAPES = (("512x512", 32, 8, 128, (512,)), ("512x512", 32, 8, 64, (512,)), ("512x512", 28, 4, 128, (512,)),
          ("16_sequences", 32, 8, 128, tuple(64 + 448 * i // 15 for i in range(16))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gqa_prefill_probe.log"))
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

    def ok(rc):
        assert rc == 0, rc

    def repeated(K, n_kv, G, dk):   # [rows, n_kv * d_k] -> [rows, n_kv * G * d_k], every head G times
        return K.view(-1, n_kv, 1, dk).expand(-1, n_kv, G, dk).reshape(-1, n_kv * G * dk).contiguous()

    for name, H, n_kv, dk, lens in SHAPES:
        G, d, w, n, rows = H // n_kv, H * dk, n_kv * dk, len(lens), sum(lens)
        scale = ctypes.c_float(1.0 / math.sqrt(dk)).value
        Q = qg.fill_uniform(torch.empty((rows, d), device=dev), seed=5)
        K = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=6)
        V = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=7)
        Kr, Vr = repeated(K, n_kv, G, dk), repeated(V, n_kv, G, dk)
        outs = [torch.full((rows, d), float("nan"), device=dev) for _ in range(3)]
        sq, row0, pos0 = _ints(lens), _longs(_prefix(lens)), _ints([0] * n)
        assert L.qgemm_attention_varlen_gqa_workspace_size(n, sq, sq, H, n_kv, dk) == 0
        need = max(L.qgemm_attention_gqa_workspace_size(s, s, H, n_kv, dk) for s in lens)
        need_r = L.qgemm_attention_varlen_workspace_size(n, sq, sq, H, dk)
        ws = torch.empty(max(need, need_r, 1), dtype=torch.uint8, device=dev)
        q, k, v, kr, vr, o_f, o_g, o_r = (t.data_ptr() for t in (Q, K, V, Kr, Vr, *outs))

        def grouped():
            for s, r0 in zip(lens, _prefix(lens)):
                ok(L.qgemm_attention_gqa(q + 4 * r0 * d, d, k + 4 * r0 * w, w, v + 4 * r0 * w, w, o_g + 4 * r0 * d, d, s, s, H,
                                         n_kv, dk, scale, 1, 0, ws.data_ptr(), need, st))

        variants = {
            "fused": lambda: ok(L.qgemm_attention_varlen_gqa(q, d, k, w, v, w, o_f, d, n, row0, sq, row0, sq, pos0, H, n_kv,
                                                             dk, scale, None, 0, st)),
            "grouped": grouped,
            "repeated": lambda: ok(L.qgemm_attention_varlen(q, d, kr, d, vr, d, o_r, d, n, row0, sq, row0, sq, pos0, H, dk,
                                                            scale, ws.data_ptr() if need_r else None, need_r, st))}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        for other in outs[1:]:
            assert torch.equal(outs[0].view(torch.int32), other.view(torch.int32)), f"{name} {H}/{n_kv}x{dk}: sides differ"
        assert bool(torch.isfinite(outs[0]).all())
        rec = measure(variants, args)
        for other in ("grouped", "repeated"):
            gap = rec["fused"]["us"] - rec[other]["us"]
            rec[f"fused_over_{other}"] = round(rec["fused"]["us"] / rec[other]["us"], 3)
            if abs(gap) > max(rec["fused"]["spread_us"], rec[other]["spread_us"]):
                rec[f"fused_over_{other}_verdict"] = "**slower**" if gap > 0 else "faster"
        rec = dict(what=name, n_heads=H, n_kv_heads=n_kv, d_k=dk, n_seqs=n, rows=rows, workgroups=sum((s + 31) // 32 for s in lens) * H,
                   plan=qg.attention_varlen_gqa_plan(lens, lens, H, n_kv, dk),
                   grouped_plan=qg.attention_gqa_plan(lens[-1], lens[-1], H, n_kv, dk), grouped_launches=n * (2 * G + 1),
                   repeated_plan=qg.attention_varlen_plan(lens, lens, H, dk), **rec, calls=args.calls, rounds=args.rounds)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del Q, K, V, Kr, Vr, outs, ws

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/gqa_prefill_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
