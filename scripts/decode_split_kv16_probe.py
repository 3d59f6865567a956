#!/usr/bin/env python3
"""Split-key decode attention over a bf16 cache against its two neighbours of the same build.
(diagnostic, GPU box)

One run; the sides alternate inside every round (standard_probe.measure: every variant takes every place), medians of
--rounds rounds of --calls calls with the round-to-round spreads.  Per shape one row with

  kv16          qgemm_attention_decode_split_kv16 with split_keys = 0, the rule of include/qgemm.h (the value is reported)
  kv16_<L>      ... with L = 128 / 256 / 512 / 1024
  f32, f32_<L>  qgemm_attention_decode_split on the same cache widened to fp32, the same L
  batched_kv16  qgemm_attention_decode_batched_kv16, the sequential launch on the bf16 cache (keys <= 4096)

at 512 / 2048 / 4096 keys x 1 / 16 / 64 sequences and 16384 / 65536 keys x 1 / 16 sequences, one masked row per
sequence, heads / KV heads x d_k: 32/8 x 128, 64/8 x 128, 32/8 x 64, 32/32 x 128 (the long keys: the first two and
32/8 x 64).  Before any timing every kv16 side must equal its f32 side BIT FOR BIT.  A kv16 side is "**slower**" /
"faster" than a neighbour when the medians differ by more than both spreads; "over_f32" / "over_batched" are the ratios of
the medians.  The last line reports the bytes of K + V per second of the default kv16 side at the largest shape (bytes
the algorithm needs from the shapes, over the call's time: launch and merge included).  Nothing here routes anything: the
figures are for DESIGN.md s36.

    python scripts/decode_split_kv16_probe.py [--out profiles/decode_split_kv16_probe.log]
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from standard_probe import measure  # noqa: E402

SHAPES = ((32, 8, 128), (64, 8, 128), (32, 8, 64), (32, 32, 128))
KEYS, SEQS = (512, 2048, 4096), (1, 16, 64)
LONG_SHAPES, LONG_KEYS, LONG_SEQS = ((32, 8, 128), (64, 8, 128), (32, 8, 64)), (16384, 65536), (1, 16)
SWEEP = (128, 256, 512, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_split_kv16_probe.log"))
    args = ap.parse_args()

    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    st = qg._stream(dev)
    lines, count, last = [], {}, None
    ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    g = torch.Generator(device=dev).manual_seed(36)

    def verdict(rec, side, other, key):
        gap = rec[side]["us"] - rec[other]["us"]
        rec[side][key] = round(rec[side]["us"] / rec[other]["us"], 3)
        if abs(gap) > max(rec[side]["spread_us"], rec[other]["spread_us"]):
            word = "**slower**" if gap > 0 else "faster"
            rec[side][key + "_verdict"] = word
            if side == "kv16":
                count[key, word] = count.get((key, word), 0) + 1

    def shape_rows(H, n_kv, dk, keys, seqs, with_batched):
        nonlocal last
        d, w, scale, n_max = H * dk, n_kv * dk, 1.0 / dk ** 0.5, max(seqs)
        Q = torch.randn((n_max, d), device=dev, generator=g)
        K16 = torch.randn((n_max, keys, w), device=dev, generator=g).bfloat16()
        V16 = torch.randn((n_max, keys, w), device=dev, generator=g).bfloat16()
        K32, V32 = K16.float(), V16.float()
        out = torch.empty((n_max, d), device=dev)
        ws = torch.empty((L.qgemm_attention_decode_split_workspace_size(n_max, 1, keys, H, dk, 128),), dtype=torch.uint8,
                         device=dev)
        for n in seqs:
            lens, pos = ints([keys] * n), ints([keys - 1] * n)

            def head(Kt, Vt):
                return (Q.data_ptr(), d, Kt.data_ptr(), w, keys * w, Vt.data_ptr(), w, keys * w, out.data_ptr(), d, n, 1,
                        None, lens, pos, H, n_kv, dk, scale)

            h16, h32 = head(K16, V16), head(K32, V32)

            def kv16(split_keys):
                return L.qgemm_attention_decode_split_kv16(*h16, split_keys, ws.data_ptr(), ws.numel(), st)

            def f32(split_keys):
                return L.qgemm_attention_decode_split(*h32, split_keys, ws.data_ptr(), ws.numel(), st)

            def batched():
                return L.qgemm_attention_decode_batched_kv16(*h16, st)

            default = ctypes.c_int(0)
            assert L.qgemm_attention_decode_split_kv16_plan(n, 1, keys, H, n_kv, dk, ctypes.byref(default), None) == 0
            rec = dict(n_heads=H, n_kv_heads=n_kv, d_k=dk, keys=keys, n_seqs=n, default_split_keys=default.value)
            variants = {"kv16": lambda: kv16(0), "f32": lambda: f32(0)}
            for s in SWEEP:
                variants[f"kv16_{s}"] = lambda s=s: kv16(s)
                variants[f"f32_{s}"] = lambda s=s: f32(s)
            if with_batched:
                variants["batched_kv16"] = batched
            for s in (0,) + SWEEP:  # the contract first: the widened cache's bits
                out.fill_(float("nan"))
                assert f32(s) == 0 and torch.cuda.synchronize() is None
                want = out[:n].clone()
                out.fill_(float("nan"))
                assert kv16(s) == 0 and torch.cuda.synchronize() is None
                assert torch.equal(out[:n].view(torch.int32), want.view(torch.int32)), ("bits differ", rec, s)
            rec.update(measure(variants, args))
            verdict(rec, "kv16", "f32", "over_f32")
            for s in SWEEP:
                verdict(rec, f"kv16_{s}", f"f32_{s}", "over_f32")
            if with_batched:
                verdict(rec, "kv16", "batched_kv16", "over_batched")
            kv_bytes = 2 * n * keys * w * 2  # K and V, bf16
            rec["kv16"]["kv_TBps"] = round(kv_bytes / rec["kv16"]["us"] / 1e6, 3)
            rec["f32"]["kv_TBps"] = round(2 * kv_bytes / rec["f32"]["us"] / 1e6, 3)
            if last is None or kv_bytes >= last[0]:
                last = (kv_bytes, rec)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)

    for H, n_kv, dk in SHAPES:
        for keys in KEYS:
            shape_rows(H, n_kv, dk, keys, SEQS, True)
    for H, n_kv, dk in LONG_SHAPES:
        for keys in LONG_KEYS:
            shape_rows(H, n_kv, dk, keys, LONG_SEQS, False)

    big = last[1]
    summary = json.dumps({"rows": len(lines), "default_kv16": {f"{k} {w}": c for (k, w), c in sorted(count.items())},
                          "largest": {k: big[k] for k in ("n_heads", "n_kv_heads", "d_k", "keys", "n_seqs")},
                          "largest_kv_bytes": last[0], "largest_kv16_TBps": big["kv16"]["kv_TBps"],
                          "largest_f32_TBps": big["f32"]["kv_TBps"], "calls": args.calls, "rounds": args.rounds})
    print(summary)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/decode_split_kv16_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n" + summary + "\n")


if __name__ == "__main__":
    main()
