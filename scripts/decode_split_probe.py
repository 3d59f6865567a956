#!/usr/bin/env python3
"""Split-key decode attention against the grouped launch of the same build.  (diagnostic, GPU box)

One run; the sides alternate inside every round (standard_probe.measure: every variant takes every place), medians of
--rounds rounds of --calls calls with the round-to-round spreads.  Per shape one row with

  grouped       qgemm_attention_decode_batched_gqa (G = 1: qgemm_attention_decode_batched), the sequential launch
  split         qgemm_attention_decode_split with split_keys = 0, the rule of include/qgemm.h (the value is reported)
  split_<L>     ... with L = 128 / 256 / 512 / 1024

at 512 / 2048 / 4096 keys x 1 / 16 / 64 sequences, one masked row per sequence, heads / KV heads x d_k: 32/8 x 128,
64/8 x 128, 32/8 x 64, 32/32 x 128.  The split path must first agree with the grouped launch to 1e-5 (two orders of
rounding, not bits).  A side is "**slower**" / "faster" than grouped by llama_probe._ratios' rule: the medians differ by
more than both spreads.  Then the split path alone at 16384 and 65536 keys, where no other launch reaches (1 and 16
sequences of 32/8 x 128 and 32/8 x 64).  Nothing here routes anything: the figures are for DESIGN.md s34.

    python scripts/decode_split_probe.py [--out profiles/decode_split_probe.log]
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
LONG_SHAPES, LONG_KEYS, LONG_SEQS = ((32, 8, 128), (32, 8, 64)), (16384, 65536), (1, 16)
SWEEP = (128, 256, 512, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_split_probe.log"))
    args = ap.parse_args()

    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    st = qg._stream(dev)
    lines, lose, win = [], 0, 0
    ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    g = torch.Generator(device=dev).manual_seed(34)

    def shape_rows(H, n_kv, dk, keys, seqs, with_grouped):
        nonlocal lose, win
        d, w, scale, n_max = H * dk, n_kv * dk, 1.0 / dk ** 0.5, max(seqs)
        Q = torch.randn((n_max, d), device=dev, generator=g)
        K = torch.randn((n_max, keys, w), device=dev, generator=g)
        V = torch.randn((n_max, keys, w), device=dev, generator=g)
        out = torch.empty((n_max, d), device=dev)
        ws = torch.empty((L.qgemm_attention_decode_split_workspace_size(n_max, 1, keys, H, dk, 128),), dtype=torch.uint8,
                         device=dev)
        for n in seqs:
            lens, pos = ints([keys] * n), ints([keys - 1] * n)
            head = (Q.data_ptr(), d, K.data_ptr(), w, keys * w, V.data_ptr(), w, keys * w, out.data_ptr(), d, n, 1, None,
                    lens, pos, H)

            def split(split_keys):
                return L.qgemm_attention_decode_split(*head, n_kv, dk, scale, split_keys, ws.data_ptr(), ws.numel(), st)

            def grouped():
                if n_kv == H:
                    return L.qgemm_attention_decode_batched(*head, dk, scale, st)
                return L.qgemm_attention_decode_batched_gqa(*head, n_kv, dk, scale, st)

            default = ctypes.c_int(0)
            assert L.qgemm_attention_decode_split_plan(n, 1, keys, H, n_kv, dk, ctypes.byref(default), None) == 0
            rec = dict(n_heads=H, n_kv_heads=n_kv, d_k=dk, keys=keys, n_seqs=n, default_split_keys=default.value)
            variants = {"split": lambda: split(0)}
            variants.update({f"split_{s}": (lambda s=s: split(s)) for s in SWEEP})
            if with_grouped:
                variants["grouped"] = grouped
                assert grouped() == 0 and torch.cuda.synchronize() is None
                want = out[:n].clone()
                for s in (0,) + SWEEP:
                    out.fill_(float("nan"))
                    assert split(s) == 0 and torch.cuda.synchronize() is None
                    diff = float((out[:n] - want).abs().max())
                    assert diff <= 1e-5, ("the split path disagrees with the grouped launch", rec, s, diff)
            else:
                for s in (0,) + SWEEP:
                    assert split(s) == 0 and torch.cuda.synchronize() is None
            rec.update(measure(variants, args))
            if with_grouped:
                for v in variants:
                    if v == "grouped":
                        continue
                    gap = rec[v]["us"] - rec["grouped"]["us"]
                    rec[v]["over_grouped"] = round(rec[v]["us"] / rec["grouped"]["us"], 3)
                    if abs(gap) > max(rec[v]["spread_us"], rec["grouped"]["spread_us"]):
                        rec[v]["verdict"] = "**slower**" if gap > 0 else "faster"
                lose += rec["split"].get("verdict") == "**slower**"
                win += rec["split"].get("verdict") == "faster"
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)

    for H, n_kv, dk in SHAPES:
        for keys in KEYS:
            shape_rows(H, n_kv, dk, keys, SEQS, True)
    for H, n_kv, dk in LONG_SHAPES:
        for keys in LONG_KEYS:
            shape_rows(H, n_kv, dk, keys, LONG_SEQS, False)

    summary = json.dumps({"rows": len(lines), "default_split_faster": win, "default_split_slower": lose,
                          "calls": args.calls, "rounds": args.rounds})
    print(summary)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/decode_split_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n" + summary + "\n")


if __name__ == "__main__":
    main()
