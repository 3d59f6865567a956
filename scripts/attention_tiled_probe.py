#!/usr/bin/env python3
"""First measurements of the tiled online-softmax prefill attention.  (diagnostic, GPU box)

qgemm_attention_varlen_tiled beside qgemm_attention_varlen_gqa of the SAME build -- its fused launch at <= 512 keys, its
per-sequence (grouped) three launches through the score workspace at 513 .. 4096 -- causal, at 32 / 8 x 128, 32 / 8 x 64 and
32 / 32 x 128 (heads / KV heads x d_k):
  square     one sequence of 512, 2048 and 4096 rows against as many keys;
  packed     16 packed sequences of 64 .. 4096 rows, each against its own keys;
  chunk      a 512-row chunk of a chunked prefill at q_pos0 3584 (4096 keys);
  alone      what only the tiled path serves: 16384 x 16384, and a 512-row chunk against 65536 keys.
The two paths have different numerical contracts, so before anything is timed their outputs are compared by a loose
bound (2e-4), not bit for bit.

One process; the two sides alternate inside every round; one JSON line per comparison with the median of ROUNDS rounds of
CALLS back-to-back calls between two device events and the round-to-round spread (max - min), in us per call.
Everything goes through the C-ABI with arguments built beforehand.  First measurements, not bars: no routing rule
follows from them.
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
PACKED = (64, 128, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 3072, 3328, 3584, 4096)
# (tag, seq_q, seq_kv, q_pos0, compared with attention_varlen_gqa)
SHAPES = [("square", (n,), (n,), (0,), True) for n in (512, 2048, 4096)] + [
    ("packed", PACKED, PACKED, (0,) * len(PACKED), True),
    ("chunk", (512,), (4096,), (3584,), True),
    ("alone", (16384,), (16384,), (0,), False),
    ("alone_chunk", (512,), (65536,), (65024,), False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attention_tiled_probe.log"))
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

    def longs(v):
        return (ctypes.c_int64 * len(v))(*v)

    for H, n_kv, dk in HEADS:
        for tag, seq_q, seq_kv, pos, both in SHAPES:
            n, d, dkv = len(seq_q), H * dk, n_kv * dk
            Q = torch.randn((sum(seq_q), d), device=dev)
            K, V = torch.randn((sum(seq_kv), dkv), device=dev), torch.randn((sum(seq_kv), dkv), device=dev)
            out = {k: torch.full((sum(seq_q), d), float("nan"), device=dev) for k in ("tiled", "existing")}
            sq, skv, p0 = _ints(list(seq_q)), _ints(list(seq_kv)), _ints(list(pos))
            q0 = longs([sum(seq_q[:b]) for b in range(n)])
            k0 = longs([sum(seq_kv[:b]) for b in range(n)])
            scale = ctypes.c_float(1.0 / math.sqrt(dk)).value
            head = (Q.data_ptr(), d, K.data_ptr(), dkv, V.data_ptr(), dkv)
            tail = (n, q0, sq, k0, skv, p0, H, n_kv, dk, scale)

            def tiled():
                rc = L.qgemm_attention_varlen_tiled(*head, out["tiled"].data_ptr(), d, *tail, st)
                assert rc == 0, rc

            variants = {"tiled": tiled}
            rec = dict(what=tag, n_heads=H, n_kv_heads=n_kv, d_k=dk, seq_q=sum(seq_q), seq_kv=max(seq_kv), n_seqs=n,
                       tiled_plan=qg.attention_varlen_tiled_plan(seq_q, seq_kv, H, n_kv, dk))
            if both:
                need = L.qgemm_attention_varlen_gqa_workspace_size(n, sq, skv, H, n_kv, dk)
                ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)

                def existing():
                    rc = L.qgemm_attention_varlen_gqa(*head, out["existing"].data_ptr(), d, *tail, ws.data_ptr(), need, st)
                    assert rc == 0, rc

                variants["existing"] = existing
                rec.update(existing_plan=qg.attention_varlen_gqa_plan(seq_q, seq_kv, H, n_kv, dk), workspace_bytes=need)
            for fn in variants.values():
                fn()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out["tiled"]).all())
            if both:
                diff = float((out["tiled"] - out["existing"]).abs().max())
                assert diff < 2e-4, f"the two paths differ by {diff}"
                rec.update(max_abs_diff=diff)
            rec.update(measure(variants, args))
            if both:
                _ratios(rec, (("tiled_over_existing", "tiled", "existing"),))
            # visible (row, key) pairs -> fp32 multiply-adds of both products, for a rate
            pairs = sum(sum(min(kv, p + r + 1) for r in range(q)) for q, kv, p in zip(seq_q, seq_kv, pos))
            rec.update(tiled_tflops=round(4.0 * pairs * dk * H / rec["tiled"]["us"] * 1e-6, 2), calls=args.calls,
                       rounds=args.rounds)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del Q, K, V, out

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/attention_tiled_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
