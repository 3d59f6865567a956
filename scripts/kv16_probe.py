#!/usr/bin/env python3
"""First measurements of decode attention over a bf16 K / V cache.  (diagnostic, GPU box)

The baseline is the fp32 launch of this same build on the widened cache -- attention_decode*.o are byte-identical to the
parent commit's, so that is the parent's code: qgemm_attention_decode_batched_gqa (G >= 2) or
qgemm_attention_decode_batched (G = 1) beside qgemm_attention_decode_batched_kv16, one query row at the last position,
causal, for 1, 16 and 64 sequences at 512, 2048 and 4096 keys per model shape; then qgemm_kv_append_bf16 on 64 x 1 rows
of width 1024 alone (it has no counterpart).

The outputs must agree bit for bit before anything is timed.  One process; the two sides alternate inside every round;
one JSON line per comparison with the median of ROUNDS rounds of CALLS back-to-back calls between two device events and
the round-to-round spread (max - min), in us per call; "**slower**" where the bf16 side is slower by more than both
spreads, "faster" where it is faster by more than both.  First measurements, not bars.
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

# (name, heads, KV heads, d_k)
MODELS = (("llama3_8b_mistral_7b", 32, 8, 128), ("llama_70b", 64, 8, 128), ("h32_kv8_dk64", 32, 8, 64),
          ("mha_h32_dk128", 32, 32, 128))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kv16_probe.log"))
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

    def emit(rec):
        rec.update(calls=args.calls, rounds=args.rounds)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def ok(rc):
        assert rc == 0, rc

    for name, H, n_kv, dk in MODELS:
        d, w = H * dk, n_kv * dk
        scale = ctypes.c_float(1.0 / math.sqrt(dk)).value
        for n in (1, 16, 64):
            for keys in (512, 2048, 4096):
                Q = qg.fill_uniform(torch.empty((n, d), device=dev), seed=4)
                K16 = torch.empty((n, keys, w), device=dev).uniform_(-1.0, 1.0).to(torch.bfloat16)
                V16 = torch.empty((n, keys, w), device=dev).uniform_(-1.0, 1.0).to(torch.bfloat16)
                K32, V32 = K16.float(), V16.float()
                O16, O32 = torch.full((n, d), float("nan"), device=dev), torch.full((n, d), float("nan"), device=dev)
                q, k16, v16, k32, v32, o16, o32 = (t.data_ptr() for t in (Q, K16, V16, K32, V32, O16, O32))
                kv, qp0 = _ints([keys] * n), _ints([keys - 1] * n)
                if n_kv == H:
                    fp32 = lambda: ok(L.qgemm_attention_decode_batched(  # noqa: E731
                        q, d, k32, w, keys * w, v32, w, keys * w, o32, d, n, 1, None, kv, qp0, H, dk, scale, st))
                else:
                    fp32 = lambda: ok(L.qgemm_attention_decode_batched_gqa(  # noqa: E731
                        q, d, k32, w, keys * w, v32, w, keys * w, o32, d, n, 1, None, kv, qp0, H, n_kv, dk, scale, st))
                variants = {
                    "kv16": lambda: ok(L.qgemm_attention_decode_batched_kv16(
                        q, d, k16, w, keys * w, v16, w, keys * w, o16, d, n, 1, None, kv, qp0, H, n_kv, dk, scale, st)),
                    "fp32": fp32}
                for fn in variants.values():
                    fn()
                torch.cuda.synchronize()
                assert torch.equal(O16.view(torch.int32), O32.view(torch.int32)), f"{name} {n} x {keys}: the sides differ"
                assert bool(torch.isfinite(O16).all())
                rec = measure(variants, args)
                _ratios(rec, (("kv16_over_fp32", "kv16", "fp32"),))
                if rec["fp32"]["us"] - rec["kv16"]["us"] > max(rec["kv16"]["spread_us"], rec["fp32"]["spread_us"]):
                    rec["kv16_over_fp32_verdict"] = "faster"
                emit(dict(what="decode", model=name, n_heads=H, n_kv_heads=n_kv, d_k=dk, n_seqs=n, keys=keys,
                          plan=qg.attention_decode_kv16_plan(1, H, n_kv, dk),
                          workgroups=n * n_kv * ((H // n_kv + 3) // 4), **rec))
                del Q, K16, V16, K32, V32

    # ---- the append: 64 sequences x 1 row of width 1024 (8 KV heads x 128) ----
    n, w, rows = 64, 1024, 16
    src = torch.empty((n, 3 * w), device=dev).uniform_(-1.0, 1.0)
    K, V = src[:, w:2 * w], src[:, 2 * w:]
    Kc, Vc = (torch.zeros((n, rows, w), dtype=torch.bfloat16, device=dev) for _ in range(2))
    pos = _ints([b % rows for b in range(n)])
    append = lambda: ok(L.qgemm_kv_append_bf16(  # noqa: E731
        K.data_ptr(), 3 * w, V.data_ptr(), 3 * w, Kc.data_ptr(), w, rows * w, Vc.data_ptr(), w, rows * w, n, 1, None, pos,
        w, st))
    append()
    torch.cuda.synchronize()
    at = torch.arange(n, device=dev)
    assert torch.equal(Kc[at, at % rows], K.to(torch.bfloat16)) and torch.equal(Vc[at, at % rows], V.to(torch.bfloat16))
    emit(dict(what="kv_append_bf16", n_seqs=n, rows_per_seq=1, width=w, **measure({"append": append}, args)))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/kv16_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
