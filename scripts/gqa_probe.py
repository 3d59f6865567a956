#!/usr/bin/env python3
"""First measurements of grouped-query decode attention.  (diagnostic, GPU box)

The baseline is what a caller did before: K and V repeated to n_heads heads (G x the cache) and the multi-head launches
of this same build -- attention_decode*.o are byte-identical to the parent commit's, so that is the parent's code.

  decode     per model shape (heads / KV heads x d_k) and per 1, 16 and 64 sequences at 512, 2048 and 4096 keys, one query
             row at the last position: qgemm_attention_gqa (1 sequence) or qgemm_attention_decode_batched_gqa beside
             qgemm_attention_causal / qgemm_attention_decode_batched on the repeated K / V;
  prefill    512 x 512 causal at 32 / 8 x 128: the grouped three launches beside qgemm_attention_causal on repeated K / V.

The outputs must agree bit for bit before anything is timed.  One process; the two sides alternate inside every round;
one JSON line per comparison with the median of ROUNDS rounds of CALLS back-to-back calls between two device events and
the round-to-round spread (max - min), in us per call; "**slower**" where the grouped side is slower by more than both
spreads.  First measurements, not bars.
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
MODELS = (("llama3_8b_mistral_7b", 32, 8, 128), ("llama_70b", 64, 8, 128), ("qwen2_7b", 28, 4, 128), ("h32_kv8_dk64", 32, 8, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gqa_probe.log"))
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

    def repeated(K, n_kv, G, dk):   # [.., n_kv * d_k] -> [.., n_kv * G * d_k], every head G times
        lead = K.shape[:-1]
        return K.view(*lead, n_kv, 1, dk).expand(*lead, n_kv, G, dk).reshape(*lead, n_kv * G * dk).contiguous()

    def compare(what, variants, outs, **tags):
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{what} {tags}: the two sides differ"
        assert bool(torch.isfinite(outs[0]).all())
        rec = measure(variants, args)
        _ratios(rec, (("gqa_over_repeated", "gqa", "repeated"),))
        emit(dict(what=what, **tags, **rec))

    # ---- decode ----
    for name, H, n_kv, dk in MODELS:
        G, d, w = H // n_kv, H * dk, n_kv * dk
        scale = ctypes.c_float(1.0 / math.sqrt(dk)).value
        for n in (1, 16, 64):
            for keys in (512, 2048, 4096):
                Q = qg.fill_uniform(torch.empty((n, d), device=dev), seed=4)
                K = torch.empty((n, keys, w), device=dev).uniform_(-1.0, 1.0)
                V = torch.empty((n, keys, w), device=dev).uniform_(-1.0, 1.0)
                Kr, Vr = repeated(K, n_kv, G, dk), repeated(V, n_kv, G, dk)
                Og, Or = torch.full((n, d), float("nan"), device=dev), torch.full((n, d), float("nan"), device=dev)
                q, k, v, kr, vr, og, orp = (t.data_ptr() for t in (Q, K, V, Kr, Vr, Og, Or))
                plan = qg.attention_gqa_plan(1, keys, H, n_kv, dk)
                if n == 1:
                    need = L.qgemm_attention_workspace_size(1, keys, H, dk)
                    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
                    variants = {
                        "gqa": lambda: ok(L.qgemm_attention_gqa(q, d, k, w, v, w, og, d, 1, keys, H, n_kv, dk, scale, 1,
                                                                keys - 1, None, 0, st)),
                        "repeated": lambda: ok(L.qgemm_attention_causal(q, d, kr, d, vr, d, orp, d, 1, keys, H, dk, scale,
                                                                        keys - 1, ws.data_ptr(), need, st))}
                else:
                    kv, qp0 = _ints([keys] * n), _ints([keys - 1] * n)
                    variants = {
                        "gqa": lambda: ok(L.qgemm_attention_decode_batched_gqa(q, d, k, w, keys * w, v, w, keys * w, og, d,
                                                                               n, 1, None, kv, qp0, H, n_kv, dk, scale, st)),
                        "repeated": lambda: ok(L.qgemm_attention_decode_batched(q, d, kr, d, keys * d, vr, d, keys * d,
                                                                                orp, d, n, 1, None, kv, qp0, H, dk, scale,
                                                                                st))}
                compare("decode", variants, (Og, Or), model=name, n_heads=H, n_kv_heads=n_kv, d_k=dk, n_seqs=n, keys=keys,
                        plan=plan, workgroups=n * n_kv * ((G + 3) // 4), repeated_workgroups=n * H)
                del Q, K, V, Kr, Vr

    # ---- prefill ----
    H, n_kv, dk, seq = 32, 8, 128, 512
    G, d, w = H // n_kv, H * dk, n_kv * dk
    scale = ctypes.c_float(1.0 / math.sqrt(dk)).value
    Q = qg.fill_uniform(torch.empty((seq, d), device=dev), seed=5)
    K = qg.fill_uniform(torch.empty((seq, w), device=dev), seed=6)
    V = qg.fill_uniform(torch.empty((seq, w), device=dev), seed=7)
    Kr, Vr = repeated(K, n_kv, G, dk), repeated(V, n_kv, G, dk)
    Og, Or = torch.full((seq, d), float("nan"), device=dev), torch.full((seq, d), float("nan"), device=dev)
    need = L.qgemm_attention_gqa_workspace_size(seq, seq, H, n_kv, dk)
    assert need == L.qgemm_attention_workspace_size(seq, seq, H, dk)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    q, k, v, kr, vr, og, orp = (t.data_ptr() for t in (Q, K, V, Kr, Vr, Og, Or))
    variants = {
        "gqa": lambda: ok(L.qgemm_attention_gqa(q, d, k, w, v, w, og, d, seq, seq, H, n_kv, dk, scale, 1, 0, ws.data_ptr(),
                                                need, st)),
        "repeated": lambda: ok(L.qgemm_attention_causal(q, d, kr, d, vr, d, orp, d, seq, seq, H, dk, scale, 0,
                                                        ws.data_ptr(), need, st))}
    compare("prefill", variants, (Og, Or), n_heads=H, n_kv_heads=n_kv, d_k=dk, seq_q=seq, seq_kv=seq,
            plan=qg.attention_gqa_plan(seq, seq, H, n_kv, dk), repeated_plan=qg.attention_plan(seq, seq, H, dk))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/gqa_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
