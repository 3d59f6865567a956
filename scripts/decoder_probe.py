#!/usr/bin/env python3
"""First measurements of the decoder counterpart and of the cross-attention launch.  (diagnostic, GPU box)

One JSON line per measurement, each the median of ROUNDS rounds of CALLS back-to-back calls between two device events
(with the round-to-round spread, max - min):

  decoder    : Decoder.forward at the decoder counterpart of bench.py's config 5 -- d_model 1024, 16 heads, d_ff 4096,
               2 blocks, seq = enc_seq = 512 -- as forwards/s, beside Encoder.forward at config 5 in the same process.
  attention  : qgemm_attention at 16 heads x d_k 64 for (seq_q, seq_kv) = (512, 512) and (128, 512): the fused launch,
               against the three-launch fallback.  The library takes the fallback only outside the fused envelope, so
               the fallback is timed at seq_kv = 516: the nearest key count past 512 that keeps the fallback's GEMMs on
               their aligned path (0.8 % more keys than the fused launch it is compared with).

Every figure is a first measurement, not a bar.  Run each invocation under its own `timeout`.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

import _pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--only", default="decoder,attention")
    args = ap.parse_args()

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    dev = torch.device("cuda", 0)
    stream = qg._stream(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.calls  # us per call

    def measure(variants):
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        res = {v: [] for v in variants}
        for r in range(args.rounds):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for v in order:
                res[v].append(timed(variants[v]))
        out = {}
        for v, t in res.items():
            t = sorted(t)
            out[v] = {"us": round(t[len(t) // 2], 2), "spread_us": round(t[-1] - t[0], 2)}
        return out

    if "decoder" in args.only:
        seq, d, H, dff, blocks = 512, 1024, 16, 4096, 2
        X = qg.fill_uniform(torch.empty((seq, d), device=dev), seed=2000)
        E = qg.fill_uniform(torch.empty((seq, d), device=dev), seed=2001)
        Y = torch.empty_like(X)
        dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=seq, seed=1000)
        enc = qg.Encoder(d, H, dff, blocks, max_seq=seq, seed=1000)
        out = measure({"decoder": lambda: dec.forward(X, E, Y), "encoder": lambda: enc.forward(X, Y)})
        for v in out.values():
            v["forwards_per_s"] = round(1e6 / v["us"], 1)
        dec.close()
        enc.close()
        print(json.dumps({"what": "forward", "seq": seq, "enc_seq": seq, "d_model": d, "n_heads": H, "d_ff": dff,
                          "n_blocks": blocks, "calls": args.calls, "rounds": args.rounds, **out,
                          "library": qg.version()}), flush=True)

    if "attention" in args.only:
        H, dk = 16, 64
        d = H * dk
        scale = 0.125
        for seq_q in (512, 128):
            Q = qg.fill_uniform(torch.empty((seq_q, d), device=dev), seed=3000)
            O = torch.empty_like(Q)
            variants = {}
            for name, seq_kv in (("fused_kv512", 512), ("fallback_kv516", 516)):
                K = qg.fill_uniform(torch.empty((seq_kv, d), device=dev), seed=3001)
                V = qg.fill_uniform(torch.empty((seq_kv, d), device=dev), seed=3002)
                need = L.qgemm_attention_workspace_size(seq_q, seq_kv, H, dk)
                assert (need == 0) == name.startswith("fused")
                ws = torch.empty(max(1, need), dtype=torch.uint8, device=dev)

                def call(K=K, V=V, ws=ws, need=need, seq_kv=seq_kv):
                    assert L.qgemm_attention(Q.data_ptr(), d, K.data_ptr(), d, V.data_ptr(), d, O.data_ptr(), d, seq_q,
                                             seq_kv, H, dk, scale, ws.data_ptr(), need, stream) == 0

                variants[name] = call
            out = measure(variants)
            print(json.dumps({"what": "cross-attention", "seq_q": seq_q, "n_heads": H, "d_k": dk, "calls": args.calls,
                              "rounds": args.rounds, **out}), flush=True)


if __name__ == "__main__":
    main()
