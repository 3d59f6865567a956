#!/usr/bin/env python3
"""First measurements of the causal mask.  (diagnostic, GPU box)

One JSON line per measurement, each the median of ROUNDS rounds of CALLS back-to-back calls between two device events
(with the round-to-round spread, max - min); the variants of one measurement alternate inside every round, in one
process:

  attention : the fused launch at 16 heads x d_k 64, seq_q = seq_kv = 512: qgemm_attention against
              qgemm_attention_causal with q_pos0 = 0.  The outputs are checked first: the masked call with
              q_pos0 = 511 must give the unmasked call's bits, the one with q_pos0 = 0 must not.
  decoder   : Decoder.forward at the decoder counterpart of bench.py's config 5 -- d_model 1024, 16 heads, d_ff 4096,
              2 blocks, seq = enc_seq = 512 -- with and without causal=True.

Exit status 1 if the masked launch is slower than the unmasked one (medians of this run); how much faster it is is a
first measurement, not a bar.  Run each invocation under its own `timeout`.
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--only", default="attention,decoder")
    ap.add_argument("--sweep", type=int, nargs="*", default=[], help="more q_pos0 values to time at 512 x 512")
    args = ap.parse_args()

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
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

    status = 0
    if "attention" in args.only:
        seq, H, dk = 512, 16, 64
        d = H * dk
        scale = 0.125
        Q = qg.fill_uniform(torch.empty((seq, d), device=dev), seed=3000)
        K = qg.fill_uniform(torch.empty((seq, d), device=dev), seed=3001)
        V = qg.fill_uniform(torch.empty((seq, d), device=dev), seed=3002)
        O = torch.empty_like(Q)
        assert L.qgemm_attention_workspace_size(seq, seq, H, dk) == 0, "the fused launch"

        def plain():
            assert L.qgemm_attention(Q.data_ptr(), d, K.data_ptr(), d, V.data_ptr(), d, O.data_ptr(), d, seq, seq, H, dk,
                                     scale, None, 0, stream) == 0

        def masked(q_pos0=0):
            assert L.qgemm_attention_causal(Q.data_ptr(), d, K.data_ptr(), d, V.data_ptr(), d, O.data_ptr(), d, seq, seq,
                                            H, dk, scale, q_pos0, None, 0, stream) == 0

        plain()
        ref = O.clone()
        masked(seq - 1)
        same = bool(torch.equal(O.view(torch.int32), ref.view(torch.int32)))
        masked(0)
        rows_changed = int((O.view(torch.int32) != ref.view(torch.int32)).any(dim=1).sum())
        assert same, "q_pos0 = seq_kv - 1 must give qgemm_attention's bits"
        assert rows_changed == seq - 1, f"q_pos0 = 0 must change every row but the last ({rows_changed} changed)"
        variants = {"unmasked": plain, "causal_q_pos0_0": masked}
        for p0 in args.sweep:   # further offsets beside the two: seq - 1 is the mask without effect
            variants[f"causal_q_pos0_{p0}"] = lambda p0=p0: masked(p0)
        out = measure(variants)
        ratio = out["causal_q_pos0_0"]["us"] / out["unmasked"]["us"]
        print(json.dumps({"what": "fused attention", "seq_q": seq, "seq_kv": seq, "n_heads": H, "d_k": dk,
                          "calls": args.calls, "rounds": args.rounds, **out, "causal_over_unmasked": round(ratio, 3),
                          "library": qg.version()}), flush=True)
        if ratio > 1.0:
            print("the masked launch is slower than the unmasked one", file=sys.stderr)
            status = 1

    if "decoder" in args.only:
        seq, d, H, dff, blocks = 512, 1024, 16, 4096, 2
        X = qg.fill_uniform(torch.empty((seq, d), device=dev), seed=2000)
        E = qg.fill_uniform(torch.empty((seq, d), device=dev), seed=2001)
        Y = torch.empty_like(X)
        dec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=seq, seed=1000)
        cdec = qg.Decoder(d, H, dff, blocks, max_seq=seq, max_enc_seq=seq, seed=1000, causal=True)
        out = measure({"decoder": lambda: dec.forward(X, E, Y), "causal_decoder": lambda: cdec.forward(X, E, Y)})
        for v in out.values():
            v["forwards_per_s"] = round(1e6 / v["us"], 1)
        dec.close()
        cdec.close()
        print(json.dumps({"what": "decoder forward", "seq": seq, "enc_seq": seq, "d_model": d, "n_heads": H, "d_ff": dff,
                          "n_blocks": blocks, "calls": args.calls, "rounds": args.rounds, **out}), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
