#!/usr/bin/env python3
"""First measurements of incremental decoding.  (diagnostic, GPU box)

One JSON line per measurement, each the median of ROUNDS rounds of CALLS back-to-back calls between two device events
(with the round-to-round spread, max - min); the variants of one measurement alternate inside every round, in one
process:

  launch : 16 heads x d_k 64, seq_q 1 and 8: attention_decode_kernel against the launch it replaces -- the fused launch
           at seq_kv 128 and 512, the three launches at seq_kv 516, 2048 and 4096.  This tree's library no longer runs
           those for seq_q <= 8 and does not export its internal launchers, so the replaced launch comes from
           --parent-lib, the parent commit's libqgemm.so built beside the tree; its output must equal the decode
           kernel's bit for bit.  The mask is the decoding step's: q_pos0 = seq_kv - seq_q.
  token  : d_model 1024, 16 heads, d_ff 4096, 2 blocks, enc_seq 512: step(n = 1) at pos 0, 511, 2047 and 4095 against
           the causal forward of the same prefix length (pos + 1 rows), the only way to get that row without a cache.
           The step's row must equal the forward's last row bit for bit.

           With a --parent-lib that already has the decode kernel (any commit after the one that added it) the variant
           is that library's own decode launch, "parent_decode": the same kernel before and after a change to it.

Exit status 1 if, at seq_kv 512, the decode launch is slower than the fused launch by more than the fused launch's own
round-to-round spread (seq_q 1 or 8); against a parent_decode, if it is slower than the parent's launch by more than the
parent's own spread at any seq_kv measured.  Everything else is a first measurement, not a bar.  Run each invocation under
its own `timeout`; for a per-kernel breakdown of one step run `--only token --pos P --no-forward` under a profiler.
"""
import argparse
import ctypes
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
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="launch,token")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libqgemm.so (the replaced launches)")
    ap.add_argument("--seq-kv", type=int, nargs="*", default=[128, 512, 516, 2048, 4096])
    ap.add_argument("--pos", type=int, nargs="*", default=[0, 511, 2047, 4095])
    ap.add_argument("--no-forward", action="store_true", help="token: time the step alone")
    args = ap.parse_args()

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    stream = qg._stream(dev)

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / calls  # us per call

    def measure(variants, calls):
        """variants: {name: fn}, calls: {name: calls per round}"""
        for v, fn in variants.items():
            for _ in range(min(args.warmup, calls[v])):
                fn()
        torch.cuda.synchronize()
        res = {v: [] for v in variants}
        for r in range(args.rounds):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for v in order:
                res[v].append(timed(variants[v], calls[v]))
        out = {}
        for v, t in res.items():
            t = sorted(t)
            out[v] = {"us": round(t[len(t) // 2], 2), "spread_us": round(t[-1] - t[0], 2)}
        return out

    status = 0
    if "launch" in args.only:
        P = None
        if args.parent_lib:
            P = ctypes.CDLL(os.path.abspath(args.parent_lib))
            for name in ("qgemm_attention_causal", "qgemm_attention_workspace_size"):
                getattr(P, name).argtypes = getattr(L, name).argtypes
                getattr(P, name).restype = getattr(L, name).restype
            same_kernel = hasattr(P, "qgemm_attention_plan")   # the parent has the decode kernel too
        H, dk = 16, 64
        d = H * dk
        scale = 0.125
        for seq_kv in args.seq_kv:
            K = qg.fill_uniform(torch.empty((seq_kv, d), device=dev), seed=3001)
            V = qg.fill_uniform(torch.empty((seq_kv, d), device=dev), seed=3002)
            for seq_q in (1, 8):
                assert qg.attention_plan(seq_q, seq_kv, H, dk).startswith("attention_decode")
                Q = qg.fill_uniform(torch.empty((seq_q, d), device=dev), seed=3000)
                O, Op = torch.empty_like(Q), torch.empty_like(Q)
                need = L.qgemm_attention_workspace_size(seq_q, seq_kv, H, dk)
                ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
                wsp = ws.data_ptr() if need else None
                q_pos0 = seq_kv - seq_q

                def call(lib, out):
                    assert lib.qgemm_attention_causal(Q.data_ptr(), d, K.data_ptr(), d, V.data_ptr(), d, out.data_ptr(),
                                                      d, seq_q, seq_kv, H, dk, scale, q_pos0, wsp, need, stream) == 0

                variants = {"decode": lambda: call(L, O)}
                replaced = "fused" if need == 0 else "three_launches"
                if P is not None and same_kernel:
                    replaced = "parent_decode"
                if P is not None:
                    assert P.qgemm_attention_workspace_size(seq_q, seq_kv, H, dk) == need
                    variants[replaced] = lambda: call(P, Op)
                    call(L, O)
                    call(P, Op)
                    assert torch.equal(O.view(torch.int32), Op.view(torch.int32)), "decode and replaced launch differ"
                out = measure(variants, {v: args.calls for v in variants})
                rec = {"what": "attention launch", "seq_q": seq_q, "seq_kv": seq_kv, "n_heads": H, "d_k": dk,
                       "q_pos0": q_pos0, "calls": args.calls, "rounds": args.rounds, **out}
                if P is not None:
                    rec["decode_over_replaced"] = round(out["decode"]["us"] / out[replaced]["us"], 3)
                    if seq_kv == 512 or same_kernel:
                        rec["check_1_passes"] = out["decode"]["us"] <= out[replaced]["us"] + out[replaced]["spread_us"]
                        if not rec["check_1_passes"]:
                            status = 1
                print(json.dumps(rec), flush=True)

    if "token" in args.only:
        d, H, dff, blocks, enc_seq, max_seq = 1024, 16, 4096, 2, 512, 4096
        X = qg.fill_uniform(torch.empty((max_seq, d), device=dev), seed=2000)
        E = qg.fill_uniform(torch.empty((enc_seq, d), device=dev), seed=2001)
        Y = torch.empty_like(X)
        y1 = torch.empty((1, d), device=dev)
        dec = qg.Decoder(d, H, dff, blocks, max_seq=max_seq, max_enc_seq=enc_seq, seed=1000, causal=True, kv_cache=True)
        dec.begin(E)
        dec.step(X[:max_seq - 1], Y=Y[:max_seq - 1])   # the caches hold the whole sequence: any pos below is a rewind
        for pos in sorted(args.pos, reverse=True):
            rows = pos + 1
            variants = {"step": lambda: dec.step(X[pos:rows], pos=pos, Y=y1)}
            calls = {"step": args.calls}
            if not args.no_forward:
                variants["forward"] = lambda: dec.forward(X[:rows], E, Y[:rows])
                calls["forward"] = max(2, min(args.calls, 20000 // rows))
                dec.forward(X[:rows], E, Y[:rows])
                dec.step(X[pos:rows], pos=pos, Y=y1)
                assert torch.equal(y1.view(torch.int32), Y[pos:rows].view(torch.int32)), "step and forward differ"
            out = measure(variants, calls)
            rec = {"what": "decoder token", "pos": pos, "enc_seq": enc_seq, "d_model": d, "n_heads": H, "d_ff": dff,
                   "n_blocks": blocks, "calls": calls, "rounds": args.rounds, **out}
            if "forward" in out:
                rec["forward_over_step"] = round(out["forward"]["us"] / out["step"]["us"], 1)
            print(json.dumps(rec), flush=True)
        dec.close()
    return status


if __name__ == "__main__":
    sys.exit(main())
