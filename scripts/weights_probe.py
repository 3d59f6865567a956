#!/usr/bin/env python3
"""First measurements of caller-supplied weights.  (diagnostic, GPU box)

  load   : every tensor of a decoder of d_model 1024, 16 heads, d_ff 4096, 2 blocks through set_weight, once from fp32
           [in, out] sources and once from bf16 [out, in] sources (the sources already on the device), beside the route
           the library offered before for the same packed bytes: widen and assemble each fused weight with torch, then
           one pack_b per fused weight (which leaves the result in a buffer of its own, not in the stack);
  kernel : one qgemm_pack_b_window launch per source path (fp32 and bf16) on one head's tensor (1024 x 64), W1
           (1024 x 4096) and W2 (4096 x 1024), beside pack_b of the same matrix.

Before timing, the window route's scale and q bytes must equal pack_b's.  One JSON line per measurement: the median of
ROUNDS rounds with the round-to-round spread (max - min); the variants alternate inside every round, in one process.
The measurements run in a child process under a time limit; after a child that fails or runs out of time nothing more
is started.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

D, H, DFF, BLOCKS = 1024, 16, 4096, 2
HEAD_KINDS = (0, 1, 2, 8, 9, 10)
FUSED = ((0, 1, 2), (3,), (4,), (6,), (8,), (9, 10), (11,))   # the kinds of wqkv, wo, w1, w2, wq2, wkv2, wo2


def _median_spread(t):
    t = sorted(t)
    return round(t[len(t) // 2], 2), round(t[-1] - t[0], 2)


def _rounds(variants, rounds, warmup, timed):
    for fn in variants.values():
        for _ in range(warmup):
            timed(fn)
    res = {v: [] for v in variants}
    for r in range(rounds):
        for v in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
            res[v].append(timed(variants[v]))
    return res


def child(args):
    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)

    def timed(fn, calls=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / calls  # us per call

    def report(rec, res):
        for v, t in res.items():
            us, spread = _median_spread(t)
            rec[v] = {"us": us, "spread_us": spread}
        print(json.dumps(rec), flush=True)

    def same(p, r):
        torch.cuda.synchronize()
        return torch.equal(p.scale.view(torch.int32), r.scale.view(torch.int32)) and torch.equal(p.q_raw, r.q_raw)

    def draw(shape, seed):   # values exact in bf16, so both source types hold the same weights
        return qg.fill_uniform(torch.empty(shape, device=dev), seed=seed).to(torch.bfloat16).to(torch.float32)

    if "load" in args.what:
        dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=16, max_enc_seq=16, seed=1)
        kn, nk = {}, {}
        for i in range(BLOCKS):
            for kind in range(12):
                r, c, heads = dec.weight_shape(kind)
                w = draw((heads, r, c) if heads > 1 else (r, c), 100 * i + kind)
                w = w.reshape(-1) if kind in (5, 7) else w
                kn[i, kind] = w
                nk[i, kind] = (w if w.dim() == 1 else w.transpose(-1, -2).contiguous()).to(torch.bfloat16)

        def fused_kn(i, kinds):   # [in, out] fp32 tensors side by side
            return torch.cat([kn[i, k][h] if k in HEAD_KINDS else kn[i, k] for k in kinds
                              for h in (range(H) if k in HEAD_KINDS else (0,))], dim=1)

        def fused_nk(i, kinds):   # [out, in] bf16 tensors stacked, widened; pack_b takes the transposed view
            return torch.cat([nk[i, k][h] if k in HEAD_KINDS else nk[i, k] for k in kinds
                              for h in (range(H) if k in HEAD_KINDS else (0,))], dim=0).to(torch.float32).t()

        def set_weight_f32_kn():
            dec.load_weights(kn)

        def set_weight_bf16_nk():
            dec.load_weights(nk, layout="nk")

        def torch_assemble_pack_b_f32_kn():
            return [qg.pack_b(fused_kn(i, kinds)) for i in range(BLOCKS) for kinds in FUSED]

        def torch_widen_assemble_pack_b_bf16_nk():
            return [qg.pack_b(fused_nk(i, kinds)) for i in range(BLOCKS) for kinds in FUSED]

        want = torch_assemble_pack_b_f32_kn()
        for load in (set_weight_f32_kn, set_weight_bf16_nk):
            dec.load_weights({key: torch.zeros_like(w) for key, w in kn.items()})
            load()
            got = [dec.packed_weight(i, which) for i in range(BLOCKS) for which in range(7)]
            assert all(same(p, r) for p, r in zip(got, want)), f"{load.__name__}: packed bytes differ from pack_b's"
        assert all(same(p, r) for p, r in zip(torch_widen_assemble_pack_b_bf16_nk(), want))
        variants = {f.__name__: f for f in (set_weight_f32_kn, torch_assemble_pack_b_f32_kn, set_weight_bf16_nk,
                                            torch_widen_assemble_pack_b_bf16_nk)}
        res = _rounds(variants, args.rounds, args.warmup, timed)
        report({"what": "load", "model": "decoder", "d_model": D, "n_heads": H, "d_ff": DFF, "n_blocks": BLOCKS,
                "tensors": len(kn), "set_weight_launches": BLOCKS * (6 * H + 6), "rounds": args.rounds}, res)
        dec.close()
        del kn, nk, want, got

    for name, k, n in (("head", D, D // H), ("w1", D, DFF), ("w2", DFF, D)) if "kernel" in args.what else ():
        W = draw((k, n), 7)
        base = qg.pack_b(draw((k, n), 8))
        big = torch.zeros((2 * k, 2 * n), device=dev)
        big[::2, ::2] = W
        src = {"f32_n_contiguous": (W, "kn"), "bf16_n_contiguous": (W.to(torch.bfloat16), "kn"),
               "f32_k_contiguous": (W.t().contiguous(), "nk"), "bf16_k_contiguous": (W.t().contiguous().to(torch.bfloat16), "nk"),
               "f32_generic": (big[::2, ::2], "kn")}
        want = qg.pack_b(W)
        variants = {"pack_b_f32_row_major": lambda: qg.pack_b(W)}
        for v, (B, layout) in src.items():
            assert v.split("_", 1)[1].replace("_", "-") in qg.pack_b_window_plan(B, base, 0, layout=layout)
            qg.pack_b_window(B, base, 0, layout=layout)
            assert same(base, want), f"{name} {v}: packed bytes differ from pack_b's"
            variants["pack_b_window_" + v] = lambda B=B, layout=layout: qg.pack_b_window(B, base, 0, layout=layout)
        res = _rounds(variants, args.rounds, args.warmup, lambda fn: timed(fn, args.calls))
        report({"what": "kernel", "tensor": name, "k": k, "n": n, "workgroups": (n + 15) // 16, "calls": args.calls,
                "rounds": args.rounds}, res)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="*", default=["load", "kernel"], choices=["load", "kernel"])
    ap.add_argument("--calls", type=int, default=20, help="launches per timed round of the kernel section")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds for the child process")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "weights_probe.log"),
                    help="the file that keeps the measurements' JSON lines")
    ap.add_argument("--child", action="store_true", help="measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", *args.what, "--calls", str(args.calls),
           "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    try:
        done = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as e:
        part = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        sys.stdout.write(part)
        print(json.dumps({"what": "weights probe", "error": f"no result within {args.limit} s"}), flush=True)
        return 2
    rc = done.returncode
    sys.stdout.write(done.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:                 # the child's lines, whole or up to its failure
        f.write(done.stdout)
    if rc != 0:
        print(json.dumps({"what": "weights probe", "error": f"child exit status {rc}"}), flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
