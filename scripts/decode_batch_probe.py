#!/usr/bin/env python3
"""First measurements of batched incremental decoding.  (diagnostic, GPU box)

d_model 1024, 16 heads, d_ff 4096, 2 blocks, enc_seq 512, one decoder with 64 cache slots; at positions 511 and 2047:

  batch   : ONE qgemm_decoder_step_batch that advances n = 1, 4, 16 and 64 sequences by one token each;
  singles : the same n tokens as n qgemm_decoder_step_slot calls back to back -- the only way a library without the
            batched step produces them, so this is the baseline.

Before timing, the rows of the batched step must equal the rows of the single steps bit for bit.  One JSON line per
(position, n): the median of ROUNDS rounds of CALLS back-to-back steps between two device events, with the
round-to-round spread (max - min), in us per step and per token; the two variants alternate inside every round, in one
process.  Both go through the C-ABI with arguments built beforehand, so the host work per call is the library's own.

Each position is measured in a child process of its own under a time limit; after a child that fails or runs out of
time nothing more is started.  Exit status 1 if, at 16 sequences, the batched step does not take less time than the 16
single steps by more than the single steps' own spread in that run.  Everything else is a first measurement, not a bar.
For a per-kernel breakdown run `--child --pos P --seqs N --calls 1 --rounds 1 --warmup 0` under a profiler, alone.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

D, H, DFF, BLOCKS, ENC_SEQ, SLOTS = 1024, 16, 4096, 2, 512, 64


def child(args):
    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    st = qg._stream(dev)
    pos = args.pos[0]
    max_seq = pos + 1

    dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=max_seq, max_enc_seq=ENC_SEQ, seed=1000, causal=True, kv_cache=True,
                     n_slots=SLOTS)
    E = qg.fill_uniform(torch.empty((ENC_SEQ, D), device=dev), seed=2001)
    X = qg.fill_uniform(torch.empty((max(pos, 1), D), device=dev), seed=2000)
    new = qg.fill_uniform(torch.empty((SLOTS, D), device=dev), seed=2002)   # every sequence its own new row
    Yb, Ys = torch.empty_like(new), torch.empty_like(new)
    # slot 0 holds pos rows; the other slots are forks of it (every step below is at `pos`: a rewind after the first)
    dec.begin_slot(0, E)
    if pos:
        dec.step_slot(0, X[:pos])
    for b in range(1, SLOTS):
        dec.copy_slot(b, 0)
    torch.cuda.synchronize()

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / calls  # us per step

    status = 0
    for n in args.seqs:
        slots = (ctypes.c_int * n)(*range(n))
        at = (ctypes.c_int * n)(*([pos] * n))
        xb, yb, ys = new.data_ptr(), Yb.data_ptr(), Ys.data_ptr()
        row = 4 * D

        def batch():
            assert L.qgemm_decoder_step_batch(dec._h, n, slots, at, 1, xb, yb, st) == 0

        def singles():
            for b in range(n):
                assert L.qgemm_decoder_step_slot(dec._h, b, xb + b * row, ys + b * row, pos, 1, st) == 0

        Yb.fill_(float("nan"))
        Ys.fill_(float("nan"))
        batch()
        singles()
        torch.cuda.synchronize()
        assert torch.equal(Yb[:n].view(torch.int32), Ys[:n].view(torch.int32)), "batched and single steps differ"
        assert bool(torch.isfinite(Yb[:n]).all())
        variants = {"batch": batch, "singles": singles}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        res = {v: [] for v in variants}
        for r in range(args.rounds):
            for v in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
                res[v].append(timed(variants[v], args.calls))
        rec = {"what": "decoder step", "pos": pos, "n_seqs": n, "enc_seq": ENC_SEQ, "d_model": D, "n_heads": H,
               "d_ff": DFF, "n_blocks": BLOCKS, "calls": args.calls, "rounds": args.rounds}
        for v, t in res.items():
            t = sorted(t)
            us, spread = t[len(t) // 2], t[-1] - t[0]
            rec[v] = {"us": round(us, 2), "spread_us": round(spread, 2), "us_per_token": round(us / n, 2)}
        rec["singles_over_batch"] = round(rec["singles"]["us"] / rec["batch"]["us"], 2)
        if n == 16:
            rec["check_passes"] = rec["batch"]["us"] < rec["singles"]["us"] - rec["singles"]["spread_us"]
            if not rec["check_passes"]:
                status = 1
        print(json.dumps(rec), flush=True)
    dec.close()
    return status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pos", type=int, nargs="*", default=[511, 2047])
    ap.add_argument("--seqs", type=int, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--limit", type=int, default=240, help="seconds for one position's child process")
    ap.add_argument("--child", action="store_true", help="measure --pos (one position) in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    status = 0
    for pos in args.pos:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pos", str(pos), "--calls", str(args.calls),
               "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--seqs", *map(str, args.seqs)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"what": "decoder step", "pos": pos, "error": f"no result within {args.limit} s"}), flush=True)
            return 2
        if rc not in (0, 1):   # a failed child: start nothing more on the GPU
            print(json.dumps({"what": "decoder step", "pos": pos, "error": f"child exit status {rc}"}), flush=True)
            return 2
        status = max(status, rc)
    return status


if __name__ == "__main__":
    sys.exit(main())
