#!/usr/bin/env python3
"""First measurements of the batched variable-length forward.  (diagnostic, GPU box)

Four comparisons, each `one call on many sequences` against `the same sequences one call each`, the only way a library
without the feature serves them:

  launch          qgemm_attention_varlen on 16 sequences x 512 queries x 512 keys, 16 heads x d_k 64, against 16
                  qgemm_attention calls (16 fused launches);
  launch_mixed    the same on 16 sequences of mixed lengths between 64 and 512;
  forward         Encoder.forward_batch of 16 x 512 rows at d_model 1024, 16 heads, d_ff 4096, 2 blocks against 16
                  forward calls;
  prefill         Decoder.step_varlen prefilling 16 slots x 128 rows against 16 step_slot calls;

and two checks:

  check1          forward_batch of ONE 512-row sequence is not slower than forward by more than forward's own
                  round-to-round spread in the same run;
  check2          bench.py --gpus 1 --config c5_encoder of this tree and of a parent tree built beside it
                  (--parent DIR), alternated in one call, three runs each: every run of this tree lies inside or above
                  the parent's own range (that range is the margin).  Skipped without --parent.

Before timing, the rows of the one call must equal the rows of the separate calls bit for bit.  One JSON line per
comparison: the median of ROUNDS rounds of CALLS back-to-back calls between two device events, with the round-to-round
spread (max - min), in us per call; the two variants alternate inside every round, in one process.  Everything goes
through the C-ABI with arguments built beforehand, so the host work per call is the library's own.

Each comparison is measured in a child process of its own under a time limit; after a child that fails or runs out of
time nothing more is started.  Exit status 1 when a check fails.  Everything else is a first measurement, not a bar.
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

D, H, DFF, BLOCKS = 1024, 16, 4096, 2
DK = D // H
MIXED = (64, 512, 96, 448, 128, 384, 160, 352, 192, 320, 224, 288, 256, 100, 500, 65)
WHATS = ("launch", "launch_mixed", "forward", "prefill", "check1")


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _longs(v):
    return (ctypes.c_int64 * len(v))(*v)


def _prefix(v):
    out, at = [], 0
    for n in v:
        out.append(at)
        at += n
    return out


def measure(variants, args):
    import torch

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.calls  # us per call

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    res = {v: [] for v in variants}
    for r in range(args.rounds):
        for v in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
            res[v].append(timed(variants[v]))
    out = {}
    for v, t in res.items():
        t = sorted(t)
        out[v] = {"us": round(t[len(t) // 2], 2), "spread_us": round(t[-1] - t[0], 2)}
    return out


def child(args):
    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    st = qg._stream(dev)
    what = args.what
    rec = {"what": what, "d_model": D, "n_heads": H, "calls": args.calls, "rounds": args.rounds}
    status = 0

    def same(a, b):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: one call and separate calls differ"
        assert bool(torch.isfinite(a).all())

    if what in ("launch", "launch_mixed"):
        lens = [512] * 16 if what == "launch" else list(MIXED)
        n, rows, row0 = len(lens), sum(lens), _prefix(lens)
        assert qg.attention_varlen_plan(lens, lens, H, DK) == "attention_fused_kernel<many>"
        qkv = qg.fill_uniform(torch.empty((rows, 3 * D), device=dev), seed=3000)
        Q, K, V = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        Om, Os = (torch.full((rows, D), float("nan"), device=dev) for _ in range(2))
        scale = ctypes.c_float(DK ** -0.5).value
        a_len, a_row0 = _ints(lens), _longs(row0)
        ld = 3 * D

        def many():
            assert L.qgemm_attention_varlen(Q.data_ptr(), ld, K.data_ptr(), ld, V.data_ptr(), ld, Om.data_ptr(), D, n,
                                            a_row0, a_len, a_row0, a_len, None, H, DK, scale, None, 0, st) == 0

        def singles():
            for b in range(n):
                o = row0[b] * 4
                assert L.qgemm_attention(Q.data_ptr() + o * ld, ld, K.data_ptr() + o * ld, ld, V.data_ptr() + o * ld, ld,
                                         Os.data_ptr() + o * D, D, lens[b], lens[b], H, DK, scale, None, 0, st) == 0

        many()
        singles()
        torch.cuda.synchronize()
        same(Om, Os)
        rec.update(seq_lens=lens, d_k=DK, **measure({"many": many, "singles": singles}, args))
    elif what in ("forward", "check1"):
        lens = [512] * (16 if what == "forward" else 1)
        n, rows, row0 = len(lens), sum(lens), _prefix(lens)
        enc = qg.Encoder(D, H, DFF, BLOCKS, max_seq=512, seed=1000, max_rows=rows)
        X = qg.fill_uniform(torch.empty((rows, D), device=dev), seed=3001)
        Ym, Ys = (torch.full((rows, D), float("nan"), device=dev) for _ in range(2))
        a_len = _ints(lens)

        def many():
            assert L.qgemm_encoder_forward_batch(enc._h, X.data_ptr(), Ym.data_ptr(), n, a_len, st) == 0

        def singles():
            for b in range(n):
                o = row0[b] * D * 4
                assert L.qgemm_encoder_forward(enc._h, X.data_ptr() + o, Ys.data_ptr() + o, lens[b], st) == 0

        many()
        singles()
        torch.cuda.synchronize()
        same(Ym, Ys)
        rec.update(seq_lens=lens, d_ff=DFF, n_blocks=BLOCKS, **measure({"many": many, "singles": singles}, args))
        if what == "check1":
            rec["check_passes"] = rec["many"]["us"] <= rec["singles"]["us"] + rec["singles"]["spread_us"]
            status = 0 if rec["check_passes"] else 1
        enc.close()
    elif what == "prefill":
        n, r, enc_seq = 16, 128, 512
        dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=r, max_enc_seq=enc_seq, seed=1000, causal=True, kv_cache=True,
                         n_slots=n, max_rows=n * r)
        E = qg.fill_uniform(torch.empty((enc_seq, D), device=dev), seed=3002)
        X = qg.fill_uniform(torch.empty((n * r, D), device=dev), seed=3003)
        Ym, Ys = (torch.full((n * r, D), float("nan"), device=dev) for _ in range(2))
        for b in range(n):
            dec.begin_slot(b, E)
        slots, zeros, a_rows = _ints(list(range(n))), _ints([0] * n), _ints([r] * n)

        def many():   # every call prefills from position 0 again: a rewind of every slot
            assert L.qgemm_decoder_step_varlen(dec._h, n, slots, zeros, a_rows, X.data_ptr(), Ym.data_ptr(), st) == 0

        def singles():
            for b in range(n):
                o = b * r * D * 4
                assert L.qgemm_decoder_step_slot(dec._h, b, X.data_ptr() + o, Ys.data_ptr() + o, 0, r, st) == 0

        many()
        singles()
        torch.cuda.synchronize()
        same(Ym, Ys)
        rec.update(n_slots=n, rows_per_slot=r, enc_seq=enc_seq, d_ff=DFF, n_blocks=BLOCKS,
                   **measure({"many": many, "singles": singles}, args))
        dec.close()
    else:
        raise SystemExit(f"unknown comparison {what}")
    rec["singles_over_many"] = round(rec["singles"]["us"] / rec["many"]["us"], 3)
    print(json.dumps(rec), flush=True)
    return status


def bench_value(tree, limit):
    """One bench.py run of `tree`: the value of its JSON result line (forwards/s), or None."""
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--config", "c5_encoder"]
    out = subprocess.run(cmd, timeout=limit, capture_output=True, text=True, cwd=tree)
    if out.returncode:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
        return None
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{") and '"value"' in line:
            return float(json.loads(line)["value"])
    return None


def check2(args):
    trees = {"parent": os.path.abspath(args.parent), "branch": REPO}
    runs = {k: [] for k in trees}
    for i in range(3):
        for k in (list(trees) if i % 2 == 0 else list(trees)[::-1]):
            try:
                v = bench_value(trees[k], args.limit)
            except subprocess.TimeoutExpired:
                v = None
            if v is None:   # a failed run: start nothing more on the GPU
                print(json.dumps({"what": "check2", "error": f"bench.py of the {k} tree gave no result"}), flush=True)
                return 2
            runs[k].append(v)
    lo, hi = min(runs["parent"]), max(runs["parent"])
    ok = all(v >= lo for v in runs["branch"])
    print(json.dumps({"what": "check2", "config": "c5_encoder", "unit": "forwards/s", "parent": runs["parent"],
                      "branch": runs["branch"], "parent_range": [lo, hi], "check_passes": ok}), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--what", nargs="*", default=list(WHATS), help=f"comparisons to run, of {WHATS}")
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: runs check2 against it")
    ap.add_argument("--limit", type=int, default=180, help="seconds for one child process or one bench.py run")
    ap.add_argument("--child", action="store_true", help="measure --what (one comparison) in this process")
    args = ap.parse_args()
    if args.child:
        args.what = args.what[0]
        return child(args)
    status = 0
    for what in args.what:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", what, "--calls", str(args.calls),
               "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"what": what, "error": f"no result within {args.limit} s"}), flush=True)
            return 2
        if rc not in (0, 1):   # a failed child: start nothing more on the GPU
            print(json.dumps({"what": what, "error": f"child exit status {rc}"}), flush=True)
            return 2
        status = max(status, rc)
    if args.parent:
        rc = check2(args)
        if rc == 2:
            return 2
        status = max(status, rc)
    return status


if __name__ == "__main__":
    sys.exit(main())
