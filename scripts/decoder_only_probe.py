#!/usr/bin/env python3
"""First measurements of decoder-only stacks and rotary embeddings, by scripts/beam_indirect_probe.py's
method.  (diagnostic, GPU box)

  rope  : qgemm_rope_rows on 16 and on 512 rows x 32 groups x d_k 64 (the Q and K thirds of d_model 1024 with 16 heads,
          at the stack's stride 3 d_model), on the float4 path and, with the stride one float longer, on the pair path;
  stack : d_model 1024, 16 heads, d_ff 4096, 2 pre-LN blocks with the final norm, max_seq 2048, 16 cache slots: ONE
          step_batch of 16 slots at position 2047 and ONE forward of 512 rows, on three models -- decoder-only without
          RoPE, decoder-only with RoPE, and the decoder with cross-attention at enc_seq 512.

One JSON line per measurement: the median of ROUNDS rounds with the round-to-round spread (max - min); the variants
alternate inside every round, in one process.  The measurements run in a child process under a time limit; after a
child that fails or runs out of time nothing more is started.
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

D, H, DFF, BLOCKS, MAX_SEQ, ENC_SEQ, SLOTS = 1024, 16, 4096, 2, 2048, 512, 16


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
    L = qg.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    st = qg._stream(dev)
    ints = lambda v: (ctypes.c_int * len(v))(*v)

    def timed(fn, calls):
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

    # ---- the row kernel
    if "rope" in args.what:
        dk, groups = D // H, 2 * H
        import rope_oracle as RO
        cos, sin = (torch.from_numpy(t).to(dev) for t in RO.make_tables(MAX_SEQ, dk))
        variants = {}
        for rows in (16, 512):
            for path, stride in (("float4", 3 * D), ("pairs", 3 * D + 1)):
                X = qg.fill_uniform(torch.empty((rows, stride), device=dev), seed=10 + rows)

                def call(X=X, rows=rows, stride=stride):
                    assert L.qgemm_rope_rows(X.data_ptr(), stride, rows, groups, dk, cos.data_ptr(), sin.data_ptr(),
                                             MAX_SEQ, MAX_SEQ - rows, st) == 0
                variants[f"rope_rows_{rows}_{path}"] = call
        res = _rounds(variants, args.rounds, args.warmup, lambda fn: timed(fn, args.calls))
        report({"what": "rope", "groups": groups, "d_k": dk, "calls": args.calls, "rounds": args.rounds,
                "bytes_moved_512_rows": 2 * 512 * groups * dk * 4}, res)

    if "stack" not in args.what:
        return 0
    # ---- the stack: three models, the same sizes and seed
    mk = dict(seed=1000, causal=True, kv_cache=True, n_slots=SLOTS, arch="standard", norm_first=True, final_norm=True)
    models = {"decoder_only": qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, 0, decoder_only=True, **mk),
              "decoder_only_rope": qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, 0, decoder_only=True, rope=True, **mk),
              "cross_decoder": qg.Decoder(D, H, DFF, BLOCKS, MAX_SEQ, ENC_SEQ, **mk)}
    enc = qg.fill_uniform(torch.empty((ENC_SEQ, D), device=dev), seed=2001)
    X = qg.fill_uniform(torch.empty((512, D), device=dev), seed=2000)
    new = qg.fill_uniform(torch.empty((SLOTS, D), device=dev), seed=2002)
    Y, Ys = torch.empty_like(X), torch.empty_like(new)
    slots, pos = ints(list(range(SLOTS))), ints([MAX_SEQ - 1] * SLOTS)
    steps, forwards = {}, {}
    for name, m in models.items():
        e = enc if name == "cross_decoder" else None
        m.begin_slot(0, e)
        for p0 in range(0, MAX_SEQ - 1, 512):
            m.step_slot(0, X[:min(512, MAX_SEQ - 1 - p0)], pos=p0)
        for b in range(1, SLOTS):
            m.copy_slot(b, 0)
        eptr, erows = (enc.data_ptr(), ENC_SEQ) if e is not None else (None, 0)

        def step(m=m):
            assert L.qgemm_decoder_step_batch(m._h, SLOTS, slots, pos, 1, new.data_ptr(), Ys.data_ptr(), st) == 0

        def forward(m=m, eptr=eptr, erows=erows):
            assert L.qgemm_decoder_forward(m._h, X.data_ptr(), eptr, Y.data_ptr(), 512, erows, st) == 0
        steps["step_batch_" + name], forwards["forward_" + name] = step, forward
    torch.cuda.synchronize()
    rec = {"d_model": D, "n_heads": H, "d_ff": DFF, "n_blocks": BLOCKS, "arch": "pre-LN + final norm", "enc_seq": ENC_SEQ,
           "rounds": args.rounds}
    res = _rounds(steps, args.rounds, args.warmup, lambda fn: timed(fn, args.step_calls))
    report(dict(rec, what="step_batch", slots=SLOTS, pos=MAX_SEQ - 1, calls=args.step_calls), res)
    res = _rounds(forwards, args.rounds, args.warmup, lambda fn: timed(fn, args.step_calls))
    report(dict(rec, what="forward", rows=512, calls=args.step_calls), res)
    for m in models.values():
        m.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="*", default=["rope", "stack"], choices=["rope", "stack"])
    ap.add_argument("--calls", type=int, default=100, help="launches per timed round of the rope section")
    ap.add_argument("--step-calls", type=int, default=10, help="calls per timed round of the stack section")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds for the child process")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "decoder_only_probe.log"),
                    help="the file that keeps the measurements' JSON lines")
    ap.add_argument("--child", action="store_true", help="measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", *args.what, "--calls", str(args.calls),
           "--step-calls", str(args.step_calls), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    try:
        done = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as e:
        part = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        sys.stdout.write(part)
        print(json.dumps({"what": "decoder-only probe", "error": f"no result within {args.limit} s"}), flush=True)
        return 2
    rc = done.returncode
    sys.stdout.write(done.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:                 # the child's lines, whole or up to its failure
        f.write(done.stdout)
    if rc != 0:
        print(json.dumps({"what": "decoder-only probe", "error": f"child exit status {rc}"}), flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
