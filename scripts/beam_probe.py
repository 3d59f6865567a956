#!/usr/bin/env python3
"""First measurements of beam search.  (diagnostic, GPU box)

  choice   : qgemm_logsumexp_rows and qgemm_beam_step (beams 4 and 8) on 16 x 32768 and 32 x 32768 fp32 logits, beside
             qgemm_argmax_rows and qgemm_sample_rows(top_k = beams) on the same tensors, all between device events;
  gather   : qgemm_decoder_gather_slots of 16 destinations (4 groups x 4 beams, a permutation of parents) x 512 and x 2048
             cache rows at d_model 1024 and 2 blocks, as bytes moved (read + written) over time, beside 16
             qgemm_decoder_copy_slot calls on the same slots;
  generate : the shape of scripts/generate_probe.py (d_model 1024, 16 heads, d_ff 4096, 2 blocks, enc_seq 512,
             vocabulary 32768, a tied head with a position table, position 511): ONE qgemm_decoder_generate_beam call
             for (groups, beams) = (4, 4) and (4, 8), beside ONE qgemm_decoder_generate call on 16 and 32 slots.

Before timing, beam_step with beams = 1 must give the argmax's indices and generate_beam with beams = 1 generate's tokens.
One JSON line per measurement: the median of ROUNDS rounds with the round-to-round spread (max - min); the variants
alternate inside every round, in one process.  Everything here is a first measurement, not a bar.  --once VARIANT runs
one call of the generate section once without timing: the run to put under a kernel trace.

The measurements run in a child process under a time limit; after a child that fails or runs out of time nothing more is
started.
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

D, H, DFF, BLOCKS, ENC_SEQ, VOCAB, POS = 1024, 16, 4096, 2, 512, 32768, 511
SEED = 5


def _median_spread(t):
    t = sorted(t)
    return round(t[len(t) // 2], 2), round(t[-1] - t[0], 2)


def _rounds(variants, rounds, warmup, timed):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
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

    # ---- the token choice
    for rows in (16, 32) if "choice" in args.what else ():
        w = VOCAB
        S = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=3000 + rows, lo=-8.0, hi=8.0)
        sp = S.data_ptr()
        amax = torch.empty(rows, dtype=torch.int32, device=dev)
        idx = torch.empty(rows, dtype=torch.int32, device=dev)
        mx, logz = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        par, tok = torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev)
        sc_in, sc = torch.zeros(rows, device=dev), torch.empty(rows, device=dev)
        a_need = L.qgemm_argmax_rows_workspace_size(rows, w)
        a_ws = torch.empty(max(a_need, 16), dtype=torch.uint8, device=dev)
        l_need = L.qgemm_logsumexp_rows_workspace_size(rows, w)
        l_ws = torch.empty(max(l_need, 16), dtype=torch.uint8, device=dev)

        def argmax():
            assert L.qgemm_argmax_rows(sp, w, rows, w, amax.data_ptr(), None, a_ws.data_ptr(), a_need, st) == 0

        def logsumexp():
            assert L.qgemm_logsumexp_rows(sp, w, rows, w, mx.data_ptr(), logz.data_ptr(), l_ws.data_ptr(), l_need, st) == 0

        def beam_step(beams):
            need = L.qgemm_beam_step_workspace_size(rows // beams, beams, w)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

            def call():
                assert L.qgemm_beam_step(sp, w, rows // beams, beams, w, sc_in.data_ptr(), None, -1, par.data_ptr(),
                                         tok.data_ptr(), sc.data_ptr(), ws.data_ptr(), need, st) == 0
            return call

        def sample(top_k):
            need = L.qgemm_sample_rows_workspace_size(rows, w, top_k)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

            def call():
                assert L.qgemm_sample_rows(sp, w, rows, w, top_k, 1.0, 1.0, SEED, 0, None, None, -1, idx.data_ptr(),
                                           None, None, None, ws.data_ptr(), need, st) == 0
            return call

        argmax()
        beam_step(1)()
        torch.cuda.synchronize()
        assert torch.equal(tok, amax), "beams = 1 is the argmax"
        variants = {"qgemm_argmax_rows": argmax, "qgemm_logsumexp_rows": logsumexp}
        for beams in (4, 8):
            variants[f"qgemm_beam_step_beams_{beams}"] = beam_step(beams)
            variants[f"qgemm_sample_rows_top_k_{beams}"] = sample(beams)
        res = _rounds(variants, args.rounds, args.warmup, lambda fn: timed(fn, args.calls))
        rec = {"what": "choice", "rows": rows, "w": w, "bytes": 4 * rows * w, "lse_parts": qg.logsumexp_rows_plan(rows, w),
               "beam_plan_4": qg.beam_step_plan(rows // 4, 4, w), "beam_plan_8": qg.beam_step_plan(rows // 8, 8, w),
               "calls": args.calls, "rounds": args.rounds}
        for v, t in res.items():
            us, spread = _median_spread(t)
            rec[v] = {"us": us, "spread_us": spread}
        print(json.dumps(rec), flush=True)
        del S

    # ---- the cache gather
    for n_rows in (512, 2048) if "gather" in args.what else ():
        groups, beams = 4, 4
        rows = groups * beams
        dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=n_rows, max_enc_seq=8, seed=1000, causal=True, kv_cache=True,
                         n_slots=2 * rows)
        enc = qg.fill_uniform(torch.empty((8, D), device=dev), seed=2001)
        X = qg.fill_uniform(torch.empty((min(n_rows, 512), D), device=dev), seed=2000)
        dec.begin_slot(0, enc)
        for p0 in range(0, n_rows, 512):
            dec.step_slot(0, X, pos=p0)
        for b in range(1, 2 * rows):
            dec.copy_slot(b, 0)
        a, b = ints(list(range(rows))), ints(list(range(rows, 2 * rows)))
        parents = torch.tensor([(3 * i + 1) % beams for i in range(rows)], dtype=torch.int32, device=dev)
        n = ints([n_rows] * groups)

        def gather():
            assert L.qgemm_decoder_gather_slots(dec._h, groups, beams, b, a, parents.data_ptr(), n, st) == 0

        def copies():
            for i in range(rows):
                assert L.qgemm_decoder_copy_slot(dec._h, rows + i, i // beams * beams + (3 * i + 1) % beams, st) == 0

        res = _rounds({"gather_slots": gather, "copy_slot_x16": copies}, args.rounds, args.warmup,
                      lambda fn: timed(fn, max(1, args.calls // 10)))
        moved = 2 * BLOCKS * rows * n_rows * 2 * D * 4        # read + written, [K | V] of every row, every block
        rec = {"what": "gather", "destinations": rows, "cache_rows": n_rows, "d_model": D, "n_blocks": BLOCKS,
               "gather_bytes_read_and_written": moved, "copy_slot_bytes_read_and_written": moved // 2 * 3 +
               2 * BLOCKS * rows * 8 * 2 * D * 4, "rounds": args.rounds}
        for v, t in res.items():
            us, spread = _median_spread(t)
            rec[v] = {"us": us, "spread_us": spread}
        rec["gather_slots"]["TB_per_s"] = round(moved / rec["gather_slots"]["us"] * 1e-6, 3)
        print(json.dumps(rec), flush=True)
        dec.close()

    if "generate" not in args.what:
        return 0
    # ---- a generate_beam step
    n_new, max_seq = args.tokens, POS + args.tokens
    dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=max_seq, max_enc_seq=ENC_SEQ, seed=1000, causal=True, kv_cache=True,
                     n_slots=64)
    E = qg.fill_uniform(torch.empty((VOCAB, D), device=dev), seed=2003)
    P = qg.fill_uniform(torch.empty((max_seq, D), device=dev), seed=2004, lo=-0.1, hi=0.1)
    head = qg.Head(qg.pack_b(E.t()), VOCAB, None, E, P, max_rows=32)
    enc = qg.fill_uniform(torch.empty((ENC_SEQ, D), device=dev), seed=2001)
    X = qg.fill_uniform(torch.empty((POS, D), device=dev), seed=2000)
    dec.begin_slot(0, enc)
    dec.step_slot(0, X)
    for b in range(1, 64):
        dec.copy_slot(b, 0)
    torch.cuda.synchronize()

    def greedy_call(n):
        cs, at = ints(list(range(n))), ints([POS] * n)
        tok_in = (torch.arange(n, device=dev, dtype=torch.int32) * 37) % VOCAB
        out = torch.empty((n_new, n), dtype=torch.int32, device=dev)

        def call():
            assert L.qgemm_decoder_generate(dec._h, head._h, n, cs, tok_in.data_ptr(), n_new, at, out.data_ptr(), st) == 0
        return call, out, tok_in

    def beam_call(groups, beams):
        rows = groups * beams
        a, b, at = ints(list(range(rows))), ints(list(range(32, 32 + rows))), ints([POS] * groups)
        tok_in = ((torch.arange(groups, device=dev, dtype=torch.int32) * 37) % VOCAB).repeat_interleave(beams).contiguous()
        outs = (torch.empty((n_new, rows), dtype=torch.int32, device=dev),
                torch.empty((n_new, rows), dtype=torch.int32, device=dev), torch.empty((n_new, rows), device=dev))

        def call():
            assert L.qgemm_decoder_generate_beam(dec._h, head._h, groups, beams, a, b, tok_in.data_ptr(), n_new, at, None,
                                                 -1, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), st) == 0
        return call, outs

    variants = {"generate_16_slots": greedy_call(16)[0], "generate_32_slots": greedy_call(32)[0],
                "generate_beam_4x4": beam_call(4, 4)[0], "generate_beam_4x8": beam_call(4, 8)[0]}
    if args.once:
        variants[args.once]()
        torch.cuda.synchronize()
        print(json.dumps({"what": "generate", "once": args.once, "tokens": n_new}), flush=True)
        head.close()
        dec.close()
        return 0
    g4, g4_out, _ = greedy_call(4)
    b1, b1_out = beam_call(4, 1)
    g4()
    b1()
    torch.cuda.synchronize()
    assert torch.equal(b1_out[0], g4_out), "generate_beam with beams = 1 and generate differ"
    res = _rounds(variants, args.rounds, 2, lambda fn: timed(fn, 1))
    rec = {"what": "generate", "tokens": n_new, "pos": POS, "vocab": VOCAB, "d_model": D, "n_heads": H, "d_ff": DFF,
           "n_blocks": BLOCKS, "enc_seq": ENC_SEQ, "rounds": args.rounds}
    for v, t in res.items():
        us, spread = _median_spread(t)
        rec[v] = {"us_per_step": round(us / n_new, 2), "spread_us_per_step": round(spread / n_new, 2)}
    print(json.dumps(rec), flush=True)
    head.close()
    dec.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="*", default=["choice", "gather", "generate"], choices=["choice", "gather", "generate"])
    ap.add_argument("--calls", type=int, default=100, help="launches per timed round of the choice section")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=16, help="tokens generated per call")
    ap.add_argument("--once", default=None, metavar="VARIANT",
                    help="run one call of the generate section once, untimed, and stop (for a kernel trace): "
                         "generate_16_slots, generate_32_slots, generate_beam_4x4 or generate_beam_4x8")
    ap.add_argument("--limit", type=int, default=300, help="seconds for the child process")
    ap.add_argument("--child", action="store_true", help="measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", *args.what, "--calls", str(args.calls),
           "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--tokens", str(args.tokens)]
    if args.once:
        cmd += ["--once", args.once]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"what": "beam probe", "error": f"no result within {args.limit} s"}), flush=True)
        return 2
    if rc != 0:
        print(json.dumps({"what": "beam probe", "error": f"child exit status {rc}"}), flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
