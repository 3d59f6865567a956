#!/usr/bin/env python3
"""First measurements of the sampled token choice.  (diagnostic, GPU box)

  sample   : the qgemm_sample_rows call (top_p 0.9, temperature 0.8) on 64 x 32768 and on 1 x 131072 fp32 logits for
             top_k 50 and 1024, beside qgemm_argmax_rows on the same tensor, beside torch's topk + softmax +
             multinomial, and beside the vocabulary GEMM of the same step (qgemm_linear of rows x 1024 hidden rows onto
             the vocabulary), all between device events;
  generate : the shape of scripts/generate_probe.py (d_model 1024, 16 heads, d_ff 4096, 2 blocks, enc_seq 512,
             vocabulary 32768, a tied head with a position table); 16 and 64 cache slots at position 511 generate TOKENS
             tokens each with ONE qgemm_decoder_generate call and with ONE qgemm_decoder_generate_sampled call for
             top_k 50 and 1024.

Before timing, top_k = 1 must give the argmax's indices and generate_sampled with top_k = 1 must give generate's tokens.
One JSON line per measurement: the median of ROUNDS rounds with the round-to-round spread (max - min); the variants
alternate inside every round, in one process.  Everything here is a first measurement, not a bar.

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
TOP_P, TEMP, SEED = 0.9, 0.8, 5


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

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / calls  # us per call

    # ---- the sample call
    for rows, w in ((64, 32768), (1, 131072)) if "sample" in args.what else ():
        S = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=3000 + rows, lo=-8.0, hi=8.0)
        Wt = qg.fill_uniform(torch.empty((w, D), device=dev), seed=3100 + rows)
        pw = qg.pack_b(Wt.t())
        del Wt
        Hd = qg.fill_uniform(torch.empty((rows, D), device=dev), seed=3200 + rows)
        logits = torch.empty((rows, w), device=dev)
        idx = torch.empty(rows, dtype=torch.int32, device=dev)
        amax = torch.empty(rows, dtype=torch.int32, device=dev)
        a_need = L.qgemm_argmax_rows_workspace_size(rows, w)
        a_ws = torch.empty(max(a_need, 16), dtype=torch.uint8, device=dev)
        sp = S.data_ptr()

        def argmax():
            assert L.qgemm_argmax_rows(sp, w, rows, w, amax.data_ptr(), None, a_ws.data_ptr(), a_need, st) == 0

        argmax()
        for top_k in (50, 1024):
            need = L.qgemm_sample_rows_workspace_size(rows, w, top_k)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            count = [0]

            def sample(k=top_k):
                count[0] += 1
                assert L.qgemm_sample_rows(sp, w, rows, w, k, TOP_P, TEMP, SEED, count[0], None, None, -1,
                                           idx.data_ptr(), None, None, None, ws.data_ptr(), need, st) == 0

            def torch_sample():
                v, i = torch.topk(S, top_k, dim=1)
                return i.gather(1, torch.multinomial(torch.softmax(v / TEMP, dim=1), 1))

            sample(1)
            assert torch.equal(idx, amax), "top_k = 1 is the argmax"
            variants = {"qgemm_sample_rows": sample, "qgemm_argmax_rows": argmax, "torch_topk_softmax_multinomial":
                        torch_sample, "vocabulary_gemm": lambda: qg.linear(Hd, pw, Y=logits)}
            res = _rounds(variants, args.rounds, args.warmup, lambda fn: timed(fn, args.calls))
            rec = {"what": "sample", "rows": rows, "w": w, "top_k": top_k, "top_p": TOP_P, "temperature": TEMP,
                   "bytes": 4 * rows * w, "parts": qg.sample_rows_plan(rows, w, top_k), "calls": args.calls,
                   "rounds": args.rounds}
            for v, t in res.items():
                us, spread = _median_spread(t)
                rec[v] = {"us": us, "spread_us": spread}
            print(json.dumps(rec), flush=True)
        del pw, S, logits

    if "generate" not in args.what:
        return 0
    # ---- generation
    n_new, max_seq = args.tokens, POS + args.tokens
    slots_max = max(args.slots)
    dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=max_seq, max_enc_seq=ENC_SEQ, seed=1000, causal=True, kv_cache=True,
                     n_slots=slots_max)
    E = qg.fill_uniform(torch.empty((VOCAB, D), device=dev), seed=2003)
    P = qg.fill_uniform(torch.empty((max_seq, D), device=dev), seed=2004, lo=-0.1, hi=0.1)
    head = qg.Head(qg.pack_b(E.t()), VOCAB, None, E, P, max_rows=slots_max)
    enc = qg.fill_uniform(torch.empty((ENC_SEQ, D), device=dev), seed=2001)
    X = qg.fill_uniform(torch.empty((POS, D), device=dev), seed=2000)
    dec.begin_slot(0, enc)
    dec.step_slot(0, X)
    for b in range(1, slots_max):
        dec.copy_slot(b, 0)
    torch.cuda.synchronize()

    for n in args.slots:
        cs = (ctypes.c_int * n)(*range(n))
        at = (ctypes.c_int * n)(*([POS] * n))
        tok_in = (torch.arange(n, device=dev, dtype=torch.int32) * 37) % VOCAB
        out = torch.empty((n_new, n), dtype=torch.int32, device=dev)
        tp, op = tok_in.data_ptr(), out.data_ptr()

        def generate():
            assert L.qgemm_decoder_generate(dec._h, head._h, n, cs, tp, n_new, at, op, st) == 0

        def sampled(top_k):
            assert L.qgemm_decoder_generate_sampled(dec._h, head._h, n, cs, tp, n_new, at, top_k, TOP_P, TEMP, SEED,
                                                    None, -1, op, st) == 0

        generate()
        greedy = out.clone()
        sampled(1)
        torch.cuda.synchronize()
        assert torch.equal(out, greedy), "generate_sampled with top_k = 1 and generate differ"
        variants = {"generate": generate, "generate_sampled_top_k_50": lambda: sampled(50),
                    "generate_sampled_top_k_1024": lambda: sampled(1024)}
        res = _rounds(variants, args.rounds, 2, lambda fn: timed(fn, 1))
        sampled(50)
        rec = {"what": "generate", "n_slots": n, "tokens": n_new, "pos": POS, "vocab": VOCAB, "d_model": D, "n_heads": H,
               "d_ff": DFF, "n_blocks": BLOCKS, "enc_seq": ENC_SEQ, "rounds": args.rounds,
               "sampled_tokens_off_the_greedy_path": f"{int((out != greedy).sum())} of {n_new * n}"}
        for v, t in res.items():
            us, spread = _median_spread(t)
            rec[v] = {"us_per_step": round(us / n_new, 2), "spread_us_per_step": round(spread / n_new, 2),
                      "us_per_token": round(us / n_new / n, 2)}
        print(json.dumps(rec), flush=True)
    head.close()
    dec.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="*", default=["sample", "generate"], choices=["sample", "generate"])
    ap.add_argument("--calls", type=int, default=100, help="launches per timed round of the sample section")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=32, help="tokens generated per call")
    ap.add_argument("--slots", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--limit", type=int, default=300, help="seconds for the child process")
    ap.add_argument("--child", action="store_true", help="measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", *args.what, "--calls", str(args.calls),
           "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--tokens", str(args.tokens), "--slots",
           *map(str, args.slots)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"what": "sample probe", "error": f"no result within {args.limit} s"}), flush=True)
        return 2
    if rc != 0:
        print(json.dumps({"what": "sample probe", "error": f"child exit status {rc}"}), flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
