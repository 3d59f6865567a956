#!/usr/bin/env python3
"""First measurements of the output end of the model.  (diagnostic, GPU box)

  argmax   : the qgemm_argmax_rows launch on 64 x 32768 and on 1 x 131072 fp32 logits, beside torch.argmax on the same
             tensor and beside a read-only pass of torch over the same bytes (torch.sum), all between device events;
  generate : d_model 1024, 16 heads, d_ff 4096, 2 blocks, enc_seq 512, vocabulary 32768, a tied head with a position
             table; 16 and 64 cache slots at position 511 generate TOKENS tokens each:
               generate      ONE qgemm_decoder_generate call;
               python        the same loop driven from Python with step_batch, linear, torch.argmax and index_select,
                             the tokens staying on the device;
               python_read   that loop with the tokens read back to the host after every step, as a caller does who
                             looks for an end token.

Before timing, generate's tokens must equal those of the loop through head.embed / step_batch / head.next_tokens; the
agreement with the torch loop is reported, not asserted (torch.argmax does not promise the lowest index among equal
maxima).  One JSON line per measurement: the median of ROUNDS rounds with the round-to-round spread (max - min); the
variants alternate inside every round, in one process.  Everything here is a first measurement, not a bar.

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

    # ---- the argmax launch
    for rows, w in ((64, 32768), (1, 131072)):
        S = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=3000 + rows)
        idx = torch.empty(rows, dtype=torch.int32, device=dev)
        need = L.qgemm_argmax_rows_workspace_size(rows, w)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        sp, ip, wp = S.data_ptr(), idx.data_ptr(), ws.data_ptr()

        def ours():
            assert L.qgemm_argmax_rows(sp, w, rows, w, ip, None, wp, need, st) == 0

        ours()
        agree = bool(torch.equal(idx.long(), torch.argmax(S, dim=1)))
        variants = {"qgemm_argmax_rows": ours, "torch_argmax": lambda: torch.argmax(S, dim=1),
                    "torch_sum": lambda: torch.sum(S)}
        res = _rounds(variants, args.rounds, args.warmup, lambda fn: timed(fn, args.calls))
        rec = {"what": "argmax", "rows": rows, "w": w, "bytes": 4 * rows * w, "parts": qg.argmax_rows_plan(rows, w),
               "equals_torch_argmax": agree, "calls": args.calls, "rounds": args.rounds}
        for v, t in res.items():
            us, spread = _median_spread(t)
            rec[v] = {"us": us, "spread_us": spread}
        print(json.dumps(rec), flush=True)

    # ---- generation
    n_new, max_seq = args.tokens, POS + args.tokens
    slots_max = max(args.slots)
    dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=max_seq, max_enc_seq=ENC_SEQ, seed=1000, causal=True, kv_cache=True,
                     n_slots=slots_max)
    E = qg.fill_uniform(torch.empty((VOCAB, D), device=dev), seed=2003)
    P = qg.fill_uniform(torch.empty((max_seq, D), device=dev), seed=2004, lo=-0.1, hi=0.1)
    pw = qg.pack_b(E.t())
    head = qg.Head(pw, VOCAB, None, E, P, max_rows=slots_max)
    enc = qg.fill_uniform(torch.empty((ENC_SEQ, D), device=dev), seed=2001)
    X = qg.fill_uniform(torch.empty((POS, D), device=dev), seed=2000)
    dec.begin_slot(0, enc)
    dec.step_slot(0, X)
    for b in range(1, slots_max):
        dec.copy_slot(b, 0)
    torch.cuda.synchronize()

    for n in args.slots:
        slots = list(range(n))
        cs = (ctypes.c_int * n)(*slots)
        at = (ctypes.c_int * n)(*([POS] * n))
        tok_in = (torch.arange(n, device=dev, dtype=torch.int32) * 37) % VOCAB
        out = torch.empty((n_new, n), dtype=torch.int32, device=dev)
        tp, op = tok_in.data_ptr(), out.data_ptr()

        def generate():
            assert L.qgemm_decoder_generate(dec._h, head._h, n, cs, tp, n_new, at, op, st) == 0

        def library_loop():
            tok, rows = tok_in, []
            for t in range(n_new):
                pos = [POS + t] * n
                tok = head.next_tokens(dec.step_batch(slots, head.embed(tok, pos), pos=pos))
                rows.append(tok)
            return torch.stack(rows)

        def python_loop(read_back):
            tok, rows = tok_in.long(), []
            for t in range(n_new):
                x = E.index_select(0, tok) + P[POS + t]
                tok = torch.argmax(qg.linear(dec.step_batch(slots, x, pos=[POS + t] * n), pw), dim=1)
                if read_back:
                    tok.cpu()
                rows.append(tok)
            return torch.stack(rows)

        generate()
        torch.cuda.synchronize()
        assert torch.equal(out, library_loop()), "generate and the loop through embed / step_batch / next_tokens differ"
        same = int((python_loop(False) == out.long()).sum())
        variants = {"generate": generate, "python": lambda: python_loop(False), "python_read": lambda: python_loop(True)}
        res = _rounds(variants, args.rounds, 2, lambda fn: timed(fn, 1))
        rec = {"what": "generate", "n_slots": n, "tokens": n_new, "pos": POS, "vocab": VOCAB, "d_model": D, "n_heads": H,
               "d_ff": DFF, "n_blocks": BLOCKS, "enc_seq": ENC_SEQ, "rounds": args.rounds,
               "tokens_equal_to_torch_loop": f"{same} of {n_new * n}"}
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
    ap.add_argument("--calls", type=int, default=200, help="argmax launches per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tokens", type=int, default=32, help="tokens generated per call")
    ap.add_argument("--slots", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--limit", type=int, default=300, help="seconds for the child process")
    ap.add_argument("--child", action="store_true", help="measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--rounds",
           str(args.rounds), "--warmup", str(args.warmup), "--tokens", str(args.tokens), "--slots",
           *map(str, args.slots)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"what": "generate probe", "error": f"no result within {args.limit} s"}), flush=True)
        return 2
    if rc != 0:
        print(json.dumps({"what": "generate probe", "error": f"child exit status {rc}"}), flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
