#!/usr/bin/env python3
"""First measurements of the copy-free beam search, by scripts/beam_probe.py's method.  (diagnostic, GPU box)

  attention : qgemm_attention_decode_indirect beside qgemm_attention_decode_batched, 16 sequences x 16 heads x d_k 64,
              one masked row each over 512 and 2048 keys, with three tables: the identity (the price of the indirection
              alone), a group-shared prefix (4 groups of 4: what a search produces) and a seeded random table;
  table     : qgemm_decoder_beam_reindex (4 groups x 4 beams and 8 x 8, 512 and 2048 columns), and
              qgemm_decoder_beam_begin beside beam_fork's qgemm_decoder_copy_slot calls for 4 x 4 beams at 512 and 2048
              prompt rows;
  generate  : the shape of scripts/beam_probe.py (d_model 1024, 16 heads, d_ff 4096, 2 blocks, enc_seq 512, vocabulary
              32768, a tied head with a position table): ONE qgemm_decoder_generate_beam_indirect call beside ONE
              qgemm_decoder_generate_beam call, (groups, beams) = (4, 4) and (4, 8), at prefixes 511 and 2047, and 8 x 8,
              which the new path alone can run.

Before timing, the indirect call must give the copy path's tokens, parents and score bits.  One JSON line per
measurement: the median of ROUNDS rounds with the round-to-round spread (max - min); the variants alternate inside every
round, in one process.  The measurements run in a child process under a time limit; after a child that fails or runs out
of time nothing more is started.
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

D, H, DFF, BLOCKS, ENC_SEQ, VOCAB = 1024, 16, 4096, 2, 512, 32768
SEED = 5


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

    def timed(fn, calls=1, prep=None):
        if prep:
            prep()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / calls  # us per call

    def report(rec, res, key="us"):
        for v, t in res.items():
            us, spread = _median_spread(t)
            rec[v] = {key: us, "spread_" + key: spread}
        print(json.dumps(rec), flush=True)

    # ---- the attention launch
    for keys in (512, 2048) if "attention" in args.what else ():
        n, dk = 16, D // H
        K = qg.fill_uniform(torch.empty((n, keys, D), device=dev), seed=3000)
        V = qg.fill_uniform(torch.empty((n, keys, D), device=dev), seed=3001)
        Q = qg.fill_uniform(torch.empty((n, D), device=dev), seed=3002)
        out = torch.empty((n, D), device=dev)
        seq_kv, q_pos0 = ints([keys] * n), ints([keys - 1] * n)
        b_, j_ = torch.arange(n, device=dev)[:, None], torch.arange(keys, device=dev)[None, :]
        shared = torch.where(j_ < keys - 16, b_ // 4 * 4, b_ // 4 * 4 + (b_ + j_) % 4)
        gen = torch.Generator(device=dev).manual_seed(31)
        tables = {"identity": b_.expand(n, keys), "group_shared_prefix": shared,
                  "random": torch.randint(0, n, (n, keys), device=dev, generator=gen)}
        tables = {k: t.to(torch.uint8).contiguous() for k, t in tables.items()}
        scale = 1.0 / 8.0

        def batched():
            assert L.qgemm_attention_decode_batched(Q.data_ptr(), D, K.data_ptr(), D, keys * D, V.data_ptr(), D, keys * D,
                                                    out.data_ptr(), D, n, 1, None, seq_kv, q_pos0, H, dk, scale, st) == 0

        def indirect(tab):
            def call():
                assert L.qgemm_attention_decode_indirect(Q.data_ptr(), D, K.data_ptr(), D, keys * D, V.data_ptr(), D,
                                                         keys * D, out.data_ptr(), D, n, 1, tab.data_ptr(), keys, n, None,
                                                         seq_kv, q_pos0, H, dk, scale, st) == 0
            return call

        batched()
        want = out.clone()
        indirect(tables["identity"])()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "the identity table is the batched call"
        variants = {"attention_decode_batched": batched}
        variants.update({f"attention_decode_indirect_{k}": indirect(t) for k, t in tables.items()})
        res = _rounds(variants, args.rounds, args.warmup, lambda fn: timed(fn, args.calls))
        report({"what": "attention", "sequences": n, "heads": H, "d_k": dk, "keys": keys, "calls": args.calls,
                "rounds": args.rounds}, res)
        del K, V

    # ---- the table launches, and begin beside the fork's copies
    for n_rows in (512, 2048) if "table" in args.what else ():
        dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=n_rows, max_enc_seq=ENC_SEQ, seed=1000, causal=True, kv_cache=True,
                         n_slots=64)
        enc = qg.fill_uniform(torch.empty((ENC_SEQ, D), device=dev), seed=2001)
        X = qg.fill_uniform(torch.empty((512, D), device=dev), seed=2000)
        for src in (60, 61, 62, 63):
            dec.begin_slot(src, enc)
            for p0 in range(0, n_rows, 512):
                dec.step_slot(src, X, pos=p0)
        variants = {}
        for groups, beams in ((4, 4), (8, 8)):
            rows = groups * beams
            slots = ints(list(range(rows)) if rows < 64 else list(range(64)))
            srcs = ints([60, 61, 62, 63] if groups == 4 else [8 * g for g in range(8)])
            if groups == 8:                     # 64 places: every prompt slot is place 0 of its group
                for g in range(8):
                    dec.begin_slot(8 * g, enc)
                    for p0 in range(0, n_rows, 512):
                        dec.step_slot(8 * g, X, pos=p0)
            pos = ints([n_rows] * groups)
            parents = torch.tensor([(3 * i + 1) % beams for i in range(rows)], dtype=torch.int32, device=dev)

            def begin(groups=groups, beams=beams, slots=slots, srcs=srcs, pos=pos):
                assert L.qgemm_decoder_beam_begin(dec._h, groups, beams, slots, srcs, pos, st) == 0

            def reindex(groups=groups, beams=beams, slots=slots, pos=pos, parents=parents):
                assert L.qgemm_decoder_beam_reindex(dec._h, groups, beams, slots, parents.data_ptr(), pos, st) == 0

            begin()
            reindex()
            variants[f"beam_begin_{groups}x{beams}"] = begin
            variants[f"beam_reindex_{groups}x{beams}"] = reindex
            if groups == 4:
                res = _rounds(dict(variants), args.rounds, args.warmup, lambda fn: timed(fn, args.calls))
                report({"what": "table", "columns": n_rows, "calls": args.calls, "rounds": args.rounds}, res)
                variants = {}
        res = _rounds(variants, args.rounds, args.warmup, lambda fn: timed(fn, args.calls))
        report({"what": "table", "columns": n_rows, "calls": args.calls, "rounds": args.rounds}, res)
        dec.close()
        # beam_fork for 4 x 4: the prompt into 2 x beams slots per group, less the prompt's own
        dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=n_rows, max_enc_seq=ENC_SEQ, seed=1000, causal=True, kv_cache=True,
                         n_slots=64)
        for g in range(4):
            dec.begin_slot(4 * g, enc)
            for p0 in range(0, n_rows, 512):
                dec.step_slot(4 * g, X, pos=p0)

        def fork():
            for g in range(4):
                for dst in [4 * g + q for q in range(1, 4)] + [32 + 4 * g + q for q in range(4)]:
                    assert L.qgemm_decoder_copy_slot(dec._h, dst, 4 * g, st) == 0

        res = _rounds({"beam_fork_4x4_copy_slot_x28": fork}, args.rounds, 2, lambda fn: timed(fn, 1))
        report({"what": "fork", "prompt_rows": n_rows, "enc_seq": ENC_SEQ, "rounds": args.rounds}, res)
        dec.close()

    if "generate" not in args.what:
        return 0
    # ---- a generate step: the copy path and the indirect path, each on its own decoder (same seed, same weights)
    n_new = args.tokens
    for pos0 in args.prefix:
        max_seq = pos0 + n_new
        E = qg.fill_uniform(torch.empty((VOCAB, D), device=dev), seed=2003)
        P = qg.fill_uniform(torch.empty((max_seq, D), device=dev), seed=2004, lo=-0.1, hi=0.1)
        head = qg.Head(qg.pack_b(E.t()), VOCAB, None, E, P, max_rows=64)
        enc = qg.fill_uniform(torch.empty((ENC_SEQ, D), device=dev), seed=2001)
        X = qg.fill_uniform(torch.empty((512, D), device=dev), seed=2000)
        decs = [qg.Decoder(D, H, DFF, BLOCKS, max_seq=max_seq, max_enc_seq=ENC_SEQ, seed=1000, causal=True,
                           kv_cache=True, n_slots=64) for _ in range(2)]
        copy, ind = decs

        def prompt(dec, slot):
            dec.begin_slot(slot, enc)
            for p0 in range(0, pos0, 512):
                dec.step_slot(slot, X[:min(512, pos0 - p0)], pos=p0)

        prompt(copy, 0)
        for b in range(1, 64):
            copy.copy_slot(b, 0)
        for g in range(8):          # the indirect path's prompts: place 0 of every group of 8 (and of 4: slots 0, 8, ..)
            prompt(ind, 8 * g)
        torch.cuda.synchronize()

        def outs(rows):
            return (torch.empty((n_new, rows), dtype=torch.int32, device=dev),
                    torch.empty((n_new, rows), dtype=torch.int32, device=dev), torch.empty((n_new, rows), device=dev))

        def tokens(groups, beams):
            return ((torch.arange(groups, device=dev, dtype=torch.int32) * 37) % VOCAB).repeat_interleave(beams).contiguous()

        def copy_call(groups, beams):
            rows = groups * beams
            a, b, at = ints(list(range(rows))), ints(list(range(32, 32 + rows))), ints([pos0] * groups)
            tok_in, o = tokens(groups, beams), outs(rows)

            def call():
                assert L.qgemm_decoder_generate_beam(copy._h, head._h, groups, beams, a, b, tok_in.data_ptr(), n_new, at,
                                                     None, -1, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), st) == 0
            return call, None, o

        def ind_call(groups, beams):
            rows = groups * beams
            sl = [8 * g + q for g in range(groups) for q in range(beams)]
            slots, srcs, at = ints(sl), ints([8 * g for g in range(groups)]), ints([pos0] * groups)
            tok_in, o = tokens(groups, beams), outs(rows)

            def begin():
                assert L.qgemm_decoder_beam_begin(ind._h, groups, beams, slots, srcs, at, st) == 0

            def call():
                assert L.qgemm_decoder_generate_beam_indirect(ind._h, head._h, groups, beams, slots, srcs,
                                                              tok_in.data_ptr(), n_new, at, None, -1, o[0].data_ptr(),
                                                              o[1].data_ptr(), o[2].data_ptr(), st) == 0
            return call, begin, o

        variants, preps = {}, {}
        for groups, beams in ((4, 4), (4, 8)):
            c, _, co = copy_call(groups, beams)
            i, begin, io = ind_call(groups, beams)
            c()
            begin()
            i()
            torch.cuda.synchronize()
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(co, io)), \
                f"{groups} x {beams}: the indirect search and the copy path differ"
            variants[f"generate_beam_{groups}x{beams}"] = c
            variants[f"generate_beam_indirect_{groups}x{beams}"], preps[f"generate_beam_indirect_{groups}x{beams}"] = i, begin
        i, begin, _ = ind_call(8, 8)
        variants["generate_beam_indirect_8x8"], preps["generate_beam_indirect_8x8"] = i, begin
        by_fn = {id(fn): preps.get(v) for v, fn in variants.items()}
        res = _rounds(variants, args.rounds, 2, lambda fn: timed(fn, 1, by_fn[id(fn)]))
        rec = {"what": "generate", "tokens": n_new, "pos": pos0, "vocab": VOCAB, "d_model": D, "n_heads": H, "d_ff": DFF,
               "n_blocks": BLOCKS, "enc_seq": ENC_SEQ, "rounds": args.rounds}
        for v, t in res.items():
            us, spread = _median_spread(t)
            rec[v] = {"us_per_step": round(us / n_new, 2), "spread_us_per_step": round(spread / n_new, 2)}
        print(json.dumps(rec), flush=True)
        head.close()
        for d in decs:
            d.close()
        del decs, copy, ind, E, P
        torch.cuda.empty_cache()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="*", default=["attention", "table", "generate"],
                    choices=["attention", "table", "generate"])
    ap.add_argument("--prefix", nargs="*", type=int, default=[511, 2047], help="prefix lengths of the generate section")
    ap.add_argument("--calls", type=int, default=100, help="launches per timed round of the attention and table sections")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=16, help="tokens generated per call")
    ap.add_argument("--limit", type=int, default=400, help="seconds for the child process")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "beam_indirect_probe.log"),
                    help="the file that keeps the measurements' JSON lines")
    ap.add_argument("--child", action="store_true", help="measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", *args.what, "--calls", str(args.calls),
           "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--tokens", str(args.tokens), "--prefix",
           *[str(p) for p in args.prefix]]
    try:
        done = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as e:
        part = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        sys.stdout.write(part)
        print(json.dumps({"what": "beam indirect probe", "error": f"no result within {args.limit} s"}), flush=True)
        return 2
    rc = done.returncode
    sys.stdout.write(done.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:                 # the child's lines, whole or up to its failure
        f.write(done.stdout)
    if rc != 0:
        print(json.dumps({"what": "beam indirect probe", "error": f"child exit status {rc}"}), flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
