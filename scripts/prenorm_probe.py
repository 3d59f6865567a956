#!/usr/bin/env python3
"""First measurements of the pre-LN block.  (diagnostic, GPU box)

  boundary       qgemm_prenorm_pack_a (S stored, in place over A as the stack runs it) beside qgemm_layernorm_pack_a (Y
                 stored) -- the post-LN instantiations are the parent commit's, register for register -- at 512 x 1024 and
                 8 x 1024: the two read A, B, gamma and beta and write one rows x w fp32 matrix and the packed view, the
                 same bytes; plus prenorm_pack_a without S (block 0's first launch), qgemm_add_rows, and the two
                 launches a pre-LN boundary would cost without the new form (add_rows, then layernorm_pack_a);
  forward        Encoder.forward of a pre-LN stack (with and without the final norm) beside the post-LN stack, relu, at
                 d_model 1024, 16 heads, d_ff 4096, 2 blocks, 512 rows;
  step_batch     Decoder.step_batch of 16 slots at position 2047, pre-LN beside post-LN, same dimensions.

One process; the variants of a comparison alternate inside every round; one JSON line per comparison with the median of
ROUNDS rounds of CALLS back-to-back calls between two device events and the round-to-round spread (max - min), in us
per call.  Everything goes through the C-ABI with arguments built beforehand.  These are first measurements, not bars.
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from standard_probe import measure  # noqa: E402 - the protocol of s25's probe, unchanged

D, H, DFF, BLOCKS = 1024, 16, 4096, 2


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "prenorm_probe.log"))
    args = ap.parse_args()

    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    st = qg._stream(dev)
    lines = []

    def emit(rec):
        rec.update(calls=args.calls, rounds=args.rounds)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def ok(rc):
        assert rc == 0, rc

    # ---- boundary ----
    for rows, w in ((512, 1024), (8, 1024)):
        # in place over A, as the stack runs it; B = 0 keeps the row the same call after call
        A = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=1)
        B = torch.zeros((rows, w), device=dev)
        g, b = torch.ones(w, device=dev), torch.zeros(w, device=dev)
        Y = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=1)
        S2 = torch.empty((rows, w), device=dev)
        pa = torch.empty(L.qgemm_packed_size(rows, w), dtype=torch.uint8, device=dev)
        a, bp, gp, bep, y, s2, p = (t.data_ptr() for t in (A, B, g, b, Y, S2, pa))
        variants = {
            "prenorm_pack_a": lambda: ok(L.qgemm_prenorm_pack_a(a, bp, gp, bep, 1e-5, a, rows, w, 127.0, p, st)),
            "layernorm_pack_a": lambda: ok(L.qgemm_layernorm_pack_a(y, bp, gp, bep, 1e-5, s2, rows, w, 127.0, p, st)),
            "prenorm_pack_a_no_S": lambda: ok(L.qgemm_prenorm_pack_a(a, 0, gp, bep, 1e-5, 0, rows, w, 127.0, p, st)),
            "add_rows": lambda: ok(L.qgemm_add_rows(a, bp, a, rows, w, st)),
            "add_rows+layernorm_pack_a": lambda: (ok(L.qgemm_add_rows(a, bp, a, rows, w, st)),
                                                  ok(L.qgemm_layernorm_pack_a(a, 0, gp, bep, 1e-5, s2, rows, w, 127.0, p,
                                                                              st))),
        }
        rec = measure(variants, args)
        rec["prenorm_over_layernorm_pack_a"] = round(rec["prenorm_pack_a"]["us"] / rec["layernorm_pack_a"]["us"], 3)
        emit(dict(what="boundary", rows=rows, w=w, **rec))

    # ---- forward ----
    seq = 512
    X = qg.fill_uniform(torch.empty((seq, D), device=dev), seed=4)
    mk = dict(max_seq=seq, seed=1000, arch="standard")
    encs = {"post_ln": qg.Encoder(D, H, DFF, BLOCKS, **mk),
            "pre_ln": qg.Encoder(D, H, DFF, BLOCKS, norm_first=True, **mk),
            "pre_ln_final_norm": qg.Encoder(D, H, DFF, BLOCKS, norm_first=True, final_norm=True, **mk)}
    Ys = {k: torch.empty((seq, D), device=dev) for k in encs}
    variants = {k: (lambda k=k: ok(L.qgemm_encoder_forward(encs[k]._h, X.data_ptr(), Ys[k].data_ptr(), seq, st)))
                for k in encs}
    rec = measure(variants, args)
    for k in encs:
        assert bool(torch.isfinite(Ys[k]).all()), k
        encs[k].close()
    emit(dict(what="forward", d_model=D, n_heads=H, d_ff=DFF, n_blocks=BLOCKS, seq=seq, **rec))

    # ---- step_batch ----
    n, pos, enc_seq = 16, 2047, 512
    E = qg.fill_uniform(torch.empty((enc_seq, D), device=dev), seed=5)
    P = qg.fill_uniform(torch.empty((pos, D), device=dev), seed=6)
    Xn = qg.fill_uniform(torch.empty((n, D), device=dev), seed=7)
    decs, Yd = {}, {}
    for k, kw in (("post_ln", {}), ("pre_ln", dict(norm_first=True)),
                  ("pre_ln_final_norm", dict(norm_first=True, final_norm=True))):
        dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=pos + 1, max_enc_seq=enc_seq, seed=1000, causal=True, kv_cache=True,
                         n_slots=n, arch="standard", **kw)
        for s in range(n):
            dec.begin_slot(s, E)
            dec.step_slot(s, P)
        decs[k], Yd[k] = dec, torch.empty((n, D), device=dev)
    slots, poss = _ints(list(range(n))), _ints([pos] * n)
    variants = {k: (lambda k=k: ok(L.qgemm_decoder_step_batch(decs[k]._h, n, slots, poss, 1, Xn.data_ptr(),
                                                              Yd[k].data_ptr(), st))) for k in decs}
    rec = measure(variants, args)
    for k in decs:
        assert bool(torch.isfinite(Yd[k]).all()), k
        decs[k].close()
    emit(dict(what="step_batch", d_model=D, n_heads=H, d_ff=DFF, n_blocks=BLOCKS, n_slots=n, pos=pos, enc_seq=enc_seq,
              **rec))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/prenorm_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
