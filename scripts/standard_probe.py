#!/usr/bin/env python3
"""First measurements of the standard post-LN block.  (diagnostic, GPU box)

  ln             qgemm_layernorm_rows against qgemm_add_layernorm_rows, and qgemm_layernorm_pack_a against
                 add_layernorm_rows followed by pack_a (the reference architecture's fused add + layernorm + pack has no
                 entry point of its own; the forward comparison below has it in place), at 512 x 1024 and 8 x 1024;
  gelu_pack      qgemm_gelu_pack_a against qgemm_pack_a at 512 x 4096 and 64 x 4096;
  forward        Encoder.forward of a standard stack with relu and with GELU against the reference architecture's, at
                 d_model 1024, 16 heads, d_ff 4096, 2 blocks, 512 rows;
  step_batch     Decoder.step_batch of 16 slots at position 2047, standard against reference, same dimensions.

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

D, H, DFF, BLOCKS = 1024, 16, 4096, 2


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


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
    names = list(variants)
    for r in range(args.rounds):
        for v in names[r % len(names):] + names[:r % len(names)]:   # every variant takes every place in a round
            res[v].append(timed(variants[v]))
    out = {}
    for v, t in res.items():
        t = sorted(t)
        out[v] = {"us": round(t[len(t) // 2], 2), "spread_us": round(t[-1] - t[0], 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "standard_probe.log"))
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

    # ---- ln ----
    for rows, w in ((512, 1024), (8, 1024)):
        A = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=1)
        B = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=2)
        g, b = torch.ones(w, device=dev), torch.zeros(w, device=dev)
        Y = torch.empty((rows, w), device=dev)
        pa = torch.empty(L.qgemm_packed_size(rows, w), dtype=torch.uint8, device=dev)
        ptr = [t.data_ptr() for t in (A, B, g, b, Y, pa)]
        variants = {
            "layernorm_rows": lambda: ok(L.qgemm_layernorm_rows(ptr[0], ptr[1], ptr[2], ptr[3], 1e-5, ptr[4], rows, w, st)),
            "add_layernorm_rows": lambda: ok(L.qgemm_add_layernorm_rows(ptr[0], ptr[1], ptr[4], rows, w, st)),
            "layernorm_pack_a": lambda: ok(L.qgemm_layernorm_pack_a(ptr[0], ptr[1], ptr[2], ptr[3], 1e-5, ptr[4], rows, w,
                                                                   127.0, ptr[5], st)),
            "add_layernorm_rows+pack_a": lambda: (ok(L.qgemm_add_layernorm_rows(ptr[0], ptr[1], ptr[4], rows, w, st)),
                                                  ok(L.qgemm_pack_a(ptr[4], w, 1, rows, w, 127.0, ptr[5], st))),
        }
        emit(dict(what="ln", rows=rows, w=w, **measure(variants, args)))

    # ---- gelu_pack ----
    for m, k in ((512, 4096), (64, 4096)):
        X = qg.fill_uniform(torch.empty((m, k), device=dev), seed=3, lo=-3.0, hi=3.0)
        pa = torch.empty(L.qgemm_packed_size(m, k), dtype=torch.uint8, device=dev)
        xp, pp = X.data_ptr(), pa.data_ptr()
        variants = {"gelu_pack_a": lambda: ok(L.qgemm_gelu_pack_a(xp, k, m, k, 127.0, pp, st)),
                    "pack_a": lambda: ok(L.qgemm_pack_a(xp, k, 1, m, k, 127.0, pp, st))}
        emit(dict(what="gelu_pack", m=m, k=k, **measure(variants, args)))

    # ---- forward ----
    seq = 512
    X = qg.fill_uniform(torch.empty((seq, D), device=dev), seed=4)
    encs = {"reference": qg.Encoder(D, H, DFF, BLOCKS, max_seq=seq, seed=1000),
            "standard_relu": qg.Encoder(D, H, DFF, BLOCKS, max_seq=seq, seed=1000, arch="standard"),
            "standard_gelu": qg.Encoder(D, H, DFF, BLOCKS, max_seq=seq, seed=1000, arch="standard", activation="gelu_tanh")}
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
    for k, kw in (("reference", {}), ("standard_relu", dict(arch="standard")),
                  ("standard_gelu", dict(arch="standard", activation="gelu_tanh"))):
        dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=pos + 1, max_enc_seq=enc_seq, seed=1000, causal=True, kv_cache=True,
                         n_slots=n, **kw)
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
        f.write(f"# scripts/standard_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
