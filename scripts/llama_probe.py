#!/usr/bin/env python3
"""First measurements of Llama-style blocks.  (diagnostic, GPU box)

  norm           qgemm_rmsnorm_pack_a and qgemm_prenorm_rms_pack_a beside qgemm_layernorm_pack_a / qgemm_prenorm_pack_a
                 at 512 x 1024: the same bytes moved, one reduction fewer;
  pack           qgemm_glu_pack_a (SiLU, and relu as the exp-free floor) at 512 x 4096 beside qgemm_gelu_pack_a and
                 qgemm_pack_a at the same k -- the gated pack reads 2k floats per row, the other two k;
  forward        Encoder.forward (512 rows) of the Llama block -- pre-norm, final norm, RoPE, RMSNorm, SwiGLU -- with
                 d_ff 2752 (about 2/3 of 4096 rounded to 64: the parameter-matched gated width) and d_ff 4096, beside
                 the pre-LN GELU block with RoPE at d_ff 4096; d_model 1024, 16 heads, 2 blocks;
  step_batch     a 16-slot Decoder.step_batch at position 2047 of the same three models, decoder-only;
  parent         with --parent-lib: qgemm_layernorm_pack_a, qgemm_prenorm_pack_a and qgemm_gelu_pack_a of THIS build
                 beside the same entry points of another build of the library (the parent commit's), alternated in
                 one process on the same buffers.

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

D, H, BLOCKS = 1024, 16, 2
LLAMA = dict(arch="standard", norm_first=True, final_norm=True, rope=True, norm="rms", gated_ffn=True, activation="silu")
PRE_GELU = dict(arch="standard", norm_first=True, final_norm=True, rope=True, activation="gelu_tanh")
MODELS = (("llama_dff2752", 2752, LLAMA), ("llama_dff4096", 4096, LLAMA), ("pre_ln_gelu_rope_dff4096", 4096, PRE_GELU))


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _ratios(rec, pairs):
    """new / old per pair, and "**slower**" where the medians differ by more than both spreads"""
    for name, new, old in pairs:
        r = rec[new]["us"] / rec[old]["us"]
        gap = rec[new]["us"] - rec[old]["us"]
        rec[name] = round(r, 3)
        if gap > max(rec[new]["spread_us"], rec[old]["spread_us"]):
            rec[name + "_verdict"] = "**slower**"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of libqgemm.so to alternate the older entry points with")
    ap.add_argument("--skip-models", action="store_true", help="the kernel comparisons only")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "llama_probe.log"))
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

    # ---- norm ----
    rows, w = 512, 1024
    A = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=1)
    B = torch.zeros((rows, w), device=dev)   # B = 0 keeps the row the same call after call
    g, b = torch.ones(w, device=dev), torch.zeros(w, device=dev)
    Y = qg.fill_uniform(torch.empty((rows, w), device=dev), seed=1)
    S2 = torch.empty((rows, w), device=dev)
    pa = torch.empty(L.qgemm_packed_size(rows, w), dtype=torch.uint8, device=dev)
    a, bp, gp, bep, y, s2, p = (t.data_ptr() for t in (A, B, g, b, Y, S2, pa))
    norm_calls = {
        "layernorm_pack_a": lambda lib: lambda: ok(lib.qgemm_layernorm_pack_a(y, bp, gp, bep, 1e-5, s2, rows, w, 127.0, p, st)),
        "prenorm_pack_a": lambda lib: lambda: ok(lib.qgemm_prenorm_pack_a(a, bp, gp, bep, 1e-5, a, rows, w, 127.0, p, st)),
    }
    variants = {k: mk(L) for k, mk in norm_calls.items()}
    variants["rmsnorm_pack_a"] = lambda: ok(L.qgemm_rmsnorm_pack_a(y, bp, gp, 1e-5, s2, rows, w, 127.0, p, st))
    variants["prenorm_rms_pack_a"] = lambda: ok(L.qgemm_prenorm_rms_pack_a(a, bp, gp, 1e-5, a, rows, w, 127.0, p, st))
    rec = measure(variants, args)
    _ratios(rec, (("rmsnorm_over_layernorm_pack_a", "rmsnorm_pack_a", "layernorm_pack_a"),
                  ("prenorm_rms_over_prenorm_pack_a", "prenorm_rms_pack_a", "prenorm_pack_a")))
    emit(dict(what="norm", rows=rows, w=w, **rec))

    # ---- pack ----
    m, k = 512, 4096
    X2 = qg.fill_uniform(torch.empty((m, 2 * k), device=dev), seed=2, lo=-3.0, hi=3.0)
    pk = torch.empty(L.qgemm_packed_size(m, k), dtype=torch.uint8, device=dev)
    x2, pkp = X2.data_ptr(), pk.data_ptr()
    pack_calls = {"gelu_pack_a": lambda lib: lambda: ok(lib.qgemm_gelu_pack_a(x2, 2 * k, m, k, 127.0, pkp, st))}
    variants = {
        "glu_pack_a_silu": lambda: ok(L.qgemm_glu_pack_a(x2, 2 * k, m, k, qg.QGEMM_ACT_SILU, 127.0, pkp, st)),
        "glu_pack_a_gelu": lambda: ok(L.qgemm_glu_pack_a(x2, 2 * k, m, k, qg.QGEMM_ACT_GELU_TANH, 127.0, pkp, st)),
        "glu_pack_a_relu": lambda: ok(L.qgemm_glu_pack_a(x2, 2 * k, m, k, qg.QGEMM_ACT_RELU, 127.0, pkp, st)),
        "gelu_pack_a": pack_calls["gelu_pack_a"](L),
        "pack_a": lambda: ok(L.qgemm_pack_a(x2, 2 * k, 1, m, k, 127.0, pkp, st)),
    }
    rec = measure(variants, args)
    _ratios(rec, (("glu_silu_over_gelu_pack_a", "glu_pack_a_silu", "gelu_pack_a"),
                  ("glu_relu_over_pack_a", "glu_pack_a_relu", "pack_a")))
    emit(dict(what="pack", m=m, k=k, **rec))

    # ---- parent ----
    if args.parent_lib:
        Lp = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for fn in ("qgemm_layernorm_pack_a", "qgemm_prenorm_pack_a", "qgemm_gelu_pack_a"):
            getattr(Lp, fn).argtypes = getattr(L, fn).argtypes
            getattr(Lp, fn).restype = ctypes.c_int
        Lp.qgemm_version.restype = ctypes.c_char_p
        variants, pairs = {}, []
        for name, mk in list(norm_calls.items()) + list(pack_calls.items()):
            variants[name], variants[name + "@parent"] = mk(L), mk(Lp)
            pairs.append((name + "_over_parent", name, name + "@parent"))
        rec = measure(variants, args)
        _ratios(rec, pairs)
        emit(dict(what="parent", parent=Lp.qgemm_version().decode(), **rec))

    if not args.skip_models:
        # ---- forward ----
        seq = 512
        X = qg.fill_uniform(torch.empty((seq, D), device=dev), seed=4)
        encs = {name: qg.Encoder(D, H, dff, BLOCKS, max_seq=seq, seed=1000, **kw) for name, dff, kw in MODELS}
        Ys = {k: torch.empty((seq, D), device=dev) for k in encs}
        variants = {k: (lambda k=k: ok(L.qgemm_encoder_forward(encs[k]._h, X.data_ptr(), Ys[k].data_ptr(), seq, st)))
                    for k in encs}
        rec = measure(variants, args)
        for k in encs:
            assert bool(torch.isfinite(Ys[k]).all()), k
            encs[k].close()
        _ratios(rec, (("llama_dff2752_over_pre_ln_gelu", "llama_dff2752", "pre_ln_gelu_rope_dff4096"),
                      ("llama_dff4096_over_pre_ln_gelu", "llama_dff4096", "pre_ln_gelu_rope_dff4096")))
        emit(dict(what="forward", d_model=D, n_heads=H, n_blocks=BLOCKS, seq=seq, **rec))

        # ---- step_batch ----
        n, pos = 16, 2047
        P = qg.fill_uniform(torch.empty((pos, D), device=dev), seed=6)
        Xn = qg.fill_uniform(torch.empty((n, D), device=dev), seed=7)
        decs, Yd = {}, {}
        for name, dff, kw in MODELS:
            dec = qg.Decoder(D, H, dff, BLOCKS, max_seq=pos + 1, max_enc_seq=0, seed=1000, causal=True, kv_cache=True,
                             n_slots=n, decoder_only=True, **kw)
            for s in range(n):
                dec.begin_slot(s)
                dec.step_slot(s, P)
            decs[name], Yd[name] = dec, torch.empty((n, D), device=dev)
        slots, poss = _ints(list(range(n))), _ints([pos] * n)
        variants = {k: (lambda k=k: ok(L.qgemm_decoder_step_batch(decs[k]._h, n, slots, poss, 1, Xn.data_ptr(),
                                                                  Yd[k].data_ptr(), st))) for k in decs}
        rec = measure(variants, args)
        for k in decs:
            assert bool(torch.isfinite(Yd[k]).all()), k
            decs[k].close()
        _ratios(rec, (("llama_dff2752_over_pre_ln_gelu", "llama_dff2752", "pre_ln_gelu_rope_dff4096"),
                      ("llama_dff4096_over_pre_ln_gelu", "llama_dff4096", "pre_ln_gelu_rope_dff4096")))
        emit(dict(what="step_batch", d_model=D, n_heads=H, n_blocks=BLOCKS, n_slots=n, pos=pos, **rec))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/llama_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
