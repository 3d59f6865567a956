#!/usr/bin/env python3
"""First measurements of the wide decode attention kernel, d_k 128.  (diagnostic, GPU box)

  single     qgemm_attention_causal at 32 heads x d_k 128, 1 query row over 512, 2048 and 4096 keys: the wide launch of
             THIS build beside the same call on the parent commit's library (--parent-tree), where the shape takes the
             three launches through the workspace; the outputs must agree bit for bit before anything is timed.  And
             the d_k 64 launch over 4096 keys on both libraries: the narrow instantiations did not change.
  batched    qgemm_attention_decode_batched of 16 and 64 sequences at position 2047 (the parent refuses the shape),
             beside the same 16 / 64 sequences as single launches back to back;
  stack      a Llama-shaped decoder-only stack, d_model 1024, d_ff 2752, 2 blocks: step_batch of 16 slots at position
             2047 with 8 heads (d_k 128) beside 16 step_slot calls of the parent's stack (which refuses the batch), 16
             step_slot calls of this build, and step_batch of the 16-head (d_k 64) stack.

One process; the variants of a comparison alternate inside every round; one JSON line per comparison with the median of
ROUNDS rounds of CALLS back-to-back calls between two device events and the round-to-round spread (max - min), in us
per call.  Everything goes through the C-ABI with arguments built beforehand.  --parent-tree names a checkout of the
parent commit with its library built; its package is imported beside this one.  First measurements, not bars.
"""
import argparse
import ctypes
import importlib.util
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from llama_probe import LLAMA, _ints, _ratios  # noqa: E402 - the model keywords and the verdict rule of s28's probe
from standard_probe import measure  # noqa: E402 - the protocol of s25's probe, unchanged

PKG = "quantized-gemm-for-transformer-inference_amd"
D, DFF, BLOCKS, SLOTS, POS = 1024, 2752, 2, 16, 2047


def _parent_package(tree):
    d = os.path.join(os.path.abspath(tree), PKG)
    spec = importlib.util.spec_from_file_location("qgemm_parent", os.path.join(d, "__init__.py"),
                                                  submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["qgemm_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-tree", required=True, help="a checkout of the parent commit with build/libqgemm.so")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_heads_probe.log"))
    args = ap.parse_args()

    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    qp = _parent_package(args.parent_tree)
    L, Lp = qg.load(), qp.load()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    st = qg._stream(dev)
    lines = [json.dumps(dict(what="libraries", child=qg.version(), parent=qp.version()))]
    print(lines[0], flush=True)

    def emit(rec):
        rec.update(calls=args.calls, rounds=args.rounds)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def ok(rc):
        assert rc == 0, rc

    # ---- single ----
    def single(H, dk, keys, tag):
        d = H * dk
        Q = qg.fill_uniform(torch.empty((1, d), device=dev), seed=1)
        K = qg.fill_uniform(torch.empty((keys, d), device=dev), seed=2)
        V = qg.fill_uniform(torch.empty((keys, d), device=dev), seed=3)
        need = L.qgemm_attention_workspace_size(1, keys, H, dk)
        assert need == Lp.qgemm_attention_workspace_size(1, keys, H, dk)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        out = {k: torch.full((1, d), float("nan"), device=dev) for k in ("child", "parent")}
        scale = ctypes.c_float(1.0 / math.sqrt(dk)).value

        def call(lib, o):
            return lambda: ok(lib.qgemm_attention_causal(Q.data_ptr(), d, K.data_ptr(), d, V.data_ptr(), d, o.data_ptr(),
                                                         d, 1, keys, H, dk, scale, keys - 1, ws.data_ptr(), need, st))

        variants = {"child": call(L, out["child"]), "parent": call(Lp, out["parent"])}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        assert torch.equal(out["child"].view(torch.int32), out["parent"].view(torch.int32)), "child and parent differ"
        assert bool(torch.isfinite(out["child"]).all())
        rec = measure(variants, args)
        _ratios(rec, (("child_over_parent", "child", "parent"),))
        emit(dict(what=tag, n_heads=H, d_k=dk, keys=keys, child_plan=qg.attention_plan(1, keys, H, dk),
                  parent_plan=qp.attention_plan(1, keys, H, dk), **rec))
        return rec["child"]["us"]

    single_us = {keys: single(32, 128, keys, "single") for keys in (512, 2048, 4096)}
    single(32, 64, 4096, "single_narrow")

    # ---- batched ----
    H, dk, keys = 32, 128, POS + 1
    d = H * dk
    for n in (16, 64):
        Q = qg.fill_uniform(torch.empty((n, d), device=dev), seed=4)
        K = torch.empty((n, keys, d), device=dev).uniform_(-1.0, 1.0)   # (2 GiB at 64 sequences)
        V = torch.empty((n, keys, d), device=dev).uniform_(-1.0, 1.0)
        Ob, Os = torch.full((n, d), float("nan"), device=dev), torch.full((n, d), float("nan"), device=dev)
        need = L.qgemm_attention_workspace_size(1, keys, H, dk)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        scale = ctypes.c_float(1.0 / math.sqrt(dk)).value
        kv, qp0 = _ints([keys] * n), _ints([POS] * n)
        q, k, v, ob, os_ = (t.data_ptr() for t in (Q, K, V, Ob, Os))
        slab = 4 * keys * d

        def batch():
            ok(L.qgemm_attention_decode_batched(q, d, k, d, keys * d, v, d, keys * d, ob, d, n, 1, None, kv, qp0, H, dk,
                                                scale, st))

        def singles():
            for b in range(n):
                ok(L.qgemm_attention_causal(q + 4 * d * b, d, k + slab * b, d, v + slab * b, d, os_ + 4 * d * b, d, 1, keys,
                                            H, dk, scale, POS, ws.data_ptr(), need, st))

        batch()
        singles()
        torch.cuda.synchronize()
        assert torch.equal(Ob.view(torch.int32), Os.view(torch.int32)), "batched and single launches differ"
        rec = measure({"batch": batch, "singles": singles}, args)
        _ratios(rec, (("batch_over_singles", "batch", "singles"),))
        emit(dict(what="batched", n_seqs=n, n_heads=H, d_k=dk, pos=POS, us_per_seq=round(rec["batch"]["us"] / n, 2),
                  n_times_single_2048_us=round(n * single_us[2048], 2), **rec))
        del Q, K, V

    # ---- stack ----
    P = qg.fill_uniform(torch.empty((POS, D), device=dev), seed=7)
    Xn = qg.fill_uniform(torch.empty((SLOTS, D), device=dev), seed=8)

    def stack(pkg, heads):
        dec = pkg.Decoder(D, heads, DFF, BLOCKS, max_seq=POS + 1, max_enc_seq=0, seed=1000, causal=True, kv_cache=True,
                          n_slots=SLOTS, decoder_only=True, **LLAMA)
        for s in range(SLOTS):
            dec.begin_slot(s)
            dec.step_slot(s, P)
        return dec

    decs = {"child_h8": stack(qg, 8), "child_h16": stack(qg, 16), "parent_h8": stack(qp, 8)}
    Y = {k: torch.full((SLOTS, D), float("nan"), device=dev) for k in ("batch_h8", "batch_h16", "slots_h8", "parent_slots_h8")}
    slots, poss = _ints(list(range(SLOTS))), _ints([POS] * SLOTS)
    assert Lp.qgemm_decoder_step_batch(decs["parent_h8"]._h, SLOTS, slots, poss, 1, Xn.data_ptr(),
                                       Y["parent_slots_h8"].data_ptr(), st) == 1, "the parent refuses the d_k 128 batch"

    def batch_of(name, y):
        return lambda: ok(L.qgemm_decoder_step_batch(decs[name]._h, SLOTS, slots, poss, 1, Xn.data_ptr(), y.data_ptr(), st))

    def slots_of(lib, name, y):
        def run():
            for b in range(SLOTS):
                ok(lib.qgemm_decoder_step_slot(decs[name]._h, b, Xn.data_ptr() + 4 * D * b, y.data_ptr() + 4 * D * b, POS,
                                               1, st))
        return run

    variants = {"batch_h8": batch_of("child_h8", Y["batch_h8"]), "batch_h16": batch_of("child_h16", Y["batch_h16"]),
                "slots_h8": slots_of(L, "child_h8", Y["slots_h8"]),
                "parent_slots_h8": slots_of(Lp, "parent_h8", Y["parent_slots_h8"])}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for k in ("slots_h8", "parent_slots_h8"):
        assert torch.equal(Y[k].view(torch.int32), Y["batch_h8"].view(torch.int32)), f"{k} differs from the batched step"
    assert bool(torch.isfinite(Y["batch_h8"]).all()) and bool(torch.isfinite(Y["batch_h16"]).all())
    rec = measure(variants, args)
    _ratios(rec, (("batch_h8_over_parent_slots_h8", "batch_h8", "parent_slots_h8"),
                  ("slots_h8_over_parent_slots_h8", "slots_h8", "parent_slots_h8"),
                  ("batch_h8_over_batch_h16", "batch_h8", "batch_h16")))
    emit(dict(what="stack", d_model=D, d_ff=DFF, n_blocks=BLOCKS, n_slots=SLOTS, pos=POS, **rec))
    for dec in decs.values():
        dec.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/wide_heads_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
