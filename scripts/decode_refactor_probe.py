#!/usr/bin/env python3
"""Parent against this build on every decode-attention instantiation.  (diagnostic, GPU box)

For a change to the decode kernels' text that moves their instruction streams (the shared prologue and softmax pieces of
s33 were measured with it, and reverted on its verdicts).  This probe loads the parent's libqgemm.so by path beside
this build's and times the same launch on both, alternating the sides inside every round
(standard_probe.measure), after asserting that the outputs are bit-equal.  A row is "slower" by llama_probe._ratios'
rule: the medians differ by more than both round-to-round spreads.

  table forms   qgemm_attention_decode_{batched,indirect}{,_gqa,_kv16}, masked and unmasked, one row per sequence, the
                indirect forms through the identity table; 512 / 2048 / 4096 keys x 1 / 16 / 64 sequences; heads / KV heads
                x d_k: 32/8 x 128, 64/8 x 128, 32/8 x 64, 32/32 x 128 (kv16_probe.py) and 16/16 x 64 (decode_probe.py)
  one sequence  qgemm_attention[_causal] and qgemm_attention_gqa (DecodeOne) at the same heads and key counts

    python scripts/decode_refactor_probe.py --parent-lib PATH [--out profiles/decode_refactor_probe.log]
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

from llama_probe import _ratios  # noqa: E402
from standard_probe import measure  # noqa: E402

SHAPES = ((32, 8, 128), (64, 8, 128), (32, 8, 64), (32, 32, 128), (16, 16, 64))
KEYS, SEQS = (512, 2048, 4096), (1, 16, 64)
ENTRIES = ("qgemm_attention_decode_batched", "qgemm_attention_decode_indirect", "qgemm_attention_decode_batched_gqa",
           "qgemm_attention_decode_indirect_gqa", "qgemm_attention_decode_batched_kv16",
           "qgemm_attention_decode_indirect_kv16", "qgemm_attention", "qgemm_attention_causal", "qgemm_attention_gqa",
           "qgemm_attention_workspace_size", "qgemm_attention_gqa_workspace_size")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", required=True, help="the parent commit's libqgemm.so")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_refactor_probe.log"))
    args = ap.parse_args()

    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    P = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in ENTRIES:  # this build's prototypes: the ABI did not change
        getattr(P, name).argtypes, getattr(P, name).restype = getattr(L, name).argtypes, getattr(L, name).restype
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda", 0)
    st = qg._stream(dev)
    lines, slower = [], 0
    ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731

    def row(rec, call, out):
        """call(lib): the launch on one library into `out`; bit equality first, then the alternating measurement"""
        nonlocal slower
        got = {}
        for side, lib in (("parent", P), ("branch", L)):
            out.fill_(float("nan"))
            assert call(lib) == 0, (rec, side)
            torch.cuda.synchronize()
            got[side] = out.clone()
        assert torch.equal(got["parent"].view(torch.int32), got["branch"].view(torch.int32)), ("bits differ", rec)
        rec.update(measure({"parent": lambda: call(P), "branch": lambda: call(L)}, args))
        _ratios(rec, [("branch_over_parent", "branch", "parent")])
        slower += "branch_over_parent_verdict" in rec
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    g = torch.Generator(device=dev).manual_seed(33)
    for H, n_kv, dk in SHAPES:
        d, w, scale = H * dk, n_kv * dk, 1.0 / dk ** 0.5
        for keys in KEYS:
            n_max = max(SEQS)
            Q = torch.rand((n_max, d), device=dev, generator=g) * 2 - 1
            K = torch.rand((n_max, keys, w), device=dev, generator=g) * 2 - 1
            V = torch.rand((n_max, keys, w), device=dev, generator=g) * 2 - 1
            K16, V16 = K.to(torch.bfloat16), V.to(torch.bfloat16)
            out = torch.empty((n_max, d), device=dev)
            ident = torch.arange(n_max, dtype=torch.uint8, device=dev)[:, None].repeat(1, keys).contiguous()
            for n in SEQS:
                for masked in (True, False):
                    lens, pos = ints([keys] * n), ints([keys - 1] * n) if masked else None
                    for cache, k, v in (("fp32", K, V), ("bf16", K16, V16)):
                        if cache == "bf16" and (H, dk) == (16, 64):
                            continue
                        for indirect in (False, True):
                            name = "qgemm_attention_decode_" + ("indirect" if indirect else "batched") + \
                                   ("_kv16" if cache == "bf16" else "_gqa" if n_kv != H else "")
                            table = (ident.data_ptr(), keys, n_max) if indirect else ()
                            heads = (H,) if name.endswith(("batched", "indirect")) else (H, n_kv)
                            a = (Q.data_ptr(), d, k.data_ptr(), w, keys * w, v.data_ptr(), w, keys * w, out.data_ptr(), d,
                                 n, 1, *table, None, lens, pos, *heads, dk, scale, st)
                            row(dict(what=name, n_heads=H, n_kv_heads=n_kv, d_k=dk, keys=keys, n_seqs=n, masked=masked),
                                lambda lib, name=name, a=a: getattr(lib, name)(*a), out[:n])
            # one sequence: DecodeOne
            for masked in (True, False):
                if n_kv != H:
                    need = L.qgemm_attention_gqa_workspace_size(1, keys, H, n_kv, dk)
                    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
                    a = (Q.data_ptr(), d, K.data_ptr(), w, V.data_ptr(), w, out.data_ptr(), d, 1, keys, H, n_kv, dk, scale,
                         masked, keys - 1 if masked else 0, ws.data_ptr(), need, st)
                    name = "qgemm_attention_gqa"
                else:
                    need = L.qgemm_attention_workspace_size(1, keys, H, dk)
                    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
                    head = (Q.data_ptr(), d, K.data_ptr(), w, V.data_ptr(), w, out.data_ptr(), d, 1, keys, H, dk, scale)
                    a = head + ((keys - 1,) if masked else ()) + (ws.data_ptr(), need, st)
                    name = "qgemm_attention_causal" if masked else "qgemm_attention"
                row(dict(what=name, n_heads=H, n_kv_heads=n_kv, d_k=dk, keys=keys, n_seqs=1, masked=masked),
                    lambda lib, name=name, a=a: getattr(lib, name)(*a), out[:1])
            del Q, K, V, K16, V16, out, ident

    summary = json.dumps({"rows": len(lines), "slower": slower, "calls": args.calls, "rounds": args.rounds})
    print(summary)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# scripts/decode_refactor_probe.py, {qg.version()}\n" + "\n".join(lines) + "\n" + summary + "\n")


if __name__ == "__main__":
    main()
