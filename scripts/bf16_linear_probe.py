#!/usr/bin/env python3
"""bf16 against fp32 activations on the prepacked linear, same process, same packed weight.  (diagnostic, GPU box)

Default mode, per shape: rounds of CALLS back-to-back qgemm_linear / qgemm_linear_dt calls between two device events,
the variants alternating round by round (and the starting variant alternating too):
  f32   : fp32 X -> fp32 Y                      (qgemm_linear)
  bf16  : bf16 X -> bf16 Y                      (qgemm_linear_dt)
  cast  : bf16 X widened by torch, fp32 linear, Y narrowed by torch -- what a bf16 caller had to do before
One JSON line per shape: per-call microseconds of each variant (median of its rounds), the round-to-round spread
(max - min), and the bytes that depend on the I/O types, computed from the shape alone.

The A/B of gemm_i8_fm's two bf16 store paths at FFN up (the wide-row switch point kBf16WideRowsMin) was a --stores mode
of this script while the library read an override from the environment; its result is profiles/bf16_store_paths.log.
A re-measurement sets GemmArgs::wide_rows from a lab harness (lab/epi_lab.hip launches the kernel with its own GemmArgs).

For the kernel-level split run the same script under `rocprofv3 --kernel-trace --stats -- python ...` with --rounds 1.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

import _pkg  # noqa: E402

SHAPES = {
    "square_4096": (4096, 4096, 4096),
    "ffn_up": (2048, 16384, 4096),
    "ffn_down": (2048, 4096, 16384),
    "encoder_linear": (512, 1024, 1024),
}


def io_bytes(m, n, k, esize):
    """Bytes that move per call and depend on the activation type (the packed weight's n_pad x k_pad read does not)."""
    m_pad, k_pad = -(-m // 256) * 256, -(-k // 128) * 128
    return {"A_in": m * k * esize, "C_out": m * n * esize, "packed_A_write": m_pad * k_pad + 4 * m_pad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    dev = torch.device("cuda", 0)
    stream = qg._stream(dev)

    def setup(m, n, k):
        X = qg.fill_uniform(torch.empty((m, k), device=dev), seed=2)
        W = qg.fill_uniform(torch.empty((k, n), device=dev), seed=3)
        pw = qg.pack_b(W)
        del W
        Xb = X.to(torch.bfloat16)
        Y = torch.empty((m, n), device=dev)
        Yb = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
        ws = torch.empty(max(1, L.qgemm_linear_workspace_size(m, n, k)), dtype=torch.uint8, device=dev)
        return X, Xb, pw, Y, Yb, ws

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / calls  # us per call

    def summary(v):
        v = sorted(v)
        return {"us": round(v[len(v) // 2], 3), "spread_us": round(v[-1] - v[0], 3), "rounds": [round(x, 3) for x in v]}

    for name in args.shapes.split(","):
        m, n, k = SHAPES[name]
        X, Xb, pw, Y, Yb, ws = setup(m, n, k)

        def f32():
            assert L.qgemm_linear(X.data_ptr(), k, m, k, pw.buf.data_ptr(), n, None, 0, Y.data_ptr(), n, ws.data_ptr(),
                                  ws.numel(), stream) == 0

        def bf16():
            assert L.qgemm_linear_dt(Xb.data_ptr(), 1, k, m, k, pw.buf.data_ptr(), n, None, 0, Yb.data_ptr(), 1, n,
                                     ws.data_ptr(), ws.numel(), stream) == 0

        def cast():
            Xw = Xb.float()
            assert L.qgemm_linear(Xw.data_ptr(), k, m, k, pw.buf.data_ptr(), n, None, 0, Y.data_ptr(), n, ws.data_ptr(),
                                  ws.numel(), stream) == 0
            Yb.copy_(Y)

        variants = {"f32": f32, "bf16": bf16, "cast": cast}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        res = {v: [] for v in variants}
        for r in range(args.rounds):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for v in order:
                res[v].append(timed(variants[v], args.calls))
        out = {"shape": name, "mnk": [m, n, k], "calls": args.calls, "rounds": args.rounds,
               "bytes_f32": io_bytes(m, n, k, 4), "bytes_bf16": io_bytes(m, n, k, 2)}
        out.update({v: summary(t) for v, t in res.items()})
        out["bf16_minus_f32_us"] = round(out["bf16"]["us"] - out["f32"]["us"], 3)
        print(json.dumps(out), flush=True)
        del X, Xb, pw, Y, Yb, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
