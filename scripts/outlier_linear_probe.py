#!/usr/bin/env python3
"""The outlier decomposition on a cached weight against the two calls it sits between.  (diagnostic, GPU box)

One process, per shape the same X (8 outlier feature columns, placed as bench.py's c2_outlier places them: |x| in
7 .. 60 with random signs in every 50th row) and the same W, three variants:
  linear          : qgemm_linear on the packed W             -- no decomposition, the outliers set Cx
  mm_outlier      : qgemm_mm_outlier on the fp32 W           -- W re-quantized (as W') on every call
  linear_outlier  : qgemm_linear_outlier on the packed W     -- the decomposition on the cached int8
Rounds of CALLS back-to-back calls between two device events, the variants alternating round by round (and the order
reversing every other round).  One JSON line per shape: per-call microseconds of each variant (median of its rounds),
the round-to-round spread (max - min), the outlier counts read back, and linear_outlier minus mm_outlier.

Run each shape under its own time limit, e.g. `timeout -k 10 240 python scripts/outlier_linear_probe.py --shapes
square_4096`.  For the kernel-level split run it under `rocprofv3 --kernel-trace --stats -- python ...` with
--rounds 1 --calls 20, in a run of its own.
"""
import argparse
import ctypes
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
}
NCOLS = 8
THRESHOLD = 6.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()

    qg = _pkg.package()
    qg.check_binary()
    L = qg.load()
    dev = torch.device("cuda", 0)
    stream = qg._stream(dev)

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

    def count(k, ws):
        c = ctypes.c_int(-1)
        assert L.qgemm_outlier_count(k, ws.data_ptr(), ctypes.byref(c)) == 0
        return c.value

    for name in args.shapes.split(","):
        m, n, k = SHAPES[name]
        X = qg.fill_uniform(torch.empty((m, k), device=dev), seed=2)
        W = qg.fill_uniform(torch.empty((k, n), device=dev), seed=3)
        stride = k // NCOLS
        cols = [stride * c + (7 * c) % (stride // 2) + 3 for c in range(NCOLS)]
        g = torch.Generator(device="cpu").manual_seed(5)
        rows = X[::50].shape[0]
        mag = torch.rand((rows, NCOLS), generator=g) * 53.0 + 7.0
        sign = torch.randint(0, 2, (rows, NCOLS), generator=g).float() * 2.0 - 1.0
        X[::50, cols] = (mag * sign).to(dev)
        pw = qg.pack_b(W)
        Y = torch.empty((m, n), device=dev)
        ws_lin = torch.empty(max(1, L.qgemm_linear_workspace_size(m, n, k)), dtype=torch.uint8, device=dev)
        ws_mmo = torch.empty(L.qgemm_mm_outlier_workspace_size(m, n, k), dtype=torch.uint8, device=dev)
        ws_lo = torch.empty(L.qgemm_linear_outlier_workspace_size(m, n, k), dtype=torch.uint8, device=dev)

        def linear():
            assert L.qgemm_linear(X.data_ptr(), k, m, k, pw.buf.data_ptr(), n, None, 0, Y.data_ptr(), n,
                                  ws_lin.data_ptr(), ws_lin.numel(), stream) == 0

        def mm_outlier():
            assert L.qgemm_mm_outlier(X.data_ptr(), W.data_ptr(), Y.data_ptr(), m, n, k, THRESHOLD, ws_mmo.data_ptr(),
                                      ws_mmo.numel(), stream) == 0

        def linear_outlier():
            assert L.qgemm_linear_outlier(X.data_ptr(), k, m, k, pw.buf.data_ptr(), n, None, 0, THRESHOLD, Y.data_ptr(),
                                          n, ws_lo.data_ptr(), ws_lo.numel(), stream) == 0

        variants = {"linear": linear, "mm_outlier": mm_outlier, "linear_outlier": linear_outlier}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        counts = {"mm_outlier": count(k, ws_mmo), "linear_outlier": count(k, ws_lo)}
        assert counts["mm_outlier"] == counts["linear_outlier"] == NCOLS, counts
        res = {v: [] for v in variants}
        for r in range(args.rounds):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for v in order:
                res[v].append(timed(variants[v], args.calls))
        out = {"shape": name, "mnk": [m, n, k], "calls": args.calls, "rounds": args.rounds, "outlier_columns": counts,
               "workspace_bytes": {"linear": ws_lin.numel(), "mm_outlier": ws_mmo.numel(),
                                   "linear_outlier": ws_lo.numel()},
               "resident_weight_bytes": {"mm_outlier": W.numel() * 4, "linear_outlier": pw.buf.numel()}}
        out.update({v: summary(t) for v, t in res.items()})
        out["linear_outlier_minus_mm_outlier_us"] = round(out["linear_outlier"]["us"] - out["mm_outlier"]["us"], 3)
        print(json.dumps(out), flush=True)
        del X, W, pw, Y, ws_lin, ws_mmo, ws_lo
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
