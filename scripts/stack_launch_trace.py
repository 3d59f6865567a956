#!/usr/bin/env python3
"""Every pass kind of the transformer stack on every architecture, once, for a launch-for-launch comparison of two
builds.  (diagnostic, GPU box)

  stack_launch_trace.py run
      the workload, to be run under `rocprofv3 --kernel-trace --output-format csv` (no counters, no other tracing), one
      fresh process per tree.  At d_model 64, 4 heads, d_ff 200, 2 blocks, max_seq 9, 3 slots, for each of the
      reference, post-LN relu, post-LN GELU, pre-LN and pre-LN + final norm stacks: an encoder forward and a
      forward_batch of two lengths; a decoder forward, plain and causal; begin + step of 1 row and of 3 rows; a
      step_batch of 3 slots; a step_varlen mixing a 4-row prefill with one decoding row; beam_begin +
      step_batch_indirect + beam_reindex + step_batch_indirect.  The weights are the seeded ones.
  stack_launch_trace.py compare A_kernel_trace.csv B_kernel_trace.csv [--names parent branch] [--out FILE]
      the two traces' launches ordered by start time as (kernel name, grid, workgroup): the counts, whether the
      sequences are identical, the first difference if not, and the launches per kernel; exit status 1 if they differ.
"""
import argparse
import collections
import csv
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

D, H, DFF, BLOCKS, SEQ, ENC_SEQ, SLOTS = 64, 4, 200, 2, 9, 7, 3
ARCHS = (("reference", {}),
         ("post_ln_relu", dict(arch="standard")),
         ("post_ln_gelu", dict(arch="standard", activation="gelu_tanh")),
         ("pre_ln", dict(arch="standard", norm_first=True)),
         ("pre_ln_final_norm", dict(arch="standard", norm_first=True, final_norm=True)))


def run():
    import torch

    import _pkg

    qg = _pkg.package()
    qg.check_binary()
    assert torch.cuda.is_available(), "the workload runs on the GPU"
    dev = torch.device("cuda", 0)
    X = qg.fill_uniform(torch.empty((SEQ, D), device=dev), seed=11)
    E = qg.fill_uniform(torch.empty((ENC_SEQ, D), device=dev), seed=12)
    two = torch.cat([X, X[2:7]])                     # forward_batch: 9 and 5 rows
    mixed = torch.cat([X[:4], X[5:6]])               # step_varlen: a 4-row prefill and one decoding row
    rows = [X[i:i + n].contiguous() for i, n in ((0, 1), (1, 3), (0, 2), (4, 3), (2, 2), (6, 2))]
    parents = torch.tensor([1, 1], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for name, kw in ARCHS:
        enc = qg.Encoder(D, H, DFF, BLOCKS, max_seq=SEQ, seed=5, max_rows=16, **kw)
        plain = qg.Decoder(D, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=5, **kw)
        dec = qg.Decoder(D, H, DFF, BLOCKS, max_seq=SEQ, max_enc_seq=ENC_SEQ, seed=5, causal=True, kv_cache=True,
                         n_slots=SLOTS, max_rows=16, **kw)
        try:
            outs = [enc.forward(X), enc.forward_batch(two, [9, 5]), plain.forward(X, E), dec.forward(X, E)]
            dec.begin(E)
            outs += [dec.step(rows[0]), dec.step(rows[1])]                        # slot 0: 1 row, then 3 rows
            dec.begin_slot(1, E)
            dec.begin_slot(2, E)
            dec.step_slot(1, rows[2])
            outs.append(dec.step_batch([0, 1, 2], rows[3], pos=[4, 2, 0]))         # slot 0 now holds 5 rows
            dec.begin_slot(1, E)
            outs.append(dec.step_varlen([1, 0], mixed, [4, 1], pos=[0, 5]))
            dec.beam_begin([0, 1], [0], [2], 2)
            outs.append(dec.step_batch_indirect([0, 1], [0, 0], rows[4], pos=[2, 2]))
            dec.beam_reindex([0, 1], parents, [3], 2)
            outs.append(dec.step_batch_indirect([0, 1], [0, 0], rows[5], pos=[3, 3]))
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(y).all()) for y in outs), name
        finally:
            for m in (enc, plain, dec):
                m.close()
        print(name, "ok", flush=True)
    print(qg.version())
    return 0


def _launches(path):
    with open(path, newline="") as f:
        recs = sorted(csv.DictReader(f), key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    return [(r["Kernel_Name"], "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"),
             "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")) for r in recs]


def compare(args):
    a, b = _launches(args.a), _launches(args.b)
    na, nb = args.names
    same = a == b
    lines = [f"whole trace: {na} {len(a)} launches, {nb} {len(b)} launches, identical: {same}"]
    if not same:
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        lines.append(f"first difference at launch {i}:")
        lines += [f"  {n}: " + (" | ".join(t[i]) if i < len(t) else "(the trace ends)") for n, t in ((na, a), (nb, b))]
    lines.append(f"# launches per kernel ({na} | {nb}): name")
    ca, cb = collections.Counter(k for k, _, _ in a), collections.Counter(k for k, _, _ in b)
    lines += [f"{ca[k]} | {cb[k]}: {k}" for k in sorted(set(ca) | set(cb))]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("run")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    c.add_argument("--names", nargs=2, default=["parent", "branch"])
    c.add_argument("--out")
    args = ap.parse_args()
    return run() if args.cmd == "run" else compare(args)


if __name__ == "__main__":
    sys.exit(main())
