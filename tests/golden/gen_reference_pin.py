"""Records tests/golden/reference_pin.npz: what the reference's own operators, compiled for gfx950
(oracle/_ref/ref_driver, `make -C oracle ref`), answer on the cases of tests/ref_cases.py.  Needs the MI355X.

    python tests/golden/gen_reference_pin.py [--out tests/golden/reference_pin.npz]

The file holds, per case, the driver's outputs (an array, or its SHA-256 where ref_cases.kept_in_full says so), the
device exp / pow(., 2) tables as bit differences from ref_cases.exp_base / square_base, and index.json with the
reference files' hashes and the hipcc version the driver was built with.  It also prints how far those tables lie
from the oracle's own choices, fl32(exp((double)x)) and fl(d * d) -- the figures DESIGN.md s2 quotes.

Nothing here consults the oracle's expectations: a disagreement is for the tests to report, not for the recording
to hide.  The one thing asserted is that the chain's O and the whole op_quantized_mm's O are the same bits, because
the fixture keeps the array of the first and only the digest of the second.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_cases as R  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=R.FIXTURE)
    args = ap.parse_args()
    if not os.path.exists(R.DRIVER):
        sys.exit(f"{R.DRIVER} is missing: {R.RECIPE}")
    with open(R.BUILD_INFO) as f:
        build_info = json.load(f)
    cases = R.build_cases(O)
    results = R.run_driver(cases)
    for c in cases:
        if c.op == R.OP_QMM:
            chain = results[c.name.replace("/whole", "/chain")]["O"]
            assert R.digest(chain) == R.digest(results[c.name]["O"]), f"{c.name}: whole O != chain O"
    arrays = R.fixture_from_results(cases, results, build_info)
    np.savez_compressed(args.out, **arrays)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(cases)} cases")
    assert os.path.getsize(args.out) <= 139416, "larger than the largest fixture committed before it (cases.npz)"

    worst = {R.OP_EXP: (0, 0, None), R.OP_POW2: (0, 0, None)}
    count = {R.OP_EXP: 0, R.OP_POW2: 0}
    for c in cases:
        if c.meta["kind"] != "table":
            continue
        got, x = results[c.name]["table"], c.inputs[0]
        own = R.libm_exp_f32(x) if c.op == R.OP_EXP else R.square_base(x)
        diff = np.abs(got.view(np.uint32).astype(np.int64) - own.view(np.uint32).astype(np.int64))
        count[c.op] += x.size
        if int(diff.max()) >= worst[c.op][0]:
            worst[c.op] = (int(diff.max()), int((diff != 0).sum()), c.name)
        print(f"  {c.name}: {x.size} arguments in [{x.min():.6g}, {x.max():.6g}], max {int(diff.max())} ulp, "
              f"{int((diff != 0).sum())} differ")
    for op, label in ((R.OP_EXP, "device exp(float) vs fl32(exp((double)x))"),
                      (R.OP_POW2, "device pow(float, 2) vs fl(d * d)")):
        print(f"{label}: max {worst[op][0]} ulp over {count[op]} arguments (worst case {worst[op][2]})")


if __name__ == "__main__":
    main()
