"""The oracle against the reference's own operators, on every machine: tests/golden/reference_pin.npz holds what
oracle/_ref/ref_driver -- the reference's headers compiled for gfx950 -- answered on the MI355X for the cases of
tests/ref_cases.py (tests/golden/gen_reference_pin.py recorded it).  Here the C oracle, oracle/literal.py and the
hooked softmax / layernorm / attention variants must reproduce those answers bit for bit, so a misreading of the
reference in the oracle fails without a GPU.  tests/test_gpu_reference_pin.py repeats this against a live run.
"""
import functools

import numpy as np
import pytest

import ref_cases as R
from util import assert_bits_equal, load_cases, load_kat


@functools.lru_cache(maxsize=None)
def _cases():
    from oracle import oracle as O
    O.build()
    return O, R.build_cases(O)


@functools.lru_cache(maxsize=None)
def _setup():
    O, cases = _cases()
    return O, cases, {c.name: c for c in cases}, R.Fixture()   # the fixture is read by the tests, not at collection


def _main_cases():
    _, cases = _cases()
    return [c.name for c in cases if c.meta["kind"] != "table"]


def _table(case, by_name, fx):
    t = by_name.get(case.name + "/table")
    return None if t is None else fx.table(t)


def test_fixture_lists_these_cases_and_its_origin():
    """The recorded run is of today's case list, and says which reference files and compiler made it."""
    _, cases, _, fx = _setup()
    assert [(c["name"], c["outputs"]) for c in fx.index["cases"]] == [(c.name, list(c.outputs)) for c in cases]
    build = fx.index["build"]
    for f in ("src/ops/op_mm.cuh", "src/ops/op_reduction.cuh", "src/ops/op_elemwise.cuh", "src/ops/op_softmax.cuh",
              "src/ops/op_layernorm.cuh", "src/modules/attention.cuh", "src/modules/linear.cuh",
              "src/utils/tensor.cuh"):
        assert len(build["reference_sha256"][f]) == 64
    assert "clang" in build["hipcc_version"] and "--offload-arch=gfx950" in build["flags"]
    assert "-ffast-math" not in build["flags"] and "-fno-fast-math" in build["flags"]


@pytest.mark.parametrize("name", _main_cases())
def test_oracle_reproduces_the_recorded_reference_run(name):
    """(a) the C oracle -- with the recorded exp / pow tables where the case has one -- gives every recorded output."""
    O, _, by_name, fx = _setup()
    case = by_name[name]
    want = R.expected(O, case, _table(case, by_name, fx))
    assert set(want) == set(case.outputs)
    for out, a in want.items():
        fx.check(case.name, out, a, "oracle vs recorded reference")
    if case.op == R.OP_QMM:   # the whole op_quantized_mm recorded the same bits as the chain of primitive calls
        assert fx.digests[f"{name}/O"] == R.digest(R.expected(O, by_name[name.replace("/whole", "/chain")])["O"])


def _chain_cases():
    _, cases = _cases()
    return [c.name for c in cases if c.op == R.OP_QCHAIN]


@pytest.mark.parametrize("name", _chain_cases())
def test_literal_walk_reproduces_the_recorded_reference_run(name):
    """(b) the second reading, oracle/literal.py, against the same recorded outputs: the whole case where it is small,
    else the rows and columns of ref_cases.literal_block, on every output the fixture keeps as an array."""
    _, _, by_name, fx = _setup()
    rows, cols, want = R.literal_expected(by_name[name])
    compared = 0
    for out, a in want.items():
        rec = fx.array(name, out)
        if rec is None:
            continue
        got = R.block_of(out, rec, rows, cols)
        if a.dtype == np.float32:
            assert_bits_equal(got, a, f"literal.py vs recorded reference {name}/{out}")
        else:
            assert (got == a).all(), f"literal.py vs recorded reference {name}/{out}"
        compared += 1
    assert compared >= 4, "the fixture keeps too few arrays of this case for the literal walk to see"


def test_recorded_kat1_is_the_committed_kat():
    """KAT-1 (test_quantize.cu:38-62) now has a run behind it: kat.json's typed-in bits and cases.npz's frozen oracle
    answers are what the reference's operators wrote."""
    _, _, _, fx = _setup()
    kat = load_kat()["kat1"]
    rec = {k: fx.npz[f"q_kat1/chain/{k}"] for k in ("Cx", "Cw", "Xq", "Acc", "O")}
    assert rec["Cx"].ravel().tolist() == kat["Cx"] and rec["Cw"].ravel().tolist() == kat["Cw"]
    assert rec["Xq"].tolist() == kat["Xq"] and rec["Acc"].tolist() == kat["Acc"]
    assert [f"0x{b:08x}" for b in rec["O"].view(np.uint32).ravel()] == kat["O_bits"]
    index, arrays = load_cases()
    same = [r for r in index if r["kind"] == "explicit" and (r["M"], r["N"], r["K"]) == (3, 2, 3)
            and np.array_equal(arrays[r["name"] + "/X"], np.array(kat["X"], np.float32))
            and np.array_equal(arrays[r["name"] + "/W"], np.array(kat["W"], np.float32))]
    for r in same:
        assert_bits_equal(arrays[r["name"] + "/O"], rec["O"], r["name"])
        assert (arrays[r["name"] + "/Acc"] == rec["Acc"]).all()


def test_documented_divergence_rows_hold_the_sentinel():
    """op_softmax / op_layernorm launch ceil(w / 256) blocks of 256 one-row threads: at 300 x 8 the reference never
    writes rows 256 .. 299 (the driver's sentinel is still there), where this project's entry points define every
    row.  Rows 0 .. 255 are the oracle's (test_oracle_reproduces_the_recorded_reference_run)."""
    _, cases, _, fx = _setup()
    seen = 0
    for c in cases:
        if c.meta["kind"] in ("softmax", "layernorm") and c.inputs[0].shape == R.DIVERGENCE:
            rec = fx.npz[f"{c.name}/{c.outputs[1]}"]
            assert list(R.sentinel_rows(c)) == list(range(256, 300))
            assert (rec[256:].view(np.uint32) == R.SENTINEL).all() and not np.isnan(rec[:256]).any()
            seen += 1
    assert seen == 2


def test_reference_pin_cases_stay_inside_defined_behaviour():
    """Outside these conditions the reference is undefined or platform-defined (float -> int8 of an out-of-range or
    NaN value, Cw[1..] at K = 1, fp32 accumulation of the int8 product past 2^24), and the project's own definitions
    apply instead of the pin."""
    O, cases, _, _ = _setup()
    planted = 0
    for c in cases:
        k = c.meta["kind"]
        if k in ("quantized", "bias_relu"):
            X, W = R.logical_operands(c) if k == "quantized" else c.inputs[:2]
            r = np.float32(c.meta.get("range", 127.0))
            assert X.shape[1] >= 2, c.name
            assert np.isfinite(X).all() and np.isfinite(W).all(), c.name
            _, d = O.quantized_mm(X, W, float(r), intermediates=True)
            assert (d["Cx"] != 0).all() and (d["Cw"] != 0).all(), c.name
            for v in (np.trunc(X * (r / d["Cx"])[:, None]), np.trunc(W * (r / d["Cw"])[None, :])):
                assert v.min() >= -128 and v.max() <= 127, c.name
            assert (O.int8_mm_fp32emu(d["Xq"], d["Wq"]) == O.int8_mm(d["Xq"], d["Wq"])).all(), c.name
            planted += int((d["Xq"] == -128).sum() + (d["Wq"] == -128).sum())
        elif k == "mm":
            assert R.logical_operands(c)[0].shape[1] >= 1
        elif k in ("softmax", "layernorm"):
            rows, w = c.inputs[0].shape
            assert (rows <= 256 * -(-w // 256)) == ((rows, w) != R.DIVERGENCE), c.name
        elif k == "attention":
            assert c.inputs[0].shape[0] <= 256
    assert planted >= 10, "the absmax seed quirk should put -128 into several rows and columns"


def test_hooks_with_the_oracles_own_functions_are_the_defaults():
    """softmax_rows_table / add_layernorm_rows_table fed fl32(exp) and fl(d * d) are softmax_rows / add_layernorm_rows:
    the hook changes where the function values come from and nothing else."""
    O, _, _, _ = _setup()
    S = O.uniform((9, 70), 5, -4.0, 4.0)
    for scale in R.SOFTMAX_SCALES:
        E = R.libm_exp_f32(O.softmax_args(S, scale))
        assert_bits_equal(O.softmax_rows_table(S, E, scale), O.softmax_rows(S, scale), f"softmax hook, scale {scale}")
    A, B = O.uniform((9, 70), 6), O.uniform((9, 70), 7)
    D = O.add_layernorm_args(A, B)
    assert_bits_equal(O.add_layernorm_rows_table(A, B, D * D), O.add_layernorm_rows(A, B), "layernorm hook")
