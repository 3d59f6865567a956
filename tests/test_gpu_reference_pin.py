"""A live run of the reference's own operators (oracle/_ref/ref_driver: the reference's headers compiled for gfx950 by
`make -C oracle ref`) on the cases of tests/ref_cases.py, against
  (a) the C oracle, with the driver's exp / pow tables through the hooks where a case has them,
  (b) oracle/literal.py where it covers the operator,
  (c) the recorded run in tests/golden/reference_pin.npz,
  (d) this project's own entry points on the same inputs, directly.
For softmax, layernorm and the attention head (d) cannot hold bit for bit across math libraries: there the product is
held to the default oracle, as everywhere else in the suite, and the reference to the hooked one.

One child process runs every case (one more process with the GPU open, 60 s at most).  If it exits non-zero, dies of
a signal or runs out of time, every test here reports the driver's stderr and nothing is run again.  Without the
binary the module skips; tests/test_reference_pin_host.py still holds the oracle to the recorded run.
"""
import os

import numpy as np
import pytest
import torch

import attn_oracle
import ref_cases as R
from util import assert_bits_equal

pytestmark = pytest.mark.gpu


def _case_list():
    from oracle import oracle as O
    O.build()
    return R.build_cases(O)


CASES = _case_list()
BY_NAME = {c.name: c for c in CASES}
MAIN = [c.name for c in CASES if c.meta["kind"] != "table"]
CHAINS = [c.name for c in CASES if c.op == R.OP_QCHAIN]


@pytest.fixture(scope="module")
def ref(device):
    """{case name: {output name: array}} from one run of the driver."""
    if not os.path.exists(R.DRIVER):
        pytest.skip(f"oracle/_ref/ref_driver is not built: {R.RECIPE}")
    try:
        return R.run_driver(CASES, timeout=60)
    except R.DriverFailed as e:
        pytest.fail(str(e))


@pytest.fixture(scope="module")
def fixture():
    return R.Fixture()


def _same(got, want, what):
    if np.asarray(want).dtype == np.float32:
        assert_bits_equal(got, want, what)
    else:
        assert got.dtype == want.dtype and got.shape == want.shape and (got == want).all(), f"{what}: integers differ"


def _dev(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)


def _view(t, spec):
    v = t.t() if spec[0] & R.TRANSPOSE else t
    return v[spec[1]:spec[2], spec[3]:spec[4]] if spec[0] & R.SLICE else v


@pytest.mark.parametrize("name", MAIN)
def test_reference_is_the_oracle(oracle, ref, name):
    """(a) every output of the reference's operators is the C oracle's, bit for bit."""
    case = BY_NAME[name]
    table = R.table_of(ref, case)
    if table is not None:
        table = table.reshape(-1, table.shape[-1])
    want = R.expected(oracle, case, table)
    assert set(want) == set(ref[name])
    for out, a in want.items():
        _same(ref[name][out], np.asarray(a), f"reference vs oracle {name}/{out}")
    if case.op == R.OP_QMM:
        assert_bits_equal(ref[name]["O"], ref[name.replace("/whole", "/chain")]["O"], f"{name}: whole vs chain")
    for r in R.sentinel_rows(case) if case.meta["kind"] in ("softmax", "layernorm") else ():
        assert (ref[name][case.outputs[1]][r].view(np.uint32) == R.SENTINEL).all(), f"{name}: row {r} was written"


@pytest.mark.parametrize("name", CHAINS)
def test_reference_is_the_literal_walk(ref, name):
    """(b) oracle/literal.py on the whole case, or on ref_cases.literal_block's rows and columns of a large one."""
    rows, cols, want = R.literal_expected(BY_NAME[name])
    for out, a in want.items():
        _same(R.block_of(out, ref[name][out], rows, cols), a, f"reference vs literal.py {name}/{out}")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_reference_is_the_recorded_run(ref, fixture, name):
    """(c) today's run equals the committed fixture, tables included."""
    case = BY_NAME[name]
    if case.meta["kind"] == "table":
        assert_bits_equal(ref[name]["table"], fixture.table(case).reshape(ref[name]["table"].shape), f"{name} table")
        return
    for out in case.outputs:
        fixture.check(name, out, ref[name][out], "live vs recorded")


@pytest.mark.parametrize("name", CHAINS)
def test_product_quantized_chain_is_the_reference(qg, device, ref, name):
    """(d) op_quantized_mm on the same views, and pack_a / pack_b / mm_packed_i32 for Cx, Cw, Xq, Wq and Acc."""
    case, want = BY_NAME[name], ref[name]
    r = case.meta["range"]
    X, W = _view(_dev(case.inputs[0], device), case.meta["xs"]), _view(_dev(case.inputs[1], device), case.meta["ws"])
    M, K = X.shape
    N = W.shape[1]
    out = torch.full((M, N), float("nan"), device=device)
    qg.op_quantized_mm(X, W, out, r)
    pa, pb = qg.pack_a(X, r), qg.pack_b(W, r)
    acc = qg.mm_packed_i32(pa, pb)
    torch.cuda.synchronize()
    assert_bits_equal(out.cpu().numpy(), want["O"], f"{name}: op_quantized_mm vs reference")
    assert_bits_equal(pa.scale[:M].cpu().numpy().reshape(-1, 1), want["Cx"], f"{name}: pack_a scale vs reference Cx")
    assert_bits_equal(pb.scale[:N].cpu().numpy().reshape(1, -1), want["Cw"], f"{name}: pack_b scale vs reference Cw")
    assert (pa.q[:M, :K].cpu().numpy() == want["Xq"]).all(), f"{name}: pack_a int8 vs reference Xq"
    assert (pb.q[:N, :K].cpu().numpy().T == want["Wq"]).all(), f"{name}: pack_b int8 vs reference Wq"
    assert (acc.cpu().numpy() == want["Acc"]).all(), f"{name}: mm_packed_i32 vs reference Acc"


@pytest.mark.parametrize("name", [c.name for c in CASES if c.meta["kind"] == "mm"])
def test_product_mm_fp32_is_the_reference(qg, device, ref, name):
    """(d) mm_fp32 on the same views; NaNs at the same places, every other value the same bits."""
    case = BY_NAME[name]
    A, B = _view(_dev(case.inputs[0], device), case.meta["xs"]), _view(_dev(case.inputs[1], device), case.meta["ws"])
    got = qg.mm_fp32(A, B)
    torch.cuda.synchronize()
    assert_bits_equal(got.cpu().numpy(), ref[name]["C"], f"{name}: mm_fp32 vs reference")


def test_product_linear_is_the_reference(qg, device, ref):
    """(d) linear = op_quantized_mm + op_add(row) [+ op_relu], with sums below and exactly at zero."""
    (name,) = [c.name for c in CASES if c.meta["kind"] == "bias_relu"]
    X, W, b = (_dev(a, device) for a in BY_NAME[name].inputs)
    want = ref[name]
    assert (want["Y"] < 0).any() and (want["Y"] == 0).any(), "the bias should leave sums below and exactly at zero"
    pw = qg.pack_b(W)
    y, r = qg.linear(X, pw, b[0].contiguous(), relu=False), qg.linear(X, pw, b[0].contiguous(), relu=True)
    torch.cuda.synchronize()
    assert_bits_equal(y.cpu().numpy(), want["Y"], "linear vs reference op_add")
    assert_bits_equal(r.cpu().numpy(), want["R"], "linear(relu) vs reference op_relu")


@pytest.mark.parametrize("name", [c.name for c in CASES if c.meta["kind"] in ("softmax", "layernorm", "attention")])
def test_product_rows_and_attention_are_the_default_oracle(qg, oracle, device, name):
    """exp and pow are the math library's on the reference's side, so the product is held to the oracle's own choices
    (fl32(exp), fl(d * d)), on every row -- the 300 x 8 rows the reference leaves unwritten included."""
    case = BY_NAME[name]
    k = case.meta["kind"]
    if k == "softmax":
        got = qg.softmax_rows(_dev(case.inputs[0], device), case.meta["scale"])
        want = oracle.softmax_rows(case.inputs[0], case.meta["scale"])
    elif k == "layernorm":
        got = qg.add_layernorm_rows(_dev(case.inputs[0], device), _dev(case.inputs[1], device))
        want = oracle.add_layernorm_rows(*case.inputs)
    else:
        Q, K, V = R.attention_qkv(oracle, case)
        scale = attn_oracle.default_scale(case.p[1])
        got = qg.attention(_dev(Q, device), _dev(K, device), _dev(V, device), 1, scale)
        want = attn_oracle.attention_ref(Q, K, V, 1, scale)
    torch.cuda.synchronize()
    assert_bits_equal(got.cpu().numpy(), want, f"{name}: product vs default oracle")
