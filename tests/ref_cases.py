"""The reference pin's cases: what oracle/_ref/ref_driver (the reference's own operators, compiled for gfx950 by
`make -C oracle ref`) is asked to compute, what the oracle says it must answer, and how the recorded answers in
tests/golden/reference_pin.npz are read.  Shared by tests/test_reference_pin_host.py (no GPU: the committed fixture
against the oracle), tests/test_gpu_reference_pin.py (a live run of the driver) and tests/golden/gen_reference_pin.py.
TEST INFRASTRUCTURE ONLY.

Inputs come from oracle.uniform / oracle.inputs with fixed seeds (and kat.json for the reference's own KAT-1), so the
fixture records outputs only.  Shapes are the smallest that cross the reference's seams: op_matmul_kernel's 32 x 32
tiles, the 1024-thread blocks of its reductions, the 256-thread blocks of softmax_kernel / layernorm_kernel.

exp and pow(., 2) are library functions, not IEEE operations, so a reference build and the oracle may differ there and
nowhere else.  Every softmax / layernorm / attention case therefore has a companion "<case>/table" case: the driver's
own kernel evaluates device exp(float) / pow(float, 2) on the arguments the ORACLE computes, and the oracle's hooked
variants (oracle.softmax_rows_table, oracle.add_layernorm_rows_table, attn_oracle.attention_ref(exp_tables=)) take
those values as given.  Max seeding, strict compares, sum order, mean, var / w and (y - mean) / var are then compared
bit for bit; were the oracle's arguments wrong, the table would answer other questions and the outputs would differ.
"""
import hashlib
import json
import math
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np

import attn_oracle
from util import GOLDEN, load_kat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "oracle", "_ref", "ref_driver")
BUILD_INFO = DRIVER + ".json"
FIXTURE = os.path.join(GOLDEN, "reference_pin.npz")
RECIPE = "make -C oracle ref (oracle.build_ref(), QGEMM_REFERENCE_DIR)"

MAGIC, VERSION = 0x4E495052, 1
SENTINEL = 0x7FC0DEAD          # the driver's fill of every fp32 output buffer
NAN_CANON = 0x7FC00000
F32, I8, I32 = 0, 1, 2
DTYPES = {F32: np.float32, I8: np.int8, I32: np.int32}
(OP_MM_F32, OP_QCHAIN, OP_QMM, OP_QMM_BIAS_RELU, OP_SCALE_SOFTMAX, OP_ADD_LAYERNORM, OP_ATTENTION, OP_LINEAR, OP_EXP,
 OP_POW2) = range(1, 11)
OUTPUTS = {
    OP_MM_F32: ("C",), OP_QCHAIN: ("Cx", "Cw", "sx", "sw", "Xq", "Wq", "Acc", "Outer", "Odq", "O"), OP_QMM: ("O",),
    OP_QMM_BIAS_RELU: ("O", "Y", "R"), OP_SCALE_SOFTMAX: ("scaled", "P"), OP_ADD_LAYERNORM: ("sum", "Y"),
    OP_ATTENTION: ("O",), OP_LINEAR: ("Y",), OP_EXP: ("table",), OP_POW2: ("table",),
}
TRANSPOSE, SLICE = 1, 2
NO_VIEW = (0, 0, 0, 0, 0)

# A recorded output above this many bytes is kept as a SHA-256 of its bits (NaNs canonical) instead of the array:
# equality of digests is the same pass / fail as equality of arrays, and the fixture stays below the largest one
# committed before it (cases.npz).  The K = 1040 case keeps Acc and O, the 300 x 8 divergence cases their P and Y
# (the sentinel rows are asserted by their bits).
FULL_LIMIT = 4096
DIGEST_ALWAYS = {"Outer", "Odq", "scaled", "sum"}   # one IEEE operation away from arrays that are recorded or inputs
FULL_ALWAYS = {("q_70x65x1040/chain", "Acc"), ("q_70x65x1040/chain", "O"), ("softmax_300x8_scale1", "P"),
               ("layernorm_300x8", "Y")}


class Case:
    def __init__(self, name, op, inputs, p=(), f=(), **meta):
        self.name, self.op = name, op
        self.inputs = [np.ascontiguousarray(a) for a in inputs]
        self.p = tuple(int(v) for v in p) + (0,) * (12 - len(p))
        self.f = tuple(float(v) for v in f) + (0.0,) * (2 - len(f))
        self.meta = meta

    @property
    def outputs(self):
        return OUTPUTS[self.op]


def apply_view(buf, spec):
    """The numpy reading of a view spec: transpose() first, then slice(h0, h1, w0, w1) -- tensor.cuh:121-149."""
    v = buf.T if spec[0] & TRANSPOSE else buf
    if spec[0] & SLICE:
        v = v[spec[1]:spec[2], spec[3]:spec[4]]
    return v


def _plant_seed_quirk(X, rows=(), cols=()):
    """Make the signed first element of some rows / columns their largest magnitude, negative, 1 % above the
    runner-up: below the 129 / 127 at which fl(x * s) would leave int8, so the quantized value is -128."""
    for i in rows:
        X[i, 0] = -np.float32(1.01) * np.abs(X[i, 1:]).max()
    for j in cols:
        X[0, j] = -np.float32(1.01) * np.abs(X[1:, j]).max()


def _tame_seed(X, W):
    """A signed first element that is negative and the largest magnitude of its row of X / column of W by more than
    1 % would quantize below -128, where the reference's float -> int8 conversion is undefined: pull it back to the
    1 % of _plant_seed_quirk.  Random inputs do this by themselves once in 2 K rows."""
    for A in (X, W.T):
        rest = np.abs(A[:, 1:]).max(axis=1)
        bad = -A[:, 0] > np.float32(1.01) * rest
        A[bad, 0] = -np.float32(1.01) * rest[bad]


def _special(O, M, N, K, seed):
    """The planting of test_unquantized_gemm_special_values on oracle.uniform inputs: products far below the smallest
    subnormal (signed zeros), rows in the subnormal range, +-inf and NaN operands."""
    X = (O.uniform((M, K), seed) * np.float32(1e-20)).astype(np.float32)
    W = (O.uniform((K, N), seed + 1) * np.float32(1e-20)).astype(np.float32)
    W[:, :8] *= np.float32(1e-6)
    X[:4, :] *= np.float32(1e19)
    X[5, 3] = np.inf
    X[6, 2] = -np.inf
    W[1, 9] = np.nan
    W[2, 11] = np.inf
    return X, W


# (name, M, N, K, seed, range, quirk rows of X, quirk columns of W)
QUANTIZED = [
    ("q_33x40x100", 33, 40, 100, 11, 127.0, (0, 5, 32), (0, 39)),
    ("q_64x64x64", 64, 64, 64, 12, 127.0, (3,), (63,)),
    ("q_70x65x1040", 70, 65, 1040, 13, 127.0, (69,), (64,)),   # three ragged tile steps; K at the 2^24 bound
    ("q_1x5x7", 1, 5, 7, 14, 127.0, (), ()),
    ("q_5x1x9", 5, 1, 9, 15, 127.0, (4,), ()),
    ("q_range63_7x9x33", 7, 9, 33, 16, 63.0, (2,), (8,)),
]
MM = [("mm_100x70x96", 100, 70, 96, 21), ("mm_33x65x130", 33, 65, 130, 22), ("mm_5x3x1", 5, 3, 1, 23),
      ("mm_1x77x33", 1, 77, 33, 24)]
MM_SPECIAL = [("mm_special_48x40x64", 48, 40, 64, 31), ("mm_special_48x40x36", 48, 40, 36, 33),
              ("mm_special_40x48x7", 40, 48, 7, 35)]
SOFTMAX_SHAPES = [(5, 7), (48, 64), (9, 1000), (1, 1)]
SOFTMAX_SCALES = [1.0, 0.125, -1.0]
LAYERNORM_SHAPES = [(33, 8), (9, 100), (7, 1000), (1, 4)]
DIVERGENCE = (300, 8)   # rows > 256 * ceil(w / 256): the reference launches one block of 256 threads
ATTENTION = dict(seq=9, d_model=16, d_k=4, d_v=4)
BIAS_RELU = (20, 24, 40)


def _inv_r2(range_):
    r = np.float32(range_)
    return np.float32(1.0) / np.float32(r * r)   # op_mm.cuh:99, evaluated in float on the host


def _quantized_pair(name, X_buf, W_buf, xs, ws, range_, qrows=(), qcols=()):
    meta = dict(kind="quantized", range=range_, xs=xs, ws=ws, qrows=qrows, qcols=qcols)
    return [Case(name + "/chain", OP_QCHAIN, [X_buf, W_buf], xs + ws, (range_, _inv_r2(range_)), **meta),
            Case(name + "/whole", OP_QMM, [X_buf, W_buf], xs + ws, (range_,), **meta)]


def _table_case(name, op, args):
    return Case(name + "/table", op, [args], kind="table", of=name)


def build_cases(O):
    """Every case, in the order the driver runs them.  The table cases' inputs are the oracle's own arguments."""
    cases = []
    kat = load_kat()["kat1"]
    cases += _quantized_pair("q_kat1", np.array(kat["X"], np.float32), np.array(kat["W"], np.float32), NO_VIEW, NO_VIEW,
                             kat["range"])
    for name, M, N, K, seed, range_, qrows, qcols in QUANTIZED:
        X, W = O.inputs(M, N, K, seed)
        _plant_seed_quirk(X, rows=qrows)
        _plant_seed_quirk(W, cols=qcols)
        _tame_seed(X, W)
        cases += _quantized_pair(name, X, W, NO_VIEW, NO_VIEW, range_, qrows, qcols)
    # X the transpose() of a K x M buffer, W a slice() inside a taller and wider one: the Index() stride rule
    Xb, Wb = O.uniform((37, 9), 34), O.uniform((39, 14), 35)
    _plant_seed_quirk(Xb.T, rows=(1,))
    _plant_seed_quirk(Wb[1:38, 3:9], cols=(2,))
    _tame_seed(Xb.T, Wb[1:38, 3:9])
    cases += _quantized_pair("q_strided_9x6x37", Xb, Wb, (TRANSPOSE, 0, 0, 0, 0), (SLICE, 1, 38, 3, 9), 127.0, (1,),
                             (2,))

    for name, M, N, K, seed in MM:
        X, W = O.inputs(M, N, K, seed)
        cases.append(Case(name, OP_MM_F32, [X, W], NO_VIEW + NO_VIEW, kind="mm", xs=NO_VIEW, ws=NO_VIEW))
    Q, Kt = O.uniform((20, 24), 50), O.uniform((34, 24), 51)   # Q K^T: B is the transpose() view of K
    cases.append(Case("mm_qkt_20x34x24", OP_MM_F32, [Q, Kt], NO_VIEW + (TRANSPOSE, 0, 0, 0, 0), kind="mm", xs=NO_VIEW,
                      ws=(TRANSPOSE, 0, 0, 0, 0)))
    for name, M, N, K, seed in MM_SPECIAL:
        X, W = _special(O, M, N, K, seed)
        cases.append(Case(name, OP_MM_F32, [X, W], NO_VIEW + NO_VIEW, kind="mm", xs=NO_VIEW, ws=NO_VIEW))

    for i, (rows, w) in enumerate(SOFTMAX_SHAPES + [DIVERGENCE]):
        S = O.uniform((rows, w), 60 + i, -4.0, 4.0)
        for scale in SOFTMAX_SCALES if (rows, w) != DIVERGENCE else [1.0]:
            name = f"softmax_{rows}x{w}_scale{scale:g}"
            cases.append(Case(name, OP_SCALE_SOFTMAX, [S], f=(scale,), kind="softmax", scale=scale))
            cases.append(_table_case(name, OP_EXP, O.softmax_args(S, scale)))
    for i, (rows, w) in enumerate(LAYERNORM_SHAPES + [DIVERGENCE]):
        A, B = O.uniform((rows, w), 70 + 2 * i), O.uniform((rows, w), 71 + 2 * i)
        name = f"layernorm_{rows}x{w}"
        cases.append(Case(name, OP_ADD_LAYERNORM, [A, B], kind="layernorm"))
        cases.append(_table_case(name, OP_POW2, O.add_layernorm_args(A, B)))

    M, N, K = BIAS_RELU
    X, W = O.inputs(M, N, K, 80)
    _tame_seed(X, W)
    b = O.uniform((1, N), 82, -0.5, 0.5)
    o = O.quantized_mm(X, W)
    for j in range(0, N, 5):          # some sums exactly zero: b[j] = -O[j % M, j]
        b[0, j] = -o[j % M, j]
    cases.append(Case(f"bias_relu_{M}x{N}x{K}", OP_QMM_BIAS_RELU, [X, W, b], f=(127.0,), kind="bias_relu"))
    cases.append(Case(f"linear_layer_{M}x{N}x{K}", OP_LINEAR, [X, W, b], kind="linear_layer"))

    a = ATTENTION
    bd = attn_oracle.init_bound(a["d_k"])
    X = O.uniform((a["seq"], a["d_model"]), 90)
    Wq, Wk = (O.uniform((a["d_model"], a["d_k"]), 91 + i, -bd, bd) for i in range(2))
    Wv = O.uniform((a["d_model"], a["d_v"]), 93, -bd, bd)
    name = "attention_head_9x16x4"
    cases.append(Case(name, OP_ATTENTION, [X, Wq, Wk, Wv], (a["d_model"], a["d_k"], a["d_v"]), kind="attention"))
    Qh, Kh, _ = attention_qkv(O, cases[-1])
    S = attn_oracle.attention_scores(Qh, Kh, 1)[0]
    cases.append(_table_case(name, OP_EXP, O.softmax_args(S, attn_oracle.default_scale(a["d_k"]))))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def attention_qkv(O, case):
    """The three projections of AttentionLayer::forward (attention.cuh:54-56), by the oracle."""
    X, Wq, Wk, Wv = case.inputs
    return O.mm_fp32(X, Wq), O.mm_fp32(X, Wk), O.mm_fp32(X, Wv)


def logical_operands(case):
    """X and W as the operator sees them through its views (quantized and mm cases)."""
    return (np.ascontiguousarray(apply_view(case.inputs[0], case.meta["xs"])),
            np.ascontiguousarray(apply_view(case.inputs[1], case.meta["ws"])))


def sentinel_rows(case):
    """Rows the reference leaves unwritten: op_softmax / op_layernorm launch ceil(w / 256) blocks of 256 threads, one
    thread per row (op_softmax.cuh:37-40, op_layernorm.cuh:40-43)."""
    rows, w = case.inputs[0].shape
    return range(min(rows, 256 * -(-w // 256)), rows)


def _with_sentinel(case, Y):
    Y = np.array(Y, np.float32)
    for r in sentinel_rows(case):
        Y[r].view(np.uint32)[:] = SENTINEL
    return Y


def expected(O, case, table=None):
    """What the oracle says the driver must have written for `case`: {output name: array}.  `table` is the companion
    table case's result where the case has one."""
    k = case.meta["kind"]
    f32 = np.float32
    if k == "quantized":
        X, W = logical_operands(case)
        r = case.meta["range"]
        out, d = O.quantized_mm(X, W, r, intermediates=True)
        if case.op == OP_QMM:
            return dict(O=out)
        Cx, Cw = d["Cx"].reshape(-1, 1), d["Cw"].reshape(1, -1)
        with np.errstate(all="ignore"):
            Outer = O.mm_fp32(Cx, Cw)                            # K = 1 op_mm: fl(Cx * Cw) + 0
            Odq = d["Acc"].astype(f32) * Outer                   # DequantizeFunc, one IEEE multiply
            return dict(Cx=Cx, Cw=Cw, sx=f32(r) / Cx, sw=f32(r) / Cw, Xq=d["Xq"], Wq=d["Wq"], Acc=d["Acc"],
                        Outer=Outer, Odq=Odq, O=out)
    if k == "mm":
        return dict(C=O.mm_fp32(*logical_operands(case)))
    if k == "softmax":
        S, scale = case.inputs[0], case.meta["scale"]
        return dict(scaled=S * f32(scale), P=_with_sentinel(case, O.softmax_rows_table(S, table, scale)))
    if k == "layernorm":
        A, B = case.inputs
        return dict(sum=A + B, Y=_with_sentinel(case, O.add_layernorm_rows_table(A, B, table)))
    if k == "bias_relu":
        X, W, b = case.inputs
        o = O.quantized_mm(X, W)
        return dict(O=o, Y=O.linear(X, W, b[0], relu=False), R=O.linear(X, W, b[0], relu=True))
    if k == "linear_layer":                                       # linear.cuh:50-54 as written: the unquantized op_mm
        X, W, b = case.inputs
        return dict(Y=O.mm_fp32(X, W) + b)
    if k == "attention":
        Q, K, V = attention_qkv(O, case)
        return dict(O=attn_oracle.attention_ref(Q, K, V, 1, attn_oracle.default_scale(case.p[1]), exp_tables=[table]))
    raise AssertionError(k)


def literal_block(case):
    """The rows and columns of a quantized chain that oracle/literal.py walks, one Fraction-exact fma at a time: all of
    them below 50 000 fmas, else the first and last, both sides of the 32-tile edge and the planted seed-quirk ones.
    Cx, Xq depend on their row alone, Cw, Wq on their column, Acc and O on the two: the walk of the sub-operands gives
    those entries of the whole case's outputs."""
    X, W = logical_operands(case)
    M, N, K = X.shape[0], W.shape[1], X.shape[1]
    if M * N * (-(-K // 32) * 32) <= 50000:
        return np.arange(M), np.arange(N)
    rows = sorted({0, 31, 32, M - 1, *case.meta["qrows"]} & set(range(M)))
    cols = sorted({0, 31, 32, N - 1, *case.meta["qcols"]} & set(range(N)))
    return np.array(rows), np.array(cols)


def literal_expected(case):
    """(rows, cols, {output: its [rows], [cols] or [rows x cols] block}) by oracle/literal.py."""
    from oracle import literal
    X, W = logical_operands(case)
    rows, cols = literal_block(case)
    out, d = literal.quantized_mm(X[rows], W[:, cols], case.meta["range"])
    return rows, cols, dict(Cx=d["Cx"].reshape(-1, 1), Cw=d["Cw"].reshape(1, -1), Xq=d["Xq"], Wq=d["Wq"],
                            Acc=d["Acc"], O=out)


def block_of(name, a, rows, cols):
    """The block of a whole output that literal_expected's `name` corresponds to."""
    a = np.asarray(a)
    if name in ("Cx", "Xq"):
        return a[rows]
    if name in ("Cw", "Wq"):
        return a[:, cols]
    return a[np.ix_(rows, cols)]


# ---- the driver's files ---------------------------------------------------------------------------------------------

def _tensor_bytes(a):
    a = np.ascontiguousarray(a)
    code = {np.dtype(np.float32): F32, np.dtype(np.int8): I8, np.dtype(np.int32): I32}[a.dtype]
    assert a.ndim == 2
    return struct.pack("<3I", code, *a.shape) + a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()


def write_case_file(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<3I", MAGIC, VERSION, len(cases)))
        for c in cases:
            f.write(struct.pack("<I12i2fI", c.op, *c.p, *c.f, len(c.inputs)))
            for a in c.inputs:
                f.write(_tensor_bytes(a))


def read_result_file(path, cases):
    with open(path, "rb") as f:
        raw = f.read()
    magic, version, n = struct.unpack_from("<3I", raw, 0)
    assert (magic, version, n) == (MAGIC, VERSION, len(cases)), "result file header"
    pos, results = 12, {}
    for c in cases:
        (nout,) = struct.unpack_from("<I", raw, pos)
        pos += 4
        assert nout == len(c.outputs), f"{c.name}: {nout} outputs"
        res = {}
        for name in c.outputs:
            code, h, w = struct.unpack_from("<3I", raw, pos)
            pos += 12
            dt = np.dtype(DTYPES[code]).newbyteorder("<")
            res[name] = np.frombuffer(raw, dt, h * w, pos).reshape(h, w).astype(DTYPES[code])
            pos += h * w * dt.itemsize
        results[c.name] = res
    assert pos == len(raw), "result file has trailing bytes"
    return results


class DriverFailed(RuntimeError):
    pass


def run_driver(cases, timeout=60):
    """One child process for every case; raises DriverFailed with the driver's stderr on a non-zero status, a signal or
    a timeout.  Nothing is retried."""
    with tempfile.TemporaryDirectory() as tmp:
        cin, cout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "results.bin")
        write_case_file(cin, cases)
        try:
            r = subprocess.run([DRIVER, cin, cout], capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired as e:
            raise DriverFailed(f"ref_driver ran past {timeout} s; stderr: {e.stderr}") from None
        if r.returncode != 0:
            raise DriverFailed(f"ref_driver exited with {r.returncode}; stderr: {r.stderr}")
        return read_result_file(cout, cases)


def table_of(results, case):
    t = results.get(case.name + "/table")
    return None if t is None else t["table"]


# ---- the recorded fixture -------------------------------------------------------------------------------------------

def canonical_bytes(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        b = a.view(np.uint32).copy()
        b[np.isnan(a)] = NAN_CANON
        a = b
    return a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()


def digest(a):
    return hashlib.sha256(canonical_bytes(a)).hexdigest()


def kept_in_full(case_name, out_name, a):
    if (case_name, out_name) in FULL_ALWAYS:
        return True
    return out_name not in DIGEST_ALWAYS and not case_name.endswith("/whole") and a.nbytes <= FULL_LIMIT


def exp_base(x):
    """exp(x) rounded to fp32, from IEEE double +, -, *, / and ldexp alone, so the same bits wherever numpy runs.  Only
    the origin the fixture's exp tables are recorded against (as differences of bit patterns, which compress to almost
    nothing); no check compares anything with it."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = np.rint(x * 1.4426950408889634)
    r = (x - n * 0.6931471803691238) - n * 1.9082149292705877e-10
    p = np.ones_like(r)
    for k in range(16, 0, -1):
        p = 1.0 + p * r / k
    return np.ldexp(p, n.astype(np.int64)).astype(np.float32)


def square_base(d):
    d = np.asarray(d, np.float32)
    return d * d


def table_base(case):
    return exp_base(case.inputs[0]) if case.op == OP_EXP else square_base(case.inputs[0])


def _bits64(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.int64)


def fixture_from_results(cases, results, build_info):
    """The arrays of reference_pin.npz for a run of the driver."""
    arrays, digests = {}, {}
    for c in cases:
        for name, a in results[c.name].items():
            key = f"{c.name}/{name}"
            if c.meta["kind"] == "table":
                arrays[key + "#delta"] = (_bits64(a) - _bits64(table_base(c))).astype(np.int32)
                digests[key] = digest(a)
            elif kept_in_full(c.name, name, a):
                arrays[key] = a
            else:
                digests[key] = digest(a)
                if a.dtype == np.int8:    # the K = 1040 operands Xq / Wq: a CRC-32 beside the digest
                    arrays[key + "#crc32"] = np.array([zlib.crc32(canonical_bytes(a))], np.uint32)
    index = dict(build=build_info, sentinel=f"0x{SENTINEL:08x}", digests=digests,
                 cases=[dict(name=c.name, op=c.op, outputs=list(c.outputs)) for c in cases])
    arrays["index.json"] = np.frombuffer(json.dumps(index, sort_keys=True).encode(), np.uint8)
    return arrays


class Fixture:
    def __init__(self, path=FIXTURE):
        self.npz = np.load(path)
        self.index = json.loads(self.npz["index.json"].tobytes().decode())
        self.digests = self.index["digests"]

    def table(self, case):
        """The recorded exp / pow table of a "<case>/table" case, rebuilt from its recorded bit differences."""
        delta = self.npz[f"{case.name}/table#delta"].astype(np.int64)
        t = (_bits64(table_base(case)) + delta).astype(np.uint32).view(np.float32)
        assert digest(t) == self.digests[f"{case.name}/table"], f"{case.name}: recorded table does not rebuild"
        return t

    def array(self, case_name, out_name):
        """The recorded array, or None where only its digest is kept."""
        key = f"{case_name}/{out_name}"
        return self.npz[key] if key in self.npz.files else None

    def check(self, case_name, out_name, got, what):
        """`got` equals the recorded output, bit for bit (NaNs at the same places): the array where it is kept, its
        SHA-256 where only that is."""
        from util import assert_bits_equal
        key = f"{case_name}/{out_name}"
        got = np.asarray(got)
        if key in self.npz.files:
            want = self.npz[key]
            assert got.shape == want.shape, f"{what} {key}: shape {got.shape} != {want.shape}"
            if want.dtype == np.float32:
                assert_bits_equal(got, want, f"{what} {key}")
            else:
                assert got.dtype == want.dtype and (got == want).all(), f"{what} {key}: integers differ"
        else:
            assert digest(got) == self.digests[key], f"{what} {key}: differs from the recorded SHA-256"
            if key + "#crc32" in self.npz.files:
                assert zlib.crc32(canonical_bytes(got)) == int(self.npz[key + "#crc32"][0]), f"{what} {key}: CRC"


def ulp_distance(a, b):
    """Max distance in units of the last place between two positive-or-zero fp32 arrays."""
    return int(np.abs(_bits64(a) - _bits64(b)).max())


def libm_exp_f32(x):
    """fl32(exp((double)x)) with the C library's exp: the oracle's own choice (oracle_softmax_rows)."""
    return np.array([math.exp(float(v)) for v in np.asarray(x, np.float32).ravel()], np.float64).astype(
        np.float32).reshape(np.shape(x))
