"""Strided operand and output views of the fp32 interface on every GEMM plan and pack path, against the CPU oracle.

include/qgemm.h promises the reference's Index() semantics (element (r, c) at ptr[r * stride_h + c * stride_w]) for A,
B and C.  The fp32 epilogues choose a store path from the column stride, the row stride modulo 4, the base alignment
and the row stride against 16384 (gemm_i8_fm: 16-B paired stores / LDS-image stores / guarded scalar stores;
gemm_i8_small: 16-B or scalar), and the packs choose a kernel from the operands' strides and alignment.  Every expected
value comes from the oracle on the dense copy of the same logical matrices, bit for bit.  Every output lives in a
NaN-filled flat buffer, and the elements outside the logical matrix must still hold the NaN afterwards; operand
buffers hold NaN outside their views as well, so a read past a view reaches a scale.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_bf16 import _assert_plan
from test_gpu_range import FUSED_SHAPES, PLAN_IDS, PLAN_SHAPES, fused_pack_path
from util import assert_bits_equal, assert_values_equal

pytestmark = pytest.mark.gpu

POISON = np.float32(np.nan).view(np.int32).item()  # the bits torch.full(..., nan) stores


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _strided_out(m, n, sh, sw, offset, device):
    """A NaN-filled flat fp32 buffer and the m x n view into it at element `offset` with strides (sh, sw)."""
    flat = torch.full((offset + (m - 1) * sh + (n - 1) * sw + 1 + 16,), float("nan"), device=device)
    assert int(flat[:1].view(torch.int32).item()) == POISON
    return flat, torch.as_strided(flat, (m, n), (sh, sw), offset)


def _check_untouched(flat, m, n, sh, sw, offset, what):
    outside = torch.ones(flat.shape, dtype=torch.bool, device=flat.device)
    rows = torch.arange(m, device=flat.device)[:, None] * sh
    cols = torch.arange(n, device=flat.device)[None, :] * sw
    outside[(offset + rows + cols).reshape(-1)] = False
    assert int(outside.sum()) == flat.numel() - m * n
    written = int((flat.view(torch.int32)[outside] != POISON).sum())
    assert written == 0, f"{what}: {written} elements outside the matrix were written"


def _view_of(a, sh, sw, offset, device):
    """The matrix `a` on the device as a view with strides (sh, sw) at `offset` of a buffer that is NaN elsewhere."""
    r, c = a.shape
    flat = torch.full((offset + (r - 1) * sh + (c - 1) * sw + 1 + 16,), float("nan"), device=device)
    v = torch.as_strided(flat, (r, c), (sh, sw), offset)
    v.copy_(torch.from_numpy(a))
    return v


# ---------------------------------------------------------------------------------- 1. output layouts
# name -> (row stride, column stride, offset) of an m x n output
OUT_LAYOUTS = {
    "contiguous": lambda m, n: (n, 1, 0),
    "rows_n+4": lambda m, n: (n + 4, 1, 0),           # 16-B periodic: the vector path with csh != n
    "rows_n+1": lambda m, n: (n + 1, 1, 0),
    "rows_n+4_offset_1": lambda m, n: (n + 4, 1, 1),  # base 4-B aligned only
    "column_major": lambda m, n: (1, m + 3, 0),
    "every_other_column": lambda m, n: (2 * n, 2, 0),
    "rows_16384": lambda m, n: (16384, 1, 0),         # gemm_i8_fm: full tiles on the LDS-image stores, n < csh
    "rows_16380": lambda m, n: (16380, 1, 0),         # just below the switch: the paired stores
}
WIDE = ("rows_16384", "rows_16380")
# the unsplit 256-tile plan at 160 full tiles, and the split-K one, for the two wide layouts.  K = 128 (and PLAN_SHAPES'
# K = 192) reaches gemm_i8_fm's plain form; the row-finish form's layouts are in test_gpu_row_finish_matrix.py
WIDE_SHAPES = [((2560, 4096, 128), 256, 1, None), ((2048, 4096, 2048), 256, 2, None)]
OUT_CASES = [(s, lay) for s in PLAN_SHAPES for lay in OUT_LAYOUTS if lay not in WIDE] + \
            [(s, lay) for s in WIDE_SHAPES for lay in WIDE]


@functools.lru_cache(maxsize=2)
def _case(m, n, k):
    """Inputs of one shape, the oracle's output and a bias, shared by the shape's tests and never changed."""
    from oracle import oracle as O
    X, W = O.inputs(m, n, k, 307)
    X[::4, 0] = -2.5
    W[0, ::3] = -1.75
    return X, W, O.quantized_mm(X, W), O.uniform((n,), 311, -0.5, 0.5)


_PACKED = {}


def _packed(qg, device, m, n, k):
    """The shape's operands, packed once per shape (only the latest shape is kept)."""
    if (m, n, k) not in _PACKED:
        _PACKED.clear()
        X, W = _case(m, n, k)[:2]
        _PACKED[(m, n, k)] = (qg.pack_a(_dev(X, device)), qg.pack_b(_dev(W, device)))
    return _PACKED[(m, n, k)]


@pytest.mark.parametrize("plan,layout", OUT_CASES, ids=["x".join(map(str, s[0])) + "-" + lay for s, lay in OUT_CASES])
def test_output_layouts_every_plan(qg, oracle, device, plan, layout):
    shape, tile, splits, depth = plan
    _assert_plan(qg, shape, tile, splits, depth)
    m, n, k = shape
    sh, sw, off = OUT_LAYOUTS[layout](m, n)
    assert layout not in WIDE or (m % 256 == 0 and n % 256 == 0 and n < sh), "full tiles inside wider rows"
    pa, pb = _packed(qg, device, m, n, k)
    flat, C = _strided_out(m, n, sh, sw, off, device)
    assert C.data_ptr() % 16 == (4 if off else 0)
    qg.mm_packed(pa, pb, C)
    torch.cuda.synchronize()
    what = f"{shape} {layout}"
    assert_bits_equal(C.contiguous().cpu().numpy(), _case(m, n, k)[2], what)
    _check_untouched(flat, m, n, sh, sw, off, what)


@pytest.mark.parametrize("plan,stride", [(PLAN_SHAPES[0], None), (PLAN_SHAPES[4], None), (WIDE_SHAPES[0], 16384)],
                         ids=["32-rows_n+4", "256-rows_n+4", "256-rows_16384"])
def test_linear_bias_relu_padded_rows(qg, oracle, device, plan, stride):
    """qgemm_linear with bias + relu into rows of n + 4 floats (and of 16384 for the 256-tile shape)."""
    shape, tile, splits, depth = plan
    _assert_plan(qg, shape, tile, splits, depth)
    m, n, k = shape
    stride = n + 4 if stride is None else stride
    X, W, _, b = _case(m, n, k)
    pb = _packed(qg, device, m, n, k)[1]
    flat, Y = _strided_out(m, n, stride, 1, 0, device)
    qg.linear(_dev(X, device), pb, bias=_dev(b, device), relu=True, Y=Y)
    torch.cuda.synchronize()
    what = f"linear {shape} y_stride_h {stride}"
    assert_bits_equal(Y.contiguous().cpu().numpy(), oracle.linear(X, W, b, True), what)
    _check_untouched(flat, m, n, stride, 1, 0, what)


# ---------------------------------------------------------------------------------- 2. operand layouts, pack intermediates
def _x_layouts(M, K):
    """name -> (row stride, column stride, offset) of an M x K activation."""
    return {
        "rows_K+4": (K + 4, 1, 0),
        "rows_K+1": (K + 1, 1, 0),
        "offset_1": (K + 4, 1, 1),  # data_ptr % 16 == 4
        # column-major: M = 300 the vector column pass, M = 9 in a leading dimension of 10 the scalar one
        "column_major": (1, M if M % 4 == 0 else M + 1, 0),
        "every_other_column": (2 * K, 2, 0),
    }


def _w_layouts(K, N):
    """name -> (row stride, column stride, offset) of a K x N weight."""
    return {
        "rows_N+8": (N + 8, 1, 0),
        "rows_N+1": (N + 1, 1, 0),
        "column_major": (1, K, 0),          # nn.Linear's [out, in] storage, transposed
        "column_major_ld_K+4": (1, K + 4, 0),
        "every_other_row": (2 * N, 1, 0),
    }


@pytest.mark.parametrize("K", [260, 1028, 4100])
def test_pack_a_operand_layouts(qg, oracle, device, K):
    for M in (9, 300):
        X = oracle.uniform((M, K), 8000 + K + M, -2.0, 2.0)
        X[::4, 0] = -2.5
        _, ref = oracle.quantized_mm(X, np.ones((K, 1), np.float32), intermediates=True)
        for name, (sh, sw, off) in _x_layouts(M, K).items():
            what = f"pack_a {M}x{K} {name}"
            Xv = _view_of(X, sh, sw, off, device)
            assert Xv.data_ptr() % 16 == (4 if off else 0)
            pa = qg.pack_a(Xv)
            torch.cuda.synchronize()
            assert_values_equal(pa.scale[:M].cpu().numpy(), ref["Cx"], f"{what} Cx")
            q = pa.q.cpu().numpy()
            assert (q[:M, :K] == ref["Xq"]).all(), f"{what} Xq: {int((q[:M, :K] != ref['Xq']).sum())} bytes differ"
            assert not q[M:].any() and not q[:, K:].any(), f"{what}: padding not zero"
            assert not pa.scale[M:].cpu().numpy().any(), f"{what}: padding scales not zero"


@pytest.mark.parametrize("K", [260, 1028, 4100])
def test_pack_b_operand_layouts(qg, oracle, device, K):
    for N in (9, 300):
        W = oracle.uniform((K, N), 8100 + K + N, -2.0, 2.0)
        W[0, ::3] = -1.75
        _, ref = oracle.quantized_mm(np.ones((1, K), np.float32), W, intermediates=True)
        for name, (sh, sw, off) in _w_layouts(K, N).items():
            what = f"pack_b {K}x{N} {name}"
            pb = qg.pack_b(_view_of(W, sh, sw, off, device))
            torch.cuda.synchronize()
            assert_values_equal(pb.scale[:N].cpu().numpy(), ref["Cw"], f"{what} Cw")
            q = pb.q.cpu().numpy()
            assert (q[:N, :K] == ref["Wq"].T).all(), f"{what} Wq: {int((q[:N, :K] != ref['Wq'].T).sum())} bytes differ"
            assert not q[N:].any() and not q[:, K:].any(), f"{what}: padding not zero"
            assert not pb.scale[N:].cpu().numpy().any(), f"{what}: padding scales not zero"


# ---------------------------------------------------------------------------------- 3. the drop-in on strided operands
def _drop_in_ws(qg, device, Xv, Wv, M, N, K):
    """op_mm_quantize_ws on views Xv, Wv with a caller workspace full of 0xFF; returns the NaN-prefilled output."""
    L = qg.load()
    ws = torch.full((L.op_mm_quantize_workspace_size(M, N, K),), 255, dtype=torch.uint8, device=device)
    O = torch.full((M, N), float("nan"), device=device)
    rc = L.op_mm_quantize_ws(Xv.data_ptr(), Xv.stride(0), Xv.stride(1), Wv.data_ptr(), Wv.stride(0), Wv.stride(1),
                             O.data_ptr(), N, 1, M, N, K, 127.0, ws.data_ptr(), ws.numel(), qg._stream(device))
    assert rc == 0
    torch.cuda.synchronize()
    return O.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _drop_in_case(M, N, K):
    from oracle import oracle as O
    X, W = O.inputs(M, N, K, 313)
    X[::4, 0] = -2.5
    W[0, ::3] = -1.75
    return X, W, O.quantized_mm(X, W)


FUSED = [f for f in FUSED_SHAPES if f[1] != "separate"]  # the fused packs: one shape per path


@pytest.mark.parametrize("shape,path", FUSED, ids=[p[1] + "-" + "x".join(map(str, p[0])) for p in FUSED])
def test_drop_in_strided_operands(qg, oracle, device, shape, path):
    """X[:, :K] of an M x (K + 4) buffer times W[:, :N] of a K x (N + 8) buffer -- the fused packs with xsh != k and
    wsh != n -- then both operands column-major (the separate row / column packs)."""
    M, N, K = shape
    assert fused_pack_path(M, N, K, K + 4, N + 8) == path
    X, W, want = _drop_in_case(M, N, K)
    got = _drop_in_ws(qg, device, _view_of(X, K + 4, 1, 0, device), _view_of(W, N + 8, 1, 0, device), M, N, K)
    assert_bits_equal(got, want, f"{shape} X rows of K + 4, W rows of N + 8")
    got = _drop_in_ws(qg, device, _view_of(X, 1, M, 0, device), _view_of(W, 1, K, 0, device), M, N, K)
    assert_bits_equal(got, want, f"{shape} X and W column-major")


@pytest.mark.parametrize("x_cm", [False, True], ids=["X_rows", "X_cols"])
@pytest.mark.parametrize("w_cm", [False, True], ids=["W_rows", "W_cols"])
def test_split_k_operand_layout_combinations(qg, oracle, device, x_cm, w_cm):
    M, N, K = 256, 256, 4096
    _assert_plan(qg, (M, N, K), 64, 2, 3)
    X, W, want = _drop_in_case(M, N, K)
    Xv = _view_of(X, 1, M, 0, device) if x_cm else _view_of(X, K + 4, 1, 0, device)
    Wv = _view_of(W, 1, K, 0, device) if w_cm else _view_of(W, N + 8, 1, 0, device)
    assert_bits_equal(_drop_in_ws(qg, device, Xv, Wv, M, N, K), want, f"split-K X cm {x_cm} W cm {w_cm}")


# ---------------------------------------------------------------------------------- 4. the 2^31-byte guard
@pytest.mark.parametrize("N,K,wsh,unguarded", [(64, 4096, 131104, "single8"), (16384, 2052, 262176, "single32")],
                         ids=["8_column_guard", "32_column_guard"])
def test_w_view_spanning_2_31_bytes(qg, oracle, device, N, K, wsh, unguarded):
    """W = the first N columns of a K-row buffer so wide that the view spans 2^31 bytes: the 8- and the 32-column
    single pass address a strip through a 32-bit buffer descriptor and must decline (can8 / can32 in
    launch_pack_single_pass_kind); the 16-column pass with its 64-bit addresses takes the call."""
    M = 33
    assert (K * wsh + 8) * 4 >= 1 << 31
    assert fused_pack_path(M, N, K, K, N) == unguarded and fused_pack_path(M, N, K, K, wsh) == "single16"
    X, W = oracle.inputs(M, N, K, 317)
    W[0, ::3] = -1.75
    want = oracle.quantized_mm(X, W)
    buf = torch.empty(K * wsh, device=device)  # about 2.1 GB, not filled: only the view is written
    Wv = buf.view(K, wsh)[:, :N]
    Wv.copy_(torch.from_numpy(W))
    try:
        got = _drop_in_ws(qg, device, _dev(X, device), Wv, M, N, K)
    finally:
        del Wv, buf
        torch.cuda.empty_cache()
    assert_bits_equal(got, want, f"{M}x{N}x{K} W rows of {wsh} floats")
