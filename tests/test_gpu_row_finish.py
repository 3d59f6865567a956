"""gemm_i8_fm's row-finish form (gemm_i8_kernels.h kRowFinish), bit for bit against the CPU oracle.

The form runs the last 4 of a tile's 64-deep k-blocks row group by row group and stores each finished row group under
the next one's MFMAs.  The launcher takes it for unsplit 256-tile plans with an fp32 output on the paired-store path
(unit column stride, row stride a multiple of 4 floats, 16-B aligned base, rows below 64 KiB), a plain / bias /
bias + relu epilogue and k_pad / 64 >= 7 with k_pad a multiple of 128 -- hence at least 8 64-deep k-blocks, K >= 385;
everything else keeps the plain kernel.  The 256-tile plan runs unsplit
from 160 tiles on, so the smallest shape here is 2560 x 4096 (10 x 16 tiles).  Each case asserts its plan through
qgemm_gemm_plan first, so none can pass by missing the kernel.

The C-ABI has no relu without a bias (qgemm_linear: "relu requires a bias"); the epilogue cases are therefore none,
bias and bias + relu -- the kernel's three instantiations.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from util import assert_bits_equal

pytestmark = pytest.mark.gpu

M0, N0 = 2560, 4096


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _plan(qg, m, n, k):
    tile, name = ctypes.c_int(0), ctypes.c_char_p()
    splits = qg.load().qgemm_gemm_plan(m, n, k, ctypes.byref(tile), ctypes.byref(name))
    return tile.value, splits, name.value.decode()


def _assert_plan(qg, m, n, k, row_finish):
    tile, splits, name = _plan(qg, m, n, k)
    assert (tile, splits) == (256, 1), (m, n, k, tile, splits)
    assert ("row-finish" in name) == row_finish, (m, n, k, name)


@functools.lru_cache(maxsize=None)
def _case(m, n, k):
    """Inputs and the oracle's output of one shape, shared by its tests and never changed."""
    from oracle import oracle as O
    X, W = O.inputs(m, n, k, 7000 + k + m)
    X[::7, 0] = -1.5  # the absmax seed quirk and int8 saturation in some rows
    want = O.quantized_mm(X, W)
    want.setflags(write=False)
    return X, W, want


# K pads to 128, so a tile has an even number of 64-deep k-blocks.  384: 6 k-blocks, below the 7 the form needs: the
# plain kernel.  448, 450 (both padded) and 512: 8 k-blocks, the shortest row-finish launch -- 2 prefetching sub-steps
# ahead of the drains and no whole group of three (the loop-free instantiation).  576 (pads to 640), 768, 896: 10, 12,
# 14 k-blocks, one or two groups of three and then the three residues 1, 0, 2 of the set rotation (K = 4096 has residue 1)
@pytest.mark.parametrize("K", [384, 448, 512, 576, 450, 768, 896])
def test_drop_in_k_residues(qg, device, K):
    _assert_plan(qg, M0, N0, K, row_finish=K >= 448)
    X, W, want = _case(M0, N0, K)
    O = torch.full((M0, N0), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, 127.0)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"row finish {M0}x{N0}x{K}")


def test_ragged_edge_tiles(qg, device):
    """2600 x 4000: the last tile row and the last tile column are ragged inside a row-finish launch (11 x 16 tiles)."""
    M, N, K = 2600, 4000, 512
    _assert_plan(qg, M, N, K, row_finish=True)
    X, W, want = _case(M, N, K)
    O = torch.full((M, N), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, 127.0)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"row finish ragged {M}x{N}x{K}")


def test_output_view_row_stride_n_plus_4(qg, device):
    """Row stride N + 4 floats: still 16-B rows, stays on the paired stores; the 4 floats between rows are not written."""
    K = 512
    _assert_plan(qg, M0, N0, K, row_finish=True)
    X, W, want = _case(M0, N0, K)
    buf = torch.full((M0, N0 + 4), float("nan"), device=device)
    O = buf[:, :N0]
    assert O.stride(0) == N0 + 4 and O.data_ptr() % 16 == 0
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, 127.0)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert_bits_equal(np.ascontiguousarray(got[:, :N0]), want, "row finish, output row stride N + 4")
    assert np.isnan(got[:, N0:]).all(), "the gap between output rows was written"


def test_output_base_off_by_one_float(qg, device):
    """A base 4 B past a 16-B boundary falls off the paired stores (and the row-finish form): scalar stores, same bits,
    nothing written in front of or behind the output."""
    K = 512
    X, W, want = _case(M0, N0, K)
    buf = torch.full((M0 * N0 + 8,), float("nan"), device=device)
    assert buf.data_ptr() % 16 == 0
    O = buf[1:1 + M0 * N0].view(M0, N0)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, 127.0)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert_bits_equal(got[1:1 + M0 * N0].reshape(M0, N0), want, "output base off by one float")
    assert np.isnan(got[0]) and np.isnan(got[1 + M0 * N0:]).all(), "written outside the output"


@pytest.mark.parametrize("bias,relu", [(False, False), (True, False), (True, True)])
def test_linear_epilogues(qg, oracle, device, bias, relu):
    """The three epilogue instantiations through qgemm_linear at 2560 x 4096 x 512."""
    K = 512
    _assert_plan(qg, M0, N0, K, row_finish=True)
    X, W, _ = _case(M0, N0, K)
    b = oracle.uniform((N0,), 7100, -0.5, 0.5) if bias else None
    pw = qg.pack_b(_dev(W, device))
    Y = qg.linear(_dev(X, device), pw, bias=None if b is None else _dev(b, device), relu=relu)
    torch.cuda.synchronize()
    assert_bits_equal(Y.cpu().numpy(), oracle.linear(X, W, b, relu), f"row finish linear bias={bias} relu={relu}")


def test_linear_epilogue_ragged(qg, oracle, device):
    """bias + relu on ragged edge tiles of a row-finish launch (the bias image is zero past n)."""
    M, N, K = 2600, 4000, 512
    _assert_plan(qg, M, N, K, row_finish=True)
    X, W, _ = _case(M, N, K)
    b = oracle.uniform((N,), 7101, -0.5, 0.5)
    pw = qg.pack_b(_dev(W, device))
    Y = qg.linear(_dev(X, device), pw, bias=_dev(b, device), relu=True)
    torch.cuda.synchronize()
    assert_bits_equal(Y.cpu().numpy(), oracle.linear(X, W, b, True), "row finish linear ragged bias + relu")


def test_128_tiles_short_k_is_unsplit_row_finish(qg, device):
    """2048 x 4096 x 1024: 128 tiles, but only 8 k-steps of 128 -- gemm_plan splits from 16 k-steps on, so this
    shape runs unsplit (one slice) and takes the row-finish form on half the CUs."""
    M, N, K = 2048, 4096, 1024
    _assert_plan(qg, M, N, K, row_finish=True)
    X, W, want = _case(M, N, K)
    O = torch.full((M, N), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, 127.0)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"row finish {M}x{N}x{K}")


def test_split_shape_keeps_the_split_kernel(qg, device):
    """2048 x 4096 x 2048: 128 tiles, two K slices -- the ticket-first split-K kernel as before, exact."""
    M, N, K = 2048, 4096, 2048
    tile, splits, name = _plan(qg, M, N, K)
    assert (tile, splits) == (256, 2) and "split-K" in name and "row-finish" not in name, (tile, splits, name)
    X, W, want = _case(M, N, K)
    O = torch.full((M, N), float("nan"), device=device)
    qg.op_quantized_mm(_dev(X, device), _dev(W, device), O, 127.0)
    torch.cuda.synchronize()
    assert_bits_equal(O.cpu().numpy(), want, f"split-K {M}x{N}x{K}")
