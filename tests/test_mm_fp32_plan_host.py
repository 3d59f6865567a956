"""qgemm_mm_fp32_plan without a GPU: the query is declared, exported and listed; over a sweep of shapes, batches and
stride sets it returns exactly the nine documented kernel names, every one of them for some input, and each answer is
the one a restatement of the selection rule gives; and the 32 x 32 single-wave step the rule once had between its last
two register-staged plans can be reached by no input.  (The stride envelope is tested on the GPU, on buffers that
really span the strides: tests/test_gpu_mm_fp32.py.)"""
import ctypes
import itertools
import re
import subprocess

import numpy as np
import pytest

INVALID = 1  # hipErrorInvalidValue

DMA_TILES = ("128x128", "64x64", "32x64")
MFMA_TILES = ("128x128", "64x64", "16x32")
DOCUMENTED = frozenset([f"mm_f32_dma_{t}_{b}" for t in DMA_TILES for b in ("bkc", "bnc")] +
                       [f"mm_f32_mfma_{t}" for t in MFMA_TILES])
WANT_WAVES = 2048  # the rule's kWant: two waves on every SIMD (4 x 256 CUs x 2)

BATCHES = (1, 2, 16, 52, 172, 256)


COARSE = (1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 17, 20, 24, 40, 48, 100, 200, 500, 1000, 1409, 1412, 2000, 2817, 2820, 3000,
          4000, 4200)


def _dims(batch=1):
    """1 .. 4200: a coarse grid plus the two neighbours of every multiple of 32 (they straddle every tile edge of
    every plan; the multiples of 4 that B row-major needs for the ring are in the coarse grid).  From batch 16 on
    every pair past 1024 x 1024 is deep inside the 128-tile plans (64 tiles x 16 x 4 waves), so the neighbours stop
    at 1100 there and the coarse grid alone goes on: the sweep stays at a few seconds."""
    top = 4200 if batch < 16 else 1100
    near = [32 * j + d for j in range(1, top // 32 + 1) for d in (-1, 1)]
    return np.array(sorted({v for v in COARSE + tuple(near) if 1 <= v <= 4200}), dtype=np.int64)


# (label, a_stride(m, n, k), b_stride(m, n, k), a_ptr, b_ptr, a_bs, b_bs, k, fast, bkc): what the selection reads
# besides m, n and batch.  Strides in floats; the pointers are integers with the alignment wanted (never dereferenced).
STRIDE_SETS = [
    ("fast, B row-major", lambda m, n, k: (k + 4, 1), lambda m, n, k: (n + 4 - n % 4, 1), 256, 512, 8, 12, 36, True,
     False),
    ("fast, B transposed", lambda m, n, k: (k, 1), lambda m, n, k: (1, k + 8), 1024, 16, 0, 0, 64, True, True),
    ("k % 4 != 0", lambda m, n, k: (k + 3, 1), lambda m, n, k: (n + 4 - n % 4, 1), 256, 512, 8, 12, 33, False, False),
    ("A column-major", lambda m, n, k: (1, m), lambda m, n, k: (n + 4 - n % 4, 1), 256, 512, 0, 0, 36, False, False),
    ("A base off by 4 bytes", lambda m, n, k: (k, 1), lambda m, n, k: (1, k), 1028, 16, 0, 0, 64, False, True),
    ("B base off by 8 bytes", lambda m, n, k: (k, 1), lambda m, n, k: (1, k), 1024, 24, 0, 0, 64, False, True),
    ("ash % 4 != 0", lambda m, n, k: (k + 1, 1), lambda m, n, k: (1, k), 1024, 16, 0, 0, 64, False, True),
    ("bsw % 4 != 0, B transposed", lambda m, n, k: (k, 1), lambda m, n, k: (1, k + 2), 1024, 16, 0, 0, 64, False, True),
    ("a_bs % 4 != 0", lambda m, n, k: (k, 1), lambda m, n, k: (1, k), 1024, 16, 6, 0, 64, False, True),
    ("b_bs % 4 != 0", lambda m, n, k: (k, 1), lambda m, n, k: (1, k), 1024, 16, 0, 5, 64, False, True),
]


def _expected(m, n, batch, fast, bkc):
    """The selection rule restated on arrays m (column) x n (row): the names as an object array."""
    up = lambda a, t: (a + t - 1) // t  # noqa: E731
    w128 = up(m, 128) * up(n, 128) * batch * 4
    w64 = up(m, 64) * up(n, 64) * batch * 4
    tile = np.where(w128 >= WANT_WAVES, 0, np.where(w64 >= WANT_WAVES, 1, 2))
    if np.ndim(fast) == 0:
        fast = np.full(tile.shape, bool(fast))
    dma = np.array([f"mm_f32_dma_{t}_{'bkc' if bkc else 'bnc'}" for t in DMA_TILES], dtype=object)
    mfma = np.array([f"mm_f32_mfma_{t}" for t in MFMA_TILES], dtype=object)
    return np.where(fast, dma[tile], mfma[tile])


def test_plan_symbol_is_declared_exported_and_listed(qg):
    header = open(qg.HEADER_PATH).read()
    declared = re.findall(r"^QGEMM_API\s+[\w\s\*]+?\b((?:op_|qgemm_)\w+)\s*\(", header, flags=re.M)
    nm = subprocess.run(["nm", "-D", "--defined-only", qg.LIB_PATH], check=True, capture_output=True, text=True).stdout
    sym = "qgemm_mm_fp32_plan"
    assert sym in declared and sym in qg.EXPORTED_SYMBOLS
    assert re.search(rf" T {sym}$", nm, flags=re.M), f"{sym} not exported by libqgemm.so"
    assert qg.load().qgemm_mm_fp32_plan.argtypes
    for name in DOCUMENTED:
        assert name in header, f"{name} is not in include/qgemm.h's list"


def test_plan_sweep_returns_exactly_the_documented_kernels(qg):
    """m, n over the grid, every batch, every stride set: the set of names is the documented nine, each is returned,
    and each answer is the restated rule's."""
    f = qg.load().qgemm_mm_fp32_plan
    name = ctypes.c_char_p()
    ref = ctypes.byref(name)
    seen = set()
    for s, (label, a_st, b_st, a_ptr, b_ptr, a_bs, b_bs, k, fast, bkc) in enumerate(STRIDE_SETS):
        for batch in BATCHES:
            # the first three sets (the ring with either B layout, register staging) on the whole grid; the other
            # ways off the ring, which change nothing but `fast`, on the coarse grid
            dims = _dims(batch) if s < 3 else np.array(COARSE, dtype=np.int64)
            M, N = dims[:, None], dims[None, :]
            ints = [int(v) for v in dims]
            got = np.empty((len(ints), len(ints)), dtype=object)
            for (i, m), (j, n) in itertools.product(enumerate(ints), enumerate(ints)):
                (ash, asw), (bsh, bsw) = a_st(m, n, k), b_st(m, n, k)
                assert f(m, n, k, batch, a_ptr, ash, asw, a_bs, b_ptr, bsh, bsw, b_bs, ref) == 0
                got[i, j] = name.value
            # B row-major rides the ring only with n % 4 == 0
            is_fast = (N % 4 == 0) & np.ones_like(M, bool) if fast and not bkc else fast
            want = _expected(M, N, batch, is_fast, bkc)
            bad = np.argwhere(got != np.vectorize(str.encode)(want.astype(str)))
            if len(bad):
                i, j = bad[0]
                raise AssertionError(f"{label}, batch {batch}, {ints[i]} x {ints[j]}: {got[i, j]}, want {want[i, j]}")
            seen |= {v.decode() for v in np.unique(got)}
    assert seen == DOCUMENTED, (sorted(seen - DOCUMENTED), sorted(DOCUMENTED - seen))


def test_the_32x32_single_wave_step_is_unreachable():
    """The rule once asked waves(32, 32, 1) >= 2048 after waves(64, 64, 4) >= 2048 had failed.  ceil(x / 32) <=
    2 ceil(x / 64), so waves(32, 32, 1) <= waves(64, 64, 4) everywhere: checked on the whole sweep, and on every
    m, n up to 4200 at batch 1."""
    up = lambda a, t: (a + t - 1) // t  # noqa: E731
    for dims in (_dims(), np.arange(1, 4201, dtype=np.int64)):
        M, N = dims[:, None], dims[None, :]
        for batch in BATCHES if dims.size < 1000 else (1,):
            w32 = up(M, 32) * up(N, 32) * batch
            w64 = up(M, 64) * up(N, 64) * batch * 4
            assert (w32 <= w64).all()
            assert not ((w32 >= WANT_WAVES) & (w64 < WANT_WAVES)).any()


def test_plan_reads_the_attention_gemms_arguments(qg):
    """The two batched GEMMs of a three-launch attention, as launch_attention passes them (Q K^T: B is the transposed
    view of K; P V: A is the scores): a 16-head forward at 2048 rows takes the 128-tile ring for Q K^T and the 64-tile
    ring for P V."""
    seq, H, dk = 2048, 16, 64
    d = H * dk
    assert qg.mm_fp32_plan(seq, seq, dk, (d, 1), (1, d), H, dk, dk) == "mm_f32_dma_128x128_bkc"
    assert qg.mm_fp32_plan(seq, dk, seq, (seq, 1), (d, 1), H, seq * seq, dk) == "mm_f32_dma_64x64_bnc"
    assert qg.mm_fp32_plan(seq, dk, seq, (seq, 1), (d, 1), H, seq * seq, dk, b_ptr=4) == "mm_f32_mfma_64x64"


def test_plan_argument_checks(qg):
    L = qg.load()
    name = ctypes.c_char_p()
    for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 1), (4, 4, 4, 0), (-1, 4, 4, 1)):
        assert L.qgemm_mm_fp32_plan(*bad, 0, 4, 1, 0, 0, 4, 1, 0, ctypes.byref(name)) == INVALID, bad
        with pytest.raises(qg.QGemmError):
            qg.mm_fp32_plan(*bad[:3], (4, 1), (4, 1), batch=bad[3])
    assert L.qgemm_mm_fp32_plan(4, 4, 4, 1, 0, 4, 1, 0, 0, 4, 1, 0, None) == 0  # the name is optional
