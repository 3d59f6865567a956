"""GPU parity of qgemm_mm_fp32 on every kernel its selection rule can reach, bit for bit against oracle.mm_fp32, and of
the two batched GEMMs inside qgemm_attention's three launches against attn_oracle / causal_oracle.

Every case first asserts the kernel qgemm_mm_fp32_plan names for its arguments, so a retuned threshold fails the case
instead of emptying it.  Shapes are the smallest that reach a plan at batch 1 (>= 512 tiles of 128 x 128, or >= 512 of
64 x 64 and fewer of 128 x 128), with a one-row tail tile in m and a few-column tail in n.

A, B and C are windows in larger NaN-filled parents: rows past m or n, columns past k, and a guard band on every side
of C.  A read past an edge that reaches a product poisons the output; a store past an edge disturbs the guard band,
which is compared bit for bit afterwards.

K schedule on the LDS-DMA ring (depth NS = 3, 3, 4 for the 128-, 64- and 32x64-tile plans), nk = ceil(k / 32) tiles:
nk in {1, 2, NS - 1, NS, NS + 1} and a larger odd count -- a prologue shorter than the ring, the first slot reuse, both
parities of the two-step unrolled loop -- with k % 32 in {0, 4, 28}.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attn_oracle
import causal_oracle
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000  # torch.full(nan)'s pattern: the parents' fill, compared bit for bit after a call
GUARD = 3              # rows / columns of C's parent on every side of the window
BIG = (2817, 2820)     # 23 x 23 = 529 tiles of 128 x 128
MID = (1409, 1412)     # 23 x 23 = 529 tiles of 64 x 64, 12 x 12 of 128 x 128
SMALL = (33, 68)       # 2 x 2 tiles of the smallest ring plan (32 x 64), 3 x 3 of the smallest staged one (16 x 32)
DMA = {BIG: "mm_f32_dma_128x128", MID: "mm_f32_dma_64x64", SMALL: "mm_f32_dma_32x64"}
MFMA = {BIG: "mm_f32_mfma_128x128", MID: "mm_f32_mfma_64x64", SMALL: "mm_f32_mfma_16x32"}
# (nk, k % 32) per K: 128-tile (NS 3, thinned): (1,4) (2,4) (2,0) (3,28) (4,4) (5,4)
#                     64-tile (NS 3): (1,4) (1,0) (2,4) (2,0) (3,4) (3,28) (4,4) (5,4) (6,4)
#                     32x64 (NS 4): (1,4) (2,4) (2,0) (3,28) (4,0) (5,4) (7,28)
DMA_K = {BIG: (4, 36, 64, 92, 100, 132), MID: (4, 32, 36, 64, 68, 92, 100, 132, 164),
         SMALL: (4, 36, 64, 92, 128, 132, 220)}
MFMA_K = (1, 7, 33, 63, 64, 97)


def _nan_parent(shape, device):
    return torch.full(shape, float("nan"), device=device)


def _dev(host, device):
    return torch.from_numpy(np.array(host, dtype=np.float32, order="C")).to(device)  # a copy: `host` may be read-only


def _window(host, device, transposed=False, r0=0, c0=0, pad_r=2, pad_c=4, ld_mult=4):
    """A device view equal to `host` (R x C) inside a NaN-filled parent.  transposed=False: rows of the parent, stride
    (ld, 1); True: the parent holds host^T and the view is its .t(), stride (1, ld).  The window starts r0 rows and c0
    columns into the parent, which has pad_r more rows and at least pad_c more columns; ld is rounded up to ld_mult."""
    src = host.T if transposed else host
    R, C = src.shape
    ld = -(-(c0 + C + pad_c) // ld_mult) * ld_mult
    parent = _nan_parent((r0 + R + pad_r, ld), device)
    parent[r0:r0 + R, c0:c0 + C] = _dev(src, device)
    view = parent[r0:r0 + R, c0:c0 + C]
    return view.t() if transposed else view


def _plan(qg, A, B):
    m, k = A.shape
    return qg.mm_fp32_plan(m, B.shape[1], k, A.stride(), B.stride(), a_ptr=A.data_ptr(), b_ptr=B.data_ptr())


def _run_checked(qg, oracle, device, X, W, A, B, plan, what, c_transposed=False):
    """Assert the plan, run qgemm_mm_fp32 into a window of a NaN parent, compare the window with the oracle and the
    guard band with the fill."""
    assert _plan(qg, A, B) == plan, f"{what}: plan"
    m, n = X.shape[0], W.shape[1]
    shape = (n + 2 * GUARD, m + 2 * GUARD + 1) if c_transposed else (m + 2 * GUARD, n + 2 * GUARD + 1)
    parent = _nan_parent(shape, device)
    C = parent[GUARD:GUARD + n, GUARD:GUARD + m].t() if c_transposed else parent[GUARD:GUARD + m, GUARD:GUARD + n]
    got = qg.mm_fp32(A, B, C)
    torch.cuda.synchronize()
    assert got is C
    full = parent.cpu().numpy()
    if c_transposed:
        full = full.T
    inner = full[GUARD:GUARD + m, GUARD:GUARD + n]
    assert_bits_equal(inner, oracle.mm_fp32(X, W), what)
    outside = np.ones(full.shape, bool)
    outside[GUARD:GUARD + m, GUARD:GUARD + n] = False
    band = np.ascontiguousarray(full).view(np.uint32)[outside]
    assert (band == NAN_BITS).all(), f"{what}: C's guard band was written"


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K, seed=0):
    from oracle import oracle as O
    X, W = O.inputs(M, N, K, 7000 + seed)
    X.flags.writeable = W.flags.writeable = False
    return X, W


# ---- the LDS-DMA ring: three tiles x two B layouts x the K schedule -------------------------------------------------

def _dma_cases():
    return [pytest.param(shape, K, bkc, id=f"{DMA[shape][11:]}-{'bkc' if bkc else 'bnc'}-k{K}")
            for shape in (BIG, MID, SMALL) for bkc in (False, True) for K in DMA_K[shape]]


@pytest.mark.parametrize("shape,K,bkc", _dma_cases())
def test_dma_ring_k_schedule(qg, oracle, device, shape, K, bkc):
    """A row-major (k % 4 == 0, row stride % 4 == 0, 16-byte aligned window); B row-major or the .t() view of an
    N x K matrix."""
    (M, N) = shape
    X, W = _inputs(M, N, K)
    A = _window(X, device, r0=1, c0=4)
    B = _window(W, device, transposed=bkc, r0=2, c0=8)
    _run_checked(qg, oracle, device, X, W, A, B, f"{DMA[shape]}_{'bkc' if bkc else 'bnc'}",
                 f"dma {M}x{N}x{K} bkc={bkc}")


def _special(rng, M, N, K):
    """test_gpu_parity.test_unquantized_gemm_special_values' recipe: products far below the smallest subnormal (signed
    zeros), rows in the subnormal range, +-inf and NaN operands."""
    X = (rng.uniform(-1, 1, (M, K)) * 1e-20).astype(np.float32)
    W = (rng.uniform(-1, 1, (K, N)) * 1e-20).astype(np.float32)
    W[:, :8] *= np.float32(1e-6)
    X[:4, :] *= np.float32(1e19)
    W[:, N - 3:] *= np.float32(1e-6)   # the same in the ragged last tile
    X[M - 1, :] *= np.float32(1e19)
    X[5, 3] = np.inf
    X[6, 2] = -np.inf
    W[1, 9] = np.nan
    W[2, 11] = np.inf
    X[M - 1, K - 1] = np.inf
    W[K - 1, N - 1] = np.nan
    W[K - 2, N - 2] = -np.inf
    return X, W


@pytest.mark.parametrize("K", [64, 36])
@pytest.mark.parametrize("bkc", [False, True], ids=["bnc", "bkc"])
@pytest.mark.parametrize("shape", [BIG, MID, SMALL], ids=lambda s: DMA[s][11:])
def test_dma_ring_special_values(qg, oracle, device, shape, bkc, K):
    """Subnormal products, -0 results (kept with k % 32 == 0, turned +0 by the padded tail otherwise), +-inf and NaN
    through every ring plan, the ragged last tile included."""
    (M, N) = shape
    X, W = _special(np.random.default_rng(63), M, N, K)
    want = oracle.mm_fp32(X, W)
    assert K % 32 or (np.signbit(want) & (want == 0)).any(), "case should produce -0 results"
    A = _window(X, device, c0=4)
    B = _window(W, device, transposed=bkc)
    _run_checked(qg, oracle, device, X, W, A, B, f"{DMA[shape]}_{'bkc' if bkc else 'bnc'}", f"dma special {M}x{N}x{K}")


# ---- register staging: three tiles x K, and the LDS layouts ---------------------------------------------------------

@pytest.mark.parametrize("K", MFMA_K)
@pytest.mark.parametrize("shape", [BIG, MID, SMALL], ids=lambda s: MFMA[s][12:])
def test_mfma_k_tails(qg, oracle, device, shape, K):
    """Row-major A and B with n % 4 != 0 (so K = 64 stays off the ring too); every other K also has k % 4 != 0."""
    M, N = shape[0], shape[1] - 2
    assert N % 4
    X, W = _inputs(M, N, K)
    A = _window(X, device, r0=1, c0=4)
    B = _window(W, device, r0=2, c0=8)
    _run_checked(qg, oracle, device, X, W, A, B, MFMA[shape], f"mfma {M}x{N}x{K}")


@pytest.mark.parametrize("a_t,b_t", [(True, False), (False, True), (True, True)],
                         ids=["A-colmajor", "B-transposed", "both"])
@pytest.mark.parametrize("shape", [BIG, MID, SMALL], ids=lambda s: MFMA[s][12:])
def test_mfma_lds_layouts(qg, oracle, device, shape, a_t, b_t):
    """A column-major and / or B the .t() view of an N x K matrix: the row-contiguous LDS layout of A (stride TM + 16)
    and the k-contiguous one of B, per tile.  K = 33 keeps the B-transposed case off the ring; C is written through a
    transposed window once as well."""
    M, N, K = shape[0], shape[1] - 2, 33
    X, W = _inputs(M, N, K)
    A = _window(X, device, transposed=a_t, r0=1, c0=3, ld_mult=1)
    B = _window(W, device, transposed=b_t, r0=2, c0=5, ld_mult=1)
    _run_checked(qg, oracle, device, X, W, A, B, MFMA[shape], f"mfma layouts {M}x{N}x{K} A^T={a_t} B^T={b_t}",
                 c_transposed=a_t and b_t)


# ---- each condition of the ring broken alone, on the 64-tile shape --------------------------------------------------

BROKEN = {
    "A base off by 4 bytes": dict(a=dict(c0=5), bkc=False),
    "B base off by 4 bytes": dict(b=dict(c0=9), bkc=False),
    "ash % 4 != 0": dict(a=dict(ld_mult=1, pad_c=5, c0=4), bkc=False),      # ld = 4 + 36 + 5
    "n % 4 != 0, B row-major": dict(n=MID[1] - 2, bkc=False),
    "bsw % 4 != 0, B transposed": dict(b=dict(ld_mult=1, pad_c=5, c0=4), bkc=True),
    "k % 4 != 0": dict(k=37, bkc=False),
    "k % 4 != 0, B transposed": dict(k=37, bkc=True),
}


@pytest.mark.parametrize("bkc", [False, True], ids=["bnc", "bkc"])
def test_ring_conditions_hold_on_the_control(qg, oracle, device, bkc):
    """The windows test_ring_condition_broken_alone starts from do ride the 64-tile ring."""
    X, W = _inputs(*MID, 36)
    A = _window(X, device, c0=4)
    B = _window(W, device, transposed=bkc, c0=8)
    _run_checked(qg, oracle, device, X, W, A, B, f"mm_f32_dma_64x64_{'bkc' if bkc else 'bnc'}", "ring control")


@pytest.mark.parametrize("what", list(BROKEN))
def test_ring_condition_broken_alone(qg, oracle, device, what):
    """One condition of the ring off, all others kept: the plan flips to register staging and the bits still match."""
    c = BROKEN[what]
    M, N, K = MID[0], c.get("n", MID[1]), c.get("k", 36)
    X, W = _inputs(M, N, K)
    A = _window(X, device, **{**dict(c0=4), **c.get("a", {})})
    B = _window(W, device, transposed=c["bkc"], **{**dict(c0=8), **c.get("b", {})})
    # exactly one of the ring's conditions is off
    bkc = B.stride(0) == 1 and B.stride(1) != 1
    conds = [A.data_ptr() % 16 == 0, B.data_ptr() % 16 == 0, A.stride(0) % 4 == 0, K % 4 == 0,
             (B.stride(1) % 4 == 0) if bkc else (B.stride(0) % 4 == 0 and N % 4 == 0)]
    assert bkc == c["bkc"] and A.stride(1) == 1 and conds.count(False) == 1, (what, conds)
    _run_checked(qg, oracle, device, X, W, A, B, "mm_f32_mfma_64x64", f"off the ring: {what}")


# ---- batch strides, through qgemm_attention's three launches --------------------------------------------------------

def _attention_plans(qg, Q, K, V, ws, H, dk):
    """The plans of launch_attention's two launch_mm_f32_batched calls, on exactly its arguments."""
    seq_q, seq_kv = Q.shape[0], K.shape[0]
    qk = qg.mm_fp32_plan(seq_q, seq_kv, dk, (Q.stride(0), 1), (1, K.stride(0)), H, dk, dk, Q.data_ptr(), K.data_ptr())
    pv = qg.mm_fp32_plan(seq_q, dk, seq_kv, (seq_kv, 1), (V.stride(0), 1), H, seq_q * seq_kv, dk, ws.data_ptr(),
                         V.data_ptr())
    return qk, pv


# (seq_q, seq_kv, H, d_k, q_pos0 or None, the Q K^T plan, the P V plan)
ATTENTION = [
    (129, 516, 52, 8, None, "mm_f32_dma_128x128_bkc", "mm_f32_dma_32x64_bnc"),
    (129, 516, 172, 4, None, "mm_f32_dma_128x128_bkc", "mm_f32_dma_64x64_bnc"),
    (129, 516, 256, 4, None, "mm_f32_dma_128x128_bkc", "mm_f32_dma_128x128_bnc"),
    (129, 513, 52, 5, None, "mm_f32_mfma_128x128", "mm_f32_mfma_16x32"),
    (129, 513, 172, 5, None, "mm_f32_mfma_128x128", "mm_f32_mfma_64x64"),
    (129, 513, 256, 5, None, "mm_f32_mfma_128x128", "mm_f32_mfma_128x128"),
    # causal: query row i sees keys 0 .. i + 300, so the mask's edge runs through the 128-wide score tiles 2, 3 and 4
    (129, 516, 52, 8, 300, "mm_f32_dma_128x128_bkc", "mm_f32_dma_32x64_bnc"),
]


def _attention_id(c):
    return f"{c[1]}keys-H{c[2]}-dk{c[3]}" + ("-causal" if c[4] is not None else "")


@pytest.mark.parametrize("seq_q,seq_kv,H,dk,q_pos0,qk_plan,pv_plan", ATTENTION,
                         ids=[_attention_id(c) for c in ATTENTION])
def test_attention_three_launches_batched_plans(qg, oracle, device, seq_q, seq_kv, H, dk, q_pos0, qk_plan, pv_plan):
    """Heads as the batch (blockIdx.z, a_bs / b_bs / c_bs) on the larger plans: Q, K, V and O are column windows of
    NaN-filled parents, the scores workspace is 0xFF bytes, the call goes through the C entry point."""
    d = H * dk
    assert qg.attention_plan(seq_q, seq_kv, H, dk) == "three_launches"
    Qh, Kh, Vh = (oracle.uniform((r, d), 9100 + i) for i, r in enumerate((seq_q, seq_kv, seq_kv)))
    Q, K, V = (_window(a, device, c0=4, pad_c=4) for a in (Qh, Kh, Vh))
    need = qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk)
    assert need == 4 * H * seq_q * seq_kv
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=device)
    assert _attention_plans(qg, Q, K, V, ws, H, dk) == (qk_plan, pv_plan)
    parent = _nan_parent((seq_q + 2 * GUARD, d + 2 * GUARD + 2), device)
    O = parent[GUARD:GUARD + seq_q, GUARD:GUARD + d]
    scale = attn_oracle.default_scale(dk)
    s = torch.cuda.current_stream(device).cuda_stream
    L = qg.load()
    args = (Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0), O.data_ptr(), O.stride(0),
            seq_q, seq_kv, H, dk, scale)
    if q_pos0 is None:
        rc = L.qgemm_attention(*args, ws.data_ptr(), need, s)
        want = attn_oracle.attention_ref(Qh, Kh, Vh, H, scale)
    else:
        rc = L.qgemm_attention_causal(*args, q_pos0, ws.data_ptr(), need, s)
        want = causal_oracle.attention_causal_ref(Qh, Kh, Vh, H, scale, q_pos0)
    assert rc == 0
    torch.cuda.synchronize()
    full = parent.cpu().numpy()
    assert_bits_equal(full[GUARD:GUARD + seq_q, GUARD:GUARD + d], want, f"attention {seq_q}x{seq_kv} H={H} d_k={dk}")
    outside = np.ones(full.shape, bool)
    outside[GUARD:GUARD + seq_q, GUARD:GUARD + d] = False
    assert (full.view(np.uint32)[outside] == NAN_BITS).all(), "O's guard band was written"


# ---- the stride envelope: right bits or an error, never silent zeros ------------------------------------------------

def _raw_mm(qg, device, a_ptr, a_st, b_ptr, b_st, C, c_ptr, c_st, m, n, k):
    rc = qg.load().qgemm_mm_fp32(a_ptr, a_st[0], a_st[1], b_ptr, b_st[0], b_st[1], c_ptr, c_st[0], c_st[1], m, n, k,
                                 torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize()
    return rc, C.cpu().numpy()


def _bits_or_refusal(rc, got, want, what):
    """The envelope's rule: the oracle's bits, or a non-zero return code with C left as it was (NaN-filled)."""
    if rc == 0:
        assert_bits_equal(got, want, what)
    else:
        assert (got.view(np.uint32) == NAN_BITS).all(), f"{what}: refused with {rc}, but C was written"


# (rows, row stride in floats, the plan): the last row starts just inside / just past 2^31 bytes from the first
ROW_STRIDES = [
    pytest.param(16, 35791390, "mm_f32_mfma_16x32", True, id="16rows-inside"),   # 15 * s * 4 + 32 = 2^31 - 216
    pytest.param(16, 35791395, "mm_f32_mfma_16x32", False, id="16rows-past"),    # 15 * s * 4 = 2^31 + 52
    pytest.param(32, 17318412, "mm_f32_dma_32x64_bnc", True, id="32rows-inside"),  # 31 * s * 4 + 32 = 2^31 - 528
    pytest.param(32, 17318420, "mm_f32_dma_32x64_bnc", False, id="32rows-past"),   # 31 * s * 4 = 2^31 + 432
]


@pytest.mark.parametrize("rows,stride,plan,inside", ROW_STRIDES)
def test_row_stride_reaching_2_31_bytes(qg, oracle, device, rows, stride, plan, inside):
    """A's rows lie `stride` floats apart in one 2.3-GB buffer that really spans them (unfilled but for the rows used).
    Just inside the envelope the call must work; just past it, it gives the oracle's bits or refuses, C untouched."""
    k, n = 8, 24
    X, W = _inputs(rows, n, k, seed=1)
    buf = torch.empty(rows * stride, device=device)
    A = buf.as_strided((rows, k), (stride, 1))
    A.copy_(_dev(X, device))
    B = _dev(W, device)
    assert (rows - 1) * stride * 4 + k * 4 < 2 ** 31 if inside else (rows - 1) * stride * 4 >= 2 ** 31
    assert _plan(qg, A, B) == plan
    C = _nan_parent((rows, n), device)
    rc, got = _raw_mm(qg, device, A.data_ptr(), A.stride(), B.data_ptr(), B.stride(), C, C.data_ptr(), C.stride(), rows,
                      n, k)
    del buf, A
    if inside:
        assert rc == 0, "a stride inside the envelope was refused"
    _bits_or_refusal(rc, got, oracle.mm_fp32(X, W), f"A row stride {stride}, {rows} rows")


@pytest.mark.parametrize("which", ["A rows", "A columns", "B rows", "B columns", "C rows", "C columns"])
@pytest.mark.parametrize("aligned", [False, True], ids=["k7", "k8-aligned"])
def test_negative_stride_through_the_raw_abi(qg, oracle, device, which, aligned):
    """One operand walked backwards: the pointer at its last row (or column) and a negative stride, inside a buffer
    that spans every element addressed.  aligned: everything else meets the ring's conditions."""
    m, n, k = 32, 64, 8 if aligned else 7
    X, W = _inputs(m, n, k, seed=2)
    want = oracle.mm_fp32(X, W)
    dev = {"A": _dev(X, device), "B": _dev(W, device), "C": _nan_parent((m, n), device)}
    ptr = {nm: t.data_ptr() for nm, t in dev.items()}
    st = {nm: list(t.stride()) for nm, t in dev.items()}
    nm, axis = which[0], 0 if which.endswith("rows") else 1
    t = dev[nm]
    if nm != "C":  # store the operand flipped, so the backwards walk reads the logical matrix
        t.copy_(torch.flip(t, dims=(axis,)))
    ptr[nm] += 4 * (t.shape[axis] - 1) * t.stride(axis)
    st[nm][axis] = -t.stride(axis)
    # the ring demands ash, bsh, bsw >= 0 and unit asw; C's strides are not read by the selection
    plan = qg.mm_fp32_plan(m, n, k, st["A"], st["B"], a_ptr=ptr["A"], b_ptr=ptr["B"])
    assert plan == ("mm_f32_dma_32x64_bnc" if aligned and nm == "C" else "mm_f32_mfma_16x32")
    rc, got = _raw_mm(qg, device, ptr["A"], st["A"], ptr["B"], st["B"], dev["C"], ptr["C"], st["C"], m, n, k)
    if rc == 0 and nm == "C":
        got = np.flip(got, axis=axis)
    _bits_or_refusal(rc, got, want, f"negative stride on {which}")


@pytest.mark.parametrize("which", ["Q", "K", "V", "O"])
def test_attention_three_launches_negative_row_stride(qg, oracle, device, which):
    """The same through qgemm_attention outside the fused envelope (d_k = 65): the oracle's bits or a refusal before
    the first launch, O untouched."""
    seq_q, seq_kv, H, dk = 20, 40, 1, 65
    Qh, Kh, Vh = (oracle.uniform((r, dk), 9300 + i) for i, r in enumerate((seq_q, seq_kv, seq_kv)))
    scale = attn_oracle.default_scale(dk)
    want = attn_oracle.attention_ref(Qh, Kh, Vh, H, scale)
    dev = {"Q": _dev(Qh, device), "K": _dev(Kh, device), "V": _dev(Vh, device), "O": _nan_parent((seq_q, dk), device)}
    ptr = {nm: t.data_ptr() for nm, t in dev.items()}
    ld = {nm: t.stride(0) for nm, t in dev.items()}
    t = dev[which]
    if which != "O":
        t.copy_(torch.flip(t, dims=(0,)))
    ptr[which] += 4 * (t.shape[0] - 1) * t.stride(0)
    ld[which] = -t.stride(0)
    need = qg.load().qgemm_attention_workspace_size(seq_q, seq_kv, H, dk)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=device)
    assert qg.attention_plan(seq_q, seq_kv, H, dk) == "three_launches"
    for plan in (qg.mm_fp32_plan(seq_q, seq_kv, dk, (ld["Q"], 1), (1, ld["K"]), H, dk, dk, ptr["Q"], ptr["K"]),
                 qg.mm_fp32_plan(seq_q, dk, seq_kv, (seq_kv, 1), (ld["V"], 1), H, seq_q * seq_kv, dk, ws.data_ptr(),
                                 ptr["V"])):
        assert plan == "mm_f32_mfma_16x32"   # k = 65 and ldv = 65 keep both GEMMs off the ring
    rc = qg.load().qgemm_attention(ptr["Q"], ld["Q"], ptr["K"], ld["K"], ptr["V"], ld["V"], ptr["O"], ld["O"], seq_q,
                                   seq_kv, H, dk, scale, ws.data_ptr(), need,
                                   torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize()
    got = dev["O"].cpu().numpy()
    if rc == 0 and which == "O":
        got = np.flip(got, axis=0)
    _bits_or_refusal(rc, got, want, f"attention, negative row stride on {which}")
    if rc:
        assert (ws.cpu().numpy() == 0xFF).all(), "refused, but the scores were written: a launch came first"
