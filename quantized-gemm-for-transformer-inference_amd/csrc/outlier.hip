// outlier.hip -- LLM.int8() mixed-precision decomposition: the feature columns of X
// that hold an outlier are multiplied in fp32, the rest through the int8 absmax path, so the outliers
// no longer set the row scales Cx.  The reference carries only the building blocks, unused:
// op_outlier_extractor / AbsCompareLTEConstFunc (op_elemwise.cuh:293-306, 698-708) and op_round_int8
// (:167-176, 685-695).  Definition (DESIGN.md "Outlier decomposition"; the oracle restates it):
//   outlier column k  : some X[i,k] is not (|x| <= t)  -- AbsCompareLTEConstFunc returns 1 (NaN: 1)
//   O8  = op_quantized_mm(X', W'), X' = X with the outlier columns zeroed, W' = W with those rows zeroed
//   Co  = fmaf chain from +0 over the outlier columns in ascending k: X[i,k] * W[k,j]
//   O   = fl(O8 + Co)            (no outlier columns: O = O8, the plain path)
//
// One call, fast path (row-major operands on the single-pass pack + 256-tile GEMM): three launches --
//   outlier_colmask: X read once; workgroup (w, p) reads columns 32 w .. +31 over row split p and writes mask word w
//                    of that split with one plain store (2 splits at K = 4096) -- every word written every
//                    call, so no state lives on between calls (no counters, no accumulator, no zeroing)
//   the pack       : the single pass with the mask (pack.hip): X'/W' quantized without materialising them, every
//                    thread reading the mask words of its own elements; its workgroup 0 writes the outlier count
//                    and the ascending column list
//   the GEMM       : the int8 part with the fp32 chain added in its store epilogue (gemm_i8_kernels.h), its
//                    operands read from X's outlier columns and W's outlier rows where they lie
// Other shapes (the fallback): the same outlier_colmask launch (scalar loads where X's rows are not 16-B pieces), a
// one-workgroup index launch (mask words, count and list: outlier_column_list, the packs' builder), X'/W' materialised
// by a masking pass, the plain drop-in on them, and a correction kernel adding the chain to O.  No outlier kernel waits
// on, counts, or reads another workgroup's writes within a launch.
#include <algorithm>

#include "qgemm_internal.h"

namespace qgemm {

namespace {

// AbsCompareLTEConstFunc (op_elemwise.cuh:296-304): 0 when a in [-b, b], else 1 (NaN -> 1)
__device__ __forceinline__ bool is_outlier(float a, float b) {
    return !(((a >= 0) & (a <= b)) | ((a <= 0) & (-a <= b)));
}

// The column mask with no cross-workgroup combine -- the only kernel that reads X for outliers.  Workgroup (w, p) owns
// mask word w (columns 32 w .. +31) over row split p (rows [p rps, (p + 1) rps)): 1024 threads, thread t reads the 16-B
// piece t & 7 of rows (t >> 3) + 128 i (a wave-instruction = 8 rows x 128 B; 16 loads in flight per thread), ORs its
// nibbles, the 128 row-threads of each piece meet by shuffles and LDS, and ONE plain store writes partial[p][w].  Every
// partial word is written every call: no counters, no accumulator, nothing kept between calls (2 splits at K = 4096:
// the pack ORs two words per mask word).  VEC: one float4 per piece (K % 4 == 0, 16-B aligned rows: x_vec_ok); else
// the same thread-to-(row, piece) map with scalar loads of the piece's columns below k.
constexpr int kScanThreads = 1024;
constexpr int kColmaskRowsPerPass = kScanThreads / 8;  // 128
template <bool VEC>
__global__ __launch_bounds__(kScanThreads) void outlier_colmask_kernel(const float *__restrict__ X, int64_t xsh, int m,
                                                                       int k, float t, int rps,
                                                                       uint32_t *__restrict__ partial, int nwords) {
    __shared__ uint32_t nibs[kScanThreads / 64][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, piece = tid & 7;
    const int c = blockIdx.x * 32 + 4 * piece;
    const int r0 = blockIdx.y * rps, r1 = min(m, r0 + rps);
    uint32_t nib = 0;
    if (c < k) {
        const float *p = X + (int64_t)(r0 + (tid >> 3)) * xsh + c;
        const int64_t step = (int64_t)kColmaskRowsPerPass * xsh;
        if constexpr (VEC) {
#pragma unroll 16
            for (int r = r0 + (tid >> 3); r < r1; r += kColmaskRowsPerPass, p += step) {
                const float4 x = *reinterpret_cast<const float4 *>(p);
                nib |= (is_outlier(x.x, t) ? 1u : 0u) | (is_outlier(x.y, t) ? 2u : 0u) | (is_outlier(x.z, t) ? 4u : 0u) |
                       (is_outlier(x.w, t) ? 8u : 0u);
            }
        } else {
            for (int r = r0 + (tid >> 3); r < r1; r += kColmaskRowsPerPass, p += step)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < k && is_outlier(p[e], t)) nib |= 1u << e;
        }
    }
    // the wave's 8 row-threads of each piece (lane bits 3..5), then the 16 waves
    nib |= (uint32_t)__shfl_xor((int)nib, 8, 64);
    nib |= (uint32_t)__shfl_xor((int)nib, 16, 64);
    nib |= (uint32_t)__shfl_xor((int)nib, 32, 64);
    if (lane < 8) nibs[wave][lane] = nib;
    __syncthreads();
    if (tid < 8) {
        uint32_t x = 0u;
#pragma unroll
        for (int v = 0; v < kScanThreads / 64; ++v) x |= nibs[v][tid];
        uint32_t word = x << (4 * tid);
        word |= (uint32_t)__shfl_xor((int)word, 1, 64);
        word |= (uint32_t)__shfl_xor((int)word, 2, 64);
        word |= (uint32_t)__shfl_xor((int)word, 4, 64);
        if (tid == 0) partial[(int64_t)blockIdx.y * nwords + blockIdx.x] = word;
    }
}

// the row splits: about 256 workgroups for the stream (128 at K = 4096 read 64 MiB in 16.0 us, 256 in
// 11.x), each split a multiple of 128 rows, at most 16
int colmask_splits(int m, int nwords, int *rps) {
    int splits = std::min(16, std::max(1, (256 + nwords - 1) / nwords));
    splits = std::min(splits, std::max(1, (m + kColmaskRowsPerPass - 1) / kColmaskRowsPerPass));
    *rps = (int)round_up((m + splits - 1) / splits, kColmaskRowsPerPass);
    return (m + *rps - 1) / *rps;
}

// (fallback) the mask words bits[w], the count and the ascending column list from the partial words of the launch
// before it: one workgroup, the packs' builder in passes of 1024 words
__global__ __launch_bounds__(kScanThreads) void outlier_index_kernel(OutlierMask om, uint32_t *__restrict__ bits) {
    __shared__ int wsum[kScanThreads / 64];
    outlier_column_list<true>(om, wsum, bits);
}

__device__ __forceinline__ bool bit_of(const uint32_t *bits, int64_t c) { return (bits[c >> 5] >> (c & 31)) & 1u; }

// X' (outlier columns zeroed) and W' (outlier rows zeroed), contiguous outputs; block = one row of X (the
// first m blocks) or of W
__global__ __launch_bounds__(256) void outlier_mask_kernel(const float *__restrict__ X, int64_t xsh, int m, int k,
                                                           const float *__restrict__ W, int64_t wsh, int n,
                                                           const uint32_t *__restrict__ bits, float *__restrict__ Xm,
                                                           float *__restrict__ Wm) {
    const int64_t row = blockIdx.x;
    if (row < m) {
        for (int c = threadIdx.x; c < k; c += 256) Xm[row * k + c] = bit_of(bits, c) ? 0.0f : X[row * xsh + c];
    } else {
        const int64_t r = row - m;
        const bool z = bit_of(bits, r);
        for (int c = threadIdx.x; c < n; c += 256) Wm[r * n + c] = z ? 0.0f : W[r * wsh + c];
    }
}

// (fallback) O[i,j] = fl(O[i,j] + Co[i,j]) -- skipped at count 0 -- then fl(+ b[j]), then relu: Co the fmaf chain from
// +0 over the outlier columns in ascending k of X[i,k] * w[k,j].  kPacked = false: w[k,j] = W[k * wld + j], the fp32
// weight.  kPacked = true: w[k,j] = Wd[k,j] = dequant_w of the packed weight's own byte (W: n_pad x k_pad
// fragment-major int8, wld = k_pad) and its scale Cw[j].  One thread per output (j fastest), rows strided over
// gridDim.y.
template <bool kPacked>
__global__ __launch_bounds__(256) void outlier_finish_kernel(const float *__restrict__ X, int64_t xsh,
                                                             const void *__restrict__ W, int64_t wld,
                                                             const float *__restrict__ Cw,
                                                             const int *__restrict__ idx,
                                                             const int *__restrict__ count,
                                                             const float *__restrict__ bias, int relu,
                                                             float *__restrict__ O, int64_t osh, int m, int n) {
    const int cnt = *count;
    if (cnt == 0 && !bias) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float cw = 0.0f;
    if constexpr (kPacked) cw = Cw[j];
    for (int i = blockIdx.y; i < m; i += gridDim.y) {
        float o = O[(int64_t)i * osh + j];
        if (cnt > 0) {
            float acc = 0.0f;
            for (int t = 0; t < cnt; ++t) {
                const int c = idx[t];
                float w;
                if constexpr (kPacked) w = dequant_w(static_cast<const int8_t *>(W)[fofs(j, c, wld)], cw);
                else w = static_cast<const float *>(W)[(int64_t)c * wld + j];
                acc = __fmaf_rn(X[(int64_t)i * xsh + c], w, acc);
            }
            o = __fadd_rn(o, acc);
        }
        if (bias) o = __fadd_rn(o, bias[j]);
        if (relu) o = (o < 0.0f) ? 0.0f : o;
        O[(int64_t)i * osh + j] = o;
    }
}

size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

// The caller's outlier scratch, [idx: count + list, k + 1 ints][partial][bits][X'][W']: the count's offset depends on
// nothing (qgemm_outlier_count), and W' comes last (a prepacked weight needs none).  scratch_view alone knows the
// layout: the sizes below are read off it.
struct OutlierScratch {
    int *idx;                  // idx[0] = count, idx[1 ..] = the outlier columns ascending
    uint32_t *partial, *bits;  // the column-mask launch's splits x nwords words; their ORs, nwords (fallback)
    float *xm, *wm;            // X' / W' (fallback)
    int nwords, splits, rps;   // the column-mask launch's grid (nwords, splits) and its rows per split
    size_t w_off;              // W''s offset: the bytes of a scratch without it
};

OutlierScratch scratch_view(void *scratch, int m, int k) {
    OutlierScratch v;
    v.nwords = (k + 31) / 32;
    v.splits = colmask_splits(std::max(m, 1), v.nwords, &v.rps);
    const uintptr_t base = reinterpret_cast<uintptr_t>(scratch);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const uintptr_t p = base + o;
        o += a256(bytes);
        return p;
    };
    v.idx = reinterpret_cast<int *>(take(sizeof(int) * ((size_t)k + 1)));
    v.partial = reinterpret_cast<uint32_t *>(take(sizeof(uint32_t) * (size_t)v.splits * v.nwords));
    v.bits = reinterpret_cast<uint32_t *>(take(sizeof(uint32_t) * v.nwords));
    v.xm = reinterpret_cast<float *>(take(sizeof(float) * (size_t)m * k));
    v.wm = reinterpret_cast<float *>(take(0));
    v.w_off = o;
    return v;
}

bool x_vec_ok(const float *X, int64_t xsh, int k) {
    return (k % 4 == 0) && (xsh % 4 == 0) && (reinterpret_cast<uintptr_t>(X) % 16 == 0);
}

// the column-mask launch into v.partial, by float4 pieces where X allows them
hipError_t launch_colmask(const float *X, int64_t xsh, int m, int k, float t, const OutlierScratch &v, hipStream_t s) {
    const dim3 grid((unsigned)v.nwords, (unsigned)v.splits);
    if (x_vec_ok(X, xsh, k))
        outlier_colmask_kernel<true><<<grid, kScanThreads, 0, s>>>(X, xsh, m, k, t, v.rps, v.partial, v.nwords);
    else
        outlier_colmask_kernel<false><<<grid, kScanThreads, 0, s>>>(X, xsh, m, k, t, v.rps, v.partial, v.nwords);
    return hipGetLastError();
}

// the fast paths' scan: the masked packs read at most 128 mask words by float4-aligned pieces (K <= 4096);
// hipErrorNotSupported (nothing launched) outside that
hipError_t launch_colmask_fast(const float *X, int64_t xsh, int m, int k, float t, const OutlierScratch &v,
                               hipStream_t s) {
    if (v.nwords > 128 || !x_vec_ok(X, xsh, k)) return hipErrorNotSupported;
    return launch_colmask(X, xsh, m, k, t, v, s);
}

}  // namespace

size_t outlier_linear_scratch_bytes(int m, int k) { return scratch_view(nullptr, m, k).w_off; }

size_t outlier_scratch_bytes(int m, int n, int k) {
    return outlier_linear_scratch_bytes(m, k) + a256(sizeof(float) * (size_t)k * (size_t)round_up(n, 256));
}

// Fast path: the partial masks, the masked single-pass pack (mask, count and column list), the 256-tile GEMM with the
// fp32 chain in its epilogue.  hipErrorNotSupported (nothing launched) outside its envelope.
hipError_t outlier_fast(const float *X, const float *W, float *O, int m, int n, int k, float t, void *scratch,
                        PackedView va, PackedView vb, float range, hipStream_t s) {
    if (!gemm_outlier_ok(m, n, (int)va.k_pad) || !pack_single_pass_outlier_ok(X, k, m, k, W, n, n)) return hipErrorNotSupported;
    const OutlierScratch v = scratch_view(scratch, m, k);
    hipError_t e = launch_colmask_fast(X, k, m, k, t, v, s);
    if (e != hipSuccess) return e;
    e = launch_pack_single_pass_outlier(X, k, m, k, va, W, n, n, vb, range, v.partial, v.splits, v.nwords, v.idx, s);
    if (e == hipErrorNotSupported) return hipErrorUnknown;  // the mask already enqueued: the envelope checks disagree
    if (e != hipSuccess) return e;
    const float inv_r2 = 1.0f / (range * range);
    // the fp32 chain reads the outlier columns of X and rows of W where they lie (the column list idx + 1); a compact
    // copy of X's outlier values written by the pack measured slower (profiles/r05_maskpack_lab_xo_staged.log)
    return launch_gemm_dequant_outlier(va, vb, O, n, m, n, inv_r2, X, k, W, n, v.idx + 1, v.idx, s);
}

// Prepacked weight, fast path: the partial masks, the masked X-only pack (mask, count and column list), the 256-tile
// GEMM with the chain on the weight's dequantized rows (+ bias / relu) in its epilogue.  hipErrorNotSupported (nothing
// launched) outside its envelope.
hipError_t outlier_linear_fast(const float *X, int64_t xsh, int m, int n, int k, float t, void *scratch, PackedView va,
                               PackedView vb, const float *bias, bool relu, float *Y, int64_t ysh, hipStream_t s) {
    if (!gemm_outlier_ok(m, n, (int)va.k_pad) || !pack_rows_outlier_ok(X, xsh, m, k)) return hipErrorNotSupported;
    const OutlierScratch v = scratch_view(scratch, m, k);
    hipError_t e = launch_colmask_fast(X, xsh, m, k, t, v, s);
    if (e != hipSuccess) return e;
    const float range = 127.0f;
    e = launch_pack_rows_outlier(X, xsh, m, k, va, range, v.partial, v.splits, v.nwords, v.idx, s);
    if (e == hipErrorNotSupported) return hipErrorUnknown;  // the mask already enqueued: the envelope checks disagree
    if (e != hipSuccess) return e;
    return launch_gemm_dequant_outlier_q(va, vb, Y, ysh, m, n, 1.0f / (range * range), X, xsh, v.idx + 1, v.idx, bias,
                                         relu, s);
}

// Fallback phase 1: the column mask, the index (mask words, count, list), then X' and -- with an fp32 W -- W' into
// the scratch.  The caller then runs the int8 chain on (X', W' or the packed weight) without bias, and phase 2
// (outlier_finish) adds the fp32 outlier products and the extras.
hipError_t outlier_prepare(const float *X, int64_t xsh, const float *W, int64_t wsh, int m, int n, int k, float t,
                           void *scratch, float **Xm, float **Wm, hipStream_t s) {
    const OutlierScratch v = scratch_view(scratch, m, k);
    *Xm = v.xm;
    if (Wm) *Wm = W ? v.wm : nullptr;
    hipError_t e = launch_colmask(X, xsh, m, k, t, v, s);
    if (e != hipSuccess) return e;
    outlier_index_kernel<<<1, kScanThreads, 0, s>>>(OutlierMask{v.partial, v.nwords, v.splits, v.idx}, v.bits);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // X's rows, then W's where there is one
    outlier_mask_kernel<<<(unsigned)(W ? m + k : m), 256, 0, s>>>(X, xsh, m, k, W, wsh, n, v.bits, v.xm, v.wm);
    return hipGetLastError();
}

// Fallback phase 2 on O = the int8 part: the chain against the fp32 W (row stride wsh), or -- W == nullptr -- against
// the packed weight vb's dequantized rows, then bias (n floats, or nullptr) and relu.
hipError_t outlier_finish(const float *X, int64_t xsh, const float *W, int64_t wsh, const PackedView *vb,
                          const float *bias, bool relu, int m, int n, int k, void *scratch, float *O, int64_t osh,
                          hipStream_t s) {
    const OutlierScratch v = scratch_view(scratch, m, k);
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)std::min(m, 65535));
    if (W)
        outlier_finish_kernel<false><<<grid, 256, 0, s>>>(X, xsh, W, wsh, nullptr, v.idx + 1, v.idx, bias, relu ? 1 : 0,
                                                          O, osh, m, n);
    else
        outlier_finish_kernel<true><<<grid, 256, 0, s>>>(X, xsh, vb->q, vb->k_pad, vb->scale, v.idx + 1, v.idx, bias,
                                                         relu ? 1 : 0, O, osh, m, n);
    return hipGetLastError();
}

int outlier_count_slot(const void *scratch, int *count_host) {
    // the count leads the scratch
    return (int)hipMemcpy(count_host, scratch, sizeof(int), hipMemcpyDeviceToHost);
}

}  // namespace qgemm
