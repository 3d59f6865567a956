// weights.hip -- caller-supplied weights into an existing packed B operand.
//
// pack_b_window packs a logical k x ncols tensor (fp32 or bf16, any element strides) into packed rows col0 ..
// col0 + ncols - 1 of a packed k x n_total weight that is already there: the fused weights of a stack ([Wq | Wk | Wv]
// and its cross-attention siblings) are assembled from one d_model x d_k tensor per (kind, head), and replacing one
// tensor must neither stage the whole fused matrix in fp32 nor repack it.
//
// Why a window can be packed alone: the quantization of B is column-local -- Cw[j] and column j's int8 depend on column
// j alone (pack.hip pack_cols: seed = row 0, candidates = |rows 1 ..|, range / Cw, truncating quantize) -- and in the
// fragment-major q layout (qgemm_internal.h fofs) a packed row owns whole 16-byte pieces: piece (row, k / 16) holds the
// row's k .. k + 15 and nothing else.  So the kernel writes scale[row] and the k_pad / 16 pieces of its own rows and
// touches no other byte: not the neighbouring rows of a 16-row fragment block, not the reserved words.
//
// Kernel: one workgroup (16 waves) owns the window's rows inside one ALIGNED group of 16 packed rows -- the 16 rows of
// one line of fragment blocks -- and reads them over k twice:
//   pass 1  the rows' absmax: seed and candidates combined as pack_cols does, Cw and range / Cw into LDS, Cw stored;
//   pass 2  lane l of wave w is (row r = l % 16, quarter kc = l / 16) of fragment block kb = w, w + 16, ..: it reads the
//           row's 16 elements k = 64 kb + 16 kc .., quantizes them and stores the piece as one 16-byte store; a wave
//           whose 16 rows all lie in the window stores the block's 1 KiB contiguously.  Pieces at k >= the tensor's k
//           are stored as zeros, as the pack leaves them.
// Three source paths, chosen on the host (pack_b_window_path), each for fp32 and bf16:
//   k-contiguous (b_stride_h == 1, the [out, in] layout of a checkpoint; rows and base 16-byte aligned): 16-byte loads
//       along k in both passes -- pass 1 one wave per row, 1 KiB per wave-instruction; pass 2 a lane's 16 elements are 4
//       (fp32) or 2 (bf16) such loads;
//   n-contiguous (b_stride_w == 1): the 16 lanes of a quarter read 16 neighbouring columns of one source row;
//   generic: the same mapping through both strides.
// The second read of a group comes from the cache: a group is 16 x k elements, at most 1 MiB.  16 waves, because a
// window is often narrow (one head: d_k columns, a handful of workgroups on the whole chip): the workgroup's time is a
// chain of load round trips, and four times the waves make that chain four times shorter.
#include "qgemm_internal.h"

namespace qgemm {

namespace {

constexpr int kWave = 64;
constexpr int kGroupRows = 16;  // packed rows of one workgroup: one line of fragment blocks
constexpr int kWaves = 16;      // one per row in the k-contiguous pass 1
constexpr int kSlots = 4 * kWaves;  // (wave, quarter) pairs: the k-slices of the strided pass 1

enum WindowPath { kPathKContig = 0, kPathNContig = 1, kPathGeneric = 2 };

// running maximum of the candidates; fmaxf returns the non-NaN operand, so a NaN never wins (the strict ">" of
// absmax_candidate's contract); candidates are >= +0 or the start value -inf
__device__ __forceinline__ float cand_max(float p, float x) { return fmaxf(p, absmax_candidate(x)); }

__device__ __forceinline__ float wave_max(float p) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = fmaxf(p, __shfl_xor(p, off, kWave));
    return p;
}

__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) {
    return (uint32_t)(a & 0xff) | ((uint32_t)(b & 0xff) << 8) | ((uint32_t)(c & 0xff) << 16) | ((uint32_t)d << 24);
}

// A 16-byte chunk of a k-contiguous row: kElems elements from element e0 on (e0 % kElems == 0, the row 16-byte
// aligned), widened; elements at or past k read as +0 (the caller masks them by index).  A chunk that crosses k is
// read element by element, so no byte past the row's k elements is touched.
template <typename SrcT>
struct Chunk;
template <>
struct Chunk<float> {
    static constexpr int kElems = 4;
    __device__ static __forceinline__ void load(const float *row, int64_t e0, int k, float (&x)[4]) {
        if (e0 + 4 <= k) {
            const float4 v = *reinterpret_cast<const float4 *>(row + e0);
            x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = e0 + e < k ? row[e0 + e] : 0.0f;
        }
    }
};
template <>
struct Chunk<bf16_t> {
    static constexpr int kElems = 8;
    __device__ static __forceinline__ void load(const bf16_t *row, int64_t e0, int k, float (&x)[8]) {
        if (e0 + 8 <= k) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row + e0);
            const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x[2 * e] = __uint_as_float(u[e] << 16);
                x[2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = e0 + e < k ? widen(row[e0 + e]) : 0.0f;
        }
    }
};

// B: the window's tensor, element (kk, c) at B[kk * sh + c * sw], c = 0 .. ncols - 1 the window's columns; packed row
// col0 + c.  Grid: the aligned 16-row groups the window touches, group (col0 / 16) + blockIdx.x.
template <typename SrcT, int kPath>
__global__ __launch_bounds__(kWaves * kWave) void pack_b_window_kernel(const SrcT *__restrict__ B, int64_t sh, int64_t sw,
                                                                      int k, int col0, int ncols, float range,
                                                                      float *__restrict__ scale, int8_t *__restrict__ q,
                                                                      int64_t k_pad) {
    __shared__ float s_inv[kGroupRows];            // range / Cw of the group's rows
    __shared__ float s_red[kSlots * kGroupRows];   // the strided paths' partial maxima, [slot][row]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t row0 = ((int64_t)(col0 >> 4) + blockIdx.x) * kGroupRows;
    // row r of the group is in the window?  (its column of B: row0 + r - col0)
    auto in_window = [&](int r) { return row0 + r >= col0 && row0 + r < (int64_t)col0 + ncols; };
    constexpr int E = Chunk<SrcT>::kElems;

    // ---- pass 1: Cw and range / Cw of the group's rows ----
    if constexpr (kPath == kPathKContig) {
        // wave w: row w; the lanes sweep the row in 16-byte chunks
        if (const int r = w; in_window(r)) {  // wave-uniform
            const SrcT *rowp = B + (row0 + r - col0) * sw;
            float p = -INFINITY;
#pragma unroll 4
            for (int64_t e0 = (int64_t)lane * E; e0 < k; e0 += (int64_t)kWave * E) {
                float x[E];
                Chunk<SrcT>::load(rowp, e0, k, x);
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (e0 + e != 0 && e0 + e < k) p = cand_max(p, x[e]);  // element 0 is the seed, no candidate
            }
            p = wave_max(p);
            if (lane == 0) {
                const float cw = absmax_finish(widen(rowp[0]), p);
                s_inv[r] = inv_divide(range, cw);
                scale[row0 + r] = cw;
            }
        }
    } else {
        // thread (row r, slot): source rows 1 + slot, 1 + slot + 64, .. of column r
        const int r = lane & 15, slot = 4 * w + (lane >> 4);
        const int64_t cs = kPath == kPathNContig ? 1 : sw;
        float p = -INFINITY;
        if (in_window(r)) {
            const SrcT *colp = B + (row0 + r - col0) * cs;
#pragma unroll 8
            for (int64_t kk = 1 + slot; kk < k; kk += kSlots) p = cand_max(p, widen(colp[kk * sh]));
        }
        s_red[slot * kGroupRows + r] = p;
        __syncthreads();
        if (t < kGroupRows && in_window(t)) {
            float m = s_red[t];
#pragma unroll
            for (int sl = 1; sl < kSlots; ++sl) m = fmaxf(m, s_red[sl * kGroupRows + t]);  // -inf or >= +0: exact
            const float cw = absmax_finish(widen(B[(row0 + t - col0) * cs]), m);
            s_inv[t] = inv_divide(range, cw);
            scale[row0 + t] = cw;
        }
    }
    __syncthreads();

    // ---- pass 2: the pieces of the group's rows, fragment block by fragment block ----
    const int r = lane & 15, kc = lane >> 4;
    if (!in_window(r)) return;
    const float s = s_inv[r];
    const int64_t c = row0 + r - col0;
    const int64_t nkb = k_pad >> 6;
    for (int64_t kb = w; kb < nkb; kb += kWaves) {
        const int64_t k0 = kb * 64 + kc * 16;
        int qv[16];
        if constexpr (kPath == kPathKContig) {
            const SrcT *rowp = B + c * sw;
#pragma unroll
            for (int ch = 0; ch < 16 / E; ++ch) {
                float x[E] = {};
                if (k0 + ch * E < k) Chunk<SrcT>::load(rowp, k0 + ch * E, k, x);
#pragma unroll
                for (int e = 0; e < E; ++e) qv[ch * E + e] = k0 + ch * E + e < k ? quant_i8(x[e], s) : 0;
            }
        } else {
            const SrcT *colp = B + c * (kPath == kPathNContig ? 1 : sw);
            float x[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) x[e] = k0 + e < k ? widen(colp[(k0 + e) * sh]) : 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) qv[e] = k0 + e < k ? quant_i8(x[e], s) : 0;
        }
        *reinterpret_cast<uint4 *>(q + fofs(row0 + r, k0, k_pad)) =
            make_uint4(pack4(qv[0], qv[1], qv[2], qv[3]), pack4(qv[4], qv[5], qv[6], qv[7]),
                       pack4(qv[8], qv[9], qv[10], qv[11]), pack4(qv[12], qv[13], qv[14], qv[15]));
    }
}

// dst[i] = widen(src[i * sw]): a bias (fp32, contiguous, on the device) from a strided fp32 or bf16 row
template <typename SrcT>
__global__ __launch_bounds__(256) void copy_row_kernel(const SrcT *__restrict__ src, int64_t sw, int n,
                                                       float *__restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = widen(src[(int64_t)i * sw]);
}

int window_path(const void *B, int es, int64_t sh, int64_t sw, int ncols) {
    const bool al16 = (reinterpret_cast<uintptr_t>(B) & 15) == 0;
    if (sh == 1 && al16 && (ncols == 1 || (sw * es) % 16 == 0)) return kPathKContig;
    if (sw == 1) return kPathNContig;
    return kPathGeneric;
}

template <typename SrcT>
hipError_t launch_window_t(const SrcT *B, int64_t sh, int64_t sw, int k, int col0, int ncols, float range,
                           const PackedView &out, hipStream_t stream) {
    const int groups = ((col0 + ncols - 1) >> 4) - (col0 >> 4) + 1;
    const dim3 grid(groups), block(kWaves * kWave);
    switch (window_path(B, (int)sizeof(SrcT), sh, sw, ncols)) {
        case kPathKContig:
            hipLaunchKernelGGL((pack_b_window_kernel<SrcT, kPathKContig>), grid, block, 0, stream, B, sh, sw, k, col0,
                               ncols, range, out.scale, out.q, out.k_pad);
            break;
        case kPathNContig:
            hipLaunchKernelGGL((pack_b_window_kernel<SrcT, kPathNContig>), grid, block, 0, stream, B, sh, sw, k, col0,
                               ncols, range, out.scale, out.q, out.k_pad);
            break;
        default:
            hipLaunchKernelGGL((pack_b_window_kernel<SrcT, kPathGeneric>), grid, block, 0, stream, B, sh, sw, k, col0,
                               ncols, range, out.scale, out.q, out.k_pad);
    }
    return hipGetLastError();
}

}  // namespace

// dtype: the element-type tags of include/qgemm.h, QGEMM_F32 = 0 and QGEMM_BF16 = 1
bool pack_b_window_ok(const void *B, int dtype, int64_t sh, int64_t sw, int k, int n_total, int col0, int ncols) {
    return B && (dtype == 0 || dtype == 1) && sh >= 0 && sw >= 0 && k >= 1 && k <= 16384 && col0 >= 0 && ncols >= 1 &&
           (int64_t)col0 + ncols <= n_total;
}

const char *pack_b_window_path(const void *B, int dtype, int64_t sh, int64_t sw, int ncols) {
    static const char *const names[2][3] = {
        {"pack_b_window<f32, k-contiguous>", "pack_b_window<f32, n-contiguous>", "pack_b_window<f32, generic>"},
        {"pack_b_window<bf16, k-contiguous>", "pack_b_window<bf16, n-contiguous>", "pack_b_window<bf16, generic>"}};
    return names[dtype == 1][window_path(B, dtype == 1 ? 2 : 4, sh, sw, ncols)];
}

hipError_t launch_pack_b_window(const void *B, int dtype, int64_t sh, int64_t sw, int k, int n_total, int col0,
                                int ncols, float range, void *packed_b, hipStream_t stream) {
    if (!packed_b || !pack_b_window_ok(B, dtype, sh, sw, k, n_total, col0, ncols)) return hipErrorInvalidValue;
    const PackedView out = packed_view(packed_b, n_total, k);
    return dtype == 1 ? launch_window_t(static_cast<const bf16_t *>(B), sh, sw, k, col0, ncols, range, out, stream)
                      : launch_window_t(static_cast<const float *>(B), sh, sw, k, col0, ncols, range, out, stream);
}

hipError_t launch_copy_row(const void *src, int dtype, int64_t sw, int n, float *dst, hipStream_t stream) {
    if (!src || !dst || (dtype != 0 && dtype != 1) || sw < 0 || n < 1) return hipErrorInvalidValue;
    const dim3 grid((n + 255) / 256), block(256);
    if (dtype == 1)
        hipLaunchKernelGGL(copy_row_kernel<bf16_t>, grid, block, 0, stream, static_cast<const bf16_t *>(src), sw, n, dst);
    else
        hipLaunchKernelGGL(copy_row_kernel<float>, grid, block, 0, stream, static_cast<const float *>(src), sw, n, dst);
    return hipGetLastError();
}

}  // namespace qgemm
