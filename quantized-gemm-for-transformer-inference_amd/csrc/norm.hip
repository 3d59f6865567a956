// norm.hip -- the standard layer normalisation of the textbook post-LN block, with the residual add in
// front of it and, where a quantized linear consumes the row, the activation pack behind it.  The contract -- every
// step one IEEE fp32 operation, the order of both sums -- is at qgemm_layernorm_rows in include/qgemm.h:
//   v = fl(A + B) (B == NULL: A), mean = fl(sum(v) / fl32(w)), d = fl(v - mean), var = fl(sum(fl(d d)) / fl32(w)),
//   rstd = fl(1 / fl(sqrt(fl(var + eps)))), Y = fl(fl(fl(d rstd) gamma) + beta).
//
// One wave per row, the row in registers from its first load to its last use: lane l holds the float4 columns
// l, l + 64, .. (elements 4 (l + 64 i) .. + 3 in x[i]), kV = 4, 8 or 16 of them by row length.  That layout IS the sum
// order of the contract: a lane's partial adds its own elements in increasing column from +0, then six butterfly steps
// p = fl(p + p[lane ^ off]), off = 32 .. 1 -- an fp32 add is commutative, so both lanes of a pair hold the same bits
// and every lane ends with the same sum.  The reference architecture's kernel (encoder_ops.hip) keeps ONE sequential
// chain per sum, two chains of about 2.3 us at w = 1024; here a sum is at most 4 kV dependent adds and 6 hops.
//   kVec  = true : 16-byte aligned rows of w % 4 == 0 floats: every load and store a float4, 1 KiB per wave-instruction;
//   kVec  = false: any w and alignment: the same registers filled float by float (element c in x[(c / 4) / 64] of lane
//                  (c / 4) % 64), elements past the row the sums' identity.  The same adds in the same order: the same
//                  bits.
// A wave loads its whole row before it stores, and a row is its wave's alone: Y may be A or B.  No pointer that may
// alias carries __restrict__.
// kPack: the row is also quantized for the next linear with the operations of pack_rows (absmax_candidate,
// absmax_finish, inv_divide, quant_i8): the packed bytes are those of packing Y afterwards; rows [rows, rows_pad) get
// zero bytes and a zero scale, columns [w, k_pad) zero bytes (as add_layernorm_rows_vec_kernel<true, .>).
// kForm: what the row's wave writes.  kFormPost, the post-LN block's: Y = LN(v).  kFormPre, the pre-LN
// boundary's: S = v, the updated residual stream, stored BEFORE the mean is subtracted (S == nullptr: not stored), then
// LN(v) exactly as above, written only as packed int8 + scale -- the normalised fp32 row is never stored.  kFormAdd: S
// = v and nothing else, the last boundary of a pre-LN model without a final norm.  S takes Y's place in the argument
// list and Y's rules: it may be A or B.
// kRms: the root-mean-square norm of Llama-style blocks (qgemm_rmsnorm_rows): no mean pass and no beta --
//   ms = fl(sum(fl(v v)) / fl32(w)), r = fl(1 / fl(sqrt(fl(ms + eps)))), Y = fl(fl(v r) gamma)
// -- the same loads, stores, sum order, pack and forms; beta is not read (nullptr).
#include "qgemm_internal.h"

namespace qgemm {

namespace {

constexpr int kRowWaves = 4;      // rows per 256-thread block
constexpr int kMaxRowLen = 4096;  // 16 float4 columns per lane

__device__ __forceinline__ float butterfly_sum(float p) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = __fadd_rn(p, __shfl_xor(p, off, 64));
    return p;
}

template <int kV>
__device__ __forceinline__ float lane_sum(const float4 (&x)[kV]) {
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        p = __fadd_rn(p, x[i].x);
        p = __fadd_rn(p, x[i].y);
        p = __fadd_rn(p, x[i].z);
        p = __fadd_rn(p, x[i].w);
    }
    return butterfly_sum(p);
}

// element c of a row of w floats, or `pad` past it
__device__ __forceinline__ float at(const float *row, int c, int w, float pad) { return c < w ? row[c] : pad; }

template <bool kVec>
__device__ __forceinline__ float4 load4(const float *row, int j, int w, float pad) {
    if constexpr (kVec) {
        return 4 * j < w ? *reinterpret_cast<const float4 *>(row + 4 * j) : make_float4(pad, pad, pad, pad);
    } else {
        return make_float4(at(row, 4 * j, w, pad), at(row, 4 * j + 1, w, pad), at(row, 4 * j + 2, w, pad),
                           at(row, 4 * j + 3, w, pad));
    }
}

// v into elements c .. c + 3 of a row of w floats (c < w)
template <bool kVec>
__device__ __forceinline__ void store4(float *row, int c, int w, float4 v) {
    if constexpr (kVec) {
        *reinterpret_cast<float4 *>(row + c) = v;
    } else {
        row[c] = v.x;
        if (c + 1 < w) row[c + 1] = v.y;
        if (c + 2 < w) row[c + 2] = v.z;
        if (c + 3 < w) row[c + 3] = v.w;
    }
}

enum { kFormPost = 0, kFormPre = 1, kFormAdd = 2 };

template <bool kPack, int kV, bool kVec, int kForm = kFormPost, bool kRms = false>
__global__ __launch_bounds__(64 * kRowWaves) void layernorm_rows_kernel(const float *A, const float *B,
                                                                       const float *__restrict__ gamma,
                                                                       const float *__restrict__ beta, float eps,
                                                                       float *Y, int64_t rows, int w, int8_t *q,
                                                                       float *qscale, int64_t k_pad, int64_t rows_pad,
                                                                       float range) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * kRowWaves + wv;
    if (kPack && row >= rows && row < rows_pad) {  // padding row of the packed view
        for (int64_t c = lane; c < k_pad / 4; c += 64) *qword(q, row, 4 * c, k_pad) = 0u;
        if (lane == 0) qscale[row] = 0.0f;
        return;
    }
    if (row >= rows) return;
    static_assert(kForm == kFormPost || kPack == (kForm == kFormPre), "pre-LN packs and only packs; the add packs nothing");
    const float *a = A + row * w, *b = B ? B + row * w : nullptr;
    float *y = Y ? Y + row * w : nullptr;  // (nullptr: kFormPre without a stream to write)
    const int w4 = (w + 3) >> 2;  // float4 columns that hold an element
    // past the row: -0, the identity of the sums (x + -0 == x for every x, -0 and NaN included)
    float4 x[kV];
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int j = lane + 64 * i;
        x[i] = load4<kVec>(a, j, w, -0.0f);
        if (b) {
            const float4 bv = load4<kVec>(b, j, w, -0.0f);
            x[i] = make_float4(__fadd_rn(x[i].x, bv.x), __fadd_rn(x[i].y, bv.y), __fadd_rn(x[i].z, bv.z),
                               __fadd_rn(x[i].w, bv.w));
        }
    }
    if constexpr (kForm != kFormPost) {  // the residual stream: every load of the row has been issued above
        if (y) {
#pragma unroll
            for (int i = 0; i < kV; ++i)
                if (lane + 64 * i < w4) store4<kVec>(y, 4 * (lane + 64 * i), w, x[i]);
        }
        if constexpr (kForm == kFormAdd) return;
    }
    const float fw = (float)w;
    // kRms: no mean -- x stays v, and below `var` is the mean square and `rstd` the scale r
    [[maybe_unused]] float mean = 0.0f;
    if constexpr (!kRms) mean = __fdiv_rn(lane_sum<kV>(x), fw);
    float4 sq[kV];
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int c = 4 * (lane + 64 * i);
        if constexpr (!kRms)
            x[i] = make_float4(__fsub_rn(x[i].x, mean), __fsub_rn(x[i].y, mean), __fsub_rn(x[i].z, mean),
                               __fsub_rn(x[i].w, mean));  // d
        sq[i] = make_float4(c < w ? __fmul_rn(x[i].x, x[i].x) : -0.0f, c + 1 < w ? __fmul_rn(x[i].y, x[i].y) : -0.0f,
                            c + 2 < w ? __fmul_rn(x[i].z, x[i].z) : -0.0f, c + 3 < w ? __fmul_rn(x[i].w, x[i].w) : -0.0f);
    }
    const float var = __fdiv_rn(lane_sum<kV>(sq), fw);
    // sqrtf, not __fsqrt_rn: this toolchain's __fsqrt_rn is the native v_sqrt_f32 (1 ulp), sqrtf the correctly rounded
    // square root (v_sqrt_f32 and a residual fix-up), which is what the contract's fl(sqrt(.)) means
    const float rstd = __fdiv_rn(1.0f, sqrtf(__fadd_rn(var, eps)));
    float cand = -INFINITY;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int j = lane + 64 * i, c = 4 * j;
        if (j < w4) {
            const float4 g = load4<kVec>(gamma, j, w, 0.0f);
            float4 v;
            if constexpr (kRms) {  // no beta: Y = fl(fl(v r) gamma)
                v = make_float4(__fmul_rn(__fmul_rn(x[i].x, rstd), g.x), __fmul_rn(__fmul_rn(x[i].y, rstd), g.y),
                                __fmul_rn(__fmul_rn(x[i].z, rstd), g.z), __fmul_rn(__fmul_rn(x[i].w, rstd), g.w));
            } else {
                const float4 be = load4<kVec>(beta, j, w, 0.0f);
                v.x = __fadd_rn(__fmul_rn(__fmul_rn(x[i].x, rstd), g.x), be.x);
                v.y = __fadd_rn(__fmul_rn(__fmul_rn(x[i].y, rstd), g.y), be.y);
                v.z = __fadd_rn(__fmul_rn(__fmul_rn(x[i].z, rstd), g.z), be.z);
                v.w = __fadd_rn(__fmul_rn(__fmul_rn(x[i].w, rstd), g.w), be.w);
            }
            if constexpr (kForm == kFormPost) store4<kVec>(y, c, w, v);
            x[i] = v;
            if constexpr (kPack) {
                if (c > 0) cand = fmaxf(cand, absmax_candidate(v.x));  // element 0 is the seed, no candidate
                if (c + 1 < w) cand = fmaxf(cand, absmax_candidate(v.y));
                if (c + 2 < w) cand = fmaxf(cand, absmax_candidate(v.z));
                if (c + 3 < w) cand = fmaxf(cand, absmax_candidate(v.w));
            }
        }
    }
    if constexpr (kPack) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cand = fmaxf(cand, __shfl_xor(cand, off, 64));
        const float seed = __shfl(x[0].x, 0, 64);  // column 0: lane 0, i = 0
        const float cx = absmax_finish(seed, cand);
        const float sc = inv_divide(range, cx);
#pragma unroll
        for (int i = 0; i < kV; ++i) {
            const int j = lane + 64 * i, c = 4 * j;
            if (j < w4)
                *qword(q, row, c, k_pad) = (uint32_t)(quant_i8(x[i].x, sc) & 0xff) |
                                           ((uint32_t)((c + 1 < w ? quant_i8(x[i].y, sc) : 0) & 0xff) << 8) |
                                           ((uint32_t)((c + 2 < w ? quant_i8(x[i].z, sc) : 0) & 0xff) << 16) |
                                           ((uint32_t)((c + 3 < w ? quant_i8(x[i].w, sc) : 0) & 0xff) << 24);
        }
        for (int64_t c4 = w4 + lane; c4 < k_pad / 4; c4 += 64) *qword(q, row, 4 * c4, k_pad) = 0u;  // padding columns
        if (lane == 0) qscale[row] = cx;
    }
}

bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool kPack, bool kVec, int kForm, bool kRms>
hipError_t launch_ln(const float *A, const float *B, const float *gamma, const float *beta, float eps, float *Y,
                     int64_t rows, int w, int8_t *q, float *qscale, int64_t k_pad, int64_t rows_pad, float range,
                     int64_t grid_rows, hipStream_t stream) {
    const unsigned grid = (unsigned)((grid_rows + kRowWaves - 1) / kRowWaves);
    if (w <= 1024)
        layernorm_rows_kernel<kPack, 4, kVec, kForm, kRms>
            <<<grid, 64 * kRowWaves, 0, stream>>>(A, B, gamma, beta, eps, Y, rows, w, q, qscale, k_pad, rows_pad, range);
    else if (w <= 2048)
        layernorm_rows_kernel<kPack, 8, kVec, kForm, kRms>
            <<<grid, 64 * kRowWaves, 0, stream>>>(A, B, gamma, beta, eps, Y, rows, w, q, qscale, k_pad, rows_pad, range);
    else
        layernorm_rows_kernel<kPack, 16, kVec, kForm, kRms>
            <<<grid, 64 * kRowWaves, 0, stream>>>(A, B, gamma, beta, eps, Y, rows, w, q, qscale, k_pad, rows_pad, range);
    return hipGetLastError();
}

template <bool kPack, int kForm = kFormPost, bool kRms = false>
hipError_t launch_ln_any(const float *A, const float *B, const float *gamma, const float *beta, float eps, float *Y,
                         int64_t rows, int w, int8_t *q, float *qscale, int64_t k_pad, int64_t rows_pad, float range,
                         int64_t grid_rows, hipStream_t stream) {
    const bool vec = w % 4 == 0 && al16(A) && al16(B) && al16(gamma) && al16(beta) && al16(Y);
    return vec ? launch_ln<kPack, true, kForm, kRms>(A, B, gamma, beta, eps, Y, rows, w, q, qscale, k_pad, rows_pad, range,
                                               grid_rows, stream)
               : launch_ln<kPack, false, kForm, kRms>(A, B, gamma, beta, eps, Y, rows, w, q, qscale, k_pad, rows_pad, range,
                                                grid_rows, stream);
}

}  // namespace

hipError_t launch_layernorm_rows(const float *A, const float *B, const float *gamma, const float *beta, float eps,
                                 float *Y, int64_t rows, int w, hipStream_t stream) {
    if (!A || !gamma || !beta || !Y || w < 1 || w > kMaxRowLen || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    return launch_ln_any<false>(A, B, gamma, beta, eps, Y, rows, w, nullptr, nullptr, 0, 0, 0.0f, rows, stream);
}

hipError_t launch_layernorm_rows_pack(const float *A, const float *B, const float *gamma, const float *beta, float eps,
                                      float *Y, int64_t rows, int w, float range, PackedView out, hipStream_t stream) {
    if (!A || !gamma || !beta || !Y || w < 1 || w > kMaxRowLen || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    if (!out.q || out.k_pad < w || out.rows_pad < rows) return hipErrorInvalidValue;
    return launch_ln_any<true>(A, B, gamma, beta, eps, Y, rows, w, out.q, out.scale, out.k_pad, out.rows_pad, range,
                               out.rows_pad, stream);
}

// the pre-LN boundary: S = A + B (S == nullptr: not stored), LN(S) written packed alone
hipError_t launch_prenorm_pack(const float *A, const float *B, const float *gamma, const float *beta, float eps,
                               float *S, int64_t rows, int w, float range, PackedView out, hipStream_t stream) {
    if (!A || !gamma || !beta || w < 1 || w > kMaxRowLen || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    if (!out.q || out.k_pad < w || out.rows_pad < rows) return hipErrorInvalidValue;
    return launch_ln_any<true, kFormPre>(A, B, gamma, beta, eps, S, rows, w, out.q, out.scale, out.k_pad, out.rows_pad,
                                         range, out.rows_pad, stream);
}

// The RMS forms (the contract is at qgemm_rmsnorm_rows in include/qgemm.h): the three launchers above on
// the kernel's kRms instantiations -- no mean pass, no beta
hipError_t launch_rmsnorm_rows(const float *A, const float *B, const float *gamma, float eps, float *Y, int64_t rows,
                               int w, hipStream_t stream) {
    if (!A || !gamma || !Y || w < 1 || w > kMaxRowLen || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    return launch_ln_any<false, kFormPost, true>(A, B, gamma, nullptr, eps, Y, rows, w, nullptr, nullptr, 0, 0, 0.0f,
                                                 rows, stream);
}

hipError_t launch_rmsnorm_rows_pack(const float *A, const float *B, const float *gamma, float eps, float *Y,
                                    int64_t rows, int w, float range, PackedView out, hipStream_t stream) {
    if (!A || !gamma || !Y || w < 1 || w > kMaxRowLen || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    if (!out.q || out.k_pad < w || out.rows_pad < rows) return hipErrorInvalidValue;
    return launch_ln_any<true, kFormPost, true>(A, B, gamma, nullptr, eps, Y, rows, w, out.q, out.scale, out.k_pad,
                                                out.rows_pad, range, out.rows_pad, stream);
}

hipError_t launch_prenorm_rms_pack(const float *A, const float *B, const float *gamma, float eps, float *S,
                                   int64_t rows, int w, float range, PackedView out, hipStream_t stream) {
    if (!A || !gamma || w < 1 || w > kMaxRowLen || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    if (!out.q || out.k_pad < w || out.rows_pad < rows) return hipErrorInvalidValue;
    return launch_ln_any<true, kFormPre, true>(A, B, gamma, nullptr, eps, S, rows, w, out.q, out.scale, out.k_pad,
                                               out.rows_pad, range, out.rows_pad, stream);
}

// S = A + B, the same rows and paths without a norm
hipError_t launch_add_rows(const float *A, const float *B, float *S, int64_t rows, int w, hipStream_t stream) {
    if (!A || !B || !S || w < 1 || w > kMaxRowLen || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    return launch_ln_any<false, kFormAdd>(A, B, nullptr, nullptr, 0.0f, S, rows, w, nullptr, nullptr, 0, 0, 0.0f, rows,
                                          stream);
}

}  // namespace qgemm
