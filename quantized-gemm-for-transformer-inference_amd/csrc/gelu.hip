// gelu.hip -- the tanh-form GELU of the standard block's FFN, elementwise and fused into the activation
// pack in front of W2.  The contract is at qgemm_gelu_rows in include/qgemm.h: x sigmoid(2u), u = sqrt(2/pi) (x +
// 0.044715 x^3), which is 0.5 x (1 + tanh(u)) algebraically and needs only the project's correctly rounded exp
// (softmax_exp's: fl32(exp((double)x))), every other step one IEEE fp32 operation.
//
// gelu_pack: the hidden layer of a GELU FFN is written once by the W1 GEMM (bias, no relu) and read once here; no fp32
// GELU'd matrix exists.  One 256-thread workgroup per packed row; thread t holds the float4 columns t, t + 256, .. of
// the row (kV = 1, 4 or 16 of them: rows up to 1024, 4096 and 16384 floats), loads them once, applies GELU once and
// keeps g in registers between the absmax and the quantization: a row of 16384 floats is 64 VGPRs per thread.  Holding
// g costs registers; recomputing it in a second pass would cost the double-precision exp twice, and that exp is the
// kernel's time.  gelu_tanh itself lives in activations.h, shared with glu.hip's gated pack.  The absmax is a maximum, exact in any order: wave_max, then the four waves' results
// through LDS.  Then the operations of pack_rows: the signed seed g[0], candidates |g[c]|, c >= 1, inv_divide, quant_i8;
// rows [m, rows_pad) zero bytes and a zero scale, columns [k, k_pad) zero bytes.
//   kVec = true : 16-byte aligned rows of k % 4 == 0 floats, float4 loads;  false: any k, stride and alignment, the same
//   registers filled float by float.
#include <algorithm>

#include "activations.h"
#include "qgemm_internal.h"

namespace qgemm {

namespace {

constexpr int kBlock = 256;
constexpr int kMaxK = 16384;

__global__ __launch_bounds__(kBlock) void gelu_rows_kernel(const float *X, int64_t xsh, float *Y, int64_t ysh,
                                                           int64_t rows, int w) {
    const int64_t n = rows * w;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / w, c = i % w;
        Y[r * ysh + c] = gelu_tanh(X[r * xsh + c]);
    }
}

template <int kV, bool kVec>
__global__ __launch_bounds__(kBlock) void gelu_pack_kernel(const float *__restrict__ X, int64_t xsh, int m, int k,
                                                           float range, float *__restrict__ scale,
                                                           int8_t *__restrict__ q, int64_t rows_pad, int64_t k_pad) {
    __shared__ float red[kBlock / 64 + 1];
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x;
    if (row >= rows_pad) return;
    if (row >= m) {  // padding row of the packed view
        for (int64_t c = t; c < k_pad / 4; c += kBlock) *qword(q, row, 4 * c, k_pad) = 0u;
        if (t == 0) scale[row] = 0.0f;
        return;
    }
    const float *x = X + row * xsh;
    const int k4 = (k + 3) >> 2;  // float4 columns that hold an element
    float4 g[kV];
    float cand = -INFINITY;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int j = t + kBlock * i, c = 4 * j;
        g[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < k4) {
            float4 v;
            if constexpr (kVec) {
                v = *reinterpret_cast<const float4 *>(x + c);
            } else {
                v = make_float4(x[c], c + 1 < k ? x[c + 1] : 0.0f, c + 2 < k ? x[c + 2] : 0.0f,
                                c + 3 < k ? x[c + 3] : 0.0f);
            }
            g[i].x = gelu_tanh(v.x);
            if (c > 0) cand = fmaxf(cand, absmax_candidate(g[i].x));  // element 0 is the seed, no candidate
            if (c + 1 < k) cand = fmaxf(cand, absmax_candidate(g[i].y = gelu_tanh(v.y)));
            if (c + 2 < k) cand = fmaxf(cand, absmax_candidate(g[i].z = gelu_tanh(v.z)));
            if (c + 3 < k) cand = fmaxf(cand, absmax_candidate(g[i].w = gelu_tanh(v.w)));
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cand = fmaxf(cand, __shfl_xor(cand, off, 64));
    if ((t & 63) == 0) red[t >> 6] = cand;
    if (t == 0) red[kBlock / 64] = g[0].x;  // the signed seed: element 0
    __syncthreads();
    float p = red[0];
#pragma unroll
    for (int wv = 1; wv < kBlock / 64; ++wv) p = fmaxf(p, red[wv]);  // -inf or >= +0: exact in any order
    const float cx = absmax_finish(red[kBlock / 64], p);
    const float sc = inv_divide(range, cx);
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int j = t + kBlock * i, c = 4 * j;
        if (j < k4)
            *qword(q, row, c, k_pad) = (uint32_t)(quant_i8(g[i].x, sc) & 0xff) |
                                       ((uint32_t)((c + 1 < k ? quant_i8(g[i].y, sc) : 0) & 0xff) << 8) |
                                       ((uint32_t)((c + 2 < k ? quant_i8(g[i].z, sc) : 0) & 0xff) << 16) |
                                       ((uint32_t)((c + 3 < k ? quant_i8(g[i].w, sc) : 0) & 0xff) << 24);
    }
    for (int64_t c4 = k4 + t; c4 < k_pad / 4; c4 += kBlock) *qword(q, row, 4 * c4, k_pad) = 0u;  // padding columns
    if (t == 0) scale[row] = cx;
}

template <bool kVec>
hipError_t launch_gelu_pack_t(const float *X, int64_t xsh, int m, int k, float range, const PackedView &out,
                              hipStream_t stream) {
    const dim3 grid((unsigned)out.rows_pad), block(kBlock);
    if (k <= 1024)
        gelu_pack_kernel<1, kVec><<<grid, block, 0, stream>>>(X, xsh, m, k, range, out.scale, out.q, out.rows_pad, out.k_pad);
    else if (k <= 4096)
        gelu_pack_kernel<4, kVec><<<grid, block, 0, stream>>>(X, xsh, m, k, range, out.scale, out.q, out.rows_pad, out.k_pad);
    else
        gelu_pack_kernel<16, kVec><<<grid, block, 0, stream>>>(X, xsh, m, k, range, out.scale, out.q, out.rows_pad, out.k_pad);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gelu_rows(const float *X, int64_t xsh, float *Y, int64_t ysh, int64_t rows, int w, hipStream_t stream) {
    if (!X || !Y || rows < 0 || w < 1 || xsh < 0 || ysh < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    const int64_t blocks = (rows * w + kBlock - 1) / kBlock;
    gelu_rows_kernel<<<(unsigned)std::min<int64_t>(blocks, 65536), kBlock, 0, stream>>>(X, xsh, Y, ysh, rows, w);
    return hipGetLastError();
}

hipError_t launch_gelu_pack(const float *X, int64_t xsh, int m, int k, float range, PackedView out, hipStream_t stream) {
    if (!X || m < 0 || k < 1 || k > kMaxK || xsh < 0) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    if (!out.q || out.k_pad < k || out.rows_pad < m) return hipErrorInvalidValue;
    const bool vec = k % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (xsh % 4 == 0 || m == 1);
    return vec ? launch_gelu_pack_t<true>(X, xsh, m, k, range, out, stream)
               : launch_gelu_pack_t<false>(X, xsh, m, k, range, out, stream);
}

}  // namespace qgemm
