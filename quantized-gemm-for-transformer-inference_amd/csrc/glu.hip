// glu.hip -- the gated FFN of Llama-style blocks (QGEMM_ARCH_GATED_FFN): h = act(gate) * up, elementwise
// and fused into the activation pack in front of W2.  The contract is at qgemm_glu_rows in include/qgemm.h.  A row of X
// holds 2k floats, what ONE GEMM on the block's packed [W1 | W3] wrote: the gate in columns 0 .. k - 1, up in
// k .. 2k - 1.
//   a = act(X[c])         relu: the GEMM epilogue's; gelu_tanh: qgemm_gelu_rows' five steps; silu: fl(g / fl(1 + e)),
//                         e = fl32(exp((double)(-g)))                                                  (activations.h)
//   h[c] = fl(a * X[k + c])
//
// glu_pack is gelu.hip's pack with two loads per element: one 256-thread workgroup per packed row; thread t holds the
// float4 columns t, t + 256, .. of h (kV = 1, 4 or 16 of them: rows up to 1024, 4096 and 16384 floats), loads gate and
// up once each and keeps h in registers between the absmax and the quantization -- the same 64 VGPRs at k = 16384; the
// product matrix is never written.  Then the operations of pack_rows: the signed seed h[0], candidates |h[c]|, c >= 1,
// inv_divide, quant_i8; rows [m, rows_pad) zero bytes and a zero scale, columns [k, k_pad) zero bytes.
//   kVec = true : X 16-byte aligned, k % 4 == 0 (so the up half is aligned too) and a row stride % 4 == 0: float4 loads;
//   kVec = false: any k, stride and alignment, the same registers filled float by float: the same bits.
// The activation is a template parameter: the relu instantiation carries no exp.
#include <algorithm>

#include "activations.h"
#include "qgemm_internal.h"

namespace qgemm {

namespace {

constexpr int kBlock = 256;
constexpr int kMaxK = 16384;
enum { kActRelu = 0, kActGelu = 1, kActSilu = 2 };  // QGEMM_ACT_*

template <int kAct>
__device__ __forceinline__ float glu(float g, float u) {
    static_assert(kAct == kActRelu || kAct == kActGelu || kAct == kActSilu, "QGEMM_ACT_*");
    if constexpr (kAct == kActRelu) return __fmul_rn(relu(g), u);
    else if constexpr (kAct == kActGelu) return __fmul_rn(gelu_tanh(g), u);
    else return __fmul_rn(silu(g), u);
}

template <int kAct>
__global__ __launch_bounds__(kBlock) void glu_rows_kernel(const float *X, int64_t xsh, float *Y, int64_t ysh,
                                                          int64_t rows, int w) {
    const int64_t n = rows * w;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / w, c = i % w;
        Y[r * ysh + c] = glu<kAct>(X[r * xsh + c], X[r * xsh + w + c]);
    }
}

template <int kAct, int kV, bool kVec>
__global__ __launch_bounds__(kBlock) void glu_pack_kernel(const float *__restrict__ X, int64_t xsh, int m, int k,
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
    const float *x = X + row * xsh, *up = x + k;
    const int k4 = (k + 3) >> 2;  // float4 columns that hold an element
    float4 h[kV];
    float cand = -INFINITY;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int j = t + kBlock * i, c = 4 * j;
        h[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < k4) {
            float4 g, u;
            if constexpr (kVec) {
                g = *reinterpret_cast<const float4 *>(x + c);
                u = *reinterpret_cast<const float4 *>(up + c);
            } else {
                g = make_float4(x[c], c + 1 < k ? x[c + 1] : 0.0f, c + 2 < k ? x[c + 2] : 0.0f,
                                c + 3 < k ? x[c + 3] : 0.0f);
                u = make_float4(up[c], c + 1 < k ? up[c + 1] : 0.0f, c + 2 < k ? up[c + 2] : 0.0f,
                                c + 3 < k ? up[c + 3] : 0.0f);
            }
            h[i].x = glu<kAct>(g.x, u.x);
            if (c > 0) cand = fmaxf(cand, absmax_candidate(h[i].x));  // element 0 is the seed, no candidate
            if (c + 1 < k) cand = fmaxf(cand, absmax_candidate(h[i].y = glu<kAct>(g.y, u.y)));
            if (c + 2 < k) cand = fmaxf(cand, absmax_candidate(h[i].z = glu<kAct>(g.z, u.z)));
            if (c + 3 < k) cand = fmaxf(cand, absmax_candidate(h[i].w = glu<kAct>(g.w, u.w)));
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cand = fmaxf(cand, __shfl_xor(cand, off, 64));
    if ((t & 63) == 0) red[t >> 6] = cand;
    if (t == 0) red[kBlock / 64] = h[0].x;  // the signed seed: element 0
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
            *qword(q, row, c, k_pad) = (uint32_t)(quant_i8(h[i].x, sc) & 0xff) |
                                       ((uint32_t)((c + 1 < k ? quant_i8(h[i].y, sc) : 0) & 0xff) << 8) |
                                       ((uint32_t)((c + 2 < k ? quant_i8(h[i].z, sc) : 0) & 0xff) << 16) |
                                       ((uint32_t)((c + 3 < k ? quant_i8(h[i].w, sc) : 0) & 0xff) << 24);
    }
    for (int64_t c4 = k4 + t; c4 < k_pad / 4; c4 += kBlock) *qword(q, row, 4 * c4, k_pad) = 0u;  // padding columns
    if (t == 0) scale[row] = cx;
}

template <int kAct, bool kVec>
hipError_t launch_glu_pack_t(const float *X, int64_t xsh, int m, int k, float range, const PackedView &out,
                             hipStream_t stream) {
    const dim3 grid((unsigned)out.rows_pad), block(kBlock);
    if (k <= 1024)
        glu_pack_kernel<kAct, 1, kVec>
            <<<grid, block, 0, stream>>>(X, xsh, m, k, range, out.scale, out.q, out.rows_pad, out.k_pad);
    else if (k <= 4096)
        glu_pack_kernel<kAct, 4, kVec>
            <<<grid, block, 0, stream>>>(X, xsh, m, k, range, out.scale, out.q, out.rows_pad, out.k_pad);
    else
        glu_pack_kernel<kAct, 16, kVec>
            <<<grid, block, 0, stream>>>(X, xsh, m, k, range, out.scale, out.q, out.rows_pad, out.k_pad);
    return hipGetLastError();
}

template <int kAct>
hipError_t launch_glu_pack_a(const float *X, int64_t xsh, int m, int k, float range, const PackedView &out,
                             hipStream_t stream) {
    const bool vec = k % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (xsh % 4 == 0 || m == 1);
    return vec ? launch_glu_pack_t<kAct, true>(X, xsh, m, k, range, out, stream)
               : launch_glu_pack_t<kAct, false>(X, xsh, m, k, range, out, stream);
}

}  // namespace

hipError_t launch_glu_rows(const float *X, int64_t xsh, float *Y, int64_t ysh, int64_t rows, int w, int activation,
                           hipStream_t stream) {
    if (!X || !Y || rows < 0 || w < 1 || xsh < 0 || ysh < 0 || activation < kActRelu || activation > kActSilu ||
        (rows > 1 && (xsh < 2 * (int64_t)w || ysh < w)))
        return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    const int64_t blocks = (rows * w + kBlock - 1) / kBlock;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks, 65536);
    if (activation == kActRelu) glu_rows_kernel<kActRelu><<<grid, kBlock, 0, stream>>>(X, xsh, Y, ysh, rows, w);
    else if (activation == kActGelu) glu_rows_kernel<kActGelu><<<grid, kBlock, 0, stream>>>(X, xsh, Y, ysh, rows, w);
    else glu_rows_kernel<kActSilu><<<grid, kBlock, 0, stream>>>(X, xsh, Y, ysh, rows, w);
    return hipGetLastError();
}

hipError_t launch_glu_pack(const float *X, int64_t xsh, int m, int k, int activation, float range, PackedView out,
                           hipStream_t stream) {
    if (!X || m < 0 || k < 1 || k > kMaxK || xsh < 0 || activation < kActRelu || activation > kActSilu ||
        (m > 1 && xsh < 2 * (int64_t)k))
        return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    if (!out.q || out.k_pad < k || out.rows_pad < m) return hipErrorInvalidValue;
    if (activation == kActRelu) return launch_glu_pack_a<kActRelu>(X, xsh, m, k, range, out, stream);
    if (activation == kActGelu) return launch_glu_pack_a<kActGelu>(X, xsh, m, k, range, out, stream);
    return launch_glu_pack_a<kActSilu>(X, xsh, m, k, range, out, stream);
}

}  // namespace qgemm
