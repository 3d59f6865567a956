// ln_legacy.h -- the superseded layouts of the register-resident add+layernorm kernel (csrc/encoder_ops.hip), kept
// for the lab comparison (ln_lab.hip variants 2 and 3; profiles/r03_ln_hop_chain_lab.log).  FROZEN: not regenerated
// from the product.  Include it after the product file (or its generated copy): it uses that file's kRowWaves,
// seq_sum and sq_dev and qgemm_internal.h's hop_left / qword / absmax / quant helpers.
//
// Both keep the INTERLEAVED layout: lane l holds the float4 columns j = l + 64 i, i < kV (element 4(l + 64 i) + c is
// x[i].c of lane l), and each packed dword is stored on its own.
//   kHop = true : both sums hop lane to lane over the registers, one hop per 4 elements (lane_chain_sum) -- the
//                 round-3 to round-6 product; the product now holds 4 kV consecutive elements per lane and hops once
//                 per block (lane_block_sum: ~4.5 cycles per element against ~6 here);
//   kHop = false: the row is staged in LDS (w floats per wave of dynamic LDS) and walked by seq_sum -- the form
//                 before the hops (~7-8 cycles per element waiting on the ds_read groups).
#pragma once

namespace qgemm {
namespace ln_legacy {

// The running sum hops from lane to lane: every step is one v_add_f32 whose first operand is the LEFT neighbour's
// sum (DPP wave_ror:1: lane l reads lane l - 1, lane 0 reads lane 63), then three in-lane adds.  Every lane runs
// every step, so after step t of group i lane t - 1 holds the chain through its own four elements (induction: each
// step extends the chain that had reached the left neighbour one step earlier), and lane 63 hands a full group on
// to lane 0 of the next.  w4 = w / 4 float4 columns; the result is the sum in lane (w4 - 1) mod 64, broadcast.
__device__ __forceinline__ float hop_step(float s, const float4 &v) {
    s = __fadd_rn(hop_left(s), v.x);
    s = __fadd_rn(s, v.y);
    s = __fadd_rn(s, v.z);
    return __fadd_rn(s, v.w);
}
template <int kV>
__device__ __forceinline__ float lane_chain_sum(const float4 (&x)[kV], int w4) {
    float s = 0.0f;
    int last = 63;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int n = w4 - 64 * i < 64 ? w4 - 64 * i : 64;
        if (n <= 0) break;
        int t = 0;
        for (; t + 8 <= n; t += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) s = hop_step(s, x[i]);
        }
        for (; t < n; ++t) s = hop_step(s, x[i]);
        last = n - 1;
    }
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), last));
}

template <bool kPack, int kV, bool kHop>
__global__ __launch_bounds__(64 * kRowWaves) void add_layernorm_rows_vec_kernel(
    const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ Y, int64_t rows, int w,
    int8_t *__restrict__ q, float *__restrict__ qscale, int64_t k_pad, int64_t rows_pad, float range) {
    extern __shared__ __attribute__((aligned(16))) float stage[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * kRowWaves + wv;
    if (kPack && row >= rows && row < rows_pad) {  // padding row of the packed view
        auto qrow = [&](int64_t c) __attribute__((always_inline)) -> uint32_t & { return *qword(q, row, 4 * c, k_pad); };  // fragment-major q
        for (int64_t c = lane; c < k_pad / 4; c += 64) qrow(c) = 0u;
        if (lane == 0) qscale[row] = 0.0f;
        return;
    }
    if (row >= rows) return;
    const int w4 = w >> 2;
    const float4 *a = reinterpret_cast<const float4 *>(A + row * w), *b = reinterpret_cast<const float4 *>(B + row * w);
    float4 *y = reinterpret_cast<float4 *>(Y + row * w);
    float *st = stage + wv * w;
    float4 x[kV];
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int j = lane + 64 * i;
        x[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < w4) {
            const float4 av = a[j], bv = b[j];
            x[i] = make_float4(__fadd_rn(av.x, bv.x), __fadd_rn(av.y, bv.y), __fadd_rn(av.z, bv.z),
                               __fadd_rn(av.w, bv.w));  // op_add (transformer.cu:58)
            if constexpr (!kHop) reinterpret_cast<float4 *>(st)[j] = x[i];
        }
    }
    if constexpr (!kHop) {
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
    }
    const float fw = (float)w;
    const float sum_x = kHop ? lane_chain_sum<kV>(x, w4) : seq_sum(st, w);
    const float mean = __fdiv_rn(sum_x, fw);  // op_layernorm.cuh:15-19
    float var;
    if constexpr (kHop) {
        float4 d[kV];
#pragma unroll
        for (int i = 0; i < kV; ++i)
            d[i] = make_float4(sq_dev(x[i].x, mean), sq_dev(x[i].y, mean), sq_dev(x[i].z, mean), sq_dev(x[i].w, mean));
        var = __fdiv_rn(lane_chain_sum<kV>(d, w4), fw);  // :21-25
    } else {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < kV; ++i) {
            const int j = lane + 64 * i;
            if (j < w4)
                reinterpret_cast<float4 *>(st)[j] =
                    make_float4(sq_dev(x[i].x, mean), sq_dev(x[i].y, mean), sq_dev(x[i].z, mean), sq_dev(x[i].w, mean));
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        var = __fdiv_rn(seq_sum(st, w), fw);                       // :21-25
    }
    float cand = -INFINITY;
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const int j = lane + 64 * i;
        if (j < w4) {
            float4 v;                                                // (x - mean) / var (:28), as written
            v.x = __fdiv_rn(__fsub_rn(x[i].x, mean), var);
            v.y = __fdiv_rn(__fsub_rn(x[i].y, mean), var);
            v.z = __fdiv_rn(__fsub_rn(x[i].z, mean), var);
            v.w = __fdiv_rn(__fsub_rn(x[i].w, mean), var);
            y[j] = v;
            x[i] = v;
            if constexpr (kPack) {
                if (j > 0) cand = fmaxf(cand, absmax_candidate(v.x));
                cand = fmaxf(cand, absmax_candidate(v.y));
                cand = fmaxf(cand, absmax_candidate(v.z));
                cand = fmaxf(cand, absmax_candidate(v.w));
            }
        }
    }
    if constexpr (kPack) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cand = fmaxf(cand, __shfl_xor(cand, off, 64));
        const float seed = __shfl(x[0].x, 0, 64);  // column 0: lane 0, i = 0
        const float cx = absmax_finish(seed, cand);
        const float sc = inv_divide(range, cx);
        auto qrow = [&](int64_t c) __attribute__((always_inline)) -> uint32_t & { return *qword(q, row, 4 * c, k_pad); };  // fragment-major q
#pragma unroll
        for (int i = 0; i < kV; ++i) {
            const int j = lane + 64 * i;
            if (j < w4)
                qrow(j) = (uint32_t)(quant_i8(x[i].x, sc) & 0xff) | ((uint32_t)(quant_i8(x[i].y, sc) & 0xff) << 8) |
                          ((uint32_t)(quant_i8(x[i].z, sc) & 0xff) << 16) | ((uint32_t)(quant_i8(x[i].w, sc) & 0xff) << 24);
        }
        for (int64_t c4 = w4 + lane; c4 < k_pad / 4; c4 += 64) qrow(c4) = 0u;  // padding columns
        if (lane == 0) qscale[row] = cx;
    }
}

}  // namespace ln_legacy
}  // namespace qgemm
