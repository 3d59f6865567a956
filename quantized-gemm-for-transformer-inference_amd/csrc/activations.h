// activations.h -- the FFN's activations as device functions, shared by gelu.hip (the ungated GELU pack) and glu.hip
// (the gated pack): one definition each, so the two packs cannot drift apart.  The contracts are at
// qgemm_gelu_rows and qgemm_glu_rows in include/qgemm.h; every step is one IEEE fp32 operation but the exp, which is the
// project's correctly rounded one (softmax_exp's: fl32(exp((double)x))).
#pragma once

#include <hip/hip_runtime.h>

namespace qgemm {

// x sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3): the tanh-form GELU
__device__ __forceinline__ float gelu_tanh(float x) {
    const float t = __fmul_rn(x, 1.59576912160573071176f);  // fl32(2 sqrt(2 / pi)) = 0x3FCC422A
    const float q = __fadd_rn(__fmul_rn(__fmul_rn(x, x), 0.044715f), 1.0f);
    const float z = __fmul_rn(t, q);
    const float e = (float)exp((double)(-z));
    return __fdiv_rn(x, __fadd_rn(1.0f, e));
}

// x sigmoid(x) (SiLU, "swish"): e = fl32(exp((double)(-x))), fl(x / fl(1 + e)); -inf gives -inf / inf = NaN
__device__ __forceinline__ float silu(float x) {
    const float e = (float)exp((double)(-x));
    return __fdiv_rn(x, __fadd_rn(1.0f, e));
}

// the GEMM epilogue's relu (gemm_i8_kernels.h): NaN and -0 pass
__device__ __forceinline__ float relu(float x) { return (x < 0.0f) ? 0.0f : x; }

}  // namespace qgemm
