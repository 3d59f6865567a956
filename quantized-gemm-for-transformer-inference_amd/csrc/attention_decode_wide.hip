// attention_decode_wide.hip -- the kW = 128 instantiations of attention_decode_kernel (attention_decode_kernel.h): the
// decode attention at d_k 96 and 128, DESIGN.md s29.  A translation unit of its own, so that attention_decode.o keeps
// the code it had before the row width became a parameter, and so that this one is built with the packed fp32
// instructions off (Makefile): every fp32 step here is one the contract names, none is worth pairing.
#include "attention_decode_kernel.h"

namespace qgemm {

hipError_t launch_decode_wide(const dim3 &grid, bool causal, const float *Q, int64_t ldq, const float *K, int64_t ldk,
                              const float *V, int64_t ldv, float *O, int64_t ldo, int dk, float scale, const DecodeOne &seqs,
                              hipStream_t stream) {
    return decode_launch<kDecWideDk>(grid, causal, Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, seqs, stream);
}

hipError_t launch_decode_wide(const dim3 &grid, bool causal, const float *Q, int64_t ldq, const float *K, int64_t ldk,
                              const float *V, int64_t ldv, float *O, int64_t ldo, int dk, float scale, const DecodeMany &seqs,
                              hipStream_t stream) {
    return decode_launch<kDecWideDk>(grid, causal, Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, seqs, stream);
}

hipError_t launch_decode_wide(const dim3 &grid, bool causal, const float *Q, int64_t ldq, const float *K, int64_t ldk,
                              const float *V, int64_t ldv, float *O, int64_t ldo, int dk, float scale, const DecodeIndirect &seqs,
                              hipStream_t stream) {
    return decode_launch<kDecWideDk>(grid, causal, Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, seqs, stream);
}

}  // namespace qgemm
