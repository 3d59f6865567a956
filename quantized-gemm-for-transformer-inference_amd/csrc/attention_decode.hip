// attention_decode.hip -- the decode attention launches: the envelopes, the checks that size the kernel's LDS arrays
// and grid, and the kW = 64 instantiations of attention_decode_kernel (attention_decode_kernel.h, where the kernel
// and its contract are written).  The kW = 128 instantiations are attention_decode_wide.hip's.
#include "attention_decode_kernel.h"

namespace qgemm {

namespace {

// the instantiation a launch takes: kW = 128 inside the wide envelope, 64 inside the narrow one (the caller has
// tested that d_k lies in one of them)
template <typename Seqs>
hipError_t decode_launch_any(const dim3 &grid, bool causal, const float *Q, int64_t ldq, const float *K, int64_t ldk,
                             const float *V, int64_t ldv, float *O, int64_t ldo, int dk, float scale, const Seqs &seqs,
                             hipStream_t stream) {
    if (dk > kDecMaxDk) return launch_decode_wide(grid, causal, Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, seqs, stream);
    return decode_launch<kDecMaxDk>(grid, causal, Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, seqs, stream);
}

}  // namespace

bool attention_decode_ok(int seq_q, int seq_kv, int dk) {
    return seq_q <= kAttnDecodeMaxQ && seq_kv <= kDecMaxSeq && dk <= kDecMaxDk;
}

// the wide instantiation's envelope: the same rows and keys, d_k 96 or 128 (a multiple of 32 above 64: the score
// chain then needs no zero padding, and 128 columns are what two waves of P V carry)
bool attention_decode_wide_ok(int seq_q, int seq_kv, int dk) {
    return seq_q <= kAttnDecodeMaxQ && seq_kv <= kDecMaxSeq && dk > kDecMaxDk && dk <= kDecWideDk && dk % 32 == 0;
}

hipError_t launch_attention_decode(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                                   float *O, int64_t ldo, int seq_q, int seq_kv, int n_heads, int dk, float scale,
                                   int q_pos0, hipStream_t stream) {
    if (n_heads < 1 || dk < 1 || seq_q < 0 || seq_kv < 1 || q_pos0 < kNoMask) return hipErrorInvalidValue;
    if (!attention_decode_any_ok(seq_q, seq_kv, dk)) return hipErrorNotSupported;
    if (seq_q == 0) return hipSuccess;
    const dim3 grid((unsigned)n_heads, (unsigned)seq_q);
    // past seq_kv - 1 the mask hides nothing: clamped, so the kernel's row limit cannot overflow
    const DecodeOne one{seq_kv, q_pos0 == kNoMask ? 0 : (q_pos0 < seq_kv ? q_pos0 : seq_kv)};
    return decode_launch_any(grid, q_pos0 != kNoMask, Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, one, stream);
}

// tab: checked and clamped by launch_attention_batched (attention_launch.hip); the envelope is tested again here
// (decode_table_ok), where the kernel's LDS arrays and grid are sized
hipError_t launch_attention_decode_batched(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                           const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                           int n_seqs, int rows_per_seq, const DecodeBatchTable &tab, bool causal,
                                           int n_heads, int dk, float scale, hipStream_t stream) {
    if (n_heads < 1 || !decode_table_ok(tab, n_seqs, rows_per_seq, dk, false, 0)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_heads, (unsigned)rows_per_seq, (unsigned)n_seqs);
    const DecodeMany many{k_stride_seq, v_stride_seq, rows_per_seq, tab};
    return decode_launch_any(grid, causal, Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, many, stream);
}

// tab (kv_slot = the table row) checked and clamped by launch_attention_indirect (attention_launch.hip); what sizes
// the kernel's LDS arrays and grid, and what keeps every table read inside the table, is tested again here
hipError_t launch_attention_decode_indirect(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                            const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                            int n_seqs, int rows_per_seq, const uint8_t *row_slab,
                                            int64_t row_slab_stride, int n_slabs, const DecodeBatchTable &tab,
                                            bool causal, int n_heads, int dk, float scale, hipStream_t stream) {
    if (n_heads < 1 || !row_slab || n_slabs < 1 || n_slabs > kDecodeMaxBatch ||
        !decode_table_ok(tab, n_seqs, rows_per_seq, dk, true, row_slab_stride))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_heads, (unsigned)rows_per_seq, (unsigned)n_seqs);
    const DecodeIndirect ind{k_stride_seq, v_stride_seq, rows_per_seq, n_slabs, row_slab, row_slab_stride, tab};
    return decode_launch_any(grid, causal, Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, ind, stream);
}

}  // namespace qgemm
