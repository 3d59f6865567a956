// attention_launch.hip -- which of the three attention launches a shape takes, for the transformer stack
// (transformer.hip) and the public qgemm_attention* entry points (api.hip): the decode launch for a few query rows
// (attention_decode.hip), one fused launch where it fits (attention.hip), else the three kernels it fuses, through
// `scores` -- the same bits on every path.  Host code only; it is a file of its own because it calls the fp32 GEMM
// launchers, which the programs that compile attention.hip's text alone do not link.
#include "qgemm_internal.h"

namespace qgemm {

const char *attention_plan_name(int seq_q, int seq_kv, int dk) {
    if (attention_decode_ok(seq_q, seq_kv, dk)) return "attention_decode_kernel";
    return attention_fused_ok(seq_kv, dk) ? "attention_fused_kernel" : "three_launches";
}

// scores only where some call can reach the three launches: never inside the fused envelope, and never with at most
// kAttnDecodeMaxQ query rows inside the decode envelope (a call of fewer rows or keys needs none either way)
bool attention_needs_scores(int max_q, int max_kv, int dk) {
    return !attention_fused_ok(max_kv, dk) && !attention_decode_ok(max_q, max_kv, dk);
}

// q_pos0: kNoMask or the causal mask's offset (qgemm_internal.h)
hipError_t launch_attention(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                            float *O, int64_t ldo, int seq_q, int seq_kv, int n_heads, int dk, float scale, int q_pos0,
                            float *scores, hipStream_t stream) {
    hipError_t e =
        launch_attention_decode(Q, ldq, K, ldk, V, ldv, O, ldo, seq_q, seq_kv, n_heads, dk, scale, q_pos0, stream);
    if (e != hipErrorNotSupported) return e;
    e = launch_attention_fused(Q, ldq, K, ldk, V, ldv, O, ldo, seq_q, seq_kv, n_heads, dk, scale, q_pos0, stream);
    if (e != hipErrorNotSupported) return e;
    if (seq_q == 0) return hipSuccess;
    if (!scores) return hipErrorInvalidValue;
    // fp32 op_mm with the transposed view of K, softmax in place, fp32 op_mm into the head's columns of O
    const int64_t sbs = (int64_t)seq_q * seq_kv;
    // The fp32 GEMMs address a tile by 32-bit offsets (mm_f32_strides_ok): a row stride of Q, K, V or O that a tile
    // cannot hold, or a negative one, is refused here for both GEMMs, before the first launch.  (The decode and fused
    // kernels above index through 64-bit pointers and have no such limit.)
    const MmF32Plan qk = mm_f32_plan(seq_q, seq_kv, dk, n_heads, ldq, 1, dk, mm_f32_al16(Q), 1, ldk, dk, mm_f32_al16(K));
    const MmF32Plan pv =
        mm_f32_plan(seq_q, dk, seq_kv, n_heads, seq_kv, 1, sbs, mm_f32_al16(scores), ldv, 1, dk, mm_f32_al16(V));
    if (!mm_f32_strides_ok(qk, ldq, 1, 1, ldk, seq_kv, 1, seq_q, seq_kv, dk) ||
        !mm_f32_strides_ok(pv, seq_kv, 1, ldv, 1, ldo, 1, seq_q, dk, seq_kv))
        return hipErrorInvalidValue;
    if ((e = launch_mm_f32_batched(Q, ldq, 1, dk, K, 1, ldk, dk, scores, seq_kv, 1, sbs, seq_q, seq_kv, dk, n_heads,
                                   stream)))
        return e;
    // (under the mask every score is still computed: the softmax reads only each row's visible columns)
    e = q_pos0 == kNoMask
            ? launch_softmax_rows(scores, scores, (int64_t)n_heads * seq_q, seq_kv, scale, stream)
            : launch_softmax_rows_causal(scores, scores, (int64_t)n_heads * seq_q, seq_kv, scale, seq_q, q_pos0, stream);
    if (e) return e;
    return launch_mm_f32_batched(scores, seq_kv, 1, sbs, V, ldv, 1, dk, O, ldo, 1, dk, seq_q, dk, seq_kv, n_heads,
                                 stream);
}

// one table launch serves a call exactly when every sequence lies inside the fused envelope (no sequence: vacuously)
static bool varlen_fused_ok(int n_seqs, const int *seq_kv, int dk) {
    for (int b = 0; b < n_seqs; ++b)
        if (!attention_fused_ok(seq_kv[b], dk)) return false;
    return attention_fused_ok(1, dk);
}

const char *attention_varlen_plan_name(int n_seqs, const int *seq_kv, int dk) {
    return varlen_fused_ok(n_seqs, seq_kv, dk) ? "attention_fused_kernel<many>" : "per_sequence";
}

// The fused launch over a table of sequences (attention.hip, FusedMany): the host arrays are read HERE, into the table
// that travels in the kernel arguments -- nothing is copied to the device, allocated or synchronized, and a captured
// graph replays the values of the capture.  Every check comes before the first launch, on either path.  Rows of O
// that two sequences share are the caller's error (not checked); Q, K and V rows may be shared.
hipError_t launch_attention_varlen(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                                   float *O, int64_t ldo, int n_seqs, const int64_t *q_row0, const int *seq_q,
                                   const int64_t *kv_row0, const int *seq_kv, const int *q_pos0, int n_heads, int dk,
                                   float scale, float *scores, hipStream_t stream) {
    if (!Q || !K || !V || !O || !q_row0 || !seq_q || !kv_row0 || !seq_kv || n_seqs < 0 || n_seqs > kVarlenMaxSeqs ||
        n_heads < 1 || dk < 1)
        return hipErrorInvalidValue;
    FusedSeqTable tab = {};  // entries past n_seqs are never read; zeroed so the arguments are defined bytes
    bool need_scores = false;
    for (int b = 0; b < n_seqs; ++b) {
        if (q_row0[b] < 0 || kv_row0[b] < 0 || seq_q[b] < 0 || seq_kv[b] < 1 || seq_kv[b] > 4096 ||
            (q_pos0 && q_pos0[b] < 0))
            return hipErrorInvalidValue;
        tab.q_row0[b] = q_row0[b];
        tab.kv_row0[b] = kv_row0[b];
        tab.seq_q[b] = seq_q[b];
        tab.seq_kv[b] = seq_kv[b];
        // past seq_kv - 1 the mask hides nothing: clamped, so the kernel's row limits cannot overflow
        tab.q_pos0[b] = q_pos0 ? (q_pos0[b] < seq_kv[b] ? q_pos0[b] : seq_kv[b]) : 0;
        need_scores = need_scores || (seq_q[b] > 0 && attention_needs_scores(seq_q[b], seq_kv[b], dk));
    }
    if (n_seqs == 0) return hipSuccess;
    if (varlen_fused_ok(n_seqs, seq_kv, dk))
        return launch_attention_fused_many(Q, ldq, K, ldk, V, ldv, O, ldo, n_seqs, tab, q_pos0 != nullptr, n_heads, dk,
                                           scale, stream);
    if (need_scores && !scores) return hipErrorInvalidValue;
    for (int b = 0; b < n_seqs; ++b) {
        const hipError_t e = launch_attention(Q + q_row0[b] * ldq, ldq, K + kv_row0[b] * ldk, ldk, V + kv_row0[b] * ldv,
                                              ldv, O + q_row0[b] * ldo, ldo, seq_q[b], seq_kv[b], n_heads, dk, scale,
                                              q_pos0 ? q_pos0[b] : kNoMask, scores, stream);
        if (e) return e;
    }
    return hipSuccess;
}

// The decode launch over a batch of sequences (attention_decode.hip, DecodeMany): the host arrays are read HERE, into
// the table that travels in the kernel arguments -- nothing is copied to the device, allocated or synchronized, and a
// captured graph replays the values of the capture.  kv_slot == nullptr: slab b for sequence b; q_pos0 == nullptr: no
// mask.  Every check comes before the launch.
hipError_t launch_attention_batched(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                    const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo, int n_seqs,
                                    int rows_per_seq, const int *kv_slot, const int *seq_kv, const int *q_pos0,
                                    int n_heads, int dk, float scale, hipStream_t stream) {
    if (!Q || !K || !V || !O || !seq_kv || n_seqs < 0 || n_seqs > kDecodeMaxBatch || n_heads < 1 ||
        !attention_decode_ok(rows_per_seq, 1, dk) || rows_per_seq < 1 || dk < 1)
        return hipErrorInvalidValue;
    DecodeBatchTable tab = {};  // entries past n_seqs are never read; zeroed so the arguments are defined bytes
    for (int b = 0; b < n_seqs; ++b) {
        if (seq_kv[b] < 1 || !attention_decode_ok(rows_per_seq, seq_kv[b], dk) || (q_pos0 && q_pos0[b] < 0) ||
            (kv_slot && kv_slot[b] < 0))
            return hipErrorInvalidValue;
        tab.kv_slot[b] = kv_slot ? kv_slot[b] : b;
        tab.seq_kv[b] = seq_kv[b];
        // past seq_kv - 1 the mask hides nothing: clamped, so the kernel's row limit cannot overflow
        tab.q_pos0[b] = q_pos0 ? (q_pos0[b] < seq_kv[b] ? q_pos0[b] : seq_kv[b]) : 0;
    }
    if (n_seqs == 0) return hipSuccess;
    return launch_attention_decode_batched(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs,
                                           rows_per_seq, tab, q_pos0 != nullptr, n_heads, dk, scale, stream);
}

// The same launch through a per-row slab table in device memory (attention_decode.hip, DecodeIndirect).
// The host arrays are read HERE as above; the table's bytes are read by the kernel.  tab_row == nullptr: table row b
// for sequence b.  Every check comes before the launch: the batched launch's, and what keeps the kernel's table reads
// inside the table's rows (a stride that covers seq_kv[b] entries) and its clamp meaningful (1 <= n_slabs <= 64).
hipError_t launch_attention_indirect(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                     const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo, int n_seqs,
                                     int rows_per_seq, const uint8_t *row_slab, int64_t row_slab_stride, int n_slabs,
                                     const int *tab_row, const int *seq_kv, const int *q_pos0, int n_heads, int dk,
                                     float scale, hipStream_t stream) {
    if (!Q || !K || !V || !O || !seq_kv || !row_slab || n_seqs < 0 || n_seqs > kDecodeMaxBatch || n_heads < 1 ||
        !attention_decode_ok(rows_per_seq, 1, dk) || rows_per_seq < 1 || dk < 1 || n_slabs < 1 ||
        n_slabs > kDecodeMaxBatch)
        return hipErrorInvalidValue;
    DecodeBatchTable tab = {};  // kv_slot: the table row
    for (int b = 0; b < n_seqs; ++b) {
        if (seq_kv[b] < 1 || !attention_decode_ok(rows_per_seq, seq_kv[b], dk) || (q_pos0 && q_pos0[b] < 0) ||
            (tab_row && tab_row[b] < 0) || row_slab_stride < seq_kv[b])
            return hipErrorInvalidValue;
        tab.kv_slot[b] = tab_row ? tab_row[b] : b;
        tab.seq_kv[b] = seq_kv[b];
        tab.q_pos0[b] = q_pos0 ? (q_pos0[b] < seq_kv[b] ? q_pos0[b] : seq_kv[b]) : 0;
    }
    if (n_seqs == 0) return hipSuccess;
    return launch_attention_decode_indirect(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs,
                                            rows_per_seq, row_slab, row_slab_stride, n_slabs, tab, q_pos0 != nullptr,
                                            n_heads, dk, scale, stream);
}

}  // namespace qgemm
