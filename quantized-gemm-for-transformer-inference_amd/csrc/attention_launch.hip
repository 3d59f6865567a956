// attention_launch.hip -- which of the three attention launches a shape takes, for the transformer stack
// (transformer.hip) and the public qgemm_attention* entry points (api.hip): the decode launch for a few query rows
// (attention_decode.hip), one fused launch where it fits (attention.hip), else the three kernels it fuses, through
// `scores` -- the same bits on every path.  Host code only; it is a file of its own because it calls the fp32 GEMM
// launchers, which the programs that compile attention.hip's text alone do not link.
#include "qgemm_internal.h"

namespace qgemm {

const char *attention_plan_name(int seq_q, int seq_kv, int dk) {
    if (attention_decode_ok(seq_q, seq_kv, dk)) return "attention_decode_kernel";
    if (attention_decode_wide_ok(seq_q, seq_kv, dk)) return "attention_decode_wide_kernel";
    return attention_fused_ok(seq_kv, dk) ? "attention_fused_kernel" : "three_launches";
}

// scores only where some call can reach the three launches: never inside the fused envelope, and never with at most
// kAttnDecodeMaxQ query rows inside the decode envelope (a call of fewer rows or keys needs none either way).  The
// wide decode envelope (d_k 96 / 128) is left out on purpose: a forward at those widths still runs the three launches,
// and a decode-shaped public call brings the workspace as it did before the wide instantiation (which never touches it)
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

// ---- the decode launches over a table of sequences ----

// What every table launch checks and fills, ONE text for the multi-head, grouped and bf16-cache forms: the host arrays
// are read HERE, into the table that travels in the kernel arguments -- nothing is copied to the device, allocated or
// synchronized, and a captured graph replays the values of the capture.  slot == nullptr: slab (indirect: table row) b
// for sequence b; q_pos0 == nullptr: no mask.  indirect: also what keeps the kernel's table reads inside the table's
// rows (a stride that covers seq_kv[b] entries) and its clamp meaningful (1 <= n_slabs <= 64).
// max_kv: the launch's key limit -- 4096 for the sequential kernels (decode_table_from_host: the score row of
// attention_decode_any_ok), kSplitMaxSeq for the split-key launch.
hipError_t decode_table_from_host_max(int n_seqs, int rows_per_seq, int dk, const int *slot, const int *seq_kv,
                                      const int *q_pos0, bool indirect, const uint8_t *row_slab, int64_t row_slab_stride,
                                      int n_slabs, int max_kv, DecodeBatchTable &tab) {
    if (!seq_kv || n_seqs < 0 || n_seqs > kDecodeMaxBatch || rows_per_seq < 1 || dk < 1 ||
        !attention_decode_any_ok(rows_per_seq, 1, dk) ||
        (indirect && (!row_slab || n_slabs < 1 || n_slabs > kDecodeMaxBatch)))
        return hipErrorInvalidValue;
    tab = {};  // entries past n_seqs are never read; zeroed so the arguments are defined bytes
    for (int b = 0; b < n_seqs; ++b) {
        if (seq_kv[b] < 1 || seq_kv[b] > max_kv || (q_pos0 && q_pos0[b] < 0) || (slot && slot[b] < 0) ||
            (indirect && row_slab_stride < seq_kv[b]))
            return hipErrorInvalidValue;
        tab.kv_slot[b] = slot ? slot[b] : b;
        tab.seq_kv[b] = seq_kv[b];
        // past seq_kv - 1 the mask hides nothing: clamped, so the kernel's row limit cannot overflow
        tab.q_pos0[b] = q_pos0 ? (q_pos0[b] < seq_kv[b] ? q_pos0[b] : seq_kv[b]) : 0;
    }
    return hipSuccess;
}

// the six sequential table launches: 4096 keys
hipError_t decode_table_from_host(int n_seqs, int rows_per_seq, int dk, const int *slot, const int *seq_kv,
                                  const int *q_pos0, bool indirect, const uint8_t *row_slab, int64_t row_slab_stride,
                                  int n_slabs, DecodeBatchTable &tab) {
    return decode_table_from_host_max(n_seqs, rows_per_seq, dk, slot, seq_kv, q_pos0, indirect, row_slab,
                                      row_slab_stride, n_slabs, 4096, tab);
}

// The re-check of a built table where a kernel's LDS arrays and grid are sized (the launches that take a table: the
// transformer stack brings its own).  indirect: the table's row stride covers every sequence's entries.
bool decode_table_ok(const DecodeBatchTable &tab, int n_seqs, int rows_per_seq, int dk, bool indirect,
                     int64_t row_slab_stride) {
    if (n_seqs < 1 || n_seqs > kDecodeMaxBatch || rows_per_seq < 1 || dk < 1 ||
        !attention_decode_any_ok(rows_per_seq, 1, dk))
        return false;
    for (int b = 0; b < n_seqs; ++b)
        if (tab.seq_kv[b] < 1 || !attention_decode_any_ok(rows_per_seq, tab.seq_kv[b], dk) || tab.kv_slot[b] < 0 ||
            tab.q_pos0[b] < 0 || tab.q_pos0[b] > tab.seq_kv[b] ||
            (indirect && row_slab_stride < tab.seq_kv[b]))
            return false;
    return true;
}

// kv_slot == nullptr: slab b for sequence b; q_pos0 == nullptr: no mask.  Every check comes before the launch.
hipError_t launch_attention_batched(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                    const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo, int n_seqs,
                                    int rows_per_seq, const int *kv_slot, const int *seq_kv, const int *q_pos0,
                                    int n_heads, int dk, float scale, hipStream_t stream) {
    DecodeBatchTable tab;  // filled by decode_table_from_host, read only after its success
    if (!Q || !K || !V || !O || n_heads < 1 ||
        decode_table_from_host(n_seqs, rows_per_seq, dk, kv_slot, seq_kv, q_pos0, false, nullptr, 0, 0, tab))
        return hipErrorInvalidValue;
    if (n_seqs == 0) return hipSuccess;
    return launch_attention_decode_batched(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs,
                                           rows_per_seq, tab, q_pos0 != nullptr, n_heads, dk, scale, stream);
}

// The same launch through a per-row slab table in device memory (attention_decode.hip, DecodeIndirect):
// the table's bytes are read by the kernel.  tab_row == nullptr: table row b for sequence b.
hipError_t launch_attention_indirect(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                     const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo, int n_seqs,
                                     int rows_per_seq, const uint8_t *row_slab, int64_t row_slab_stride, int n_slabs,
                                     const int *tab_row, const int *seq_kv, const int *q_pos0, int n_heads, int dk,
                                     float scale, hipStream_t stream) {
    DecodeBatchTable tab;  // filled by decode_table_from_host (kv_slot: the table row), read only after its success
    if (!Q || !K || !V || !O || n_heads < 1 ||
        decode_table_from_host(n_seqs, rows_per_seq, dk, tab_row, seq_kv, q_pos0, true, row_slab, row_slab_stride,
                               n_slabs, tab))
        return hipErrorInvalidValue;
    if (n_seqs == 0) return hipSuccess;
    return launch_attention_decode_indirect(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs,
                                            rows_per_seq, row_slab, row_slab_stride, n_slabs, tab, q_pos0 != nullptr,
                                            n_heads, dk, scale, stream);
}

// ---- grouped-query attention ----

const char *attention_gqa_plan_name(int seq_q, int seq_kv, int dk, int n_heads, int n_kv_heads) {
    if (n_heads == n_kv_heads) return attention_plan_name(seq_q, seq_kv, dk);
    if (!attention_decode_gqa_ok(seq_q, seq_kv, dk, n_heads, n_kv_heads)) return "grouped_three_launches";
    return attention_decode_ok(seq_q, seq_kv, dk) ? "attention_decode_gqa_kernel" : "attention_decode_gqa_wide_kernel";
}

// q_pos0: kNoMask or the causal mask's offset.  Outside the decode kernel's envelope: launch_attention's three launches
// with batch = n_kv_heads, in G rounds.  Round j serves head j of every group: Q, O and the scores start j heads in and
// step a whole group per batch (G d_k columns, G seq_q x seq_kv scores), K and V step one KV head.  The scores end up
// laid out as launch_attention's, so ONE softmax runs over all n_heads x seq_q rows between the GEMM rounds.  Each
// head's GEMMs are launch_mm_f32_batched's on the operands launch_attention would hand it with K / V repeated, and the
// fp32 GEMM gives the same bits on every plan.
hipError_t launch_attention_gqa(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                                float *O, int64_t ldo, int seq_q, int seq_kv, int n_heads, int n_kv_heads, int dk,
                                float scale, int q_pos0, float *scores, hipStream_t stream) {
    if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads) return hipErrorInvalidValue;
    const int G = n_heads / n_kv_heads;
    if (G == 1) return launch_attention(Q, ldq, K, ldk, V, ldv, O, ldo, seq_q, seq_kv, n_heads, dk, scale, q_pos0, scores, stream);
    hipError_t e = launch_attention_decode_gqa(Q, ldq, K, ldk, V, ldv, O, ldo, seq_q, seq_kv, n_heads, n_kv_heads, dk,
                                               scale, q_pos0, stream);
    if (e != hipErrorNotSupported) return e;
    if (seq_q == 0) return hipSuccess;
    if (!scores) return hipErrorInvalidValue;
    const int64_t sbs = (int64_t)seq_q * seq_kv, gd = (int64_t)G * dk;
    // launch_attention's stride-envelope checks, for every round (the rounds' bases differ in alignment), before the
    // first launch
    for (int j = 0; j < G; ++j) {
        const MmF32Plan qk = mm_f32_plan(seq_q, seq_kv, dk, n_kv_heads, ldq, 1, gd, mm_f32_al16(Q + j * dk), 1, ldk, dk,
                                         mm_f32_al16(K));
        const MmF32Plan pv = mm_f32_plan(seq_q, dk, seq_kv, n_kv_heads, seq_kv, 1, G * sbs, mm_f32_al16(scores + j * sbs),
                                         ldv, 1, dk, mm_f32_al16(V));
        if (!mm_f32_strides_ok(qk, ldq, 1, 1, ldk, seq_kv, 1, seq_q, seq_kv, dk) ||
            !mm_f32_strides_ok(pv, seq_kv, 1, ldv, 1, ldo, 1, seq_q, dk, seq_kv))
            return hipErrorInvalidValue;
    }
    for (int j = 0; j < G; ++j)
        if ((e = launch_mm_f32_batched(Q + j * dk, ldq, 1, gd, K, 1, ldk, dk, scores + j * sbs, seq_kv, 1, G * sbs, seq_q,
                                       seq_kv, dk, n_kv_heads, stream)))
            return e;
    e = q_pos0 == kNoMask
            ? launch_softmax_rows(scores, scores, (int64_t)n_heads * seq_q, seq_kv, scale, stream)
            : launch_softmax_rows_causal(scores, scores, (int64_t)n_heads * seq_q, seq_kv, scale, seq_q, q_pos0, stream);
    if (e) return e;
    for (int j = 0; j < G; ++j)
        if ((e = launch_mm_f32_batched(scores + j * sbs, seq_kv, 1, G * sbs, V, ldv, 1, dk, O + j * dk, ldo, 1, gd, seq_q,
                                       dk, seq_kv, n_kv_heads, stream)))
            return e;
    return hipSuccess;
}

// ---- grouped-query prefill over a table of sequences ----

// one table launch serves a grouped call exactly when every sequence lies inside the kernel's envelope
bool attention_varlen_fused_gqa_ok(int n_seqs, const int *seq_kv, int dk) {
    for (int b = 0; b < n_seqs; ++b)
        if (!attention_fused_gqa_ok(seq_kv[b], dk)) return false;
    return attention_fused_gqa_ok(1, dk);
}

const char *attention_varlen_gqa_plan_name(int n_seqs, const int *seq_kv, int dk, int n_heads, int n_kv_heads) {
    if (n_heads == n_kv_heads) return attention_varlen_plan_name(n_seqs, seq_kv, dk);
    if (!attention_varlen_fused_gqa_ok(n_seqs, seq_kv, dk)) return "per_sequence";
    return dk <= 64 ? "attention_fused_gqa_kernel<many>" : "attention_fused_gqa_wide_kernel<many>";
}

// launch_attention_varlen's checks and table; the host arrays are read HERE, nothing is copied, allocated or
// synchronized.  Every check comes before the first launch (per sequence, the fp32 GEMMs' stride envelope alone is
// tested when its sequence is reached, as by launch_attention_varlen).
hipError_t launch_attention_varlen_gqa(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V,
                                       int64_t ldv, float *O, int64_t ldo, int n_seqs, const int64_t *q_row0,
                                       const int *seq_q, const int64_t *kv_row0, const int *seq_kv, const int *q_pos0,
                                       int n_heads, int n_kv_heads, int dk, float scale, float *scores,
                                       hipStream_t stream) {
    if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads) return hipErrorInvalidValue;
    if (n_kv_heads == n_heads)
        return launch_attention_varlen(Q, ldq, K, ldk, V, ldv, O, ldo, n_seqs, q_row0, seq_q, kv_row0, seq_kv, q_pos0,
                                       n_heads, dk, scale, scores, stream);
    if (!Q || !K || !V || !O || !q_row0 || !seq_q || !kv_row0 || !seq_kv || n_seqs < 0 || n_seqs > kVarlenMaxSeqs ||
        dk < 1)
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
        need_scores = need_scores ||
                      (seq_q[b] > 0 && !attention_decode_gqa_ok(seq_q[b], seq_kv[b], dk, n_heads, n_kv_heads));
    }
    if (n_seqs == 0) return hipSuccess;
    if (attention_varlen_fused_gqa_ok(n_seqs, seq_kv, dk))
        return launch_attention_fused_gqa_many(Q, ldq, K, ldk, V, ldv, O, ldo, n_seqs, tab, q_pos0 != nullptr, n_heads,
                                               n_kv_heads, dk, scale, stream);
    if (need_scores && !scores) return hipErrorInvalidValue;
    for (int b = 0; b < n_seqs; ++b) {
        const hipError_t e =
            launch_attention_gqa(Q + q_row0[b] * ldq, ldq, K + kv_row0[b] * ldk, ldk, V + kv_row0[b] * ldv, ldv,
                                 O + q_row0[b] * ldo, ldo, seq_q[b], seq_kv[b], n_heads, n_kv_heads, dk, scale,
                                 q_pos0 ? q_pos0[b] : kNoMask, scores, stream);
        if (e) return e;
    }
    return hipSuccess;
}

// ---- prefill tiled over the keys, online softmax ----

// launch_attention_varlen_gqa's checks with kSplitMaxSeq keys in the place of 4096 (G = 1 is served here too: nothing is
// rerouted), its table and clamp; then the one launch, which tests the envelope (d_k, the work map) again.  T: float
// (launch_attention_tiled) or bf16_t (launch_attention_tiled_kv16) -- one text for both tables.
template <typename T, typename Launch>
static hipError_t tiled_from_host(Launch launch, const float *Q, int64_t ldq, const T *K, int64_t ldk, const T *V,
                                  int64_t ldv, float *O, int64_t ldo, int n_seqs, const int64_t *q_row0, const int *seq_q,
                                  const int64_t *kv_row0, const int *seq_kv, const int *q_pos0, int n_heads,
                                  int n_kv_heads, int dk, float scale, hipStream_t stream) {
    if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads || !Q || !K || !V || !O || !q_row0 || !seq_q || !kv_row0 ||
        !seq_kv || n_seqs < 0 || n_seqs > kVarlenMaxSeqs || !attention_tiled_ok(1, dk))
        return hipErrorInvalidValue;
    FusedSeqTable tab = {};  // entries past n_seqs are never read; zeroed so the arguments are defined bytes
    for (int b = 0; b < n_seqs; ++b) {
        if (q_row0[b] < 0 || kv_row0[b] < 0 || seq_q[b] < 0 || !attention_tiled_ok(seq_kv[b], dk) ||
            (q_pos0 && q_pos0[b] < 0))
            return hipErrorInvalidValue;
        tab.q_row0[b] = q_row0[b];
        tab.kv_row0[b] = kv_row0[b];
        tab.seq_q[b] = seq_q[b];
        tab.seq_kv[b] = seq_kv[b];
        // past seq_kv - 1 the mask hides nothing: clamped, so the kernel's row limits cannot overflow
        tab.q_pos0[b] = q_pos0 ? (q_pos0[b] < seq_kv[b] ? q_pos0[b] : seq_kv[b]) : 0;
    }
    if (n_seqs == 0) return hipSuccess;
    return launch(Q, ldq, K, ldk, V, ldv, O, ldo, n_seqs, tab, q_pos0 != nullptr, n_heads, n_kv_heads, dk, scale, stream);
}

hipError_t launch_attention_tiled(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                                  float *O, int64_t ldo, int n_seqs, const int64_t *q_row0, const int *seq_q,
                                  const int64_t *kv_row0, const int *seq_kv, const int *q_pos0, int n_heads,
                                  int n_kv_heads, int dk, float scale, hipStream_t stream) {
    return tiled_from_host(launch_attention_tiled_many, Q, ldq, K, ldk, V, ldv, O, ldo, n_seqs, q_row0, seq_q, kv_row0,
                           seq_kv, q_pos0, n_heads, n_kv_heads, dk, scale, stream);
}

hipError_t launch_attention_tiled_kv16(const float *Q, int64_t ldq, const bf16_t *K, int64_t ldk, const bf16_t *V,
                                       int64_t ldv, float *O, int64_t ldo, int n_seqs, const int64_t *q_row0,
                                       const int *seq_q, const int64_t *kv_row0, const int *seq_kv, const int *q_pos0,
                                       int n_heads, int n_kv_heads, int dk, float scale, hipStream_t stream) {
    return tiled_from_host(launch_attention_tiled_kv16_many, Q, ldq, K, ldk, V, ldv, O, ldo, n_seqs, q_row0, seq_q,
                           kv_row0, seq_kv, q_pos0, n_heads, n_kv_heads, dk, scale, stream);
}

// decode_table_from_host's checks and table and the group check, then the grouped decode launch
static hipError_t batched_gqa(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                              const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo, int n_seqs,
                              int rows_per_seq, bool indirect, const uint8_t *row_slab, int64_t row_slab_stride,
                              int n_slabs, const int *slot, const int *seq_kv, const int *q_pos0, int n_heads,
                              int n_kv_heads, int dk, float scale, hipStream_t stream) {
    DecodeBatchTable tab;  // filled by decode_table_from_host, read only after its success
    if (!Q || !K || !V || !O || !attention_decode_gqa_ok(rows_per_seq, 1, dk, n_heads, n_kv_heads) ||
        decode_table_from_host(n_seqs, rows_per_seq, dk, slot, seq_kv, q_pos0, indirect, row_slab, row_slab_stride,
                               n_slabs, tab))
        return hipErrorInvalidValue;
    if (n_seqs == 0) return hipSuccess;
    if (indirect)
        return launch_attention_decode_indirect_gqa(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs,
                                                    rows_per_seq, row_slab, row_slab_stride, n_slabs, tab,
                                                    q_pos0 != nullptr, n_heads, n_kv_heads, dk, scale, stream);
    return launch_attention_decode_batched_gqa(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs,
                                               rows_per_seq, tab, q_pos0 != nullptr, n_heads, n_kv_heads, dk, scale,
                                               stream);
}

hipError_t launch_attention_batched_gqa(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                        const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                        int n_seqs, int rows_per_seq, const int *kv_slot, const int *seq_kv,
                                        const int *q_pos0, int n_heads, int n_kv_heads, int dk, float scale,
                                        hipStream_t stream) {
    if (n_heads >= 1 && n_kv_heads == n_heads)
        return launch_attention_batched(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs, rows_per_seq,
                                        kv_slot, seq_kv, q_pos0, n_heads, dk, scale, stream);
    return batched_gqa(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs, rows_per_seq, false, nullptr,
                       0, 0, kv_slot, seq_kv, q_pos0, n_heads, n_kv_heads, dk, scale, stream);
}

hipError_t launch_attention_indirect_gqa(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                         const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                         int n_seqs, int rows_per_seq, const uint8_t *row_slab, int64_t row_slab_stride,
                                         int n_slabs, const int *tab_row, const int *seq_kv, const int *q_pos0,
                                         int n_heads, int n_kv_heads, int dk, float scale, hipStream_t stream) {
    if (n_heads >= 1 && n_kv_heads == n_heads)
        return launch_attention_indirect(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs,
                                         rows_per_seq, row_slab, row_slab_stride, n_slabs, tab_row, seq_kv, q_pos0,
                                         n_heads, dk, scale, stream);
    return batched_gqa(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs, rows_per_seq, true, row_slab,
                       row_slab_stride, n_slabs, tab_row, seq_kv, q_pos0, n_heads, n_kv_heads, dk, scale, stream);
}

// ---- split-key decode attention ----

const char *attention_split_plan_name(int dk) {
    return dk <= 64 ? "attention_decode_split_kernel" : "attention_decode_split_wide_kernel";
}

// The rule of include/qgemm.h, in integers.  W: the workgroups of an unsplit launch; want: the splits per row that bring
// the launch to 512 workgroups, two per CU on 256 CUs -- a round figure that rests on no measurement.
int attention_split_default_keys(int n_seqs, int rows_per_seq, int max_seq_kv, int n_heads, int n_kv_heads) {
    const int group = n_heads / n_kv_heads;
    const int64_t w = (int64_t)n_seqs * rows_per_seq * n_kv_heads * ((group + 3) / 4);
    const int64_t want = (512 + w - 1) / w;
    const int64_t keys = (max_seq_kv + want - 1) / want;
    const int64_t split = (keys + kSplitStep - 1) / kSplitStep * kSplitStep;
    return (int)(split < kSplitStep ? kSplitStep : split > kSplitMaxKeys ? kSplitMaxKeys : split);
}

size_t attention_split_workspace_bytes(int n_seqs, int rows_per_seq, int max_seq_kv, int n_heads, int dk, int split) {
    return (size_t)n_seqs * rows_per_seq * n_heads * ((max_seq_kv + split - 1) / split) * (dk + 2) * sizeof(float);
}

// decode_table_from_host's checks and table with kSplitMaxSeq keys, the group check from G = 1, the split and the
// workspace it needs for the batch's longest sequence; then the two launches.  T: float (launch_attention_decode_split)
// or bf16_t (launch_attention_decode_split_kv16) -- one text, so both resolve split_keys == 0 alike.
template <typename T, typename Launch>
static hipError_t split_from_host(Launch launch, const float *Q, int64_t ldq, const T *K, int64_t ldk,
                                  int64_t k_stride_seq, const T *V, int64_t ldv, int64_t v_stride_seq, float *O,
                                  int64_t ldo, int n_seqs, int rows_per_seq, const int *kv_slot, const int *seq_kv,
                                  const int *q_pos0, int n_heads, int n_kv_heads, int dk, float scale, int split_keys,
                                  void *workspace, size_t ws_bytes, hipStream_t stream) {
    DecodeBatchTable tab;  // filled by decode_table_from_host_max, read only after its success
    if (!Q || !K || !V || !O || !attention_split_ok(1, rows_per_seq, 1, dk, n_heads, n_kv_heads) ||
        (split_keys != 0 && !split_keys_ok(split_keys)) ||
        decode_table_from_host_max(n_seqs, rows_per_seq, dk, kv_slot, seq_kv, q_pos0, false, nullptr, 0, 0, kSplitMaxSeq,
                                   tab))
        return hipErrorInvalidValue;
    if (n_seqs == 0) return hipSuccess;
    int max_kv = 1;
    for (int b = 0; b < n_seqs; ++b) max_kv = seq_kv[b] > max_kv ? seq_kv[b] : max_kv;
    const int split =
        split_keys ? split_keys : attention_split_default_keys(n_seqs, rows_per_seq, max_kv, n_heads, n_kv_heads);
    if (!workspace || ws_bytes < attention_split_workspace_bytes(n_seqs, rows_per_seq, max_kv, n_heads, dk, split))
        return hipErrorInvalidValue;
    return launch(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs, rows_per_seq, tab,
                  q_pos0 != nullptr, n_heads, n_kv_heads, dk, scale, split, static_cast<float *>(workspace), ws_bytes,
                  stream);
}

hipError_t launch_attention_split(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                  const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo, int n_seqs,
                                  int rows_per_seq, const int *kv_slot, const int *seq_kv, const int *q_pos0, int n_heads,
                                  int n_kv_heads, int dk, float scale, int split_keys, void *workspace, size_t ws_bytes,
                                  hipStream_t stream) {
    return split_from_host(launch_attention_decode_split, Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo,
                           n_seqs, rows_per_seq, kv_slot, seq_kv, q_pos0, n_heads, n_kv_heads, dk, scale, split_keys,
                           workspace, ws_bytes, stream);
}

hipError_t launch_attention_split_kv16(const float *Q, int64_t ldq, const bf16_t *K, int64_t ldk, int64_t k_stride_seq,
                                       const bf16_t *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                       int n_seqs, int rows_per_seq, const int *kv_slot, const int *seq_kv,
                                       const int *q_pos0, int n_heads, int n_kv_heads, int dk, float scale, int split_keys,
                                       void *workspace, size_t ws_bytes, hipStream_t stream) {
    return split_from_host(launch_attention_decode_split_kv16, Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O,
                           ldo, n_seqs, rows_per_seq, kv_slot, seq_kv, q_pos0, n_heads, n_kv_heads, dk, scale, split_keys,
                           workspace, ws_bytes, stream);
}

}  // namespace qgemm
