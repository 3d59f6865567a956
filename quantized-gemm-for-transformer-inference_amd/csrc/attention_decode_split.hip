// attention_decode_split.hip -- split-key decode attention.  The sequential decode kernels give one
// workgroup ALL keys of its (head block, row, sequence): the score row in LDS stops them at 4096 keys, and a small batch
// leaves most of the 256 CUs idle (s29, s30).  Here the keys of one row are cut into runs of `split` keys (128 .. 1024),
// every run goes to a workgroup of its own, and a second kernel merges the runs' partial softmaxes, as flash-decoding
// does.  The result is NOT the sequential kernels' bit for bit; its own definition (include/qgemm.h):
//   row r of sequence b sees keys 0 .. lim - 1, lim = min(seq_kv, q_pos0 + r + 1) (no mask: seq_kv); split s covers keys
//   [s split, min((s + 1) split, lim)) and gives, per query head,
//     m_s    = max fl(score * scale)              strict >, from -inf: a NaN score never wins
//     l_s    = sum exp(fl(fl(score * scale) - m_s))      per-lane sums in key order with stride 64, then six butterfly adds
//     a_s[c] = sum exp(..) * V[key][c]            one fmaf chain per column over the split's keys ascending, from +0
//   and the merge gives O[c] = (sum_s w_s a_s[c]) / (sum_s w_s l_s), w_s = exp(m_s - max_s m_s), both sums fmaf chains from
//   +0 with s ascending.  A key at or past lim is never part of any sum.
// attention_decode_split_kernel<causal, kW>: ONE WORKGROUP of 256 threads owns ONE (KV head, block of up to 4 query heads
// of its group, row, sequence, split) -- attention_decode_gqa_kernel's block geometry (attention_decode_gqa.hip), its
// constants, its tables in the kernel arguments, its stream (K chunks then V chunks, two chunks in flight in registers,
// the branch-free clamped fetch, zeros selected in `put`).  What the split changes:
//   * the score rows are 4 x 1024 floats, 16 KiB instead of 64;
//   * kW = 128 stages 64-key chunks (33 KiB instead of 66): 51 KiB of LDS at BOTH widths, three workgroups per CU by LDS
//     (the grouped kernel: one), and 8 float4 pieces per thread and chunk in flight at both widths;
//   * scores: kW = 64 as the grouped kernel (thread = key x head pair, 128 keys); kW = 128 thread = key x head (lane = key
//     of the 64-key chunk, wave = head), one chain per thread, all 256 threads busy;
//   * softmax: wave w owns head w; the maximum by butterflies, the sum as per-lane partial sums and butterflies -- no
//     serial chain, no divide (the merge normalises);
//   * P V runs over the split's keys alone and is stored unnormalised.
// No matrix instructions: a workgroup's M dimension is its <= 4 (head, row) pairs, so three quarters of a 16-row
// v_mfma_f32_16x16x4_f32 tile would be padding, and the kernel waits on its loads, not on the VALU (s16, s29).
// attention_decode_merge_kernel: one wave per (sequence, row, head) reads the row's S = ceil(lim / split) records --
// exactly the ones the first kernel wrote: a workgroup whose split starts at or past lim returns without writing.
// Workspace: records of d_k + 2 floats, [sequence][row][head][split] (the split dimension sized for the batch's longest
// sequence): m, l, a[0 .. d_k - 1].
// Built with the packed fp32 instructions off, as attention_decode_gqa.o (Makefile).
#include "attention_decode_kernel.h"

namespace qgemm {

namespace {

// the record of (query row `row` of the launch, head h, split s)
__device__ __forceinline__ int64_t split_record(int64_t row, int n_heads, int h, int ws_splits, int s, int dk) {
    return ((row * n_heads + h) * ws_splits + s) * (dk + 2);
}

// group: G.  grid x = n_kv_heads * ceil(G / 4), y = rows * sequences, z = the most splits a row of the batch has.
// split: keys per split.  ws_splits: the workspace's split dimension.
template <bool kCausal, int kW>
__global__ __launch_bounds__(kDecThreads) void attention_decode_split_kernel(
    const float *__restrict__ Q, int64_t ldq, const float *__restrict__ K, int64_t ldk, const float *__restrict__ V,
    int64_t ldv, float *__restrict__ ws, int dk, float scale, int group, int n_heads, int split, int ws_splits,
    DecodeMany seqs) {
    constexpr int kChunk = kW == 64 ? 128 : 64;                       // keys per staged K / V chunk
    constexpr int kPieces = kW / 4, kShift = kW == 64 ? 4 : 5;       // float4 pieces of a row: f >> kShift = the key
    constexpr int kStride = kW + 4;                                   // chunk row stride (floats), = 4 mod 32
    constexpr int kPer = kChunk * kPieces / kDecThreads;              // float4 pieces of a chunk per thread: 8
    __shared__ __attribute__((aligned(16))) float S[kDecGroupHeads][kSplitMaxKeys];
    __shared__ __attribute__((aligned(16))) float KV[kChunk * kStride];
    __shared__ __attribute__((aligned(16))) float Qs[kDecGroupHeads][kW];
    const int rows = seqs.rows_per_seq;
    const int b = blockIdx.y / rows, qi = blockIdx.y - b * rows;
    const int seq = seqs.tab.seq_kv[b];
    // the row's limit (q_pos0 <= seq_kv: the launcher clamps it, so the sum stays in int range)
    const int lim = kCausal ? min(seq, qi + seqs.tab.q_pos0[b] + 1) : seq;
    const int k0 = blockIdx.z * split;
    if (k0 >= lim) return;  // no key of this split is visible: nothing is written (the merge reads ceil(lim / split))
    const int k1 = min(k0 + split, lim), n = k1 - k0;  // the split's keys k0 .. k1 - 1: 1 <= n <= split
    const int nc = (n + kChunk - 1) / kChunk;            // K chunks, and V chunks
    const int nblk = (group + kDecGroupHeads - 1) / kDecGroupHeads;
    const int kvh = blockIdx.x / nblk, blk = blockIdx.x - kvh * nblk;
    const int h0 = kvh * group + kDecGroupHeads * blk;                // the block's first query head
    const int nh = min(kDecGroupHeads, group - kDecGroupHeads * blk); // its heads: 1 .. 4
    const int64_t qrow = (int64_t)b * rows + qi, slab = seqs.tab.kv_slot[b];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float *Qb = Q + qrow * ldq + (int64_t)h0 * dk;
    const float *Kb = K + slab * seqs.k_stride_seq + (int64_t)kvh * dk;
    const float *Vb = V + slab * seqs.v_stride_seq + (int64_t)kvh * dk;
    const int dk4 = (dk + 3) >> 2;  // float4 columns of a row (the last one zero-padded)

    // ---- the K / V stream over keys k0 .. k1 - 1: attention_decode_gqa_kernel's fetch / put / two chunks in flight.
    // Every address is clamped into the split (row to k1 - 1 < seq_kv, column to d_k - 1); `put` writes zeros past k1 and
    // past d_k, so nothing a key at or past lim holds -- a NaN, an infinity -- reaches LDS.
    auto aligned = [&](const float *base, int64_t ld) {
        return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && (ld & 3) == 0 && (dk & 3) == 0;
    };
    const bool vec_k = aligned(Kb, ldk), vec_v = aligned(Vb, ldv);  // workgroup-uniform
    auto fetch = [&](float4 (&r)[kPer], const float *src, int64_t ld, int c0, bool vec) __attribute__((always_inline)) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const int f = t + i * kDecThreads, row = f >> kShift, c4 = f & (kPieces - 1);
                r[i] = *reinterpret_cast<const float4 *>(src + min(c0 + row, k1 - 1) * ld + 4 * min(c4, dk4 - 1));
            }
        } else {
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const int f = t + i * kDecThreads, row = f >> kShift, c4 = f & (kPieces - 1);
                const float *p = src + min(c0 + row, k1 - 1) * ld;
                r[i].x = p[min(4 * c4, dk - 1)];
                r[i].y = p[min(4 * c4 + 1, dk - 1)];
                r[i].z = p[min(4 * c4 + 2, dk - 1)];
                r[i].w = p[min(4 * c4 + 3, dk - 1)];
            }
        }
    };
    auto put = [&](const float4 (&r)[kPer], int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int f = t + i * kDecThreads, row = f >> kShift, c4 = f & (kPieces - 1);
            const bool in = c0 + row < k1;
            const float4 x = r[i];
            float4 v;
            v.x = in && 4 * c4 < dk ? x.x : 0.0f;
            v.y = in && 4 * c4 + 1 < dk ? x.y : 0.0f;
            v.z = in && 4 * c4 + 2 < dk ? x.z : 0.0f;
            v.w = in && 4 * c4 + 3 < dk ? x.w : 0.0f;
            *reinterpret_cast<float4 *>(KV + row * kStride + 4 * c4) = v;
        }
    };
    // chunk g of the stream: K chunk g, then V chunk g - nc
    auto fetch_g = [&](float4 (&r)[kPer], int g) __attribute__((always_inline)) {
        if (g < nc) fetch(r, Kb, ldk, k0 + g * kChunk, vec_k);
        else if (g < 2 * nc) fetch(r, Vb, ldv, k0 + (g - nc) * kChunk, vec_v);
    };
    float4 pfa[kPer], pfb[kPer];
    fetch_g(pfa, 0);
    fetch_g(pfb, 1);
    // the block's query rows, zeros past d_k and in the rows of heads the block does not have
    for (int i = t; i < kDecGroupHeads * kW; i += kDecThreads) {
        const int hh = i / kW, c = i & (kW - 1);
        Qs[hh][c] = hh < nh && c < dk ? Qb[(int64_t)hh * dk + c] : 0.0f;
    }

    // ---- s_h[j] = Q_h . K[k0 + j], j < n: the fmaf chain from +0 over k ascending, d_k zero-padded to 32 (the sequential
    // kernels' `steps`).  kW = 64: thread t owns key t & 127 of the chunk and the head pair 2 (t >> 7), the K row read
    // from LDS once for both chains.  kW = 128: lane = key of the 64-key chunk, wave = head, one chain.
    const bool more = dk > (kW == 64 ? 32 : 96);
    auto k_step = [&](float4 (&pf)[kPer], int c) __attribute__((always_inline)) {
        if (c) __syncthreads();  // every thread is done with the previous chunk
        put(pf, k0 + c * kChunk);
        __syncthreads();
        fetch_g(pf, c + 2);
        const int key = t & (kChunk - 1), j = c * kChunk + key;
        const float4 *kr = reinterpret_cast<const float4 *>(KV + key * kStride);
        if constexpr (kW == 64) {
            const int pair = wave >> 1;
            if (2 * pair < nh && j < n) {
                const float4 *q0 = reinterpret_cast<const float4 *>(Qs[2 * pair]);
                const float4 *q1 = reinterpret_cast<const float4 *>(Qs[2 * pair + 1]);
                float res0 = 0.0f, res1 = 0.0f;
                auto steps = [&](int s0) __attribute__((always_inline)) {
#pragma unroll
                    for (int s = s0; s < s0 + 8; ++s) {
                        const float4 kk = kr[s], a0 = q0[s], a1 = q1[s];
                        res0 = fmaf(a0.x, kk.x, res0);
                        res0 = fmaf(a0.y, kk.y, res0);
                        res0 = fmaf(a0.z, kk.z, res0);
                        res0 = fmaf(a0.w, kk.w, res0);
                        res1 = fmaf(a1.x, kk.x, res1);
                        res1 = fmaf(a1.y, kk.y, res1);
                        res1 = fmaf(a1.z, kk.z, res1);
                        res1 = fmaf(a1.w, kk.w, res1);
                    }
                };
                steps(0);
                if (more) steps(8);
                S[2 * pair][j] = res0;
                S[2 * pair + 1][j] = res1;
            }
        } else {
            if (wave < nh && j < n) {
                const float4 *q0 = reinterpret_cast<const float4 *>(Qs[wave]);
                float res = 0.0f;
                auto steps = [&](int s0) __attribute__((always_inline)) {
#pragma unroll
                    for (int s = s0; s < s0 + 8; ++s) {
                        const float4 kk = kr[s], a0 = q0[s];
                        res = fmaf(a0.x, kk.x, res);
                        res = fmaf(a0.y, kk.y, res);
                        res = fmaf(a0.z, kk.z, res);
                        res = fmaf(a0.w, kk.w, res);
                    }
                };
                steps(0);
                steps(8);
                steps(16);
                if (more) steps(24);
                S[wave][j] = res;
            }
        }
    };
    for (int c = 0; c < nc; c += 2) {
        k_step(pfa, c);
        if (c + 1 < nc) k_step(pfb, c + 1);
    }
    __syncthreads();

    // ---- the partial softmax of head `wave` over its n scores, in place: everything is wave-local.  m from -inf with
    // the strict > (softmax_row_max), the exps by softmax_exp, l as 64 per-lane sums (keys lane, lane + 64, .. in order)
    // and six butterfly adds -- fl(a + b) = fl(b + a), so every lane ends with the same bits.
    const int64_t rec0 = split_record(qrow, n_heads, h0, ws_splits, blockIdx.z, dk);
    const int64_t rec_h = (int64_t)ws_splits * (dk + 2);  // from a head's record to the next head's
    if (wave < nh) {
        float *row = S[wave];
        const float mx = softmax_row_max(row, lane, n, 64, scale);
        float part = 0.0f;
        for (int c = lane; c < n; c += 64) {
            const float e = softmax_exp(row[c], scale, mx);
            row[c] = e;
            part = __fadd_rn(part, e);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) part = __fadd_rn(part, __shfl_xor(part, off, 64));
        if (lane == 0) {
            float *rec = ws + rec0 + wave * rec_h;
            rec[0] = mx;
            rec[1] = part;
        }
    }

    // ---- a_h = p_h V over the split's keys: lane = output column, the accumulators carried across the chunks in key
    // order.  kW = 64: wave w carries head w.  kW = 128: wave w carries columns 64 (w & 1) .. + 63 of heads 2 (w >> 1) and
    // + 1, one V element from LDS feeding both chains.  (A second head the block lacks: its chain runs on a score row
    // nobody wrote and is not stored.)
    const int hd = kW == 64 ? wave : 2 * (wave >> 1);       // the (first) head this wave carries
    const bool pv = hd < nh, two = kW == 128 && hd + 1 < nh;
    const int col = kW == 64 ? lane : 64 * (wave & 1) + lane;
    float acc0 = 0.0f, acc1 = 0.0f;
    auto v_step = [&](float4 (&pf)[kPer], int c) __attribute__((always_inline)) {
        __syncthreads();  // P complete (c = 0) / the previous chunk consumed
        put(pf, k0 + c * kChunk);
        __syncthreads();
        fetch_g(pf, nc + c + 2);
        if (pv) {
            const int j0 = c * kChunk, kn = min(kChunk, n - j0);
            const float *vcol = KV + col, *p0 = S[hd] + j0;
            const float *p1 = S[kW == 64 ? hd : hd + 1] + j0;
            int k = 0;
            for (; k + 8 <= kn; k += 8) {
                const float4 a0 = *reinterpret_cast<const float4 *>(p0 + k);
                const float4 a1 = *reinterpret_cast<const float4 *>(p0 + k + 4);
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = vcol[(k + u) * kStride];
                acc0 = fmaf(a0.x, v[0], acc0);
                acc0 = fmaf(a0.y, v[1], acc0);
                acc0 = fmaf(a0.z, v[2], acc0);
                acc0 = fmaf(a0.w, v[3], acc0);
                acc0 = fmaf(a1.x, v[4], acc0);
                acc0 = fmaf(a1.y, v[5], acc0);
                acc0 = fmaf(a1.z, v[6], acc0);
                acc0 = fmaf(a1.w, v[7], acc0);
                if constexpr (kW == 128) {
                    const float4 b0 = *reinterpret_cast<const float4 *>(p1 + k);
                    const float4 b1 = *reinterpret_cast<const float4 *>(p1 + k + 4);
                    acc1 = fmaf(b0.x, v[0], acc1);
                    acc1 = fmaf(b0.y, v[1], acc1);
                    acc1 = fmaf(b0.z, v[2], acc1);
                    acc1 = fmaf(b0.w, v[3], acc1);
                    acc1 = fmaf(b1.x, v[4], acc1);
                    acc1 = fmaf(b1.y, v[5], acc1);
                    acc1 = fmaf(b1.z, v[6], acc1);
                    acc1 = fmaf(b1.w, v[7], acc1);
                }
            }
            for (; k < kn; ++k) {
                const float v = vcol[k * kStride];
                acc0 = fmaf(p0[k], v, acc0);
                if constexpr (kW == 128) acc1 = fmaf(p1[k], v, acc1);
            }
        }
    };
    // V chunk c is chunk nc + c of the stream: it sits in pfa when nc + c is even
    auto v_phase = [&](float4 (&first)[kPer], float4 (&second)[kPer]) __attribute__((always_inline)) {
        for (int c = 0; c < nc; c += 2) {
            v_step(first, c);
            if (c + 1 < nc) v_step(second, c + 1);
        }
    };
    if (nc & 1) v_phase(pfb, pfa);
    else v_phase(pfa, pfb);
    // the a-row: a wave's 64 lanes store 256 contiguous bytes (lane = column, so a float4 store would first need a
    // transpose across lanes, and a record of d_k + 2 floats leaves every other one off a 16-byte boundary)
    if (pv && col < dk) {
        float *a = ws + rec0 + hd * rec_h + 2 + col;
        a[0] = acc0;
        if (two) a[rec_h] = acc1;
    }
}

// One wave per (head, row of a sequence): grid x = heads, y = rows * sequences.  Lane l owns output columns l and l + 64.
__global__ __launch_bounds__(64) void attention_decode_merge_kernel(const float *__restrict__ ws, float *__restrict__ O,
                                                                    int64_t ldo, int dk, int n_heads, int split,
                                                                    int ws_splits, int causal, DecodeMany seqs) {
    const int rows = seqs.rows_per_seq, h = blockIdx.x;
    const int b = blockIdx.y / rows, qi = blockIdx.y - b * rows, lane = threadIdx.x;
    const int seq = seqs.tab.seq_kv[b];
    const int lim = causal ? min(seq, qi + seqs.tab.q_pos0[b] + 1) : seq;
    const int ns = (lim + split - 1) / split;  // the records the first kernel wrote for this row: 1 .. ws_splits
    const int64_t qrow = (int64_t)b * rows + qi;
    const int w = dk + 2;
    const float *rec = ws + split_record(qrow, n_heads, h, ws_splits, 0, dk);
    // M = max_s m_s: the m column in strides of 64, then butterflies (an m is never NaN: the strict > from -inf)
    float mx = -INFINITY;
    for (int s = lane; s < ns; s += 64) {
        const float x = rec[(int64_t)s * w];
        mx = (x > mx) ? x : mx;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(mx, off, 64);
        mx = (o > mx) ? o : mx;
    }
    // the two serial sums over s ascending; lane u of a block of 64 splits makes w_s and reads l_s for split s0 + u.
    // With ns == 1: m_0 - M = 0, w_0 = exp(0) = 1 and fmaf(1, a, +0) = a.
    float acc0 = 0.0f, acc1 = 0.0f, den = 0.0f;
    for (int s0 = 0; s0 < ns; s0 += 64) {
        const float *mine = rec + (int64_t)min(s0 + lane, ns - 1) * w;
        const float w_l = softmax_exp(mine[0], 1.0f, mx), l_l = mine[1];
        const int nu = min(64, ns - s0);
        for (int u = 0; u < nu; ++u) {
            const float ws_u = __shfl(w_l, u, 64), l_u = __shfl(l_l, u, 64);
            const float *a = rec + (int64_t)(s0 + u) * w + 2;
            den = fmaf(ws_u, l_u, den);
            if (lane < dk) acc0 = fmaf(ws_u, a[lane], acc0);
            if (lane + 64 < dk) acc1 = fmaf(ws_u, a[lane + 64], acc1);
        }
    }
    float *o = O + qrow * ldo + (int64_t)h * dk;
    if (lane < dk) o[lane] = __fdiv_rn(acc0, den);
    if (lane + 64 < dk) o[lane + 64] = __fdiv_rn(acc1, den);
}

}  // namespace

bool attention_split_ok(int n_seqs, int rows_per_seq, int max_seq_kv, int dk, int n_heads, int n_kv_heads) {
    return n_seqs >= 1 && n_seqs <= kDecodeMaxBatch && rows_per_seq >= 1 && dk >= 1 && max_seq_kv >= 1 &&
           max_seq_kv <= kSplitMaxSeq && attention_decode_any_ok(rows_per_seq, 1, dk) &&
           groups_ok(n_heads, n_kv_heads, 1);
}

// What sizes the grid, the kernels' LDS rows and the workspace records of a split-key launch, tested again on the
// built table: ws_splits = the workspace's split dimension, grid_z = the most splits a row of the batch has
hipError_t attention_split_launch_dims(int n_seqs, int rows_per_seq, const DecodeBatchTable &tab, bool causal,
                                       int n_heads, int n_kv_heads, int dk, int split, const float *workspace,
                                       size_t ws_bytes, int &ws_splits, int &grid_z) {
    if (!workspace || !split_keys_ok(split) || !attention_split_ok(n_seqs, rows_per_seq, 1, dk, n_heads, n_kv_heads))
        return hipErrorInvalidValue;
    int max_kv = 1, max_lim = 1;
    for (int b = 0; b < n_seqs; ++b) {
        if (tab.seq_kv[b] < 1 || tab.seq_kv[b] > kSplitMaxSeq || tab.kv_slot[b] < 0 || tab.q_pos0[b] < 0 ||
            tab.q_pos0[b] > tab.seq_kv[b])
            return hipErrorInvalidValue;
        const int seen = causal ? (tab.q_pos0[b] + rows_per_seq < tab.seq_kv[b] ? tab.q_pos0[b] + rows_per_seq
                                                                               : tab.seq_kv[b])
                                : tab.seq_kv[b];  // the last row's limit: the sequence's most visible keys
        max_kv = tab.seq_kv[b] > max_kv ? tab.seq_kv[b] : max_kv;
        max_lim = seen > max_lim ? seen : max_lim;
    }
    if (ws_bytes < attention_split_workspace_bytes(n_seqs, rows_per_seq, max_kv, n_heads, dk, split))
        return hipErrorInvalidValue;
    ws_splits = (max_kv + split - 1) / split;
    grid_z = (max_lim + split - 1) / split;
    return hipSuccess;
}

// the second launch of a split-key call: one wave per (head, row of a sequence) over the records the first one wrote
hipError_t launch_attention_decode_merge(const float *workspace, float *O, int64_t ldo, int n_seqs, int rows_per_seq,
                                         const DecodeBatchTable &tab, bool causal, int n_heads, int dk, int split,
                                         int ws_splits, hipStream_t stream) {
    const DecodeMany many{0, 0, rows_per_seq, tab};  // (the merge reads no K / V: the strides are not used)
    attention_decode_merge_kernel<<<dim3((unsigned)n_heads, (unsigned)(rows_per_seq * n_seqs)), 64, 0, stream>>>(
        workspace, O, ldo, dk, n_heads, split, ws_splits, causal ? 1 : 0, many);
    return hipGetLastError();
}

// tab: checked and clamped by launch_attention_split (attention_launch.hip)
hipError_t launch_attention_decode_split(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                         const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                         int n_seqs, int rows_per_seq, const DecodeBatchTable &tab, bool causal,
                                         int n_heads, int n_kv_heads, int dk, float scale, int split, float *workspace,
                                         size_t ws_bytes, hipStream_t stream) {
    int ws_splits, grid_z;
    if (attention_split_launch_dims(n_seqs, rows_per_seq, tab, causal, n_heads, n_kv_heads, dk, split, workspace, ws_bytes,
                                    ws_splits, grid_z))
        return hipErrorInvalidValue;
    const int group = n_heads / n_kv_heads;
    const DecodeMany many{k_stride_seq, v_stride_seq, rows_per_seq, tab};
    const dim3 grid((unsigned)(n_kv_heads * ((group + kDecGroupHeads - 1) / kDecGroupHeads)),
                    (unsigned)(rows_per_seq * n_seqs), (unsigned)grid_z);
    auto *kernel = dk > kDecMaxDk ? (causal ? attention_decode_split_kernel<true, kDecWideDk>
                                            : attention_decode_split_kernel<false, kDecWideDk>)
                                  : (causal ? attention_decode_split_kernel<true, kDecMaxDk>
                                            : attention_decode_split_kernel<false, kDecMaxDk>);
    kernel<<<grid, kDecThreads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, workspace, dk, scale, group, n_heads, split,
                                             ws_splits, many);
    hipError_t e = hipGetLastError();
    if (e) return e;
    return launch_attention_decode_merge(workspace, O, ldo, n_seqs, rows_per_seq, tab, causal, n_heads, dk, split,
                                         ws_splits, stream);
}

}  // namespace qgemm
