// attention_gqa.hip -- the fused prefill attention for grouped-query heads: attention_fused_kernel
// (attention.hip) with a head map and the row width as a compile-time parameter, over a table of sequences.  Q and O
// have n_heads * d_k columns, K and V n_kv_heads * d_k; query head h reads KV head h / G, G = n_heads / n_kv_heads.
// For every (sequence, query head, 32-query tile) a workgroup computes S = Q_h K_{h/G}^T, P = softmax(S * scale) and
// O[:, h*d_k..] = P V_{h/G} with S and P kept in LDS -- ONE launch where the grouped three launches
// (attention_launch.hip launch_attention_gqa) take 2 G + 1 per sequence and send the scores through HBM twice.
// A text of its own, not a fold into attention.hip: attention.o keeps its instruction stream.
// Contract: nothing new numerically.  The rows of query head h are bit for bit attention_fused_kernel's -- and so the
// three launches' -- on K and V with every head repeated G times:
//   * both products are v_mfma_f32_16x16x4_f32 chains from +0 over k ascending; Q K^T over d_k zero-padded to a
//     multiple of 32 (8 or 16 k-steps at kW 64, 24 or 32 at kW 128), P V over ALL of seq_kv zero-padded to 32;
//   * the max and exp by the contract at softmax_row_max (qgemm_internal.h), ONE sequential fp32 sum in column order
//     (the hop_left chain of attention.hip, unchanged in arithmetic), then fl(e / sum);
//   * under the mask P = +0 past a row's limit and those keys still contribute fmaf(+0, v, acc).
// Envelope: seq_kv <= 512 per sequence; d_k <= 64 (kW 64) or d_k 96 / 128 (kW 128); any G >= 2 that divides n_heads;
// any seq_q; up to kVarlenMaxSeqs sequences.
// Geometry (GqaTile): 1024 threads, 32 query rows, the S tile 32 x 516 floats in LDS at both widths.
//   kW 64 : the narrow kernel's -- 256-key K / V chunks (strides 68 / 80), Q stride 68; in Q K^T wave w owns column
//           tile w of the chunk for both row fragments (two A fragments of <= 16 k-steps, one B fragment).
//   kW 128: a 256-key chunk does not fit beside the 64-KiB S tile, so 128-key chunks (K stride 132 = 4 mod 32, V stride
//           144 = 16 mod 32: the same bank patterns as 68 / 80), Q stride 132; in Q K^T the 16 waves cover 8 column
//           tiles x 2 row fragments, ONE A fragment of <= 32 k-steps per wave, so a wave still holds 32 A and <= 32 B
//           registers.  In P V all 16 waves own an output tile (2 row fragments x 8 column tiles; at d_k 96 the last
//           two column tiles idle).
// Either way 153 KiB of LDS, one workgroup per CU, 4 waves per SIMD (<= 128 VGPRs).
// Work items run sequence by sequence and inside a sequence query head by query head: the G heads of one KV head,
// and their query tiles, are contiguous under the XCD remap, so one XCD's L2 serves a KV head's K / V to all of them.
// Built with the packed fp32 instructions off (Makefile), as attention_decode_wide.o: every fp32 step here is one the
// contract names.
#include "qgemm_internal.h"

#include <type_traits>

namespace qgemm {

namespace {

constexpr int kGqaMaxSeq = 512;
constexpr int kGqaTQ = 32;                // query rows per workgroup
constexpr int kGqaThreads = 1024;
constexpr int kGqaSStride = kGqaMaxSeq + 4;  // S row stride (floats): consecutive rows 4 banks apart

template <int kW>
struct GqaTile {
    static_assert(kW == 64 || kW == 128, "the row widths of the decode kernels");
    static constexpr int kWaves = kGqaThreads / 64;
    static constexpr int kChunk = kW == 64 ? 256 : 128;  // keys per K / V chunk
    static constexpr int kKStride = kW + 4;              // K chunk [key][d_k]: B-fragment reads (16 keys x 4 k)
    static constexpr int kVStride = kW + 16;             // V chunk [key][d_k]: B-fragment reads (4 keys x 16 cols)
    static constexpr int kQStride = kW + 4;              // Q tile [query][d_k]: A-fragment reads
    static constexpr int kF4 = kW / 4;                   // float4 pieces of a staged row
    static constexpr int kColTiles = kChunk / 16;        // Q K^T column tiles of a chunk: 16 or 8
    static constexpr int kRFw = kGqaTQ / 16 * kColTiles / kWaves;  // row fragments a wave computes in Q K^T: 2 or 1
    static constexpr int kSteps = kW / 4;                // k-steps of a full-width row
    static constexpr int kPer = kChunk * kF4 / kGqaThreads;  // float4 pieces per thread and chunk: 4 at both widths
    static constexpr int kKVFloats = kChunk * kVStride;
    static_assert(kRFw * kWaves == 2 * kColTiles && kPer * kGqaThreads == kChunk * kF4 && kChunk % 32 == 0, "");
    static_assert((kGqaTQ * kGqaSStride + kKVFloats + kGqaTQ * kQStride) * 4 <= 160 * 1024, "the LDS of a CU");
};

typedef float v4f __attribute__((ext_vector_type(4)));

// The sequences of a launch, the kernel's last argument by value (FusedMany of attention.hip): work item w (after the
// XCD remap) belongs to the sequence b with item0[b] <= w < item0[b + 1]; inside it the items run query head by query
// head, a head's query tiles one after another.  Everything is uniform per workgroup: scalar loads from the kernel
// arguments, nothing in device memory.
struct GqaSeqs {
    int n_seqs;
    FusedSeqTable tab;
};
static_assert(sizeof(GqaSeqs) + 88 < 4096, "the table travels in the kernel arguments");

template <int kW, bool kCausal>
__global__ __launch_bounds__(kGqaThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void attention_fused_gqa_kernel(
    const float *__restrict__ Q, int64_t ldq, const float *__restrict__ K, int64_t ldk, const float *__restrict__ V,
    int64_t ldv, float *__restrict__ O, int64_t ldo, int dk, int group, float scale, GqaSeqs seqs) {
    using T = GqaTile<kW>;
    constexpr int kTQ = kGqaTQ, kChunk = T::kChunk, kF4 = T::kF4, kPer = T::kPer, kRFw = T::kRFw;
    constexpr int kSStride = kGqaSStride, kKStride = T::kKStride, kVStride = T::kVStride, kQStride = T::kQStride;
    __shared__ __attribute__((aligned(16))) float S[kTQ * kSStride];
    __shared__ __attribute__((aligned(16))) float KV[T::kKVFloats];
    __shared__ __attribute__((aligned(16))) float Qs[kTQ * kQStride];
    // XCD-aware: blocks b, b+8, ... share an XCD; each XCD gets a contiguous range of work items, so the G query heads
    // of a KV head (and their K / V re-reads) stay in one L2
    const int nwg = gridDim.x, lin = blockIdx.x;
    const int xq = nwg >> 3, xr = nwg & 7, xc = lin & 7;
    const int logical = (xc < xr ? xc * (xq + 1) : xr * (xq + 1) + (xc - xr) * xq) + (lin >> 3);
    // the last sequence whose first work item is at or below `logical` (an empty sequence shares its first item with
    // the next one and is passed over): a wave-uniform binary search, at most 6 scalar loads
    int b = 0, hi = seqs.n_seqs;
    while (hi - b > 1) {
        const int mid = (b + hi) >> 1;
        if (seqs.tab.item0[mid] <= logical) b = mid;
        else hi = mid;
    }
    const int seq_q = seqs.tab.seq_q[b], seq = seqs.tab.seq_kv[b], q_pos0 = seqs.tab.q_pos0[b];
    const int tiles = (seq_q + kTQ - 1) / kTQ, local = logical - seqs.tab.item0[b];
    const int h = local / tiles, q0 = (local - h * tiles) * kTQ;
    {
        const int64_t qr = seqs.tab.q_row0[b], kr = seqs.tab.kv_row0[b];
        Q += qr * ldq;
        O += qr * ldo;
        K += kr * ldk;
        V += kr * ldv;
    }
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // the head map: the one difference from the multi-head kernel
    const int hkv = h / group;
    const float *Qb = Q + (int64_t)h * dk, *Kb = K + (int64_t)hkv * dk, *Vb = V + (int64_t)hkv * dk;
    const int lr = lane & 15, lk = lane >> 4;  // MFMA operand lane: row lr of the fragment, k offset lk
    const int rows = seq_q - q0 < kTQ ? seq_q - q0 : kTQ;
    const int nchunks = (seq + kChunk - 1) / kChunk;
    const int seq32 = (seq + 31) & ~31;  // the reference's k extent for P V: seq zero-padded to its 32-wide tile
    const int dk4 = (dk + 3) >> 2;       // float4 columns of a K / V row (the last one zero-padded)
    // kCausal: query row i sees keys 0 .. limit(i) - 1, limit(i) = min(seq, i + q_pos0 + 1) >= 1 (q_pos0 <= seq: the
    // launcher clamps it); lmax = the largest limit of this workgroup's rows.  Q K^T runs only up to lmax; every
    // softmax row runs to its own limit and stores +0 past it; P V runs all of seq32
    auto limit = [&](int rl) __attribute__((always_inline)) { return kCausal ? min(seq, q0 + rl + q_pos0 + 1) : seq; };
    const int lmax = limit(rows - 1);
    const int nck = (lmax + kChunk - 1) / kChunk;  // the K chunks that start below lmax (= nchunks without a mask)
    // kCausal: the exp and divide loops of a row run to its limit rounded up to 64, so every lane of the wave makes the
    // same number of trips (attention.hip `upto`); the columns passed over lie inside the S row and reach no result
    auto upto = [&](int li) __attribute__((always_inline)) { return kCausal ? (li + 63) & ~63 : seq; };

    // K / V chunks as float4 pieces, kPer per thread, fetched into registers one chunk ahead -- chunk c+1's global
    // loads are in flight under chunk c's MFMAs, V chunk 0's under the last QK chunk and the softmax -- then written
    // to KV ([key][stride], zero past seq and past d_k).  A piece that is unaligned or crosses d_k goes by elements.
    auto fetch = [&](float4 (&r)[kPer], const float *src, int64_t ld, int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int f = t + i * kGqaThreads, row = f / kF4, c4 = f % kF4, j = c0 + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < seq && c4 < dk4) {
                const float *p = src + j * ld + 4 * c4;
                if (4 * c4 + 3 < dk && ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) {
                    v = *reinterpret_cast<const float4 *>(p);
                } else {
                    v.x = p[0];
                    v.y = 4 * c4 + 1 < dk ? p[1] : 0.f;
                    v.z = 4 * c4 + 2 < dk ? p[2] : 0.f;
                    v.w = 4 * c4 + 3 < dk ? p[3] : 0.f;
                }
            }
            r[i] = v;
        }
    };
    auto put = [&](const float4 (&r)[kPer], int stride) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int f = t + i * kGqaThreads;
            *reinterpret_cast<float4 *>(KV + (f / kF4) * stride + 4 * (f % kF4)) = r[i];
        }
    };

    // ---- S[32][seq_kv] = Q K^T, one K chunk at a time: wave w computes column tile w % kColTiles of the chunk, for
    // both 16-row halves at kW 64 (two A fragments), for half w / kColTiles at kW 128 (one A fragment)
    const int ns32 = ((dk + 31) & ~31) >> 2;  // k-steps over d_k zero-padded to 32: 8 / 16, or 24 / 32
    const int ctile = wave % T::kColTiles, rf0 = kRFw == 2 ? 0 : wave / T::kColTiles;
    // the Q tile through LDS (coalesced row loads once per workgroup, not per wave), with K chunk 0
    float4 pf[kPer];
    fetch(pf, Kb, ldk, 0);
    for (int f = t; f < kTQ * kF4; f += kGqaThreads) {
        const int row = f / kF4, c4 = f % kF4, i = q0 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < seq_q && c4 < dk4) {
            const float *p = Qb + i * ldq + 4 * c4;
            v.x = p[0];
            v.y = 4 * c4 + 1 < dk ? p[1] : 0.f;
            v.z = 4 * c4 + 2 < dk ? p[2] : 0.f;
            v.w = 4 * c4 + 3 < dk ? p[3] : 0.f;
        }
        *reinterpret_cast<float4 *>(Qs + row * kQStride + 4 * c4) = v;
    }
    float qa[kRFw][T::kSteps];
    for (int c = 0; c < nck; ++c) {
        if (c) __syncthreads();  // every wave is done with the previous chunk
        put(pf, kKStride);
        __syncthreads();
        if (c + 1 < nck) fetch(pf, Kb, ldk, (c + 1) * kChunk);
        else fetch(pf, Vb, ldv, 0);
        if (c == 0) {
#pragma unroll
            for (int rf = 0; rf < kRFw; ++rf)
#pragma unroll
                for (int s = 0; s < T::kSteps; ++s) qa[rf][s] = Qs[((rf0 + rf) * 16 + lr) * kQStride + 4 * s + lk];
        }
        const int col = c * kChunk + ctile * 16 + lr;
        if (c * kChunk + ctile * 16 < lmax) {  // wave-uniform; a tile at or past lmax is never read
            const float *krow = KV + (ctile * 16 + lr) * kKStride + lk;
            v4f acc[kRFw];
#pragma unroll
            for (int rf = 0; rf < kRFw; ++rf) acc[rf] = v4f{0.f, 0.f, 0.f, 0.f};
            // k-steps over the reference's zero-padded extent (Q and K are zero past d_k, so those steps are its padded
            // tile's +0 adds) with no per-step condition, the B fragments read together
            auto steps = [&](auto kSteps) __attribute__((always_inline)) {
                constexpr int kS = decltype(kSteps)::value;
                float kb[kS];
#pragma unroll
                for (int s = 0; s < kS; ++s) kb[s] = krow[4 * s];
#pragma unroll
                for (int s = 0; s < kS; ++s)
#pragma unroll
                    for (int rf = 0; rf < kRFw; ++rf)
                        acc[rf] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[rf][s], kb[s], acc[rf], 0, 0, 0);
            };
            if (ns32 == T::kSteps) steps(std::integral_constant<int, T::kSteps>());
            else steps(std::integral_constant<int, T::kSteps - 8>());  // d_k <= 32 at kW 64, d_k 96 at kW 128
            if (col < seq) {
#pragma unroll
                for (int rf = 0; rf < kRFw; ++rf)
#pragma unroll
                    for (int r = 0; r < 4; ++r) S[((rf0 + rf) * 16 + 4 * lk + r) * kSStride + col] = acc[rf][r];
            }
        }
    }
    __syncthreads();

    // ---- softmax of rows 2w and 2w+1: max and exp across the lanes, the two sequential sums at once (lanes 0 and
    // 32), the division across the lanes -- all through the LDS row, as attention_fused_kernel
    for (int rr = 0; rr < 2; ++rr) {
        const int rl = wave * 2 + rr;
        if (rl >= rows) break;
        float *srow = S + rl * kSStride;
        const int li = limit(rl);  // the row's softmax width: nothing at or past it reaches the result
        const float seed = __fmul_rn(srow[0], scale);
        const float cand = softmax_row_max(srow, lane + 1, li, 64, scale);
        const float mx = (cand > seed) ? cand : seed;
        for (int c = lane, cu = upto(li); c < cu; c += 64) srow[c] = softmax_exp(srow[c], scale, mx);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's exps are in LDS
    __builtin_amdgcn_wave_barrier();
    // the two sums at once, each hopping lane to lane (hop_left): row 2w in lanes 0-31, row 2w+1 in lanes 32-63, lane h
    // of a half holding elements 16h .. 16h+15 of its row in registers; after step t the chain through lane h = t - 1
    // of each half sits in that lane.  Elements past the half's own limit are -0.0f, which leaves any sum unchanged;
    // both halves run to the lane count of row 2w+1, the larger limit, and both sums are read at that lane.
    const int hl = lane & 31, lh = limit(wave * 2 + (lane >> 5));  // lh: the limit of this half's row
    const int nl = (limit(wave * 2 + 1) + 15) >> 4;  // lanes per half that hold elements (nl <= 32)
    const float *erow = S + (wave * 2 + (lane >> 5)) * kSStride + 16 * hl;
    float e[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (hl < nl && wave * 2 + (lane >> 5) < rows) v = *reinterpret_cast<const float4 *>(erow + 4 * j);
        e[4 * j] = v.x; e[4 * j + 1] = v.y; e[4 * j + 2] = v.z; e[4 * j + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (16 * hl + j >= lh) e[j] = -0.0f;
    float s = 0.0f;
    for (int i = 0; i < nl; ++i) {
        s = __fadd_rn(hop_left(s), e[0]);
#pragma unroll
        for (int j = 1; j < 16; ++j) s = __fadd_rn(s, e[j]);
    }
    const float sum_a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), nl - 1));
    const float sum_b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), 32 + nl - 1));
    for (int rr = 0; rr < 2; ++rr) {
        const int rl = wave * 2 + rr;
        const float srr = rr == 0 ? sum_a : sum_b;
        if (rl >= rows) break;
        float *srow = S + rl * kSStride;
        const int li = limit(rl);
        for (int c = lane, cu = upto(li); c < cu; c += 64) srow[c] = __fdiv_rn(srow[c], srr);
        if constexpr (kCausal) {
            // P = +0 at the masked keys, the passed-over columns and the padding (to the end of what `upto` covered)
            for (int c = li + lane, ce = max(seq32, upto(li)); c < ce; c += 64) srow[c] = 0.0f;
        } else {
            if (lane < seq32 - seq) srow[seq + lane] = 0.0f;  // P over the zero-padded k range (< 32 columns)
        }
    }

    // ---- O = P V, one V chunk at a time: waves 0 .. 2*ceil(d_k/16)-1 own output tile (row fragment w % 2, column
    // tile w / 2) and carry its accumulator across the chunks (the k chain stays in order)
    const int nct2 = (dk + 15) >> 4, nks32 = seq32 >> 2;
    const bool pv_wave = wave < 2 * nct2;
    const int rf = wave & 1, ct = wave >> 1;
    const int col = ct * 16 + lr;
    const float *prow = S + (rf * 16 + lr) * kSStride + lk;
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();  // P complete (c = 0) / the previous V chunk consumed
        put(pf, kVStride);
        __syncthreads();
        if (c + 1 < nchunks) fetch(pf, Vb, ldv, (c + 1) * kChunk);
        if (pv_wave) {
            // k-steps over the reference's zero-padded extent (P and V are zero past seq), in groups of 8 -- a whole
            // number of groups per chunk, no per-step conditions; group g+1's operands are read from LDS while group
            // g's MFMAs run (the accumulation chain itself stays in k order)
            const int s_beg = c * (kChunk / 4), s_end = min(nks32, (c + 1) * (kChunk / 4));
            const float *vcol = KV + (lk - c * kChunk) * kVStride + col;
            auto read = [&](float (&pa)[8], float (&vb)[8], int s0) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    pa[u] = prow[4 * (s0 + u)];
                    vb[u] = vcol[4 * (s0 + u) * kVStride];
                }
            };
            auto mfma8 = [&](const float (&pa)[8], const float (&vb)[8]) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[u], vb[u], acc, 0, 0, 0);
            };
            float pa0[8], vb0[8], pa1[8], vb1[8];
            if (s_beg < s_end) read(pa0, vb0, s_beg);
            for (int s0 = s_beg; s0 < s_end; s0 += 16) {
                const bool two = s0 + 8 < s_end;
                if (two) read(pa1, vb1, s0 + 8);
                mfma8(pa0, vb0);
                if (s0 + 16 < s_end) read(pa0, vb0, s0 + 16);
                if (two) mfma8(pa1, vb1);
            }
        }
    }
    if (pv_wave && col < dk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = rf * 16 + 4 * lk + r;
            if (rl < rows) O[(q0 + rl) * ldo + (int64_t)h * dk + col] = acc[r];
        }
    }
}

}  // namespace

bool attention_fused_gqa_ok(int seq_kv, int dk) {
    return seq_kv >= 1 && seq_kv <= kGqaMaxSeq && dk >= 1 && (dk <= 64 || dk == 96 || dk == 128);
}

// tab.q_row0, kv_row0, seq_q, seq_kv and q_pos0 (clamped to seq_kv) come checked from launch_attention_varlen_gqa
// (attention_launch.hip); the work map item0 is built HERE, where the tile height is known, and the envelope and the
// ranges are tested again, where the kernel's LDS arrays and grid are sized
hipError_t launch_attention_fused_gqa_many(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V,
                                           int64_t ldv, float *O, int64_t ldo, int n_seqs, const FusedSeqTable &tab,
                                           bool causal, int n_heads, int n_kv_heads, int dk, float scale,
                                           hipStream_t stream) {
    if (n_seqs < 1 || n_seqs > kVarlenMaxSeqs || n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads ||
        !attention_fused_gqa_ok(1, dk))
        return hipErrorInvalidValue;
    GqaSeqs many;
    many.n_seqs = n_seqs;
    many.tab = tab;
    int64_t items = 0;
    for (int b = 0; b < n_seqs; ++b) {
        if (tab.seq_q[b] < 0 || !attention_fused_gqa_ok(tab.seq_kv[b], dk) || tab.q_row0[b] < 0 || tab.kv_row0[b] < 0 ||
            tab.q_pos0[b] < 0 || tab.q_pos0[b] > tab.seq_kv[b])
            return hipErrorInvalidValue;
        many.tab.item0[b] = (int)items;
        items += (int64_t)((tab.seq_q[b] + kGqaTQ - 1) / kGqaTQ) * n_heads;
        if (items > INT32_MAX) return hipErrorInvalidValue;
    }
    for (int b = n_seqs; b <= kVarlenMaxSeqs; ++b) many.tab.item0[b] = (int)items;
    if (items == 0) return hipSuccess;
    const dim3 grid((unsigned)items);
    const int group = n_heads / n_kv_heads;
    auto go = [&](auto kernel) {
        kernel<<<grid, kGqaThreads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, O, ldo, dk, group, scale, many);
        return hipGetLastError();
    };
    if (dk <= 64) return causal ? go(attention_fused_gqa_kernel<64, true>) : go(attention_fused_gqa_kernel<64, false>);
    return causal ? go(attention_fused_gqa_kernel<128, true>) : go(attention_fused_gqa_kernel<128, false>);
}

}  // namespace qgemm
