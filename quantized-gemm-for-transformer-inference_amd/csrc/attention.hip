// attention.hip -- the fp32 attention core (attention.cuh:58-69) in ONE launch: for every (head, 32-query
// tile) a workgroup computes
//   S = Q_h K_h^T                  op_mm<float> on the transposed view    (attention.cuh:58-60)
//   P = softmax(S * scale)         op_multiply + op_softmax               (attention.cuh:65-68)
//   O[:, h*d_k..] = P V_h          op_mm<float>                           (attention.cuh:69)
// with S and P kept in LDS (the three-launch form writes and re-reads the H x seq_q x seq_kv score tensor
// through HBM twice).
// Q (seq_q rows), K and V (seq_kv rows) and O (seq_q rows) are four matrices with their own base pointers
// and row strides, head h at columns h*d_k .. h*d_k + d_k - 1 of each: the encoder's self-attention passes
// the three thirds of its [Q | K | V] buffer (seq_q = seq_kv), the decoder's cross-attention its own
// queries and the projections of the encoder's output.  Query rows run to seq_q; everything along a score
// row (K / V chunks, the softmax, the P V reduction) runs to seq_kv.
// Every step keeps the arithmetic of the separate kernels bit for bit:
//   * both products are v_mfma_f32_16x16x4_f32 chains from +0 over k ascending, zero-padded to a
//     multiple of 4, then fl(res + 0) when k % 32 != 0 -- the reference's op_matmul_kernel chain
//     (op_mm.cuh:37-39) with its zero-padded last 32-wide tile, exactly as gemm_f32.hip;
//   * softmax as softmax_rows_kernel: max and exp by the contract at softmax_row_max (qgemm_internal.h), ONE
//     sequential fp32 sum in column order, then fl(e / sum).
// Envelope: d_k <= 64, seq_kv <= 512, any seq_q (S tile 32 x 512 fp32 = 64 KiB of LDS, Q tile and K / V
// staged through LDS in 256-key chunks: 155 KiB in all); outside it launch_attention (attention_launch.hip) runs the
// three kernels.
// The same kernel runs up to 64 independent sequences of their own lengths in one launch (FusedMany below, DESIGN.md
// s19): a workgroup finds its (sequence, head, query tile) in a table in the kernel arguments and offsets its four
// base pointers; everything after that is the single launch's workgroup.
// kCausal: query row i sees keys 0 .. L_i - 1, L_i = min(seq_kv, i + q_pos0 + 1).  The softmax of
// row i is softmax_rows_kernel's on a row of width L_i and P is +0 from column L_i on; P V still runs over all of
// seq_kv (a masked key contributes fmaf(+0, v, acc), so 0 * inf is NaN as without a mask).  Q K^T tiles that lie
// past the workgroup's largest limit are not computed.  kCausal = false is the kernel without any of this.
#include "qgemm_internal.h"

#include <type_traits>

namespace qgemm {

namespace {

constexpr int kAttnMaxSeq = 512;
constexpr int kAttnMaxDk = 64;
constexpr int kFusedTQ = 32;               // query rows per workgroup of the library's tile configuration
constexpr int kSStride = kAttnMaxSeq + 4;  // S row stride (floats): consecutive rows 4 banks apart
constexpr int kKStride = 68;               // K chunk [key][d_k]: B-fragment reads (16 keys x 4 k) conflict-free
constexpr int kVStride = 80;               // V chunk [key][d_k]: B-fragment reads (4 keys x 16 cols) conflict-free
constexpr int kQStride = 68;               // Q tile [query][d_k]: A-fragment reads conflict-free

// Tile configurations.  kTQ query rows per workgroup, kChunk keys per K / V chunk, one 16-column QK tile
// per wave (kChunk = 16 x waves), two softmax rows per wave (kTQ = 2 x waves).
//   <32, 256, 1024>: 153 KiB of LDS, one workgroup per CU (the library's choice);
//   <16, 128, 512> : 77 KiB, two workgroups per CU whose phases could overlap -- measured slower
//                    (36.5 vs 30.6 us at config 5: twice the K / V staging, one QK chain per wave).
template <int kTQ, int kChunk, int kThreads>
struct AttnTile {
    static constexpr int kWaves = kThreads / 64;
    static_assert(kChunk == 16 * kWaves && kTQ == 2 * kWaves, "one QK column tile and two softmax rows per wave");
    static constexpr int kRowFrags = kTQ / 16;
    static constexpr int kKVFloats = kChunk * kVStride;
    static constexpr int kWavesPerEu = 4;  // 4 waves per SIMD either way: <= 128 VGPRs
};

typedef float v4f __attribute__((ext_vector_type(4)));

// The sequences of a launch, the kernel's last argument (by value), as DecodeOne / DecodeMany of
// attention_decode.hip.  FusedOne: the single-sequence launch, grid (query tiles, heads).  FusedMany:
// up to kVarlenMaxSeqs independent sequences of their own lengths, a one-dimensional grid of
// sum_b ceil(seq_q[b] / kTQ) * n_heads workgroups.  Work item w (after the XCD remap) belongs to the sequence b with
// item0[b] <= w < item0[b + 1]; inside it the items run head by head, a head's query tiles one after another, so the
// tiles of one (sequence, head) are contiguous and share an XCD's L2 like a head's tiles in the single launch.
// Sequence b's query and output rows start at row q_row0[b] of Q and O, its keys at row kv_row0[b] of K and V.
// Everything is uniform per workgroup: scalar loads from the kernel arguments, nothing in device memory.
// The single sequence's seq_q, seq_kv and q_pos0 stay plain kernel arguments, where they were before there was a table,
// and FusedOne is empty: carried inside a by-value struct they reached the kernel through other loads, and hipcc
// ordered this kernel's setup differently (it is sensitive to that, see the softmax max).  FusedMany overwrites the
// three from its table, and the launcher passes zeros for them.
struct FusedOne {};
struct FusedMany {
    int n_seqs;
    FusedSeqTable tab;
};
static_assert(sizeof(FusedMany) + 80 < 4096, "the table travels in the kernel arguments");

template <int kTQ, int kChunk, int kThreads, bool kCausal, typename Seqs>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void attention_fused_kernel(
    const float *__restrict__ Q, int64_t ldq, const float *__restrict__ K, int64_t ldk, const float *__restrict__ V,
    int64_t ldv, float *__restrict__ O, int64_t ldo, int dk, int seq_q, int seq_kv, float scale, int q_pos0, Seqs seqs) {
    using T = AttnTile<kTQ, kChunk, kThreads>;
    constexpr int kAttnThreads = kThreads, kRF = T::kRowFrags;
    __shared__ __attribute__((aligned(16))) float S[kTQ * kSStride];
    __shared__ __attribute__((aligned(16))) float KV[T::kKVFloats];
    __shared__ __attribute__((aligned(16))) float Qs[kTQ * kQStride];
    // XCD-aware: blocks b, b+8, ... share an XCD; each XCD gets a contiguous range of (head, query tile)
    // pairs, so a head's query tiles (and its K / V re-reads) stay in one L2
    const int nwg = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
    const int xq = nwg >> 3, xr = nwg & 7, xc = lin & 7;
    const int logical = (xc < xr ? xc * (xq + 1) : xr * (xq + 1) + (xc - xr) * xq) + (lin >> 3);
    int h, q0;
    if constexpr (std::is_same<Seqs, FusedMany>::value) {
        // the last sequence whose first work item is at or below `logical` (an empty sequence shares its first item
        // with the next one and is passed over): a wave-uniform binary search, at most 6 scalar loads
        int b = 0, hi = seqs.n_seqs;
        while (hi - b > 1) {
            const int mid = (b + hi) >> 1;
            if (seqs.tab.item0[mid] <= logical) b = mid;
            else hi = mid;
        }
        seq_q = seqs.tab.seq_q[b];
        seq_kv = seqs.tab.seq_kv[b];
        q_pos0 = seqs.tab.q_pos0[b];
        const int tiles = (seq_q + kTQ - 1) / kTQ, local = logical - seqs.tab.item0[b];
        h = local / tiles;
        q0 = (local - h * tiles) * kTQ;
        const int64_t qr = seqs.tab.q_row0[b], kr = seqs.tab.kv_row0[b];
        Q += qr * ldq;
        O += qr * ldo;
        K += kr * ldk;
        V += kr * ldv;
    } else {
        h = logical / gridDim.x;
        q0 = (logical - h * gridDim.x) * kTQ;
    }
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float *Qb = Q + (int64_t)h * dk, *Kb = K + (int64_t)h * dk, *Vb = V + (int64_t)h * dk;
    const int lr = lane & 15, lk = lane >> 4;  // MFMA operand lane: row lr of the fragment, k offset lk
    const int rows = seq_q - q0 < kTQ ? seq_q - q0 : kTQ;
    const int seq = seq_kv;  // the extent of a score row: keys, softmax columns, the P V reduction
    const int nchunks = (seq + kChunk - 1) / kChunk;
    const int seq32 = (seq + 31) & ~31;  // the reference's k extent for P V: seq zero-padded to its 32-wide tile
    const int dk4 = (dk + 3) >> 2;  // float4 columns of a K / V row (the last one zero-padded)
    // kCausal: query row i sees keys 0 .. limit(i) - 1, limit(i) = min(seq, i + q_pos0 + 1) >= 1 (q_pos0 <= seq: the
    // launcher clamps it, so the sums stay in int range); lmax = the largest limit of this workgroup's rows.  Q K^T
    // runs only up to lmax; every softmax row runs to its own limit and stores +0 past it; P V runs all of seq32
    auto limit = [&](int rl) __attribute__((always_inline)) { return kCausal ? min(seq, q0 + rl + q_pos0 + 1) : seq; };
    const int lmax = limit(rows - 1);
    const int nck = (lmax + kChunk - 1) / kChunk;  // the K chunks that start below lmax (= nchunks without a mask)
    // kCausal: the exp and divide loops of a row run to its limit ROUNDED UP to 64 (`upto`), so every lane of the wave
    // makes the same number of trips.  A tile's limits are no multiples of 64; with the loops ending at the limit
    // itself some lanes had 8 columns and others 7, and the 4-way unrolled exp loop ran its main form twice for the
    // first and its main, 2-element and 1-element forms for the others: 11 passes over the double-precision exp
    // instead of 8, measured 2.2 us per launch at 512 x 512.  The at most 63 columns past the limit
    // that these loops pass over hold raw scores or stale LDS on the way in and garbage on the way out (NaN
    // included); nothing that reaches the output reads them -- the max stops at the limit, the sum chain puts -0.0f
    // in their place, and the row stores +0 over them before P V.  They lie inside the S row (limit <= 512 < kSStride)
    auto upto = [&](int li) __attribute__((always_inline)) { return kCausal ? (li + 63) & ~63 : seq; };

    // K / V chunks as float4 pieces, kPer per thread, fetched into registers one chunk ahead -- chunk
    // c+1's global loads are in flight under chunk c's MFMAs, V chunk 0's under the last QK chunk and
    // the softmax -- then written to KV ([key][stride], zero past seq and past d_k)
    constexpr int kPer = kChunk * 16 / kThreads;
    auto fetch = [&](float4 (&r)[kPer], const float *src, int64_t ld, int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int f = t + i * kThreads, row = f >> 4, c4 = f & 15, j = c0 + row;
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
            const int f = t + i * kThreads;
            *reinterpret_cast<float4 *>(KV + (f >> 4) * stride + 4 * (f & 15)) = r[i];
        }
    };

    // ---- S[32][seq_kv] = Q K^T, one K chunk at a time: wave w computes 16-column tile w of the chunk for
    // both 16-row halves (one B fragment, two A fragments)
    const int ns32 = ((dk + 31) & ~31) >> 2;  // k-steps over d_k zero-padded to 32: 8 or 16
    // the Q tile through LDS (coalesced row loads once per workgroup, not per wave), with K chunk 0
    float4 pf[kPer];
    fetch(pf, Kb, ldk, 0);
    for (int f = t; f < kTQ * 16; f += kAttnThreads) {
        const int row = f >> 4, c4 = f & 15, i = q0 + row;
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
    float qa[kRF][16];
    for (int c = 0; c < nck; ++c) {
        if (c) __syncthreads();  // every wave is done with the previous chunk
        put(pf, kKStride);
        __syncthreads();
        if (c + 1 < nck) fetch(pf, Kb, ldk, (c + 1) * kChunk);
        else fetch(pf, Vb, ldv, 0);
        if (c == 0) {
#pragma unroll
            for (int rf = 0; rf < kRF; ++rf)
#pragma unroll
                for (int s = 0; s < 16; ++s) qa[rf][s] = Qs[(rf * 16 + lr) * kQStride + 4 * s + lk];
        }
        const int col = c * kChunk + wave * 16 + lr;
        if (c * kChunk + wave * 16 < lmax) {  // wave-uniform; a tile at or past lmax is never read
            const float *krow = KV + (wave * 16 + lr) * kKStride + lk;
            v4f acc[kRF];
#pragma unroll
            for (int rf = 0; rf < kRF; ++rf) acc[rf] = v4f{0.f, 0.f, 0.f, 0.f};
            // k-steps over the reference's zero-padded extent (d_k rounded up to 32: Q and K are zero past
            // d_k, so those steps are its padded tile's +0 adds) -- 8 or 16 steps with no per-step
            // condition, the B fragments read together
            auto steps = [&](auto kSteps) __attribute__((always_inline)) {
                constexpr int kS = decltype(kSteps)::value;
                float kb[kS];
#pragma unroll
                for (int s = 0; s < kS; ++s) kb[s] = krow[4 * s];
#pragma unroll
                for (int s = 0; s < kS; ++s)
#pragma unroll
                    for (int rf = 0; rf < kRF; ++rf)
                        acc[rf] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[rf][s], kb[s], acc[rf], 0, 0, 0);
            };
            if (ns32 == 16) steps(std::integral_constant<int, 16>());
            else steps(std::integral_constant<int, 8>());
            if (col < seq) {
#pragma unroll
                for (int rf = 0; rf < kRF; ++rf)
#pragma unroll
                    for (int r = 0; r < 4; ++r) S[(rf * 16 + 4 * lk + r) * kSStride + col] = acc[rf][r];
            }
        }
    }
    __syncthreads();

    // ---- softmax of rows 2w and 2w+1: max and exp across the lanes, the two sequential sums at once
    // (lanes 0 and 1), the division across the lanes -- all through the LDS row (keeping the scaled
    // scores and exps in registers instead measured 1 us slower per launch)
    for (int rr = 0; rr < 2; ++rr) {
        const int rl = wave * 2 + rr;
        if (rl >= rows) break;
        float *srow = S + rl * kSStride;
        const int li = limit(rl);  // the row's softmax width: nothing at or past it reaches the result
        // the max keeps its own text (softmax_row_max's, spelled out: through the helper hipcc orders this kernel's
        // register initialisation differently); the contract of both steps is at the helper (qgemm_internal.h)
        const float seed = __fmul_rn(srow[0], scale);
        float cand = -INFINITY;
        for (int c = lane + 1; c < li; c += 64) {
            const float x = __fmul_rn(srow[c], scale);  // op_multiply(QK_T, scale_factor)
            cand = (x > cand) ? x : cand;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float o = __shfl_xor(cand, off, 64);
            cand = (o > cand) ? o : cand;
        }
        const float mx = (cand > seed) ? cand : seed;
        for (int c = lane, cu = upto(li); c < cu; c += 64) srow[c] = softmax_exp(srow[c], scale, mx);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's exps are in LDS
    __builtin_amdgcn_wave_barrier();
    // the two sums at once, each hopping lane to lane (hop_left): row 2w in lanes 0-31, row 2w+1 in lanes
    // 32-63, lane h of a half holding elements 16h .. 16h+15 of its row in registers; after step t the
    // chain through lane h = t - 1 of each half sits in that lane (lane 32 starts from lane 31's initial
    // zero; both halves run the same instructions).  Elements past seq are -0.0f, which leaves any sum
    // unchanged, so the last lane's 16 adds stay uniform.  Per element one dependent add, no LDS reads
    // inside the chain (the LDS-walking form exposed one read latency per 64 elements).
    // kCausal: a half's elements past its own row's limit are -0.0f too (raw scores or stale LDS sit there), both
    // halves run to the lane count of row 2w+1, the larger limit, and row 2w's sum passes through its -0.0f lanes
    // unchanged, so both sums are read at that lane.
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
    for (int t = 0; t < nl; ++t) {
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

    // ---- O = P V, one V chunk at a time: waves 0 .. kRF*ceil(d_k/16)-1 own output tile (row
    // fragment w % kRF, column tile w / kRF) and carry its accumulator across the chunks (the k chain
    // stays in order)
    const int nct2 = (dk + 15) >> 4, nks32 = seq32 >> 2;
    const bool pv_wave = wave < kRF * nct2;
    const int rf = wave % kRF, ct = wave / kRF;
    const int col = ct * 16 + lr;
    const float *prow = S + (rf * 16 + lr) * kSStride + lk;
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();  // P complete (c = 0) / the previous V chunk consumed
        put(pf, kVStride);
        __syncthreads();
        if (c + 1 < nchunks) fetch(pf, Vb, ldv, (c + 1) * kChunk);
        if (pv_wave) {
            // k-steps over the reference's zero-padded extent (seq rounded up to 32: P and V are zero
            // past seq, so those steps are its padded tile's +0 adds), in groups of 8 -- a whole number
            // of groups per chunk, no per-step conditions; group g+1's operands are read from LDS while
            // group g's MFMAs run (the accumulation chain itself stays in k order)
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

bool attention_fused_ok(int seq_kv, int dk) { return seq_kv <= kAttnMaxSeq && dk <= kAttnMaxDk; }

hipError_t launch_attention_fused(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                                  float *O, int64_t ldo, int seq_q, int seq_kv, int n_heads, int dk, float scale,
                                  int q_pos0, hipStream_t stream) {
    if (n_heads < 1 || dk < 1 || seq_q < 0 || seq_kv < 1 || q_pos0 < kNoMask) return hipErrorInvalidValue;
    if (!attention_fused_ok(seq_kv, dk)) return hipErrorNotSupported;
    if (seq_q == 0) return hipSuccess;
    constexpr int kTQ = kFusedTQ;
    const dim3 grid((unsigned)((seq_q + kTQ - 1) / kTQ), (unsigned)n_heads);
    if (q_pos0 == kNoMask)
        attention_fused_kernel<kTQ, 256, 1024, false, FusedOne><<<grid, 1024, 0, stream>>>(
            Q, ldq, K, ldk, V, ldv, O, ldo, dk, seq_q, seq_kv, scale, 0, FusedOne{});
    else  // past seq_kv - 1 the mask hides nothing: clamped, so the kernel's row limits cannot overflow
        attention_fused_kernel<kTQ, 256, 1024, true, FusedOne><<<grid, 1024, 0, stream>>>(
            Q, ldq, K, ldk, V, ldv, O, ldo, dk, seq_q, seq_kv, scale, q_pos0 < seq_kv ? q_pos0 : seq_kv, FusedOne{});
    return hipGetLastError();
}

// tab.q_row0, kv_row0, seq_q, seq_kv and q_pos0 (clamped to seq_kv) come checked from launch_attention_varlen
// (attention_launch.hip); the work map item0 is built HERE, where the tile height is known, and the envelope and the
// ranges are tested again, where the kernel's LDS arrays and grid are sized
hipError_t launch_attention_fused_many(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V,
                                       int64_t ldv, float *O, int64_t ldo, int n_seqs, const FusedSeqTable &tab,
                                       bool causal, int n_heads, int dk, float scale, hipStream_t stream) {
    if (n_seqs < 1 || n_seqs > kVarlenMaxSeqs || n_heads < 1 || dk < 1 || dk > kAttnMaxDk) return hipErrorInvalidValue;
    FusedMany many;
    many.n_seqs = n_seqs;
    many.tab = tab;
    int64_t items = 0;
    for (int b = 0; b < n_seqs; ++b) {
        if (tab.seq_q[b] < 0 || tab.seq_kv[b] < 1 || tab.seq_kv[b] > kAttnMaxSeq || tab.q_row0[b] < 0 ||
            tab.kv_row0[b] < 0 || tab.q_pos0[b] < 0 || tab.q_pos0[b] > tab.seq_kv[b])
            return hipErrorInvalidValue;
        many.tab.item0[b] = (int)items;
        items += (int64_t)((tab.seq_q[b] + kFusedTQ - 1) / kFusedTQ) * n_heads;
        if (items > INT32_MAX) return hipErrorInvalidValue;
    }
    for (int b = n_seqs; b <= kVarlenMaxSeqs; ++b) many.tab.item0[b] = (int)items;
    if (items == 0) return hipSuccess;
    const dim3 grid((unsigned)items);
    if (causal)
        attention_fused_kernel<kFusedTQ, 256, 1024, true, FusedMany><<<grid, 1024, 0, stream>>>(
            Q, ldq, K, ldk, V, ldv, O, ldo, dk, 0, 0, scale, 0, many);
    else
        attention_fused_kernel<kFusedTQ, 256, 1024, false, FusedMany><<<grid, 1024, 0, stream>>>(
            Q, ldq, K, ldk, V, ldv, O, ldo, dk, 0, 0, scale, 0, many);
    return hipGetLastError();
}

}  // namespace qgemm
