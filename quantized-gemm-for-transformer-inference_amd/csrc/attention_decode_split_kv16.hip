// attention_decode_split_kv16.hip -- split-key decode attention over a bf16 K / V cache: the split-key
// launch of attention_decode_split.hip (s34) reading the bf16 slabs of attention_decode_kv16.hip (s32).  Q, O and the
// workspace are fp32, K and V are bf16 slabs [slabs, rows, n_kv_heads * d_k] with strides in bf16 elements.  bf16 -> fp32
// is exact and the arithmetic is the s34 definition (include/qgemm.h), so every output row is BIT FOR BIT what
// attention_decode_split_kernel + attention_decode_merge_kernel give on K / V widened to fp32 with the same split: the
// definition fixes the order of every sum (a score's fmaf chain over k ascending, d_k zero-padded to 32; l_s as 64
// stride-64 partial sums and six butterfly adds; one fmaf chain per column over the split's keys ascending) and not how
// many keys a staged chunk holds.
// attention_decode_split_kv16_kernel<causal, kW>: the s34 grid, tables, early return, score rows and records -- ONE
// WORKGROUP of 256 threads owns ONE (KV head, block of up to 4 query heads of its group, row, sequence, split) and writes
// the records attention_decode_merge_kernel reads (launch_attention_decode_merge).  What the halved row changes:
//   chunk     rows stay bf16 in registers and LDS and are widened where they are used (x << 16, x & 0xffff0000: no
//             conversion instruction).  The halved bytes buy LONGER CHUNKS at the fp32 kernel's footprint, not a third
//             workgroup: 256 keys at kW = 64 and 128 at kW = 128 (the fp32 kernel: 128 / 64), 8 16-byte pieces per thread
//             and chunk in flight at both widths as there, half the barriers and memory round trips per key
//   LDS row   kW bf16 + 8 of padding: 36 / 68 dwords, both = 4 mod 32.  K row read (thread = key, b128 along the row):
//             the 8 lanes the LDS serves together start at banks 4 i, i < 8, and cover all 32.  V column read: the 64
//             lanes of a wave read ONE key's row at consecutive addresses, 32 (kW = 64, 16-bit reads, two lanes per
//             dword) or 64 (kW = 128) consecutive dwords: no two lanes meet in a bank on different dwords at any stride.
//             Staging write (8 lanes per row, b128): the 8 lanes served together fill one row's 32 consecutive dwords
//   s_h[j]    a thread reads its key's staged row ONCE, piece by piece, and feeds every chain it owns from it.  kW = 64:
//             thread t = key t of the chunk, the chains of all the block's heads (two when the block has <= 2).  kW = 128:
//             the 128-key chunk leaves two threads per key: thread t = key t & 127 and the head pair t >> 7, two chains
//             per read (the fp32 wide kernel: one read per head).  A kW = 64 chunk that holds at most 128 keys (a
//             128-key split) takes the second form too: one thread per key would idle two waves of four
//   softmax   attention_decode_split_kernel's text: wave w = head w
//   a_h = p V wave w = head w at both widths, every lane busy at d_k = kW.  kW = 64: lane = column, a 16-bit LDS read
//             per key (s32's two columns per lane idled half of every wave here).  kW = 128: lane l = columns 2 l and
//             2 l + 1, one 32-bit read per key feeding both chains
// LDS: four score rows (16 KiB) + one chunk (36 / 34 KiB) + four query rows (1 / 2 KiB) = 53 / 52 KiB, three workgroups
// per CU by LDS; the registers make it two, as for the fp32 kernel.
// No matrix instructions: s34's argument (<= 4 (head, row) pairs against a 16-row tile; the kernel waits on its loads).
// Built with the packed fp32 instructions off, as attention_decode_split.o (Makefile).
#include "attention_decode_kernel.h"

namespace qgemm {

namespace {

constexpr int kSplit16Pad = 8;  // bf16 elements of padding behind a staged row

__device__ __forceinline__ float bf16_lo(uint32_t x) { return __uint_as_float(x << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t x) { return __uint_as_float(x & 0xffff0000u); }

// group: G.  grid x = n_kv_heads * ceil(G / 4), y = rows * sequences, z = the most splits a row of the batch has.
// split: keys per split.  ws_splits: the workspace's split dimension.  The strides of K / V count bf16 elements.
template <bool kCausal, int kW>
__global__ __launch_bounds__(kDecThreads) void attention_decode_split_kv16_kernel(
    const float *__restrict__ Q, int64_t ldq, const bf16_t *__restrict__ K, int64_t ldk, const bf16_t *__restrict__ V,
    int64_t ldv, float *__restrict__ ws, int dk, float scale, int group, int n_heads, int split, int ws_splits,
    DecodeMany seqs) {
    constexpr int kChunk = kW == 64 ? 256 : 128;                      // keys per staged K / V chunk
    constexpr int kPieces = kW / 8;                                   // 8-element pieces of a row: 8 / 16
    constexpr int kStride = (kW + kSplit16Pad) / 2;                   // chunk row stride (dwords): 36 / 68
    constexpr int kPer = kChunk * kPieces / kDecThreads;              // pieces of a chunk per thread: 8
    // Piece i of thread t: 8 threads share a row and read 128 contiguous bytes of it; a thread holds kSeg = 1 / 2 pieces
    // of each of its kRows = 8 / 4 rows (t >> 3) + 32 r
    constexpr int kSeg = kPieces / 8, kRows = kPer / kSeg;
    static_assert(kPer == 8 && kRows * 32 == kChunk, "rows (t >> 3) + 32 r, r < kRows, cover the chunk");
    static_assert(kSplitMaxKeys % kChunk == 0 && kStride % 32 == 4, "whole chunks per longest split; stride = 4 mod 32");
    __shared__ __attribute__((aligned(16))) float S[kDecGroupHeads][kSplitMaxKeys];
    __shared__ __attribute__((aligned(16))) uint32_t KV[kChunk * kStride];
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
    const bf16_t *Kb = K + slab * seqs.k_stride_seq + (int64_t)kvh * dk;
    const bf16_t *Vb = V + slab * seqs.v_stride_seq + (int64_t)kvh * dk;
    const int dk8 = (dk + 7) >> 3;  // 8-element pieces of a row (the last one zero-padded)

    // ---- the K / V stream over keys k0 .. k1 - 1: attention_decode_kv16_kernel's fetch / put on pieces of 8 bf16, two
    // chunks in flight in registers.  Every address is clamped into the split (row to k1 - 1 < seq_kv, column to
    // d_k - 1) and the zeros past k1 and past d_k are selected when the chunk is staged, so nothing a key at or past lim
    // holds -- a NaN, an infinity -- reaches LDS.  The 16-byte loads need an aligned first row, a row stride that is a
    // multiple of 8 elements and d_k % 8 == 0 (the slab's offset is part of the first row's address); anything else
    // takes element loads, chosen once per matrix.
    auto aligned = [&](const bf16_t *base, int64_t ld) {
        return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && (ld & 7) == 0 && (dk & 7) == 0;
    };
    const bool vec_k = aligned(Kb, ldk), vec_v = aligned(Vb, ldv);  // workgroup-uniform
    const int trow = t >> 3, tc8 = t & 7;
    auto row_of = [&](int i) { return trow + 32 * (i / kSeg); };
    auto c8_of = [&](int i) { return tc8 + 8 * (i % kSeg); };
    // (a matrix on element loads fetches nothing ahead: `stage` below loads it when the chunk is staged)
    auto fetch = [&](uint4 (&r)[kPer], const bf16_t *src, int64_t ld, int c0, bool vec) __attribute__((always_inline)) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const int row = row_of(i), c8 = c8_of(i);
                r[i] = *reinterpret_cast<const uint4 *>(src + min(c0 + row, k1 - 1) * ld + 8 * min(c8, dk8 - 1));
            }
        }
    };
    auto put = [&](const uint4 (&r)[kPer], int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int row = row_of(i), c8 = c8_of(i);
            const bool in = c0 + row < k1 && 8 * c8 < dk;  // (d_k % 8 == 0 here: a piece lies below d_k or past it)
            *reinterpret_cast<uint4 *>(KV + row * kStride + 4 * c8) = in ? r[i] : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    // The element loads -- any alignment, any stride, any d_k -- go from memory to LDS when the chunk is staged, piece by
    // piece in a loop that is NOT unrolled, with the same clamps and zeros (attention_decode_kv16_kernel has the reason:
    // fetched ahead they were 128 16-bit loads and addresses per chunk beside the two buffers).
    auto put_elements = [&](const bf16_t *src, int64_t ld, int c0) __attribute__((always_inline)) {
#pragma unroll 1
        for (int i = 0; i < kPer; ++i) {
            const int row = row_of(i), c8 = c8_of(i);
            const bf16_t *p = src + min(c0 + row, k1 - 1) * ld;
            const int keep = c0 + row < k1 ? dk - 8 * c8 : 0;  // the piece's columns to keep: the rest are zeros
            uint32_t w[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int c = 8 * c8 + 2 * d;
                const uint32_t x = (uint32_t)p[min(c, dk - 1)].bits | (uint32_t)p[min(c + 1, dk - 1)].bits << 16;
                w[d] = x & (uint32_t)((1ull << 16 * min(max(keep - 2 * d, 0), 2)) - 1ull);
            }
            *reinterpret_cast<uint4 *>(KV + row * kStride + 4 * c8) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    };
    // chunk c of K (v false) or V into LDS
    auto stage = [&](const uint4 (&r)[kPer], int c, bool v) __attribute__((always_inline)) {
        if (v ? vec_v : vec_k) put(r, k0 + c * kChunk);
        else if (v) put_elements(Vb, ldv, k0 + c * kChunk);
        else put_elements(Kb, ldk, k0 + c * kChunk);
    };
    // chunk g of the stream: K chunk g, then V chunk g - nc
    auto fetch_g = [&](uint4 (&r)[kPer], int g) __attribute__((always_inline)) {
        if (g < nc) fetch(r, Kb, ldk, k0 + g * kChunk, vec_k);
        else if (g < 2 * nc) fetch(r, Vb, ldv, k0 + (g - nc) * kChunk, vec_v);
    };
    uint4 pfa[kPer], pfb[kPer];
    fetch_g(pfa, 0);
    fetch_g(pfb, 1);
    // the block's query rows, zeros past d_k and in the rows of heads the block does not have
    for (int i = t; i < kDecGroupHeads * kW; i += kDecThreads) {
        const int hh = i / kW, c = i & (kW - 1);
        Qs[hh][c] = hh < nh && c < dk ? Qb[(int64_t)hh * dk + c] : 0.0f;
    }

    // ---- s_h[j] = Q_h . K[k0 + j], j < n: the fmaf chain from +0 over k ascending, d_k zero-padded to 32.  A thread
    // reads each 8-element piece of its key's row from LDS once, widens it in registers and feeds kN chains, the query
    // rows as broadcast reads.  kW = 64: thread t owns key t of the chunk and the block's first 2 or all 4 heads.
    // kW = 128, and a kW = 64 chunk of at most 128 keys: thread t owns key t & 127 and the head pair t >> 7
    // (wave-uniform).  A head the block lacks runs on the zero query row into a score row nobody reads.
    const int nsteps = dk > (kW == 64 ? 32 : 96) ? kPieces : kPieces - 4;  // pieces of a chain: d_k zero-padded to 32
    auto chains = [&](const uint4 *kr, int hq, int j, auto count) __attribute__((always_inline)) {
        constexpr int kN = decltype(count)::value;
        float res[kN];
#pragma unroll
        for (int h = 0; h < kN; ++h) res[h] = 0.0f;
        // (a loop over the pieces, not unrolled: attention_decode_kv16_kernel measured the unrolled form at 410 - 450
        // registers with every read of the row issued together)
#pragma unroll 1
        for (int s = 0; s < nsteps; ++s) {
            const uint4 x = kr[s];
            const float e0 = bf16_lo(x.x), e1 = bf16_hi(x.x), e2 = bf16_lo(x.y), e3 = bf16_hi(x.y);
            const float e4 = bf16_lo(x.z), e5 = bf16_hi(x.z), e6 = bf16_lo(x.w), e7 = bf16_hi(x.w);
#pragma unroll
            for (int h = 0; h < kN; ++h) {
                const float4 a0 = reinterpret_cast<const float4 *>(Qs[hq + h])[2 * s];
                const float4 a1 = reinterpret_cast<const float4 *>(Qs[hq + h])[2 * s + 1];
                res[h] = fmaf(a0.x, e0, res[h]);
                res[h] = fmaf(a0.y, e1, res[h]);
                res[h] = fmaf(a0.z, e2, res[h]);
                res[h] = fmaf(a0.w, e3, res[h]);
                res[h] = fmaf(a1.x, e4, res[h]);
                res[h] = fmaf(a1.y, e5, res[h]);
                res[h] = fmaf(a1.z, e6, res[h]);
                res[h] = fmaf(a1.w, e7, res[h]);
            }
        }
#pragma unroll
        for (int h = 0; h < kN; ++h) S[hq + h][j] = res[h];
    };
    auto k_step = [&](uint4 (&pf)[kPer], int c) __attribute__((always_inline)) {
        if (c) __syncthreads();  // every thread is done with the previous chunk
        stage(pf, c, false);
        __syncthreads();
        fetch_g(pf, c + 2);
        // (workgroup-uniform) a chunk with at most 128 keys -- every kW = 128 chunk; at kW = 64 the only chunk of a
        // 128-key split and the last one of L = 384, 640, 896 -- goes two threads to a key, or half the waves would idle
        const bool halved = kW == 128 || n - c * kChunk <= 128;
        const int key = halved ? t & 127 : t, j = c * kChunk + key;
        const uint4 *kr = reinterpret_cast<const uint4 *>(KV + key * kStride);
        if (halved) {
            const int pair = wave >> 1;
            if (2 * pair < nh && j < n) chains(kr, 2 * pair, j, std::integral_constant<int, 2>{});
        } else if (j < n) {
            if (nh > 2) chains(kr, 0, j, std::integral_constant<int, 4>{});  // workgroup-uniform
            else chains(kr, 0, j, std::integral_constant<int, 2>{});
        }
    };

    // ---- the partial softmax of head `wave` over its n scores, in place: attention_decode_split_kernel's text.  m from
    // -inf with the strict > (softmax_row_max), the exps by softmax_exp, l as 64 per-lane sums (keys lane, lane + 64, ..
    // in order) and six butterfly adds -- fl(a + b) = fl(b + a), so every lane ends with the same bits.
    // head `wave`'s record: [sequence][row][head][split] of d_k + 2 floats (m, l, a)
    float *rec = ws + ((qrow * n_heads + h0 + wave) * ws_splits + blockIdx.z) * (dk + 2);
    const bool mine = wave < nh;
    float *row = S[wave];
    auto softmax = [&]() __attribute__((always_inline)) {
        __syncthreads();  // the scores are complete
        if (mine) {
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
                rec[0] = mx;
                rec[1] = part;
            }
        }
    };

    // ---- a_h = p_h V over the split's keys: wave w carries head w, the accumulators carried across the chunks in key
    // order, P from one broadcast row.  kW = 64: lane = column, the bf16 read alone as 16 bits.  kW = 128: lane l =
    // columns 2 l and 2 l + 1, the dword of the staged row that holds both (2 l < d_k <= kW keeps the read in the row).
    const bool pv = mine && (kW == 64 ? lane : 2 * lane) < dk;
    float acc0 = 0.0f, acc1 = 0.0f;
    auto v_step = [&](uint4 (&pf)[kPer], int c) __attribute__((always_inline)) {
        __syncthreads();  // P complete (c = 0) / the previous chunk consumed
        stage(pf, c, true);
        __syncthreads();
        fetch_g(pf, nc + c + 2);
        if (pv) {
            const int j0 = c * kChunk, kn = min(kChunk, n - j0);
            const float *p = row + j0;
            auto element = [&](int k) __attribute__((always_inline)) -> uint32_t {
                if constexpr (kW == 64) return reinterpret_cast<const uint16_t *>(KV + k * kStride)[lane];
                else return KV[k * kStride + lane];
            };
            auto add = [&](float pk, uint32_t v) __attribute__((always_inline)) {
                if constexpr (kW == 64) {
                    acc0 = fmaf(pk, bf16_lo(v), acc0);
                } else {
                    acc0 = fmaf(pk, bf16_lo(v), acc0);
                    acc1 = fmaf(pk, bf16_hi(v), acc1);
                }
            };
            int k = 0;
            for (; k + 8 <= kn; k += 8) {
                const float4 a0 = *reinterpret_cast<const float4 *>(p + k);
                const float4 a1 = *reinterpret_cast<const float4 *>(p + k + 4);
                uint32_t v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = element(k + u);
                add(a0.x, v[0]);
                add(a0.y, v[1]);
                add(a0.z, v[2]);
                add(a0.w, v[3]);
                add(a1.x, v[4]);
                add(a1.y, v[5]);
                add(a1.z, v[6]);
                add(a1.w, v[7]);
            }
            for (; k < kn; ++k) add(p[k], element(k));
        }
    };
    // ---- the stream: chunk g sits in pfa (g even) or pfb (g odd), K chunks first, the softmax between chunk nc - 1 and
    // chunk nc, every branch workgroup-uniform (ONE loop over the whole stream, as attention_decode_kv16_kernel: a K
    // loop and a V loop that starts on either buffer cost copies of both buffers there)
    auto step = [&](uint4 (&pf)[kPer], int g) __attribute__((always_inline)) {
        if (g < nc) {
            k_step(pf, g);
        } else {
            if (g == nc) softmax();
            v_step(pf, g - nc);
        }
    };
    for (int g = 0; g < 2 * nc; g += 2) {
        step(pfa, g);
        step(pfb, g + 1);
    }
    // the a-row: lane = column(s), a wave stores 256 / 512 contiguous bytes
    if (pv) {
        if constexpr (kW == 64) {
            rec[2 + lane] = acc0;
        } else {
            rec[2 + 2 * lane] = acc0;
            rec[3 + 2 * lane] = acc1;  // (d_k is 96 or 128: column 2 l + 1 < d_k with 2 l)
        }
    }
}

}  // namespace

const char *attention_split_kv16_plan_name(int dk) {
    return dk <= kDecMaxDk ? "attention_decode_split_kv16_kernel" : "attention_decode_split_kv16_wide_kernel";
}

// tab: checked and clamped by launch_attention_split_kv16 (attention_launch.hip); attention_split_launch_dims tests again
// what sizes the grid, the kernels' LDS rows and the workspace records
hipError_t launch_attention_decode_split_kv16(const float *Q, int64_t ldq, const bf16_t *K, int64_t ldk,
                                              int64_t k_stride_seq, const bf16_t *V, int64_t ldv, int64_t v_stride_seq,
                                              float *O, int64_t ldo, int n_seqs, int rows_per_seq,
                                              const DecodeBatchTable &tab, bool causal, int n_heads, int n_kv_heads, int dk,
                                              float scale, int split, float *workspace, size_t ws_bytes,
                                              hipStream_t stream) {
    int ws_splits, grid_z;
    if (attention_split_launch_dims(n_seqs, rows_per_seq, tab, causal, n_heads, n_kv_heads, dk, split, workspace, ws_bytes,
                                    ws_splits, grid_z))
        return hipErrorInvalidValue;
    const int group = n_heads / n_kv_heads;
    const DecodeMany many{k_stride_seq, v_stride_seq, rows_per_seq, tab};
    const dim3 grid((unsigned)(n_kv_heads * ((group + kDecGroupHeads - 1) / kDecGroupHeads)),
                    (unsigned)(rows_per_seq * n_seqs), (unsigned)grid_z);
    auto *kernel = dk > kDecMaxDk ? (causal ? attention_decode_split_kv16_kernel<true, kDecWideDk>
                                            : attention_decode_split_kv16_kernel<false, kDecWideDk>)
                                  : (causal ? attention_decode_split_kv16_kernel<true, kDecMaxDk>
                                            : attention_decode_split_kv16_kernel<false, kDecMaxDk>);
    kernel<<<grid, kDecThreads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, workspace, dk, scale, group, n_heads, split,
                                             ws_splits, many);
    hipError_t e = hipGetLastError();
    if (e) return e;
    return launch_attention_decode_merge(workspace, O, ldo, n_seqs, rows_per_seq, tab, causal, n_heads, dk, split,
                                         ws_splits, stream);
}

}  // namespace qgemm
