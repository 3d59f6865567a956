// attention_decode_kv16.hip -- decode attention over a bf16 K / V cache, and the kernel that fills one.
// Q and O are fp32, K and V are bf16 slabs [slabs, rows, n_kv_heads * d_k]; the arithmetic is fp32 and, because
// bf16 -> fp32 is exact, every output row is BIT FOR BIT what attention_decode_gqa_kernel (G >= 2) and
// attention_decode_kernel (G = 1) give on K / V widened to fp32: a score is the fmaf chain from +0 over k ascending,
// zero-padded to 32; the softmax is softmax_row_max / softmax_exp, the ONE sequential sum in column order (hop_left
// over 16-element blocks), __fdiv_rn; P V is each column's fmaf chain over ALL keys in key order, then fl(acc + 0) when
// seq_kv % 32 != 0; a masked key has P = +0 and still contributes; an indirect table entry that names no slab reads as
// quiet NaNs (bf16 0x7fc0 widens to the fp32 quiet NaN the fp32 kernels select).
// The grid is attention_decode_gqa_kernel's: ONE WORKGROUP of 256 threads per (KV head, block of up to 4 query heads of
// its group, query row, sequence), G = 1 included (a block of one head).  What the halved row changes is the geometry:
//   chunk      256 keys (the fp32 kernels: 128) at the fp32 kernels' LDS and register footprint: a row is kW bf16 + 8
//              of padding, 144 / 272 bytes (36 / 68 dwords, both = 4 mod 32: a thread-per-key b128 read is
//              conflict-free and every row starts on 16 bytes), a chunk 36 / 68 KiB; rows stay bf16 in LDS
//   fetch      16-byte pieces of 8 bf16, 8 / 16 per thread and chunk (the register count of the fp32 buffers), two
//              chunks in flight; branch-free and clamped, the zero / NaN select in `put`, the indirect form's nxo
//              read before the refilled buffer is `put` (attention_decode_kernel.h has the reasons).  A matrix that
//              cannot take 16-byte loads is read element by element when its chunk is staged, not ahead
//   s_h[j]     thread t owns key t of the chunk: it reads its K row from LDS ONCE as b128 reads of 8 elements, widens
//              in registers (low half x << 16, high half x & 0xffff0000) and runs the chains of ALL the block's heads
//              against it; the upper two chains are skipped by a workgroup-uniform branch when the block has <= 2 heads
//   softmax    wave w = head w, everything wave-local: attention_decode_gqa_kernel's text (a copy on purpose: shared
//              with the prologue it measured 1 - 2 % slower through the indirect table)
//   O_h = p V  wave w = head w at both widths; lane l owns columns 2l and 2l + 1: ONE b32 LDS read per key feeds both
//              columns' fmaf chains, P comes from one broadcast row; lanes with 2l >= d_k sit idle
// so a key costs half the barriers and half the memory round trips of the fp32 kernels.
// LDS: four score rows (64 KiB) + one chunk (36 / 68 KiB) + four query rows (1 / 2 KiB) + the indirect form's tables
// (5 KiB): 139 KiB at kW = 128, one workgroup per CU.
// kv_append_bf16_kernel rounds new fp32 K / V rows to bf16 (pk_bf16: the GEMM epilogue's rounding) into rows
// pos[b] .. of slab kv_slot[b], the tables in the kernel arguments.
// Built with the packed fp32 instructions off, as attention_decode_gqa.o (Makefile).
#include <climits>

#include "attention_decode_kernel.h"

namespace qgemm {

namespace {

constexpr int kKv16Chunk = 256;     // keys per staged K / V chunk: one per thread
constexpr int kKv16Pad = 8;         // bf16 elements of padding behind a staged row

__device__ __forceinline__ float bf16_lo(uint32_t x) { return __uint_as_float(x << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t x) { return __uint_as_float(x & 0xffff0000u); }

// group: G.  grid x = n_kv_heads * ceil(G / 4), y = query rows, z = sequences (DecodeMany, DecodeIndirect; their
// strides count bf16 elements).
template <bool kCausal, typename Seqs, int kW>
__global__ __launch_bounds__(kDecThreads) void attention_decode_kv16_kernel(
    const float *__restrict__ Q, int64_t ldq, const bf16_t *__restrict__ K, int64_t ldk, const bf16_t *__restrict__ V,
    int64_t ldv, float *__restrict__ O, int64_t ldo, int dk, float scale, int group, Seqs seqs) {
    static_assert(kKv16Chunk == kDecThreads, "thread t owns key t of a chunk");
    __shared__ __attribute__((aligned(16))) float S[kDecGroupHeads][kDecMaxSeq];
    constexpr int kPieces = kW / 8;                                   // 8-element pieces of a row: 8 / 16
    constexpr int kStride = (kW + kKv16Pad) / 2;                      // chunk row stride (dwords): 36 / 68
    constexpr int kPer = kKv16Chunk * kPieces / kDecThreads;          // pieces of a chunk per thread: 8 / 16
    // Piece i of thread t: 8 threads share a row and read 128 contiguous bytes of it, a thread holds kSeg = 1 / 2
    // pieces of each of its 8 rows -- so the indirect form keeps 8 slab offsets per thread at both widths
    constexpr int kSeg = kPieces / 8, kRows = kPer / kSeg;
    static_assert(kRows == 8 && kRows * 32 == kKv16Chunk, "rows (t >> 3) + 32 r, r < 8, cover the chunk");
    __shared__ __attribute__((aligned(16))) uint32_t KV[kKv16Chunk * kStride];
    __shared__ __attribute__((aligned(16))) float Qs[kDecGroupHeads][kW];
    const int nblk = (group + kDecGroupHeads - 1) / kDecGroupHeads;
    const int kvh = blockIdx.x / nblk, blk = blockIdx.x - kvh * nblk, qi = blockIdx.y;
    const int h0 = kvh * group + kDecGroupHeads * blk;                // the block's first query head
    const int nh = min(kDecGroupHeads, group - kDecGroupHeads * blk); // its heads: 1 .. 4
    int seq_kv, q_pos0;
    constexpr bool kIndirect = std::is_same<Seqs, DecodeIndirect>::value;
    // DecodeIndirect alone, as attention_decode_kernel: the sequence's table row and the slabs' offsets in LDS
    const uint8_t *own = nullptr;
    const int64_t *ko = nullptr, *vo = nullptr;
    int64_t kss = 0, vss = 0;
    int n_slabs = 0;
    if constexpr (kIndirect) {
        __shared__ __attribute__((aligned(16))) uint8_t Own[kDecMaxSeq + 16];
        __shared__ int64_t SlabOff[2][kDecodeMaxBatch];
        const int b = blockIdx.z;
        const int64_t row0 = (int64_t)b * seqs.rows_per_seq;
        Q += row0 * ldq;
        O += row0 * ldo;
        seq_kv = seqs.tab.seq_kv[b];
        q_pos0 = seqs.tab.q_pos0[b];
        const uint8_t *tp = seqs.row_slab + seqs.tab.kv_slot[b] * seqs.row_slab_stride;
        const int off = (int)(reinterpret_cast<uintptr_t>(tp) & 15);
        // (4096 entries from an odd start span 257 pieces: the first thread takes the last one too)
        for (int i = threadIdx.x; 16 * i < off + seq_kv; i += kDecThreads)
            reinterpret_cast<uint4 *>(Own)[i] = reinterpret_cast<const uint4 *>(tp - off)[i];
        if (threadIdx.x < 2 * kDecodeMaxBatch) {
            const int e = min((int)threadIdx.x & (kDecodeMaxBatch - 1), seqs.n_slabs - 1);
            SlabOff[threadIdx.x / kDecodeMaxBatch][threadIdx.x & (kDecodeMaxBatch - 1)] =
                e * (threadIdx.x < kDecodeMaxBatch ? seqs.k_stride_seq : seqs.v_stride_seq);
        }
        __syncthreads();
        own = Own + off;
        ko = SlabOff[0];
        vo = SlabOff[1];
        kss = seqs.k_stride_seq;
        vss = seqs.v_stride_seq;
        n_slabs = seqs.n_slabs;
    } else {
        const int b = blockIdx.z;
        const int64_t row0 = (int64_t)b * seqs.rows_per_seq, slab = seqs.tab.kv_slot[b];
        Q += row0 * ldq;
        O += row0 * ldo;
        K += slab * seqs.k_stride_seq;
        V += slab * seqs.v_stride_seq;
        seq_kv = seqs.tab.seq_kv[b];
        q_pos0 = seqs.tab.q_pos0[b];
    }
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float *Qb = Q + qi * ldq + (int64_t)h0 * dk;
    const bf16_t *Kb = K + (int64_t)kvh * dk, *Vb = V + (int64_t)kvh * dk;
    const int seq = seq_kv;
    // the row's limit (q_pos0 <= seq_kv: the launcher clamps it, so the sum stays in int range)
    const int L = kCausal ? min(seq, qi + q_pos0 + 1) : seq;
    const int nck = (L + kKv16Chunk - 1) / kKv16Chunk;    // K chunks that hold a visible key
    const int ncv = (seq + kKv16Chunk - 1) / kKv16Chunk;  // V chunks: every key
    const int dk8 = (dk + 7) >> 3;                        // 8-element pieces of a row (the last one zero-padded)

    // ---- the K / V stream: attention_decode_kernel's fetch / put / two chunks in flight on pieces of 8 bf16.  The
    // 16-byte loads need an aligned first row, strides that are multiples of 8 elements and d_k % 8 == 0; anything else
    // takes element loads, chosen once per matrix.
    auto aligned = [&](const bf16_t *base, int64_t ld, int64_t ss) {
        return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && (ld & 7) == 0 && (dk & 7) == 0 && (ss & 7) == 0;
    };
    const bool vec_k = aligned(Kb, ldk, kss), vec_v = aligned(Vb, ldv, vss);  // workgroup-uniform
    const int trow = t >> 3, tc8 = t & 7;
    auto row_of = [&](int i) { return trow + 32 * (i / kSeg); };
    auto c8_of = [&](int i) { return tc8 + 8 * (i % kSeg); };
    int64_t nxo[kRows];  // (DecodeIndirect) the slab offsets of the rows the NEXT fetch brings
    auto slabs_of = [&](const int64_t *so, int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < kRows; ++r)
            nxo[r] = so[min((int)own[min(c0 + trow + 32 * r, seq - 1)], kDecodeMaxBatch - 1)];
    };
    auto slab_at = [&](const bf16_t *src, int i) __attribute__((always_inline)) {
        if constexpr (kIndirect) src += nxo[i / kSeg];
        return src;
    };
    // (a matrix on element loads fetches nothing ahead: `stage` below loads it when the chunk is staged)
    auto fetch = [&](uint4 (&r)[kPer], const bf16_t *src, int64_t ld, int c0, bool vec) __attribute__((always_inline)) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const int row = row_of(i), c8 = c8_of(i);
                r[i] = *reinterpret_cast<const uint4 *>(slab_at(src, i) + min(c0 + row, seq - 1) * ld +
                                                        8 * min(c8, dk8 - 1));
            }
        }
    };
    auto put = [&](const uint4 (&r)[kPer], int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int row = row_of(i), c8 = c8_of(i);
            const bool in = c0 + row < seq && 8 * c8 < dk;  // (d_k % 8 == 0 here: a piece lies below d_k or past it)
            uint4 x = r[i];
            if constexpr (kIndirect) {  // an entry that names no slab: the row reads as quiet NaNs (under the zeros)
                const uint32_t qn = 0x7fc07fc0u;
                if ((int)own[min(c0 + row, seq - 1)] >= n_slabs) x = make_uint4(qn, qn, qn, qn);
            }
            *reinterpret_cast<uint4 *>(KV + row * kStride + 4 * c8) = in ? x : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    // The element loads -- any alignment, any stride, any d_k -- go from memory to LDS when the chunk is staged, piece
    // by piece in a loop that is NOT unrolled, with the same clamps, zeros and NaNs.  (Fetched two chunks ahead like the
    // 16-byte pieces they were 128 loads of 16 bits and as many 64-bit addresses per chunk beside the two buffers: every
    // wide instantiation then spilled registers.  The price is one exposed memory latency per chunk on this path.)
    auto put_elements = [&](const bf16_t *src, int64_t ld, const int64_t *so, int c0) __attribute__((always_inline)) {
#pragma unroll 1
        for (int i = 0; i < kPer; ++i) {
            const int row = row_of(i), c8 = c8_of(i), key = min(c0 + row, seq - 1);
            const bool in = c0 + row < seq;
            const bf16_t *p = src + key * ld;
            bool none = false;
            if constexpr (kIndirect) {
                const int e = own[key];
                p += so[min(e, kDecodeMaxBatch - 1)];
                none = e >= n_slabs;
            }
            const int keep = in ? dk - 8 * c8 : 0;  // the piece's columns to keep: the rest are zeros
            uint32_t w[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int c = 8 * c8 + 2 * d;
                uint32_t x = (uint32_t)p[min(c, dk - 1)].bits | (uint32_t)p[min(c + 1, dk - 1)].bits << 16;
                if (none) x = 0x7fc07fc0u;
                // (a shift, not two compares per dword: as compares the masks of every column were kept in scalar
                // register pairs across the chunk loops and spilled them)
                w[d] = x & (uint32_t)((1ull << 16 * min(max(keep - 2 * d, 0), 2)) - 1ull);
            }
            *reinterpret_cast<uint4 *>(KV + row * kStride + 4 * c8) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    };
    // chunk c of K (v false) or V into LDS
    auto stage = [&](const uint4 (&r)[kPer], int c, bool v) __attribute__((always_inline)) {
        if (v ? vec_v : vec_k) put(r, c * kKv16Chunk);
        else if (v) put_elements(Vb, ldv, vo, c * kKv16Chunk);
        else put_elements(Kb, ldk, ko, c * kKv16Chunk);
    };
    auto fetch_g = [&](uint4 (&r)[kPer], int g) __attribute__((always_inline)) {
        if (g < nck) fetch(r, Kb, ldk, g * kKv16Chunk, vec_k);
        else if (g < nck + ncv) fetch(r, Vb, ldv, (g - nck) * kKv16Chunk, vec_v);
    };
    auto slabs_g = [&](int g) __attribute__((always_inline)) {
        if (g < nck) slabs_of(ko, g * kKv16Chunk);
        else if (g < nck + ncv) slabs_of(vo, (g - nck) * kKv16Chunk);
    };
    uint4 pfa[kPer], pfb[kPer];
    if constexpr (kIndirect) slabs_g(0);
    fetch_g(pfa, 0);
    if constexpr (kIndirect) slabs_g(1);
    fetch_g(pfb, 1);
    // the block's query rows, zeros past d_k and in the rows of heads the block does not have
    for (int i = t; i < kDecGroupHeads * kW; i += kDecThreads) {
        const int hh = i / kW, c = i & (kW - 1);
        Qs[hh][c] = hh < nh && c < dk ? Qb[(int64_t)hh * dk + c] : 0.0f;
    }

    // ---- s_h[j] = Q_h[i] . K[j], j < L: thread t runs the chains of key t of the chunk for every head of the block --
    // each 8-element piece of the K row read from LDS ONCE and widened in registers, the query rows as broadcast reads.
    // Each chain is attention_decode_kernel's `steps` in order: k ascending from +0 over d_k zero-padded to 32.  A head
    // the block lacks runs on the zero query row into a score row nobody reads; with at most two heads the upper two
    // chains are skipped.
    const int nsteps = dk > (kW == 64 ? 32 : 96) ? kPieces : kPieces - 4;  // pieces of a chain: d_k zero-padded to 32
    const bool upper = nh > 2;  // workgroup-uniform
    auto k_step = [&](uint4 (&pf)[kPer], int c) __attribute__((always_inline)) {
        if constexpr (kIndirect) slabs_g(c + 2);
        if (c) __syncthreads();  // every thread is done with the previous chunk
        stage(pf, c, false);
        __syncthreads();
        fetch_g(pf, c + 2);
        const int j = c * kKv16Chunk + t;
        if (j < L) {
            const uint4 *kr = reinterpret_cast<const uint4 *>(KV + t * kStride);
            auto chains = [&](auto four) __attribute__((always_inline)) {
                constexpr int kN = decltype(four)::value ? 4 : 2;
                float res[kN];
#pragma unroll
                for (int h = 0; h < kN; ++h) res[h] = 0.0f;
                // (a loop over the 8-column pieces, not unrolled.  Unrolled as the fp32 kernels' `steps`, the whole row's
                // reads were issued together and the wide forms took 410 - 450 registers and spilled scalar ones; a
                // loop over 32-column steps measured 3 % slower than this one at 64 sequences x 32 / 8 heads x d_k 128.)
#pragma unroll 1
                for (int s = 0; s < nsteps; ++s) {
                    {
                        const uint4 b = kr[s];
                        const float k0 = bf16_lo(b.x), k1 = bf16_hi(b.x), k2 = bf16_lo(b.y), k3 = bf16_hi(b.y);
                        const float k4 = bf16_lo(b.z), k5 = bf16_hi(b.z), k6 = bf16_lo(b.w), k7 = bf16_hi(b.w);
#pragma unroll
                        for (int h = 0; h < kN; ++h) {
                            const float4 a0 = reinterpret_cast<const float4 *>(Qs[h])[2 * s];
                            const float4 a1 = reinterpret_cast<const float4 *>(Qs[h])[2 * s + 1];
                            res[h] = fmaf(a0.x, k0, res[h]);
                            res[h] = fmaf(a0.y, k1, res[h]);
                            res[h] = fmaf(a0.z, k2, res[h]);
                            res[h] = fmaf(a0.w, k3, res[h]);
                            res[h] = fmaf(a1.x, k4, res[h]);
                            res[h] = fmaf(a1.y, k5, res[h]);
                            res[h] = fmaf(a1.z, k6, res[h]);
                            res[h] = fmaf(a1.w, k7, res[h]);
                        }
                    }
                }
#pragma unroll
                for (int h = 0; h < kN; ++h) S[h][j] = res[h];
            };
            if (upper) chains(std::true_type{});
            else chains(std::false_type{});
        }
    };

    // ---- softmax of head `wave` over its first L columns, in place in its score row: everything is wave-local (no
    // cross-wave step for the maximum, no LDS for the sum); the barrier between the exps and the sum chain orders the
    // lanes' LDS writes before the other lanes' reads.
    float *row = S[wave];
    const bool mine = wave < nh;
    auto softmax = [&]() __attribute__((always_inline)) {
        __syncthreads();  // the scores are complete
        if (mine) {
            const float seed = __fmul_rn(row[0], scale);
            const float cand = softmax_row_max(row, lane + 1, L, 64, scale);
            const float mx = (cand > seed) ? cand : seed;  // (depends on every lane's read of row[0]: the exps follow it)
            for (int c = lane; c < L; c += 64) row[c] = softmax_exp(row[c], scale, mx);
        }
        __syncthreads();
        if (mine) {
            // the ONE sequential sum: attention_decode_kernel's chain, here in the head's own wave
            const int nl = (L + 15) >> 4;  // 16-element blocks that hold an element
            float s = 0.0f;
            for (int b0 = 0; b0 < nl; b0 += 64) {
                const int e0 = 16 * (b0 + lane);
                float e[16];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float4 v = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
                    if (e0 + 4 * j < L) v = *reinterpret_cast<const float4 *>(row + e0 + 4 * j);
                    e[4 * j] = v.x; e[4 * j + 1] = v.y; e[4 * j + 2] = v.z; e[4 * j + 3] = v.w;
                }
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (e0 + j >= L) e[j] = -0.0f;
                const int ns = min(64, nl - b0);
                for (int u = 0; u < ns; ++u) {
                    s = __fadd_rn(hop_left(s), e[0]);
#pragma unroll
                    for (int j = 1; j < 16; ++j) s = __fadd_rn(s, e[j]);
                }
            }
            const float sum = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), (nl - 1) & 63));
            for (int c = lane; c < L; c += 64) row[c] = __fdiv_rn(row[c], sum);
            if constexpr (kCausal)
                for (int c = L + lane; c < seq; c += 64) row[c] = 0.0f;  // P = +0 at the masked keys
        }
    };

    // ---- O_h[i] = p_h V over every key: wave w carries head w, lane l the output columns 2l and 2l + 1 -- the dword
    // of a staged row that holds both -- with the accumulators carried across the chunks in key order.  2l < d_k <= kW
    // keeps the read inside the row.
    const bool pv = mine && 2 * lane < dk;
    float acc0 = 0.0f, acc1 = 0.0f;
    auto v_step = [&](uint4 (&pf)[kPer], int c) __attribute__((always_inline)) {
        if constexpr (kIndirect) slabs_g(nck + c + 2);
        __syncthreads();  // P complete (c = 0) / the previous chunk consumed
        stage(pf, c, true);
        __syncthreads();
        fetch_g(pf, nck + c + 2);
        if (pv) {
            const int k0 = c * kKv16Chunk, kn = min(kKv16Chunk, seq - k0);
            const uint32_t *vcol = KV + lane;
            const float *p = row + k0;
            int k = 0;
            for (; k + 8 <= kn; k += 8) {
                const float4 a0 = *reinterpret_cast<const float4 *>(p + k);
                const float4 a1 = *reinterpret_cast<const float4 *>(p + k + 4);
                uint32_t v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = vcol[(k + u) * kStride];
                acc0 = fmaf(a0.x, bf16_lo(v[0]), acc0);
                acc1 = fmaf(a0.x, bf16_hi(v[0]), acc1);
                acc0 = fmaf(a0.y, bf16_lo(v[1]), acc0);
                acc1 = fmaf(a0.y, bf16_hi(v[1]), acc1);
                acc0 = fmaf(a0.z, bf16_lo(v[2]), acc0);
                acc1 = fmaf(a0.z, bf16_hi(v[2]), acc1);
                acc0 = fmaf(a0.w, bf16_lo(v[3]), acc0);
                acc1 = fmaf(a0.w, bf16_hi(v[3]), acc1);
                acc0 = fmaf(a1.x, bf16_lo(v[4]), acc0);
                acc1 = fmaf(a1.x, bf16_hi(v[4]), acc1);
                acc0 = fmaf(a1.y, bf16_lo(v[5]), acc0);
                acc1 = fmaf(a1.y, bf16_hi(v[5]), acc1);
                acc0 = fmaf(a1.z, bf16_lo(v[6]), acc0);
                acc1 = fmaf(a1.z, bf16_hi(v[6]), acc1);
                acc0 = fmaf(a1.w, bf16_lo(v[7]), acc0);
                acc1 = fmaf(a1.w, bf16_hi(v[7]), acc1);
            }
            for (; k < kn; ++k) {
                const uint32_t v = vcol[k * kStride];
                acc0 = fmaf(p[k], bf16_lo(v), acc0);
                acc1 = fmaf(p[k], bf16_hi(v), acc1);
            }
        }
    };
    // ---- the stream: chunk g sits in pfa (g even) or pfb (g odd), K chunks first, the softmax between chunk nck - 1
    // and chunk nck, every branch workgroup-uniform.  (ONE loop over the whole stream, not a K loop and a V loop that
    // starts on either buffer: the two V loops merged into one text and the compiler paid for it with copies of both
    // buffers, 128 registers at kW = 128.)
    auto step = [&](uint4 (&pf)[kPer], int g) __attribute__((always_inline)) {
        if (g < nck) {
            k_step(pf, g);
        } else {
            if (g == nck) softmax();
            v_step(pf, g - nck);
        }
    };
    for (int g = 0; g < nck + ncv; g += 2) {
        step(pfa, g);
        if (g + 1 < nck + ncv) step(pfb, g + 1);
    }
    if (pv) {
        if (seq & 31) {  // the zero-padded rest of the last 32-key tile: -0 becomes +0
            acc0 = __fadd_rn(acc0, 0.0f);
            acc1 = __fadd_rn(acc1, 0.0f);
        }
        float *o = O + qi * ldo + (int64_t)(h0 + wave) * dk + 2 * lane;
        o[0] = acc0;
        if (2 * lane + 1 < dk) o[1] = acc1;
    }
}

// the instantiation a launch takes (the caller has tested the envelope), on the grid (KV heads x blocks of a group,
// rows, sequences)
template <typename Seqs>
hipError_t kv16_launch(int rows, int n_seqs, bool causal, const float *Q, int64_t ldq, const bf16_t *K, int64_t ldk,
                       const bf16_t *V, int64_t ldv, float *O, int64_t ldo, int n_heads, int n_kv_heads, int dk,
                       float scale, const Seqs &seqs, hipStream_t stream) {
    auto *kernel = dk > kDecMaxDk ? (causal ? attention_decode_kv16_kernel<true, Seqs, kDecWideDk>
                                            : attention_decode_kv16_kernel<false, Seqs, kDecWideDk>)
                                  : (causal ? attention_decode_kv16_kernel<true, Seqs, kDecMaxDk>
                                            : attention_decode_kv16_kernel<false, Seqs, kDecMaxDk>);
    kernel<<<decode_group_grid(n_heads, n_kv_heads, rows, n_seqs), kDecThreads, 0, stream>>>(
        Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, n_heads / n_kv_heads, seqs);
    return hipGetLastError();
}

// ---- kv_append_bf16_kernel: grid (source rows, 2048-column blocks, K | V); a thread rounds one piece of 8 columns.
struct AppendTable {
    int kv_slot[kDecodeMaxBatch], pos[kDecodeMaxBatch];
};
struct AppendSide {
    const float *src;
    int64_t src_ld;
    bf16_t *dst;
    int64_t dst_ld, dst_ss;
};

__global__ __launch_bounds__(kDecThreads) void kv_append_bf16_kernel(AppendSide k, AppendSide v, int rows_per_seq,
                                                                     int width, AppendTable tab) {
    const AppendSide m = blockIdx.z ? v : k;
    const int r = blockIdx.x, b = r / rows_per_seq, c0 = 8 * (blockIdx.y * kDecThreads + threadIdx.x);
    if (c0 >= width) return;
    const float *s = m.src + r * m.src_ld + c0;
    bf16_t *d = m.dst + tab.kv_slot[b] * m.dst_ss + (tab.pos[b] + (r - b * rows_per_seq)) * m.dst_ld + c0;
    const bool whole = c0 + 8 <= width;
    // every piece of a matrix is aligned when its first row is and its strides are multiples of a piece
    const bool vec_s = (reinterpret_cast<uintptr_t>(m.src) & 15) == 0 && (m.src_ld & 3) == 0;
    const bool vec_d = (reinterpret_cast<uintptr_t>(m.dst) & 15) == 0 && (m.dst_ld & 7) == 0 && (m.dst_ss & 7) == 0;
    float x[8];
    if (whole && vec_s) {
        const float4 a = reinterpret_cast<const float4 *>(s)[0], c = reinterpret_cast<const float4 *>(s)[1];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
        x[4] = c.x; x[5] = c.y; x[6] = c.z; x[7] = c.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = s[min(e, width - 1 - c0)];
    }
    const uint4 p = make_uint4(pk_bf16(x[0], x[1]), pk_bf16(x[2], x[3]), pk_bf16(x[4], x[5]), pk_bf16(x[6], x[7]));
    if (whole && vec_d) {
        *reinterpret_cast<uint4 *>(d) = p;
    } else {
        const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (c0 + e < width) d[e].bits = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
    }
}

}  // namespace

// whole groups of 1 .. 16 heads inside either decode envelope
bool attention_decode_kv16_ok(int rows_per_seq, int seq_kv, int dk, int n_heads, int n_kv_heads) {
    return rows_per_seq >= 1 && seq_kv >= 1 && dk >= 1 && attention_decode_any_ok(rows_per_seq, seq_kv, dk) &&
           groups_ok(n_heads, n_kv_heads, 1);
}

const char *attention_decode_kv16_plan_name(int dk) {
    return dk <= kDecMaxDk ? "attention_decode_kv16_kernel" : "attention_decode_kv16_wide_kernel";
}

// decode_table_from_host's checks and table (attention_launch.hip) and the envelope.  Every check comes before the
// launch, and nothing outside the envelope has another path: hipErrorInvalidValue.
static hipError_t batched_kv16(const float *Q, int64_t ldq, const bf16_t *K, int64_t ldk, int64_t k_stride_seq,
                               const bf16_t *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo, int n_seqs,
                               int rows_per_seq, bool indirect, const uint8_t *row_slab, int64_t row_slab_stride,
                               int n_slabs, const int *slot, const int *seq_kv, const int *q_pos0, int n_heads,
                               int n_kv_heads, int dk, float scale, hipStream_t stream) {
    DecodeBatchTable tab;  // filled by decode_table_from_host, read only after its success
    if (!Q || !K || !V || !O || !attention_decode_kv16_ok(rows_per_seq, 1, dk, n_heads, n_kv_heads) ||
        decode_table_from_host(n_seqs, rows_per_seq, dk, slot, seq_kv, q_pos0, indirect, row_slab, row_slab_stride,
                               n_slabs, tab))
        return hipErrorInvalidValue;
    if (n_seqs == 0) return hipSuccess;
    if (indirect) {
        const DecodeIndirect ind{k_stride_seq, v_stride_seq, rows_per_seq, n_slabs, row_slab, row_slab_stride, tab};
        return kv16_launch(rows_per_seq, n_seqs, q_pos0 != nullptr, Q, ldq, K, ldk, V, ldv, O, ldo, n_heads, n_kv_heads,
                           dk, scale, ind, stream);
    }
    const DecodeMany many{k_stride_seq, v_stride_seq, rows_per_seq, tab};
    return kv16_launch(rows_per_seq, n_seqs, q_pos0 != nullptr, Q, ldq, K, ldk, V, ldv, O, ldo, n_heads, n_kv_heads, dk,
                       scale, many, stream);
}

hipError_t launch_attention_batched_kv16(const float *Q, int64_t ldq, const bf16_t *K, int64_t ldk, int64_t k_stride_seq,
                                         const bf16_t *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                         int n_seqs, int rows_per_seq, const int *kv_slot, const int *seq_kv,
                                         const int *q_pos0, int n_heads, int n_kv_heads, int dk, float scale,
                                         hipStream_t stream) {
    return batched_kv16(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs, rows_per_seq, false, nullptr,
                        0, 0, kv_slot, seq_kv, q_pos0, n_heads, n_kv_heads, dk, scale, stream);
}

hipError_t launch_attention_indirect_kv16(const float *Q, int64_t ldq, const bf16_t *K, int64_t ldk,
                                          int64_t k_stride_seq, const bf16_t *V, int64_t ldv, int64_t v_stride_seq,
                                          float *O, int64_t ldo, int n_seqs, int rows_per_seq, const uint8_t *row_slab,
                                          int64_t row_slab_stride, int n_slabs, const int *tab_row, const int *seq_kv,
                                          const int *q_pos0, int n_heads, int n_kv_heads, int dk, float scale,
                                          hipStream_t stream) {
    return batched_kv16(Q, ldq, K, ldk, k_stride_seq, V, ldv, v_stride_seq, O, ldo, n_seqs, rows_per_seq, true, row_slab,
                        row_slab_stride, n_slabs, tab_row, seq_kv, q_pos0, n_heads, n_kv_heads, dk, scale, stream);
}

// the tables travel in the kernel arguments: nothing is copied, allocated or synchronized
hipError_t launch_kv_append_bf16(const float *K, int64_t k_ld, const float *V, int64_t v_ld, bf16_t *Kc, int64_t kc_ld,
                                 int64_t kc_stride_seq, bf16_t *Vc, int64_t vc_ld, int64_t vc_stride_seq, int n_seqs,
                                 int rows_per_seq, const int *kv_slot, const int *pos, int width, hipStream_t stream) {
    constexpr int kBlockCols = 8 * kDecThreads;
    if (!K || !V || !Kc || !Vc || !pos || n_seqs < 1 || n_seqs > kDecodeMaxBatch || rows_per_seq < 1 ||
        rows_per_seq > INT_MAX / kDecodeMaxBatch || width < 1 || width > 65535 * kBlockCols)
        return hipErrorInvalidValue;
    AppendTable tab = {};  // entries past n_seqs are never read; zeroed so the arguments are defined bytes
    for (int b = 0; b < n_seqs; ++b) {
        if (pos[b] < 0 || pos[b] > INT_MAX - rows_per_seq || (kv_slot && kv_slot[b] < 0)) return hipErrorInvalidValue;
        tab.kv_slot[b] = kv_slot ? kv_slot[b] : b;
        tab.pos[b] = pos[b];
    }
    const dim3 grid((unsigned)(n_seqs * rows_per_seq), (unsigned)((width + kBlockCols - 1) / kBlockCols), 2);
    const AppendSide k{K, k_ld, Kc, kc_ld, kc_stride_seq}, v{V, v_ld, Vc, vc_ld, vc_stride_seq};
    kv_append_bf16_kernel<<<grid, kDecThreads, 0, stream>>>(k, v, rows_per_seq, width, tab);
    return hipGetLastError();
}

}  // namespace qgemm
