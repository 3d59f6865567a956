// attention_tiled_kv16.hip -- tiled online-softmax prefill attention over a bf16 K / V cache: the launch of
// attention_tiled.hip (s35) with K and V as bf16 rows (strides in bf16 elements), Q and O fp32.  bf16 -> fp32 is exact and
// the arithmetic is the s35 definition (include/qgemm.h), so every output row is BIT FOR BIT what attention_tiled_kernel
// gives on K / V widened to fp32: the definition fixes the 64-key chunks, the MFMA step order of a score, the order of
// the per-lane maximum and sum chains, the two xor steps, the rescale, the key order of the P V steps and the chunks a
// wave passes over -- and not how a chunk is staged or where a column sits inside a staged row.
// Work split and data path: s35's.  A workgroup of 4 waves owns (sequence, query head, tile of 64 query rows), wave w the
// rows 16 w .. 16 w + 15; both products run transposed on v_mfma_f32_16x16x4_f32 with P register-resident; m, l and the
// accumulator never leave registers.  What the halved row changes:
//   rows      stay bf16 through the global loads, the registers and LDS and are widened where an MFMA operand is formed
//             (x << 16, x & 0xffff0000: no conversion instruction, nothing can round)
//   buffers   TWO chunks of K and V in LDS at the fp32 kernel's footprint (38 / 68 KiB against 34 / 66), so ONE barrier
//             per chunk: chunk c + 1 is written into the other buffer while a slower wave still reads chunk c, and the
//             barrier of chunk c + 1 is what orders chunk c + 2's writes behind chunk c's reads
//   columns   are PERMUTED inside a staged row so that what one lane needs for consecutive MFMA steps is adjacent:
//             K   column 4 s + lk sits at 32 (s / 8) + 8 lk + s % 8: lane (lr, lk) reads the eight columns of steps
//                 8 g .. 8 g + 7 with ONE 128-bit read (the fp32 kernel: eight 32-bit reads)
//             V   column 16 ct + lr sits at (kW / 16) lr + ct: lane (lr, lk) reads one key's columns of all the column
//                 tiles with ONE 128-bit (kW 128) or 64-bit (kW 64) read (the fp32 kernel: eight or four 32-bit reads)
//             kW 128: 16 + 16 LDS reads per wave, lane and chunk in the place of 128 + 128.
//   staging   thread t owns row t >> 2 of the chunk and a quarter of it: for K 16 / 32 consecutive columns (all four lk of
//             4 / 8 steps), for V the 8-column halves (t & 1) of the column tiles (kW / 32) (t >> 1 & 1) + j -- so that
//             the values that end up adjacent come from ONE thread's registers: two 16-bit halves are paired by and / shift
//             / or and written as 4 x 128 (K, kW 128), 4 x 64 (K, kW 64), 8 x 64 (V, kW 128) or 8 x 32 bits (V, kW 64)
//   prefetch  chunk c + 1 in registers under chunk c's MFMAs: 2 + 2 (kW 64) or 4 + 4 (kW 128) 16-byte pieces per thread,
//             half the fp32 kernel's
//   Q         goes from global memory straight to the B fragments (one 32-bit load per step and lane, once per
//             workgroup): no LDS pass and no barrier before the first chunk
// LDS rows and banks (counted as s35 counts them: 64 banks of 4 bytes; a 128-bit access is served 16 lanes at a time, a
// 64-bit one 32 lanes, a 32-bit one 64 lanes):
//   K row     kW / 2 + 4 dwords (36 / 68, = 4 mod 32).  Fragment read (128 bits): the 16 lanes lr = 0 .. 15 of one lk
//             start at dwords 36 lr or 68 lr + const -- mod 64 the 16 multiples of 4, each once: every bank once.
//             Staging write, kW 128 (128 bits): the 16 lanes are 4 rows x 4 quarters at 68 row + 16 quarter = 4 row + 16
//             quarter mod 64: every bank once.  kW 64 (64 bits): 8 rows x 4 quarters at 36 row + {0, 2, 16, 18}; rows
//             four apart are 16 mod 64 apart and meet the other half's quarters: TWO lanes per bank, 4 writes per chunk
//   V row     kW 128: 68 dwords.  Fragment read (128 bits): the 16 lanes of one lk read 64 consecutive dwords of one
//             key's row.  Staging write (64 bits): 8 rows x 4 quarters at 68 row + 32 half + 2 pair = 4 row + 32 half + 2
//             pair mod 64: every bank once.  kW 64: 40 dwords (4 x 40 = 32 mod 64).  Fragment read (64 bits): the 32
//             lanes of two lk read 2 x 32 consecutive dwords of rows four apart: banks 0 .. 31 and 32 .. 63.  Staging
//             write (32 bits): 16 rows x 4 quarters at 40 row + 16 half + pair: FOUR lanes per bank, 8 writes per chunk.
//             Both conflicts are on the writes of the narrow kernel, 12 instructions per thread and chunk beside 128
//             MFMAs per wave, and are left as they are: a stride that frees the writes puts the conflict on the reads
// K / V loads: 16-byte loads where the matrix's first row is 16-byte aligned, its row stride a multiple of 8 elements and
// d_k % 8 == 0, else element loads -- chosen once per matrix (the kv16 rule, attention_decode_kv16.hip).  Every address
// is clamped into the tile's visible keys and below d_k and the zeros are selected: nothing a key at or past the tile's
// largest limit holds reaches a register that is used.
#include "qgemm_internal.h"

#include <type_traits>

namespace qgemm {

namespace {

constexpr int kT16TQ = 64;        // query rows per workgroup: 16 per wave
constexpr int kT16C = 64;         // keys per chunk (s35's arithmetic chunk, and the staged block)
constexpr int kT16Threads = 256;  // 4 waves

template <int kW>
struct Tiled16Tile {
    static_assert(kW == 64 || kW == 128, "the row widths of the other attention kernels");
    static constexpr int kPieces = kW / 32;              // 16-byte pieces per thread, matrix and chunk: 2 / 4
    static constexpr int kStrideK = kW / 2 + 4;          // dwords of a staged K row: 36 / 68
    static constexpr int kStrideV = kW == 64 ? 40 : 68;  // ... of a staged V row
    static constexpr int kBuf = kT16C * (kStrideK + kStrideV);  // dwords of one buffer: K rows, then V rows
    static constexpr int kSteps = kW / 4;                // k-steps of a full-width row in S^T
    static constexpr int kColTiles = kW / 16;            // 16-column tiles of O
    static_assert(kT16C * 4 == kT16Threads, "four threads stage a row");
    static_assert(2 * kBuf * 4 * 2 <= 160 * 1024, "two workgroups per CU");
};

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_lo(uint32_t x) { return __uint_as_float(x << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t x) { return __uint_as_float(x & 0xffff0000u); }
// the low (high) halves of a and b as one dword, a's in the low half
__device__ __forceinline__ uint32_t pair_lo(uint32_t a, uint32_t b) { return (a & 0xffffu) | (b << 16); }
__device__ __forceinline__ uint32_t pair_hi(uint32_t a, uint32_t b) { return (a >> 16) | (b & 0xffff0000u); }
// element e of a row of bf16 pairs
__device__ __forceinline__ float bf16_at(const uint32_t *x, int e) { return e & 1 ? bf16_hi(x[e >> 1]) : bf16_lo(x[e >> 1]); }

// the sequences of a launch, by value in the kernel arguments (TiledSeqs of attention_tiled.hip)
struct Tiled16Seqs {
    int n_seqs;
    FusedSeqTable tab;
};
static_assert(sizeof(Tiled16Seqs) + 88 < 4096, "the table travels in the kernel arguments");

template <bool kCausal, int kW>
__global__ __launch_bounds__(kT16Threads) __attribute__((amdgpu_waves_per_eu(2))) void attention_tiled_kv16_kernel(
    const float *__restrict__ Q, int64_t ldq, const bf16_t *__restrict__ K, int64_t ldk, const bf16_t *__restrict__ V,
    int64_t ldv, float *__restrict__ O, int64_t ldo, int dk, int group, float scale2, Tiled16Seqs seqs) {
    using T = Tiled16Tile<kW>;
    constexpr int kStrideK = T::kStrideK, kStrideV = T::kStrideV, kPieces = T::kPieces, kC = kT16C, kTQ = kT16TQ;
    constexpr int kVD = T::kColTiles / 2;  // dwords a lane reads of a staged V row: 2 / 4
    __shared__ __attribute__((aligned(16))) uint32_t lds[2 * T::kBuf];
    // the work map of attention_tiled_kernel: XCD-aware, head by head, inside a head the LAST tile first
    const int nwg = gridDim.x, lin = blockIdx.x;
    const int xq = nwg >> 3, xr = nwg & 7, xc = lin & 7;
    const int logical = (xc < xr ? xc * (xq + 1) : xr * (xq + 1) + (xc - xr) * xq) + (lin >> 3);
    int b = 0, hi = seqs.n_seqs;
    while (hi - b > 1) {  // the last sequence whose first item is at or below `logical`: wave-uniform, scalar loads
        const int mid = (b + hi) >> 1;
        if (seqs.tab.item0[mid] <= logical) b = mid;
        else hi = mid;
    }
    const int seq_q = seqs.tab.seq_q[b], seq = seqs.tab.seq_kv[b], q_pos0 = seqs.tab.q_pos0[b];
    const int tiles = (seq_q + kTQ - 1) / kTQ, local = logical - seqs.tab.item0[b];
    const int h = local / tiles, q0 = (tiles - 1 - (local - h * tiles)) * kTQ;
    {
        const int64_t qr = seqs.tab.q_row0[b], kr = seqs.tab.kv_row0[b];
        Q += qr * ldq;
        O += qr * ldo;
        K += kr * ldk;
        V += kr * ldv;
    }
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int hkv = h / group;
    const float *Qb = Q + (int64_t)h * dk;
    const bf16_t *Kb = K + (int64_t)hkv * dk, *Vb = V + (int64_t)hkv * dk;
    const int lr = lane & 15, lk = lane >> 4;
    const int rows = seq_q - q0 < kTQ ? seq_q - q0 : kTQ;  // >= 1: the work map holds no empty tile
    const int dk4 = (dk + 3) >> 2, dk8 = (dk + 7) >> 3;
    // row i of the sequence sees keys 0 .. limit(i) - 1, 1 <= limit(i) <= seq (q_pos0 <= seq: the launcher clamps it)
    auto limit = [&](int i) __attribute__((always_inline)) {
        return kCausal ? (int)min((int64_t)seq, (int64_t)q_pos0 + i + 1) : seq;
    };
    const int lmax = limit(q0 + rows - 1);       // the tile's largest limit: nothing at or past it is used
    const int nck = (lmax + kC - 1) / kC;        // >= 1
    // the wave's largest limit; a wave without rows computes nothing (it still stages and meets the barriers)
    const int wmax = wave * 16 < rows ? limit(q0 + min(wave * 16 + 15, rows - 1)) : 0;
    const int myrow = q0 + min(wave * 16 + lr, rows - 1);  // a lane past the tile's rows shadows the last row
    const int mylim = limit(myrow);

    // ---- the K / V stream: thread t fetches kPieces 16-byte pieces of row t >> 2 of the chunk, pieces p0, p0 + pstep, ..
    // (8 columns each).  The row is clamped to the tile's last visible key, the piece (the column) below d_k; what lies at
    // or past lmax or d_k is selected to zero here, before it can reach LDS.
    auto aligned = [&](const bf16_t *base, int64_t ld) {
        return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && (ld & 7) == 0 && (dk & 7) == 0;
    };
    const bool vec_k = aligned(Kb, ldk), vec_v = aligned(Vb, ldv);  // workgroup-uniform
    const int frow = t >> 2, fq = t & 3;
    auto fetch = [&](uint4 (&r)[kPieces], const bf16_t *src, int64_t ld, int c0, int p0, int pstep, bool vec)
                     __attribute__((always_inline)) {
        if (vec) {  // (d_k % 8 == 0: a piece lies below d_k or past it; a matrix on element loads fetches nothing ahead)
            const int j = c0 + frow;
            const bf16_t *row = src + min(j, lmax - 1) * ld;
#pragma unroll
            for (int i = 0; i < kPieces; ++i) {
                const int p = p0 + i * pstep;
                const uint4 v = *reinterpret_cast<const uint4 *>(row + 8 * min(p, dk8 - 1));
                r[i] = j < lmax && p < dk8 ? v : make_uint4(0u, 0u, 0u, 0u);
            }
        }
    };
    // The element loads -- any alignment, any stride, any d_k -- go from memory to LDS when the chunk is staged, column by
    // column in a loop that is NOT unrolled, with the same clamps and zeros and 16-bit writes to the permuted places
    // (attention_decode_kv16_kernel has the reason: fetched ahead and unrolled they cost the registers of the fast path).
    // The thread's columns are its quarter of the row, kW / 4 fq ..; v: V's permutation, else K's
    auto put_elements = [&](const bf16_t *src, int64_t ld, int c0, uint32_t *dst, int stride, bool v)
                            __attribute__((always_inline)) {
        const int j = c0 + frow;
        const bf16_t *row = src + min(j, lmax - 1) * ld;
        uint16_t *out = reinterpret_cast<uint16_t *>(dst + frow * stride);
#pragma unroll 1
        for (int e = 0; e < kW / 4; ++e) {
            const int c = kW / 4 * fq + e;
            const uint16_t x = row[min(c, dk - 1)].bits;
            const int at = v ? (c & 15) * T::kColTiles + (c >> 4) : 32 * (c >> 5) + 8 * (c & 3) + ((c >> 2) & 7);
            out[at] = j < lmax && c < dk ? x : (uint16_t)0;
        }
    };
    // K: the quarter's pieces are consecutive -- columns 8 kPieces fq .., the steps s = 2 kPieces fq .. of all four lk.
    // Piece j holds steps 2 j' and 2 j' + 1: .x = (lk 0, lk 1) and .y = (lk 2, lk 3) of the first, .z and .w of the second
    auto put_k = [&](const uint4 (&r)[kPieces], uint32_t *Ks) __attribute__((always_inline)) {
        uint32_t *dst = Ks + frow * kStrideK + ((fq * kPieces) >> 2) * 16 + ((fq * kPieces) & 3);
        uint32_t o[4][kPieces];
#pragma unroll
        for (int j = 0; j < kPieces; ++j) {
            o[0][j] = pair_lo(r[j].x, r[j].z);
            o[1][j] = pair_hi(r[j].x, r[j].z);
            o[2][j] = pair_lo(r[j].y, r[j].w);
            o[3][j] = pair_hi(r[j].y, r[j].w);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (kPieces == 4) *reinterpret_cast<uint4 *>(dst + 4 * k) = make_uint4(o[k][0], o[k][1], o[k][2], o[k][3]);
            else *reinterpret_cast<uint2 *>(dst + 4 * k) = make_uint2(o[k][0], o[k][1]);
        }
    };
    // V: piece j is the half fq & 1 (columns lr = 8 (fq & 1) .. + 7) of column tile ct = kPieces (fq >> 1) + j; column
    // lr's kPieces tiles are adjacent in the staged row
    auto put_v = [&](const uint4 (&r)[kPieces], uint32_t *Vs) __attribute__((always_inline)) {
        uint32_t *dst = Vs + frow * kStrideV + 8 * (fq & 1) * kVD + (fq >> 1) * (kPieces / 2);
        uint32_t w[kPieces][4];
#pragma unroll
        for (int j = 0; j < kPieces; ++j) w[j][0] = r[j].x, w[j][1] = r[j].y, w[j][2] = r[j].z, w[j][3] = r[j].w;
#pragma unroll
        for (int d = 0; d < 4; ++d) {  // columns lr = 2 d (low halves) and 2 d + 1 (high halves) of the half
            if constexpr (kPieces == 4) {
                *reinterpret_cast<uint2 *>(dst + 2 * d * kVD) = make_uint2(pair_lo(w[0][d], w[1][d]), pair_lo(w[2][d], w[3][d]));
                *reinterpret_cast<uint2 *>(dst + (2 * d + 1) * kVD) =
                    make_uint2(pair_hi(w[0][d], w[1][d]), pair_hi(w[2][d], w[3][d]));
            } else {
                dst[2 * d * kVD] = pair_lo(w[0][d], w[1][d]);
                dst[(2 * d + 1) * kVD] = pair_hi(w[0][d], w[1][d]);
            }
        }
    };
    const int kp0 = kPieces * fq, vp0 = 2 * kPieces * (fq >> 1) + (fq & 1);
    uint4 kf[kPieces], vf[kPieces];
    fetch(kf, Kb, ldk, 0, kp0, 1, vec_k);
    fetch(vf, Vb, ldv, 0, vp0, 2, vec_v);

    // the wave's B fragments for the whole kernel, straight from global memory: qb[s] = Q[row lr][4 s + lk], zero past
    // d_k and in the lanes past the tile's rows
    float qb[T::kSteps];
    {
        const bool mine = wave * 16 + lr < rows;
        const float *qrow = Qb + (int64_t)myrow * ldq;
#pragma unroll
        for (int s = 0; s < T::kSteps; ++s) {
            const int c = 4 * s + lk;
            const float x = qrow[min(c, dk - 1)];
            qb[s] = mine && c < dk ? x : 0.f;
        }
    }

    const int nsteps = dk4;            // k-steps that hold a column below d_k; run in groups of 8
    const int nct = (dk + 15) >> 4;    // O's column tiles below d_k
    float m = -INFINITY, l = 0.f;      // of query lr, the same in the four lanes lr + 16 lk
    v4f acc[T::kColTiles];
#pragma unroll
    for (int ct = 0; ct < T::kColTiles; ++ct) acc[ct] = v4f{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nck; ++c) {
        const int c0 = c * kC;
        uint32_t *Ks = lds + (c & 1) * T::kBuf, *Vs = Ks + kC * kStrideK;
        if (vec_k) put_k(kf, Ks);
        else put_elements(Kb, ldk, c0, Ks, kStrideK, false);
        if (vec_v) put_v(vf, Vs);
        else put_elements(Vb, ldv, c0, Vs, kStrideV, true);
        // the ONE barrier of a chunk.  It also orders these writes behind every wave's reads of chunk c - 2 (the same
        // buffer): a wave is past chunk c - 2's reads when it arrives at chunk c - 1's barrier, which this wave has left
        __syncthreads();
        if (c + 1 < nck) {
            fetch(kf, Kb, ldk, c0 + kC, kp0, 1, vec_k);
            fetch(vf, Vb, ldv, c0 + kC, vp0, 2, vec_v);
        }
        // a chunk at or past the wave's largest limit changes nothing for its rows (alpha = 1, p = 0): passed over.
        // Chunk 0 is never passed over by a wave with rows (wmax >= 1): it holds key 0, which every row sees, so m is
        // finite from the first chunk on and exp2(m - m') never meets -inf - (-inf).
        if (c0 < wmax) {
            v4f st[4];
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) st[kb] = v4f{0.f, 0.f, 0.f, 0.f};
            const uint32_t *krow = Ks + lr * kStrideK + 4 * lk;
#pragma unroll
            for (int g = 0; g < T::kSteps / 8; ++g) {
                if (g * 8 < nsteps) {  // wave-uniform; Q and K are zero past d_k inside a group
                    uint32_t ka[4][4];  // eight steps' fragments of the four key blocks: 16 registers
#pragma unroll
                    for (int kb = 0; kb < 4; ++kb) {
                        const uint4 x = *reinterpret_cast<const uint4 *>(krow + kb * 16 * kStrideK + 16 * g);
                        ka[kb][0] = x.x, ka[kb][1] = x.y, ka[kb][2] = x.z, ka[kb][3] = x.w;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
#pragma unroll
                        for (int kb = 0; kb < 4; ++kb)
                            st[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf16_at(ka[kb], u), qb[8 * g + u], st[kb], 0, 0, 0);
                }
            }
            // mask, chunk maximum of query lr: 16 values here, then the lanes lr + 16 lk
            float cmax = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float x = c0 + kb * 16 + 4 * lk + i < mylim ? st[kb][i] * scale2 : -INFINITY;
                    st[kb][i] = x;
                    cmax = fmaxf(cmax, x);
                }
            cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
            cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
            const float mn = fmaxf(m, cmax);  // finite: see above
            const float alpha = __builtin_amdgcn_exp2f(m - mn);  // 0 in chunk 0, 1 where the row sees nothing here
            float ps = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = __builtin_amdgcn_exp2f(st[kb][i] - mn);  // +0 at a masked key
                    st[kb][i] = p;
                    ps += p;
                }
            ps += __shfl_xor(ps, 16);
            ps += __shfl_xor(ps, 32);
            l = l * alpha + ps;
            m = mn;
#pragma unroll
            for (int ct = 0; ct < T::kColTiles; ++ct) acc[ct] *= alpha;
            // O^T += V^T P^T: P straight from the score accumulators, one read per key for all the column tiles.  Over
            // 3/4 of the column tiles or all of them (d_k <= 48 or 96: V is zero past d_k), chosen per wave, so the MFMA
            // stream has no condition inside
            const uint32_t *vcol = Vs + 4 * lk * kStrideV + lr * kVD;
            auto pv = [&](auto kTiles) __attribute__((always_inline)) {
                constexpr int kN = decltype(kTiles)::value;
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
                    uint32_t va[4][kVD];  // a key block's four steps: <= 16 registers
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint32_t *p = vcol + (kb * 16 + i) * kStrideV;
                        if constexpr (kVD == 4) {
                            const uint4 x = *reinterpret_cast<const uint4 *>(p);
                            va[i][0] = x.x, va[i][1] = x.y, va[i][2] = x.z, va[i][3] = x.w;
                        } else {
                            const uint2 x = *reinterpret_cast<const uint2 *>(p);
                            va[i][0] = x.x, va[i][1] = x.y;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int ct = 0; ct < kN; ++ct)
                            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf16_at(va[i], ct), st[kb][i], acc[ct], 0, 0, 0);
                }
            };
            if (nct <= T::kColTiles * 3 / 4) pv(std::integral_constant<int, T::kColTiles * 3 / 4>());
            else pv(std::integral_constant<int, T::kColTiles>());
        }
    }

    // O[row lr][16 ct + 4 lk + i] = acc / l
    if (wave * 16 + lr < rows) {
        float *orow = O + (int64_t)myrow * ldo + (int64_t)h * dk + 4 * lk;
#pragma unroll
        for (int ct = 0; ct < T::kColTiles; ++ct) {
            const int col = ct * 16 + 4 * lk;
            float *p = orow + ct * 16;
            const float o0 = __fdiv_rn(acc[ct][0], l), o1 = __fdiv_rn(acc[ct][1], l), o2 = __fdiv_rn(acc[ct][2], l),
                        o3 = __fdiv_rn(acc[ct][3], l);
            if (col + 3 < dk && ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) {
                *reinterpret_cast<float4 *>(p) = make_float4(o0, o1, o2, o3);
            } else {
                if (col < dk) p[0] = o0;
                if (col + 1 < dk) p[1] = o1;
                if (col + 2 < dk) p[2] = o2;
                if (col + 3 < dk) p[3] = o3;
            }
        }
    }
}

}  // namespace

const char *attention_tiled_kv16_plan_name(int dk) {
    return dk <= 64 ? "attention_tiled_kv16_kernel" : "attention_tiled_kv16_wide_kernel";
}

// launch_attention_tiled_many's checks and work map (the tile height is the fp32 kernel's) for the bf16 kernel: tab comes
// checked and clamped from launch_attention_tiled_kv16 (attention_launch.hip), and what sizes the grid and bounds the
// kernel's reads is tested again
hipError_t launch_attention_tiled_kv16_many(const float *Q, int64_t ldq, const bf16_t *K, int64_t ldk, const bf16_t *V,
                                            int64_t ldv, float *O, int64_t ldo, int n_seqs, const FusedSeqTable &tab,
                                            bool causal, int n_heads, int n_kv_heads, int dk, float scale,
                                            hipStream_t stream) {
    if (n_seqs < 1 || n_seqs > kVarlenMaxSeqs || n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads ||
        !attention_tiled_ok(1, dk))
        return hipErrorInvalidValue;
    Tiled16Seqs many;
    many.n_seqs = n_seqs;
    many.tab = tab;
    int64_t items = 0;
    for (int b = 0; b < n_seqs; ++b) {
        if (tab.seq_q[b] < 0 || !attention_tiled_ok(tab.seq_kv[b], dk) || tab.q_row0[b] < 0 || tab.kv_row0[b] < 0 ||
            tab.q_pos0[b] < 0 || tab.q_pos0[b] > tab.seq_kv[b])
            return hipErrorInvalidValue;
        many.tab.item0[b] = (int)items;
        items += ((int64_t)tab.seq_q[b] + kT16TQ - 1) / kT16TQ * n_heads;
        if (items > INT32_MAX) return hipErrorInvalidValue;
    }
    for (int b = n_seqs; b <= kVarlenMaxSeqs; ++b) many.tab.item0[b] = (int)items;
    if (items == 0) return hipSuccess;
    const dim3 grid((unsigned)items);
    const int group = n_heads / n_kv_heads;
    const float scale2 = scale * 1.44269504088896340736f;  // the fp32 launch's expression: the same bits
    auto go = [&](auto kernel) {
        kernel<<<grid, kT16Threads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, O, ldo, dk, group, scale2, many);
        return hipGetLastError();
    };
    if (dk <= 64) return causal ? go(attention_tiled_kv16_kernel<true, 64>) : go(attention_tiled_kv16_kernel<false, 64>);
    return causal ? go(attention_tiled_kv16_kernel<true, 128>) : go(attention_tiled_kv16_kernel<false, 128>);
}

}  // namespace qgemm
