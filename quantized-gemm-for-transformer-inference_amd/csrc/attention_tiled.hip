// attention_tiled.hip -- prefill attention tiled over the keys with a running maximum and sum: no score
// tensor, no workspace, ONE launch for a packed batch of sequences of up to kSplitMaxSeq keys each, grouped heads
// included.  A numerical contract of its own (include/qgemm.h), not the fused or three-launch bits.
// Work split: a workgroup of 4 waves owns (sequence, query head, tile of 64 query rows), wave w the tile's rows
// 16 w .. 16 w + 15, and walks the sequence's keys in chunks of 64 staged in LDS -- K and V side by side, rows of
// kW + 4 floats.  The running maximum m, the running sum l and the output accumulator never leave registers.
// Data path: BOTH products are computed transposed on v_mfma_f32_16x16x4_f32, operands fp32.
//   S^T = K_chunk Q^T : A = K rows from LDS (lane (lr, lk): key 16 kb + lr, column 4 s + lk), B = the wave's Q rows, held
//         in registers for the whole kernel (kW / 4 values per lane).  In the 16 x 16 accumulator lane (lr, lk) then
//         holds the scores of QUERY lr against keys 16 kb + 4 lk + i, i = 0 .. 3: 16 scores of one query per lane and
//         chunk, the other 48 in lanes lr + 16, lr + 32, lr + 48.
//   O^T = V^T P^T     : MFMA step i of key block kb reduces over the keys {16 kb + 4 lk' + i}; its B fragment is
//         P[query lr][16 kb + 4 lk + i] -- the lane's OWN accumulator register i of block kb, after the exp -- and its A
//         fragment V[16 kb + 4 lk + i][16 ct + lr] from LDS.  P goes from accumulator registers to the next MFMA's
//         operand with no LDS round trip and no cross-lane move (the order of a sum is free under this contract).  The
//         result lane (lr, lk) holds O[query lr][16 ct + 4 lk + i]: every value a lane keeps -- scores, m, l, acc --
//         belongs to query lr, so the rescale by alpha is lane-local and the row maximum and sum are a per-lane chain
//         plus two cross-lane steps (xor 16, xor 32).
// LDS bank patterns at stride kW + 4 (= 4 mod 32): the K fragment read (16 keys x 4 adjacent columns) touches banks
// 4 lr + lk, the V fragment read (keys 4 apart x 16 adjacent columns) banks 16 lk + lr (4 (kW + 4) = 16 mod 64): both
// distinct over the 64 lanes.
// K / V staging: coalesced float4 global loads of chunk c + 1 into registers under chunk c's MFMAs (4 + 4 float4 per
// thread at kW 64, 8 + 8 at kW 128), zero past d_k and at or past the tile's largest limit, by elements where a piece
// is misaligned or crosses d_k (`fetch` of attention_gqa.hip).
// exp: v_exp_f32 on scores prescaled by scale * log2(e) (1 ulp; include/qgemm.h states the choice).
#include "qgemm_internal.h"

#include <type_traits>

namespace qgemm {

namespace {

constexpr int kTiledTQ = 64;        // query rows per workgroup: 16 per wave
constexpr int kTiledC = 64;         // keys per chunk
constexpr int kTiledThreads = 256;  // 4 waves

template <int kW>
struct TiledTile {
    static_assert(kW == 64 || kW == 128, "the row widths of the other attention kernels");
    static constexpr int kStride = kW + 4;  // K and V chunk rows [key][d_k]
    static constexpr int kF4 = kW / 4;      // float4 pieces of a staged row
    static constexpr int kPer = kTiledC * kF4 / kTiledThreads;  // pieces per thread and chunk: 4 or 8
    static constexpr int kSteps = kW / 4;   // k-steps of a full-width row in S^T
    static constexpr int kColTiles = kW / 16;  // 16-column tiles of O
    static_assert(kPer * kTiledThreads == kTiledC * kF4 && kTiledTQ == kTiledC, "Q is staged through the K chunk");
    static_assert(2 * kTiledC * kStride * 4 * 2 <= 160 * 1024, "two workgroups per CU");
};

typedef float v4f __attribute__((ext_vector_type(4)));

// the sequences of a launch, by value in the kernel arguments (GqaSeqs of attention_gqa.hip)
struct TiledSeqs {
    int n_seqs;
    FusedSeqTable tab;
};
static_assert(sizeof(TiledSeqs) + 88 < 4096, "the table travels in the kernel arguments");

template <bool kCausal, int kW>
__global__ __launch_bounds__(kTiledThreads) __attribute__((amdgpu_waves_per_eu(2))) void attention_tiled_kernel(
    const float *__restrict__ Q, int64_t ldq, const float *__restrict__ K, int64_t ldk, const float *__restrict__ V,
    int64_t ldv, float *__restrict__ O, int64_t ldo, int dk, int group, float scale2, TiledSeqs seqs) {
    using T = TiledTile<kW>;
    constexpr int kStride = T::kStride, kF4 = T::kF4, kPer = T::kPer, kC = kTiledC, kTQ = kTiledTQ;
    __shared__ __attribute__((aligned(16))) float Ks[kC * kStride];
    __shared__ __attribute__((aligned(16))) float Vs[kC * kStride];
    // XCD-aware (attention_gqa.hip): each XCD gets a contiguous range of work items, so the G query heads of a KV head
    // stay in one L2
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
    // head by head; inside a head the LAST tile first: under the mask it carries the most chunks
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
    const float *Qb = Q + (int64_t)h * dk, *Kb = K + (int64_t)hkv * dk, *Vb = V + (int64_t)hkv * dk;
    const int lr = lane & 15, lk = lane >> 4;
    const int rows = seq_q - q0 < kTQ ? seq_q - q0 : kTQ;  // >= 1: the work map holds no empty tile
    const int dk4 = (dk + 3) >> 2;
    // row i of the sequence sees keys 0 .. limit(i) - 1, 1 <= limit(i) <= seq (q_pos0 <= seq: the launcher clamps it)
    auto limit = [&](int i) __attribute__((always_inline)) {
        return kCausal ? (int)min((int64_t)seq, (int64_t)q_pos0 + i + 1) : seq;
    };
    const int lmax = limit(q0 + rows - 1);       // the tile's largest limit: nothing at or past it is read
    const int nck = (lmax + kC - 1) / kC;        // >= 1
    // the wave's largest limit; a wave without rows computes nothing (it still stages and meets the barriers)
    const int wmax = wave * 16 < rows ? limit(q0 + min(wave * 16 + 15, rows - 1)) : 0;
    const int myrow = q0 + min(wave * 16 + lr, rows - 1);  // a lane past the tile's rows shadows the last row
    const int mylim = limit(myrow);

    // piece i of a thread: row frow + i * kRowsPer of the chunk, float4 column fc4 -- the column and what it means for
    // d_k are the same for all of a thread's pieces
    constexpr int kRowsPer = kTiledThreads / kF4;
    const int frow = t / kF4, fc4 = t % kF4;
    const bool fcol = fc4 < dk4, fwhole = 4 * fc4 + 3 < dk;
    auto fetch = [&](float4 (&r)[kPer], const float *src, int64_t ld, int c0, int nrows) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int j = c0 + frow + i * kRowsPer;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < nrows && fcol) {
                const float *p = src + j * ld + 4 * fc4;
                if (fwhole && ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) {
                    v = *reinterpret_cast<const float4 *>(p);
                } else {
                    v.x = p[0];
                    v.y = 4 * fc4 + 1 < dk ? p[1] : 0.f;
                    v.z = 4 * fc4 + 2 < dk ? p[2] : 0.f;
                    v.w = fwhole ? p[3] : 0.f;
                }
            }
            r[i] = v;
        }
    };
    auto put = [&](const float4 (&r)[kPer], float *dst) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i)
            *reinterpret_cast<float4 *>(dst + (frow + i * kRowsPer) * kStride + 4 * fc4) = r[i];
    };

    // the Q tile through the K buffer (coalesced row loads, zero past d_k and past the tile's rows), then the wave's B
    // fragments for the whole kernel: qb[s] = Q[row lr][4 s + lk]
    float4 kf[kPer], vf[kPer];
    fetch(kf, Qb + (int64_t)q0 * ldq, ldq, 0, rows);
    put(kf, Ks);
    fetch(kf, Kb, ldk, 0, lmax);
    fetch(vf, Vb, ldv, 0, lmax);
    __syncthreads();
    float qb[T::kSteps];
#pragma unroll
    for (int s = 0; s < T::kSteps; ++s) qb[s] = Ks[(wave * 16 + lr) * kStride + 4 * s + lk];
    __syncthreads();

    const int nsteps = dk4;            // k-steps that hold a column below d_k; run in groups of 8
    const int nct = (dk + 15) >> 4;    // O's column tiles below d_k
    float m = -INFINITY, l = 0.f;      // of query lr, the same in the four lanes lr + 16 lk
    v4f acc[T::kColTiles];
#pragma unroll
    for (int ct = 0; ct < T::kColTiles; ++ct) acc[ct] = v4f{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nck; ++c) {
        const int c0 = c * kC;
        put(kf, Ks);
        put(vf, Vs);
        __syncthreads();
        if (c + 1 < nck) {
            fetch(kf, Kb, ldk, c0 + kC, lmax);
            fetch(vf, Vb, ldv, c0 + kC, lmax);
        }
        // a chunk at or past the wave's largest limit changes nothing for its rows (alpha = 1, p = 0): passed over.
        // Chunk 0 is never passed over by a wave with rows (wmax >= 1): it holds key 0, which every row sees, so m is
        // finite from the first chunk on and exp2(m - m') never meets -inf - (-inf).
        if (c0 < wmax) {
            v4f st[4];
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) st[kb] = v4f{0.f, 0.f, 0.f, 0.f};
            const float *krow = Ks + lr * kStride + lk;
#pragma unroll
            for (int g = 0; g < T::kSteps / 8; ++g) {
                if (g * 8 < nsteps) {  // wave-uniform; Q and K are zero past d_k inside a group
#pragma unroll
                    for (int s0 = g * 8; s0 < g * 8 + 8; s0 += 4) {  // four steps' fragments at a time: 16 registers
                        float ka[4][4];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int kb = 0; kb < 4; ++kb) ka[kb][u] = krow[kb * 16 * kStride + 4 * (s0 + u)];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int kb = 0; kb < 4; ++kb)
                                st[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[kb][u], qb[s0 + u], st[kb], 0, 0, 0);
                    }
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
            // O^T += V^T P^T: P straight from the score accumulators.  Over 3/4 of the column tiles or all of them (d_k <=
            // 48 or 96: V is zero past d_k), chosen per wave, so the MFMA stream has no condition inside
            const float *vcol = Vs + 4 * lk * kStride + lr;
            auto pv = [&](auto kTiles) __attribute__((always_inline)) {
                constexpr int kN = decltype(kTiles)::value;
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
                    for (int i0 = 0; i0 < 4; i0 += 2) {  // two steps' fragments at a time: <= 16 registers
                        float va[2][kN];
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int ct = 0; ct < kN; ++ct) va[i][ct] = vcol[(kb * 16 + i0 + i) * kStride + ct * 16];
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int ct = 0; ct < kN; ++ct)
                                acc[ct] =
                                    __builtin_amdgcn_mfma_f32_16x16x4f32(va[i][ct], st[kb][i0 + i], acc[ct], 0, 0, 0);
                    }
                }
            };
            if (nct <= T::kColTiles * 3 / 4) pv(std::integral_constant<int, T::kColTiles * 3 / 4>());
            else pv(std::integral_constant<int, T::kColTiles>());
        }
        __syncthreads();  // every wave is done with the chunk before the next one is written
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

bool attention_tiled_ok(int seq_kv, int dk) {
    return seq_kv >= 1 && seq_kv <= kSplitMaxSeq && dk >= 1 && (dk <= 64 || dk == 96 || dk == 128);
}

const char *attention_tiled_plan_name(int dk) {
    return dk <= 64 ? "attention_tiled_kernel" : "attention_tiled_wide_kernel";
}

// tab.q_row0, kv_row0, seq_q, seq_kv and q_pos0 (clamped to seq_kv) come checked from launch_attention_tiled
// (attention_launch.hip); the work map item0 is built HERE, where the tile height is known, and what sizes the grid and
// bounds the kernel's reads is tested again
hipError_t launch_attention_tiled_many(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V,
                                       int64_t ldv, float *O, int64_t ldo, int n_seqs, const FusedSeqTable &tab,
                                       bool causal, int n_heads, int n_kv_heads, int dk, float scale,
                                       hipStream_t stream) {
    if (n_seqs < 1 || n_seqs > kVarlenMaxSeqs || n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads ||
        !attention_tiled_ok(1, dk))
        return hipErrorInvalidValue;
    TiledSeqs many;
    many.n_seqs = n_seqs;
    many.tab = tab;
    int64_t items = 0;
    for (int b = 0; b < n_seqs; ++b) {
        if (tab.seq_q[b] < 0 || !attention_tiled_ok(tab.seq_kv[b], dk) || tab.q_row0[b] < 0 || tab.kv_row0[b] < 0 ||
            tab.q_pos0[b] < 0 || tab.q_pos0[b] > tab.seq_kv[b])
            return hipErrorInvalidValue;
        many.tab.item0[b] = (int)items;
        items += ((int64_t)tab.seq_q[b] + kTiledTQ - 1) / kTiledTQ * n_heads;
        if (items > INT32_MAX) return hipErrorInvalidValue;
    }
    for (int b = n_seqs; b <= kVarlenMaxSeqs; ++b) many.tab.item0[b] = (int)items;
    if (items == 0) return hipSuccess;
    const dim3 grid((unsigned)items);
    const int group = n_heads / n_kv_heads;
    const float scale2 = scale * 1.44269504088896340736f;  // the scores in units of log2: exp(x) = exp2(x log2 e)
    auto go = [&](auto kernel) {
        kernel<<<grid, kTiledThreads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, O, ldo, dk, group, scale2, many);
        return hipGetLastError();
    };
    if (dk <= 64) return causal ? go(attention_tiled_kernel<true, 64>) : go(attention_tiled_kernel<false, 64>);
    return causal ? go(attention_tiled_kernel<true, 128>) : go(attention_tiled_kernel<false, 128>);
}

}  // namespace qgemm
