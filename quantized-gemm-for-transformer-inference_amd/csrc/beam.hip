// beam.hip -- beam search's device side: the log-sum-exp of every fp32 row (the normaliser that makes
// scores comparable across rows), the beam step (every live beam's best `beams` columns scored onto the beam, finished
// beams held, the best `beams` of a group chosen with a tie rule) and the KV-cache gather by a permutation that exists
// only on the device.  The contracts are at qgemm_logsumexp_rows / qgemm_beam_step / qgemm_decoder_gather_slots
// (include/qgemm.h); tests/beam_oracle.py restates them in numpy and predicts every bit.
//
// Log-sum-exp.  Two passes over the row (a step's logits are a few MiB and stay cache-resident): the greatest candidate
// m in the argmax's order (the greatest composite, topk_select.h), then e_i = fl32(exp((double)fl(S[i] - m))) for the
// candidates and +0 elsewhere, summed by ONE fixed tree: e padded with +0 to P, the least power of two >= max(w, 1024),
// the root of the perfect binary tree over adjacent pairs.  An aligned block of 1024 columns is a subtree, and a
// workgroup of 256 threads sums one as: a thread's four adjacent columns (two levels), an xor-butterfly over the wave
// (six levels; fl(a + b) == fl(b + a), so every lane holds the tree's bits), the four waves through LDS (two levels).
// The tree's quads follow the COLUMN index, the 16-byte loads the ADDRESS: a block is staged through LDS, written as it
// was loaded (scalar head, float4s, scalar tail) and read back as thread t's columns 4 t .. 4 t + 3.  The block sums are
// the leaves of the upper tree: 1024 of them are again one workgroup tree (+0 past the last block: fl(x + +0) == x for
// every x >= +0 and for NaN, so all-padding subtrees are identities), and the at most 16 roots of those are summed by
// one thread.  Nothing in the tree depends on who computes a block, so the result does not depend on the split.
// Launches.  parts == 1: one workgroup per row does everything.  parts > 1 (few, wide rows): every (row, part) gets a
// workgroup over `bpp` whole blocks in each of two launches -- the part's greatest composite into the workspace, then,
// with the row's m known, its block sums into the workspace -- and a third launch, one workgroup per row, runs the upper
// tree.  Workgroups meet only through the workspace between launches.
//
// Beam step.  logsumexp_rows gives (m_r, logz_r); the per-row lists are sample.hip's selection with k = beams (split
// rows: select_part per part, then the select over a row's parts * beams composites); beam_row_kernel sorts a row's at
// most 8 kept composites by counting and writes the candidates (c, token) of the row into the workspace, place
// b * beams + j of its group; beam_group_kernel, one wave per group, ranks the group's at most 64 candidates by
// counting -- greater c first, the lower place among == values -- and stores the first `beams`.
//
// Everything here is a C-ABI entry point's body: argument checks first, then launches only.
#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/qgemm.h"
#include "qgemm_internal.h"
#include "topk_select.h"

namespace qgemm {

namespace {

constexpr int kLseBlock = 1024;  // the columns of one tree block: a float4 per thread of a workgroup
constexpr int kLseMaxW = 1 << 24;
constexpr int kLseMaxSuper = kLseMaxW / kLseBlock / kLseBlock;  // roots of 1024-block trees per row: 16
// the split rule: as argmax_plan (head.hip), in whole blocks
constexpr int kLseManyRows = 256;
constexpr int kLseMinBlocks = 4;
constexpr int kLseTargetGroups = 512;
constexpr int kLseMaxParts = 64;
constexpr int kBeamMax = 8;
constexpr int kBeamMaxRows = 64;
static_assert(kSampleThreads * 4 == kLseBlock, "a thread's float4 is two levels of a block's tree");

// ---- the tree ---------------------------------------------------------------------------------------------------
// The root of the perfect tree over the workgroup's 1024 values, thread t holding values 4 t .. 4 t + 3.  wsum: 4
// floats (LDS).  Every thread returns the root.
__device__ __forceinline__ float tree1024(float4 x, float *wsum) {
    float s = __fadd_rn(__fadd_rn(x.x, x.y), __fadd_rn(x.z, x.w));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s = __fadd_rn(s, __shfl_xor(s, off, 64));
    __syncthreads();  // wsum's last readers
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    return __fadd_rn(__fadd_rn(wsum[0], wsum[1]), __fadd_rn(wsum[2], wsum[3]));
}

// the tree over values 0 .. n - 1 (n <= 1024) of v, +0 past them
__device__ __forceinline__ float tree_of(const float *v, int n, float *wsum) {
    const int i = 4 * threadIdx.x;
    float4 x;
    x.x = i < n ? v[i] : 0.0f;
    x.y = i + 1 < n ? v[i + 1] : 0.0f;
    x.z = i + 2 < n ? v[i + 2] : 0.0f;
    x.w = i + 3 < n ? v[i + 3] : 0.0f;
    return tree1024(x, wsum);
}

// the top of the tree over top[0 .. n), n <= 16, by one thread (top is overwritten)
__device__ __forceinline__ float top_tree(float *top, int n) {
    int p = 1;
    while (p < n) p <<= 1;
    for (int i = n; i < p; ++i) top[i] = 0.0f;
    for (; p > 1; p >>= 1)
        for (int i = 0; i < p / 2; ++i) top[i] = __fadd_rn(top[2 * i], top[2 * i + 1]);
    return top[0];
}

// ---- a block of the row -----------------------------------------------------------------------------------------
// columns b0 .. min(w, b0 + 1024) - 1 of the row at p as the loads bring them: this thread's float4 between a scalar
// head (up to the first 16-byte aligned element) and a scalar tail; nothing outside the row's w floats is read
struct BlockGeom {
    int n, head, nvec, t0;
    __device__ __forceinline__ BlockGeom(const float *p, int b0, int w) {
        n = min(w - b0, kLseBlock);
        head = min(n, (int)((4 - ((reinterpret_cast<uintptr_t>(p + b0) >> 2) & 3)) & 3));
        nvec = (n - head) >> 2;
        t0 = head + 4 * nvec;
    }
};
struct BlockRegs {
    float4 q;
    float h, tl;
};
__device__ __forceinline__ BlockRegs load_block(const float *p, int b0, int w) {
    const int t = threadIdx.x;
    const BlockGeom g(p, b0, w);
    BlockRegs r;
    r.q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    r.h = r.tl = 0.0f;
    if (t < g.head) r.h = p[b0 + t];
    if (t < g.nvec) r.q = reinterpret_cast<const float4 *>(p + b0 + g.head)[t];
    if (t < g.n - g.t0) r.tl = p[b0 + g.t0 + t];
    return r;
}
// into stage (1024 floats, LDS) at their columns, -inf (no candidate) past the row's end
__device__ __forceinline__ void stage_block(const BlockRegs &r, const float *p, int b0, int w, float *stage) {
    const int t = threadIdx.x;
    const BlockGeom g(p, b0, w);
    __syncthreads();  // stage's last readers
    if (t < g.head) stage[t] = r.h;
    if (t < g.nvec) {
        float *o = stage + g.head + 4 * t;
        o[0] = r.q.x;
        o[1] = r.q.y;
        o[2] = r.q.z;
        o[3] = r.q.w;
    }
    if (t < g.n - g.t0) stage[g.t0 + t] = r.tl;
    for (int i = g.n + t; i < kLseBlock; i += kSampleThreads) stage[i] = -INFINITY;
    __syncthreads();
}
__device__ __forceinline__ float cand_exp(float x, float m) { return x > -INFINITY ? softmax_exp(x, 1.0f, m) : 0.0f; }
// the block's sum: thread t takes columns 4 t .. 4 t + 3 of the staged block
__device__ __forceinline__ float block_sum(const float *stage, float m, float *wsum) {
    const float4 x = reinterpret_cast<const float4 *>(stage)[threadIdx.x];
    return tree1024(make_float4(cand_exp(x.x, m), cand_exp(x.y, m), cand_exp(x.z, m), cand_exp(x.w, m)), wsum);
}

__device__ __forceinline__ uint64_t wave_best(uint64_t c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)c, off, 64);
        c = o > c ? o : c;
    }
    return c;
}
// the greatest composite of columns [c0, c1) of the row, in every thread.  wbest: 4 words (LDS)
__device__ __forceinline__ uint64_t range_best(const float *p, int c0, int c1, int w, uint64_t *wbest) {
    uint64_t best = 0;
    const RowSource src = {p, c0, c1, w};
    src.each([&](uint64_t c) { best = c > best ? c : best; });
    best = wave_best(best);
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSampleThreads / 64; ++j) best = wbest[j] > best ? wbest[j] : best;
    return best;
}
// the greatest of a row's `parts` (<= 64) composites in the workspace, in every thread
__device__ __forceinline__ uint64_t parts_best(const uint64_t *c, int parts) {
    const int lane = threadIdx.x & 63;
    return wave_best(lane < parts ? c[lane] : 0);
}
// m of the contract: the own bits of the column the greatest composite stands for, -inf without a candidate
__device__ __forceinline__ float best_value(const float *p, uint64_t best, int w) {
    return best ? p[composite_column(best, w)] : -INFINITY;
}
__device__ __forceinline__ void lse_store(float m, float sum, float *mx, float *logz, int64_t row) {
    mx[row] = m;
    logz[row] = (float)log((double)sum);
}

// ---- log-sum-exp launches -----------------------------------------------------------------------------------------
// parts == 1: one workgroup per row.  sums holds the block sums of the super-block (1024 blocks) under way.
__global__ __launch_bounds__(kSampleThreads) void lse_row_kernel(const float *__restrict__ S, int64_t stride, int w,
                                                                 float *__restrict__ mx, float *__restrict__ logz) {
    __shared__ __align__(16) float stage[kLseBlock];
    __shared__ float sums[kLseBlock];
    __shared__ float wsum[4], top[kLseMaxSuper];
    __shared__ uint64_t wbest[4];
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x;
    const float *p = S + row * stride;
    const float m = best_value(p, range_best(p, 0, w, w, wbest), w);
    const int nblk = (w + kLseBlock - 1) / kLseBlock;
    BlockRegs r = load_block(p, 0, w);
    for (int k = 0; k < nblk; ++k) {
        stage_block(r, p, k * kLseBlock, w, stage);
        if (k + 1 < nblk) r = load_block(p, (k + 1) * kLseBlock, w);  // in flight under this block's exps
        const float s = block_sum(stage, m, wsum);
        if (t == 0) sums[k & (kLseBlock - 1)] = s;
        if ((k & (kLseBlock - 1)) == kLseBlock - 1 || k == nblk - 1) {  // a super-block is complete
            __syncthreads();
            const float root = tree_of(sums, (k & (kLseBlock - 1)) + 1, wsum);
            if (t == 0) top[k / kLseBlock] = root;
        }
    }
    if (t == 0) lse_store(m, top_tree(top, (nblk + kLseBlock - 1) / kLseBlock), mx, logz, row);
}

// split rows, launch 1: the greatest composite of blocks [part * bpp, (part + 1) * bpp) of the row
__global__ __launch_bounds__(kSampleThreads) void lse_max_kernel(const float *__restrict__ S, int64_t stride, int w,
                                                                 int bpp, int parts, uint64_t *__restrict__ wsmax) {
    __shared__ uint64_t wbest[4];
    const int64_t row = blockIdx.x / parts;
    const int part = blockIdx.x % parts;
    const int c0 = part * bpp * kLseBlock;
    const uint64_t best = range_best(S + row * stride, c0, min(w, c0 + bpp * kLseBlock), w, wbest);
    if (threadIdx.x == 0) wsmax[blockIdx.x] = best;
}

// split rows, launch 2: the sums of those blocks, with the row's m from launch 1
__global__ __launch_bounds__(kSampleThreads) void lse_sum_kernel(const float *__restrict__ S, int64_t stride, int w,
                                                                 int bpp, int parts, int nblk,
                                                                 const uint64_t *__restrict__ wsmax,
                                                                 float *__restrict__ wssum) {
    __shared__ __align__(16) float stage[kLseBlock];
    __shared__ float wsum[4];
    const int64_t row = blockIdx.x / parts;
    const int part = blockIdx.x % parts;
    const float *p = S + row * stride;
    const float m = best_value(p, parts_best(wsmax + row * parts, parts), w);
    const int k0 = part * bpp, k1 = min(nblk, k0 + bpp);
    BlockRegs r = load_block(p, k0 * kLseBlock, w);
    for (int k = k0; k < k1; ++k) {
        stage_block(r, p, k * kLseBlock, w, stage);
        if (k + 1 < k1) r = load_block(p, (k + 1) * kLseBlock, w);
        const float s = block_sum(stage, m, wsum);
        if (threadIdx.x == 0) wssum[row * nblk + k] = s;
    }
}

// split rows, launch 3: the upper tree over the row's block sums
__global__ __launch_bounds__(kSampleThreads) void lse_finish_kernel(const float *__restrict__ S, int64_t stride, int w,
                                                                    int parts, int nblk,
                                                                    const uint64_t *__restrict__ wsmax,
                                                                    const float *__restrict__ wssum,
                                                                    float *__restrict__ mx, float *__restrict__ logz) {
    __shared__ float wsum[4], top[kLseMaxSuper];
    const int64_t row = blockIdx.x;
    const float *p = S + row * stride;
    const float m = best_value(p, parts_best(wsmax + row * parts, parts), w);
    const int nsuper = (nblk + kLseBlock - 1) / kLseBlock;
    for (int sb = 0; sb < nsuper; ++sb) {
        const float root = tree_of(wssum + row * nblk + sb * kLseBlock, min(kLseBlock, nblk - sb * kLseBlock), wsum);
        if (threadIdx.x == 0) top[sb] = root;
    }
    if (threadIdx.x == 0) lse_store(m, top_tree(top, nsuper), mx, logz, row);
}

// ---- beam step launches -------------------------------------------------------------------------------------------
// split rows: select_part with k = beams (sample.hip's launch 1)
__global__ __launch_bounds__(kSampleThreads) void beam_part_kernel(const float *__restrict__ S, int64_t stride, int w,
                                                                   int chunk, int parts, int k,
                                                                   uint64_t *__restrict__ lists) {
    __shared__ int hist[256];
    __shared__ int pick[4];
    __shared__ int count;
    const int64_t row = blockIdx.x / parts;
    const int part = blockIdx.x % parts;
    const int c0 = part * chunk;
    const RowSource src = {S + row * stride, c0, min(w, c0 + chunk), w};
    select_part(src, k, lists + (int64_t)blockIdx.x * k, hist, pick, &count);
}

// One workgroup per row: the candidates the beam contributes, (c, token) at places row * beams + j of cs / ct, c = -inf
// in the places it leaves empty.  A dead beam (score not > -inf) leaves all of them empty; a finished one (prev == eos)
// holds (score, eos) at j = 0; a live one takes its first k' columns in the argmax's order (over the row, or with kList
// over the n_list composites its parts left in the workspace), c_j = fl(score + fl(fl(v_j - m) - logz)).
template <bool kList>
__global__ __launch_bounds__(kSampleThreads) void beam_row_kernel(
    const float *__restrict__ S, int64_t stride, int w, int beams, int n_list, const uint64_t *__restrict__ lists,
    const float *__restrict__ mx, const float *__restrict__ logz, const float *__restrict__ scores_in,
    const int *__restrict__ prev, int eos, float *__restrict__ cs, int *__restrict__ ct) {
    __shared__ uint64_t kept[kBeamMax], sorted[kBeamMax];
    __shared__ int hist[256];
    __shared__ int pick[4];
    __shared__ int count;
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x;
    const float *p = S + row * stride;
    float *oc = cs + row * beams;
    int *ot = ct + row * beams;
    const float score = scores_in ? scores_in[row] : (row % beams == 0 ? 0.0f : -INFINITY);  // NULL: the start
    const bool live = score > -INFINITY;
    const bool finished = live && eos >= 0 && prev && prev[row] == eos;
    if (!live || finished) {  // the whole workgroup: the logits are not used
        if (t < beams) {
            const bool held = finished && t == 0;
            oc[t] = held ? score : -INFINITY;
            ot[t] = held ? eos : 0;
        }
        return;
    }
    if (t == 0) count = 0;
    Select sel;
    const auto collect = [&](uint64_t c) {
        if (c == 0 || c < sel.thr) return;
        const int at = atomicAdd(&count, 1);
        if (at < kBeamMax) kept[at] = c;
    };
    if constexpr (kList) {
        const ListSource src = {lists + row * n_list, n_list};
        sel = radix_select(src, beams, hist, pick);
        src.each(collect);
    } else {
        const RowSource src = {p, 0, w, w};
        sel = radix_select(src, beams, hist, pick);
        src.each(collect);
    }
    const int kk = sel.kept;  // k' of the contract
    __syncthreads();
    if (t < kk) {  // distinct composites: the number of greater ones is the place
        const uint64_t me = kept[t];
        int rank = 0;
        for (int i = 0; i < kk; ++i) rank += kept[i] > me ? 1 : 0;
        sorted[rank] = me;
    }
    __syncthreads();
    if (t < beams) {
        if (t < kk) {
            const int col = composite_column(sorted[t], w);
            const float lp = __fsub_rn(__fsub_rn(p[col], mx[row]), logz[row]);
            oc[t] = __fadd_rn(score, lp);
            ot[t] = col;
        } else {
            oc[t] = -INFINITY;
            ot[t] = 0;
        }
    }
}

// One wave per group: lane i < beams^2 holds candidate i = b * beams + j.  Those with c > -inf are ranked by counting
// the candidates ahead of them -- a greater c, or an == c (+0 equals -0) at a lower i -- and place `rank` < beams of the
// group gets (b, token, the bits of c).  Places past the number of candidates: parent = the place itself, token 0,
// score -inf.
__global__ __launch_bounds__(64) void beam_group_kernel(int beams, const float *__restrict__ cs,
                                                        const int *__restrict__ ct, int *__restrict__ parents,
                                                        int *__restrict__ tokens, float *__restrict__ scores_out) {
    const int g = blockIdx.x, lane = threadIdx.x, n = beams * beams;
    const float c = lane < n ? cs[g * n + lane] : -INFINITY;
    const bool valid = c > -INFINITY;
    int rank = 0;
    for (int l = 0; l < n; ++l) {
        const float o = __shfl(c, l, 64);  // a NaN or a -inf is ahead of nothing
        rank += (o > c || (o == c && l < lane)) ? 1 : 0;
    }
    const int n_valid = __popcll(__ballot(valid));
    if (valid && rank < beams) {
        const int at = g * beams + rank;
        parents[at] = lane / beams;
        tokens[at] = ct[g * n + lane];
        scores_out[at] = c;
    }
    if (lane >= n_valid && lane < beams) {
        const int at = g * beams + lane;
        parents[at] = lane;
        tokens[at] = 0;
        scores_out[at] = -INFINITY;
    }
}

// ---- the cache gather ---------------------------------------------------------------------------------------------
// per destination i = g * beams + q: its slot, the slot of the group's source place i and the rows to copy: a kernel
// argument passed by value (768 bytes), filled on the host at enqueue
struct GatherTable {
    int dst[kBeamMaxRows], src[kBeamMaxRows], n_rows[kBeamMaxRows];
};

// Workgroup (x, i) copies the [K | V] of cache rows x * rows_per_wg .. of destination i from the slot of its parent:
// the 2 d contiguous floats at offset d of every 3 d row, as V = float4 where d % 4 == 0 (then every row and third is
// 16-byte aligned), else float.  2^tpr_log2 threads share a row; a thread has four rows' loads in flight before its
// first store.  The workgroup reads its parent once; a parent outside [0, beams) gives rows of quiet NaNs and no load.
template <typename V>
__global__ __launch_bounds__(256) void gather_kv_kernel(float *cache, int64_t slab, int d, int beams, int rows_per_wg,
                                                        int tpr_log2, const int *__restrict__ parents,
                                                        GatherTable tab) {
    constexpr int kPer = sizeof(V) / sizeof(float);
    const int t = threadIdx.x, i = blockIdx.y;
    const int r0 = blockIdx.x * rows_per_wg, r1 = min(tab.n_rows[i], r0 + rows_per_wg);
    if (r0 >= r1) return;
    const int par = parents[i];
    const bool ok = par >= 0 && par < beams;
    const int per = 2 * d / kPer;      // a row's [K | V] ...
    const int64_t ld = 3 * d / kPer;   // ... and a cache row, in V
    V *__restrict__ dst = reinterpret_cast<V *>(cache + tab.dst[i] * slab + d);
    const int tpr = 1 << tpr_log2, rpi = 256 >> tpr_log2;
    const int tr = t >> tpr_log2, tc = t & (tpr - 1);
    if (!ok) {  // the whole workgroup
        const float qn = __uint_as_float(0x7fc00000u);
        V nan_v;
        if constexpr (kPer == 4)
            nan_v = make_float4(qn, qn, qn, qn);
        else
            nan_v = qn;
        for (int c = tc; c < per; c += tpr)
            for (int r = r0 + tr; r < r1; r += rpi) dst[r * ld + c] = nan_v;
        return;
    }
    // another slab than dst's: a destination is no source (checked on the host)
    const V *__restrict__ src = reinterpret_cast<const V *>(cache + tab.src[i / beams * beams + par] * slab + d);
    for (int c = tc; c < per; c += tpr)
        for (int r = r0 + tr; r < r1; r += 4 * rpi) {
            const int ra = r + rpi, rb = ra + rpi, rc = rb + rpi;  // past the end: the last row again, not stored
            const V q0 = src[r * ld + c], q1 = src[min(ra, r1 - 1) * ld + c], q2 = src[min(rb, r1 - 1) * ld + c],
                    q3 = src[min(rc, r1 - 1) * ld + c];
            dst[r * ld + c] = q0;
            if (ra < r1) dst[ra * ld + c] = q1;
            if (rb < r1) dst[rb * ld + c] = q2;
            if (rc < r1) dst[rc * ld + c] = q3;
        }
}

// ---- the row table of the copy-free search --------------------------------------------------------
// own[s][j]: the slot whose slab holds, at row j, the K and V of position j of the sequence in slot s; one byte each.
// 16 columns of a table row as they lie: one 16-byte access where the piece is whole and aligned, else byte by byte
// (the table may start at any byte and have any row stride).  Nothing outside the cnt bytes is touched.
__device__ __forceinline__ uint4 load_cols(const uint8_t *p, int cnt) {
    if (cnt == 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const uint4 *>(p);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < cnt) w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void store_cols(uint8_t *p, uint4 v, int cnt) {
    if (cnt == 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<uint4 *>(p) = v;
        return;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < cnt) p[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
}

// per place i = g * beams + q its table row, per group its column count: a kernel argument passed by value
struct ReindexTable {
    int slot[kBeamMaxRows], n_rows[kBeamMaxRows];
};

// The reorder, IN PLACE in the one table: thread (g, x) owns columns 16 x .. 16 x + 15 of group g's `beams` rows.  It
// first reads all `beams` entries of each of its columns and then writes them, new[q][j] = old[parent[q]][j].  The
// reorder is column-local -- new[.][j] of a group depends on old[.][j] of that group alone -- and no other thread
// touches this thread's columns of these rows (the groups' rows are distinct: checked on the host), so there is no
// second table, no barrier and no order to agree on.  A parent outside [0, beams) gives 255, the invalid entry.
__global__ __launch_bounds__(64) void beam_reindex_kernel(uint8_t *own, int64_t stride, int beams,
                                                          const int *__restrict__ parents, ReindexTable tab) {
    const int g = blockIdx.y, c0 = 16 * (blockIdx.x * 64 + threadIdx.x), cnt = min(16, tab.n_rows[g] - c0);
    if (cnt <= 0) return;
    uint4 old[kBeamMax];
#pragma unroll
    for (int q = 0; q < kBeamMax; ++q)
        if (q < beams) old[q] = load_cols(own + tab.slot[g * beams + q] * stride + c0, cnt);
#pragma unroll
    for (int q = 0; q < kBeamMax; ++q) {
        if (q >= beams) break;
        const int par = parents[g * beams + q];
        uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
#pragma unroll
        for (int p = 0; p < kBeamMax; ++p)
            if (p < beams && p == par) v = old[p];
        store_cols(own + tab.slot[g * beams + q] * stride + c0, v, cnt);
    }
}

// entries first[i] .. first[i] + count[i] - 1 of table row slot[i] = value[i]: begin's prefix (the prompt's slot) and
// a step's append (the slot itself).  By value, 1 KiB.
struct FillTable {
    int slot[kBeamMaxRows], first[kBeamMaxRows], count[kBeamMaxRows], value[kBeamMaxRows];
};

__global__ __launch_bounds__(256) void beam_fill_kernel(uint8_t *own, int64_t stride, FillTable tab) {
    const int i = blockIdx.y, c0 = 16 * (blockIdx.x * blockDim.x + threadIdx.x), cnt = min(16, tab.count[i] - c0);
    if (cnt <= 0) return;
    const uint32_t w = 0x01010101u * (uint32_t)tab.value[i];
    store_cols(own + tab.slot[i] * stride + tab.first[i] + c0, make_uint4(w, w, w, w), cnt);
}

// rows * beams <= 64 and 1 <= beams <= 8, from the counts alone
bool beam_counts_ok(int n_groups, int beams) {
    return n_groups >= 0 && beams >= 1 && beams <= kBeamMax && (int64_t)n_groups * beams <= kBeamMaxRows;
}

}  // namespace

// ---- plans and workspaces -----------------------------------------------------------------------------------------
// the plan from rows and w alone: a row's nblk = ceil(w / 1024) blocks over `parts` workgroups of bpp blocks each
// (every part but the last bpp blocks, at least kLseMinBlocks where the row is split)
bool logsumexp_plan(int64_t rows, int w, int *parts, int *bpp) {
    if (rows < 0 || w < 1 || w > kLseMaxW) return false;
    const int nblk = (w + kLseBlock - 1) / kLseBlock;
    int p = 1;
    if (rows > 0 && rows < kLseManyRows) {
        const int by_width = nblk / kLseMinBlocks;
        const int by_rows = (int)((kLseTargetGroups + rows - 1) / rows);
        p = std::max(1, std::min(std::min(by_width, by_rows), kLseMaxParts));
    }
    *bpp = (nblk + p - 1) / p;
    *parts = (nblk + *bpp - 1) / *bpp;
    return true;
}

// [rows x parts composites][rows x nblk block sums]
size_t logsumexp_ws_bytes(int64_t rows, int w) {
    int parts, bpp;
    if (!logsumexp_plan(rows, w, &parts, &bpp) || parts == 1) return 0;
    const size_t nblk = (size_t)(w + kLseBlock - 1) / kLseBlock;
    return sizeof(uint64_t) * (size_t)rows * parts + sizeof(float) * (size_t)rows * nblk;
}

hipError_t launch_logsumexp_rows(const float *S, int64_t stride, int64_t rows, int w, float *mx, float *logz, void *ws,
                                 size_t ws_bytes, hipStream_t s) {
    int parts, bpp;
    if (!S || !mx || !logz || !logsumexp_plan(rows, w, &parts, &bpp) || stride < w || rows * parts > INT_MAX)
        return hipErrorInvalidValue;
    if (parts > 1 && (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < logsumexp_ws_bytes(rows, w)))
        return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    if (parts == 1) {
        lse_row_kernel<<<(unsigned)rows, kSampleThreads, 0, s>>>(S, stride, w, mx, logz);
        return hipGetLastError();
    }
    const int nblk = (w + kLseBlock - 1) / kLseBlock;
    uint64_t *wsmax = static_cast<uint64_t *>(ws);
    float *wssum = reinterpret_cast<float *>(wsmax + rows * parts);
    hipError_t e;
    lse_max_kernel<<<(unsigned)(rows * parts), kSampleThreads, 0, s>>>(S, stride, w, bpp, parts, wsmax);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    lse_sum_kernel<<<(unsigned)(rows * parts), kSampleThreads, 0, s>>>(S, stride, w, bpp, parts, nblk, wsmax, wssum);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    lse_finish_kernel<<<(unsigned)rows, kSampleThreads, 0, s>>>(S, stride, w, parts, nblk, wsmax, wssum, mx, logz);
    return hipGetLastError();
}

// the beam step's plan: the parts of its selection (sample_plan at top_k = beams) and of its log-sum-exp
bool beam_step_plan(int n_groups, int beams, int w, int *select_parts, int *lse_parts) {
    int chunk, bpp;
    return beam_counts_ok(n_groups, beams) && sample_plan((int64_t)n_groups * beams, w, beams, select_parts, &chunk) &&
           logsumexp_plan((int64_t)n_groups * beams, w, lse_parts, &bpp);
}

// [split selection: rows x parts x beams composites][the log-sum-exp's, rounded up to 8 bytes]
// [mx: rows floats][logz: rows floats][c: rows x beams floats][token: rows x beams ints]
size_t beam_step_ws_bytes(int n_groups, int beams, int w) {
    int sp, lp;
    if (!beam_step_plan(n_groups, beams, w, &sp, &lp)) return 0;
    const size_t rows = (size_t)n_groups * beams;
    return (sp > 1 ? sizeof(uint64_t) * rows * sp * beams : 0) + (size_t)round_up(logsumexp_ws_bytes(rows, w), 8) +
           sizeof(float) * rows * (2 + 2 * (size_t)beams);
}

hipError_t launch_beam_step(const float *S, int64_t stride, int n_groups, int beams, int w, const float *scores_in,
                            const int *prev, int eos, int *parents, int *tokens, float *scores_out, void *ws,
                            size_t ws_bytes, hipStream_t s) {
    int sp, lp, chunk;
    if (!S || !parents || !tokens || !scores_out || !beam_step_plan(n_groups, beams, w, &sp, &lp) || stride < w)
        return hipErrorInvalidValue;
    if (n_groups == 0) return hipSuccess;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < beam_step_ws_bytes(n_groups, beams, w))
        return hipErrorInvalidValue;
    const int rows = n_groups * beams;
    sample_plan(rows, w, beams, &sp, &chunk);
    char *at = static_cast<char *>(ws);
    uint64_t *lists = reinterpret_cast<uint64_t *>(at);
    at += sp > 1 ? sizeof(uint64_t) * (size_t)rows * sp * beams : 0;
    void *lse_ws = at;
    const size_t lse_bytes = (size_t)round_up(logsumexp_ws_bytes(rows, w), 8);
    at += lse_bytes;
    float *mx = reinterpret_cast<float *>(at), *logz = mx + rows, *cs = logz + rows;
    int *ct = reinterpret_cast<int *>(cs + (size_t)rows * beams);
    hipError_t e;
    if ((e = launch_logsumexp_rows(S, stride, rows, w, mx, logz, lse_ws, lse_bytes, s)) != hipSuccess) return e;
    if (sp == 1) {
        beam_row_kernel<false><<<(unsigned)rows, kSampleThreads, 0, s>>>(S, stride, w, beams, 0, nullptr, mx, logz,
                                                                         scores_in, prev, eos, cs, ct);
    } else {
        beam_part_kernel<<<(unsigned)(rows * sp), kSampleThreads, 0, s>>>(S, stride, w, chunk, sp, beams, lists);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        beam_row_kernel<true><<<(unsigned)rows, kSampleThreads, 0, s>>>(S, stride, w, beams, sp * beams, lists, mx,
                                                                        logz, scores_in, prev, eos, cs, ct);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    beam_group_kernel<<<(unsigned)n_groups, 64, 0, s>>>(beams, cs, ct, parents, tokens, scores_out);
    return hipGetLastError();
}

// The [K | V] thirds of rows 0 .. n_rows[g] - 1 of one cache (n_slabs slabs of slab_rows x 3 d floats) from slab
// src_slots[g * beams + parents[g * beams + q]] into slab dst_slots[g * beams + q].  Checked here: every slot inside
// the cache, every row count inside a slab, no destination among the sources or named twice -- so no store leaves the
// cache or lands on a row another workgroup reads.  The caller checks what the rows mean (transformer.hip).
hipError_t launch_gather_kv(float *cache, int64_t slab_rows, int n_slabs, int d, int n_groups, int beams,
                            const int *dst_slots, const int *src_slots, const int *n_rows, const int *parents,
                            hipStream_t s) {
    if (!cache || !dst_slots || !src_slots || !n_rows || !parents || d < 1 || n_groups < 1 || n_slabs < 1 ||
        n_slabs > kBeamMaxRows || !beam_counts_ok(n_groups, beams))
        return hipErrorInvalidValue;
    const int rows = n_groups * beams;
    GatherTable tab = {};
    uint64_t is_dst = 0, is_src = 0;  // n_slabs <= 64
    int max_n = 0;
    for (int i = 0; i < rows; ++i) {
        const int ds = dst_slots[i], ss = src_slots[i], n = n_rows[i / beams];
        if (ds < 0 || ds >= n_slabs || ss < 0 || ss >= n_slabs || n < 0 || n > slab_rows || (is_dst >> ds & 1))
            return hipErrorInvalidValue;
        is_dst |= (uint64_t)1 << ds;
        is_src |= (uint64_t)1 << ss;
        tab.dst[i] = ds;
        tab.src[i] = ss;
        tab.n_rows[i] = n;
        max_n = std::max(max_n, n);
    }
    if (is_dst & is_src) return hipErrorInvalidValue;
    if (max_n == 0) return hipSuccess;
    const bool vec = d % 4 == 0;
    const int per = vec ? d / 2 : 2 * d;  // a row's [K | V] in float4 / float
    int tpr_log2 = 0;
    while (tpr_log2 < 8 && (1 << tpr_log2) < per) ++tpr_log2;
    const int step = 4 * (256 >> tpr_log2);  // rows a workgroup has in flight
    const int rows_per_wg = (int)round_up(std::max(1, 4096 / per), step);  // about 64 KiB per workgroup
    const dim3 grid((unsigned)((max_n + rows_per_wg - 1) / rows_per_wg), (unsigned)rows);
    const int64_t slab = slab_rows * 3 * d;
    if (vec)
        gather_kv_kernel<float4><<<grid, 256, 0, s>>>(cache, slab, d, beams, rows_per_wg, tpr_log2, parents, tab);
    else
        gather_kv_kernel<float><<<grid, 256, 0, s>>>(cache, slab, d, beams, rows_per_wg, tpr_log2, parents, tab);
    return hipGetLastError();
}

// The in-place reorder of a row table (beam_reindex_kernel).  Checked here: every table row inside the table, no row
// named twice (so no two threads share a byte), every column count inside a row -- so no access leaves the named rows'
// first `stride` bytes.
hipError_t launch_beam_reindex(uint8_t *own, int64_t stride, int n_table_rows, int n_groups, int beams, const int *slots,
                               const int *parents, const int *n_rows, hipStream_t s) {
    if (!own || !slots || !parents || !n_rows || stride < 1 || n_table_rows < 1 || n_table_rows > kBeamMaxRows ||
        n_groups < 1 || !beam_counts_ok(n_groups, beams))
        return hipErrorInvalidValue;
    ReindexTable tab = {};
    uint64_t seen = 0;  // n_table_rows <= 64
    int max_n = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (n_rows[g] < 0 || n_rows[g] > stride) return hipErrorInvalidValue;
        tab.n_rows[g] = n_rows[g];
        max_n = std::max(max_n, n_rows[g]);
        for (int q = 0; q < beams; ++q) {
            const int sl = slots[g * beams + q];
            if (sl < 0 || sl >= n_table_rows || (seen >> sl & 1)) return hipErrorInvalidValue;
            seen |= (uint64_t)1 << sl;
            tab.slot[g * beams + q] = sl;
        }
    }
    if (max_n == 0) return hipSuccess;
    const dim3 grid((unsigned)((max_n + 16 * 64 - 1) / (16 * 64)), (unsigned)n_groups);
    beam_reindex_kernel<<<grid, 64, 0, s>>>(own, stride, beams, parents, tab);
    return hipGetLastError();
}

// Constant runs into a row table (beam_fill_kernel): row slots[i] gets value[i] at entries first[i] .. + count[i] - 1.
// Checked here: every row inside the table, every run inside a row, every value a byte.  Rows may repeat (the runs of
// one call are the caller's to keep apart).
hipError_t launch_beam_fill(uint8_t *own, int64_t stride, int n_table_rows, int n, const int *slots, const int *first,
                            const int *count, const int *value, hipStream_t s) {
    if (!own || !slots || !first || !count || !value || stride < 1 || n_table_rows < 1 ||
        n_table_rows > kBeamMaxRows || n < 1 || n > kBeamMaxRows)
        return hipErrorInvalidValue;
    FillTable tab = {};
    int max_n = 0;
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= n_table_rows || first[i] < 0 || count[i] < 0 || first[i] > stride - count[i] ||
            value[i] < 0 || value[i] > 255)
            return hipErrorInvalidValue;
        tab.slot[i] = slots[i];
        tab.first[i] = first[i];
        tab.count[i] = count[i];
        tab.value[i] = value[i];
        max_n = std::max(max_n, count[i]);
    }
    if (max_n == 0) return hipSuccess;
    const int threads = max_n <= 16 * 64 ? 64 : 256;
    const dim3 grid((unsigned)((max_n + 16 * threads - 1) / (16 * threads)), (unsigned)n);
    beam_fill_kernel<<<grid, threads, 0, s>>>(own, stride, tab);
    return hipGetLastError();
}

}  // namespace qgemm

using namespace qgemm;

extern "C" {

int qgemm_beam_reindex(uint8_t *row_slab, int64_t row_slab_stride, int n_groups, int beams, const int *slots,
                       const int32_t *parents, const int *n_rows, void *stream) {
    return (int)launch_beam_reindex(row_slab, row_slab_stride, kBeamMaxRows, n_groups, beams, slots, parents, n_rows,
                                    static_cast<hipStream_t>(stream));
}

int qgemm_logsumexp_rows_plan(int64_t rows, int w, int *parts) {
    int p, bpp;
    if (!logsumexp_plan(rows, w, &p, &bpp)) return (int)hipErrorInvalidValue;
    if (parts) *parts = p;
    return 0;
}

size_t qgemm_logsumexp_rows_workspace_size(int64_t rows, int w) { return logsumexp_ws_bytes(rows, w); }

int qgemm_logsumexp_rows(const float *S, int64_t s_stride_h, int64_t rows, int w, float *mx, float *logz,
                         void *workspace, size_t ws_bytes, void *stream) {
    return (int)launch_logsumexp_rows(S, s_stride_h, rows, w, mx, logz, workspace, ws_bytes,
                                      static_cast<hipStream_t>(stream));
}

int qgemm_beam_step_plan(int n_groups, int beams, int w, int *select_parts, int *lse_parts) {
    int sp, lp;
    if (!beam_step_plan(n_groups, beams, w, &sp, &lp)) return (int)hipErrorInvalidValue;
    if (select_parts) *select_parts = sp;
    if (lse_parts) *lse_parts = lp;
    return 0;
}

size_t qgemm_beam_step_workspace_size(int n_groups, int beams, int w) { return beam_step_ws_bytes(n_groups, beams, w); }

int qgemm_beam_step(const float *S, int64_t s_stride_h, int n_groups, int beams, int w, const float *scores_in,
                    const int32_t *prev, int eos, int32_t *parents, int32_t *tokens, float *scores_out, void *workspace,
                    size_t ws_bytes, void *stream) {
    return (int)launch_beam_step(S, s_stride_h, n_groups, beams, w, scores_in, prev, eos, parents, tokens, scores_out,
                                 workspace, ws_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
