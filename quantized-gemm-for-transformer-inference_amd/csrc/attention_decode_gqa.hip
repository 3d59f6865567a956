// attention_decode_gqa.hip -- decode attention for grouped-query heads: n_kv_heads < n_heads, query head
// h reads K / V head h / G, G = n_heads / n_kv_heads.  attention_decode_kernel (attention_decode_kernel.h) gives every
// query head a workgroup of its own, so the G heads of a group would each stream the SAME K / V rows from memory -- and
// that stream's latency is the whole cost of a decode workgroup (s16, s29).  Here ONE WORKGROUP of 256 threads owns ONE
// (KV head, block of up to 4 query heads of its group, query row[, sequence]) and stages every K / V chunk ONCE for
// the block:
//   s_h[j] = Q_h[i] . K[j]        all 256 threads: thread t owns key t & 127 of the chunk and the head pair 2 (t >> 7),
//                                 reads its K row from LDS once and runs both heads' chains against it
//   p_h    = softmax(s_h * scale) wave w owns head w: max, exps, the sequential sum chain and the divides are
//                                 wave-local, so the four serial sums run side by side on the four SIMDs
//   O_h[i] = p_h V                kW = 64: wave w carries head w's columns; kW = 128: wave w carries column half w & 1
//                                 of the head pair w >> 1, one V read from LDS feeding two fmaf chains
// The rows of every query head are BIT FOR BIT attention_decode_kernel's on K / V with each head repeated G times: a
// score is the same fmaf chain from +0 over k ascending, zero-padded to 32 (`steps`, the same text per head); the
// softmax is softmax_row_max / softmax_exp, the ONE sequential sum in column order (hop_left over 16-element blocks),
// __fdiv_rn; P V is each column's fmaf chain over ALL keys in key order, then fl(acc + 0) when seq_kv % 32 != 0; a masked
// key has P = +0 and still contributes; an indirect table entry that names no slab reads as quiet NaNs.  (The maximum
// is reduced in another order than there, 64 lanes instead of 256 threads: with the strict > a NaN never wins, and a
// maximum of either zero gives the same exps, so the order of the candidates changes no bit, as it does not between
// that kernel and softmax_rows_kernel.)
// The stream is attention_decode_kernel's, text and reasons: K chunks then V chunks of 128 keys, two chunks in flight
// in registers, the branch-free clamped fetch, the zero / NaN select in `put`, vector or scalar loads chosen once per
// matrix, the indirect form's table row and slab offsets in LDS with nxo read before the refilled buffer is `put`.
// (The kernel's text is a copy on purpose: with the prologue and the softmax as shared functions this kernel measured
// up to 6 % slower, and the shared stream moved its register table; DESIGN.md s33, profiles/decode_refactor_probe.log.)
// LDS: four score rows (64 KiB) + one chunk (34 / 66 KiB) + four query rows + the indirect form's tables (5 KiB): 137
// KiB at kW = 128, one workgroup per CU.  Four heads per workgroup is what that budget holds; a group of G > 4 heads
// takes ceil(G / 4) workgroups, the last of them with G % 4 heads (a runtime count: G = 3, 5, 7 are real models').
// Built with the packed fp32 instructions off, as attention_decode_wide.o (Makefile).
#include "attention_decode_kernel.h"

namespace qgemm {

namespace {

// group: G.  grid x = n_kv_heads * ceil(G / 4), y = query rows, z = sequences (DecodeMany, DecodeIndirect).
template <bool kCausal, typename Seqs, int kW>
__global__ __launch_bounds__(kDecThreads) void attention_decode_gqa_kernel(
    const float *__restrict__ Q, int64_t ldq, const float *__restrict__ K, int64_t ldk, const float *__restrict__ V,
    int64_t ldv, float *__restrict__ O, int64_t ldo, int dk, float scale, int group, Seqs seqs) {
    __shared__ __attribute__((aligned(16))) float S[kDecGroupHeads][kDecMaxSeq];
    constexpr int kPieces = kW / 4, kShift = kW == 64 ? 4 : 5;       // float4 pieces of a row: f >> kShift = the key
    constexpr int kDecStride = kW + 4;                                // chunk row stride (floats)
    constexpr int kDecPer = kDecChunk * kPieces / kDecThreads;        // float4 pieces of a chunk per thread
    __shared__ __attribute__((aligned(16))) float KV[kDecChunk * kDecStride];
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
    } else if constexpr (std::is_same<Seqs, DecodeMany>::value) {
        const int b = blockIdx.z;
        const int64_t row0 = (int64_t)b * seqs.rows_per_seq, slab = seqs.tab.kv_slot[b];
        Q += row0 * ldq;
        O += row0 * ldo;
        K += slab * seqs.k_stride_seq;
        V += slab * seqs.v_stride_seq;
        seq_kv = seqs.tab.seq_kv[b];
        q_pos0 = seqs.tab.q_pos0[b];
    } else {
        seq_kv = seqs.seq_kv;
        q_pos0 = seqs.q_pos0;
    }
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float *Qb = Q + qi * ldq + (int64_t)h0 * dk, *Kb = K + (int64_t)kvh * dk, *Vb = V + (int64_t)kvh * dk;
    const int seq = seq_kv;
    // the row's limit (q_pos0 <= seq_kv: the launcher clamps it, so the sum stays in int range)
    const int L = kCausal ? min(seq, qi + q_pos0 + 1) : seq;
    const int nck = (L + kDecChunk - 1) / kDecChunk;      // K chunks that hold a visible key
    const int ncv = (seq + kDecChunk - 1) / kDecChunk;    // V chunks: every key
    const int dk4 = (dk + 3) >> 2;                        // float4 columns of a row (the last one zero-padded)

    // ---- the K / V stream: attention_decode_kernel's fetch / put / two chunks in flight, one KV head's rows
    auto aligned = [&](const float *base, int64_t ld, int64_t ss) {
        return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && (ld & 3) == 0 && (dk & 3) == 0 && (ss & 3) == 0;
    };
    const bool vec_k = aligned(Kb, ldk, kss), vec_v = aligned(Vb, ldv, vss);  // workgroup-uniform
    int64_t nxo[kDecPer];  // (DecodeIndirect) the slab offsets of the rows the NEXT fetch brings
    auto slabs_of = [&](const int64_t *so, int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kDecPer; ++i) {
            const int row = (t + i * kDecThreads) >> kShift;
            nxo[i] = so[min((int)own[min(c0 + row, seq - 1)], kDecodeMaxBatch - 1)];
        }
    };
    auto slab_at = [&](const float *src, int i) __attribute__((always_inline)) {
        if constexpr (kIndirect) src += nxo[i];
        return src;
    };
    auto fetch = [&](float4 (&r)[kDecPer], const float *src, int64_t ld, int c0, bool vec) __attribute__((always_inline)) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < kDecPer; ++i) {
                const int f = t + i * kDecThreads, row = f >> kShift, c4 = f & (kPieces - 1);
                r[i] = *reinterpret_cast<const float4 *>(slab_at(src, i) + min(c0 + row, seq - 1) * ld +
                                                         4 * min(c4, dk4 - 1));
            }
        } else {
#pragma unroll
            for (int i = 0; i < kDecPer; ++i) {
                const int f = t + i * kDecThreads, row = f >> kShift, c4 = f & (kPieces - 1);
                const float *p = slab_at(src, i) + min(c0 + row, seq - 1) * ld;
                r[i].x = p[min(4 * c4, dk - 1)];
                r[i].y = p[min(4 * c4 + 1, dk - 1)];
                r[i].z = p[min(4 * c4 + 2, dk - 1)];
                r[i].w = p[min(4 * c4 + 3, dk - 1)];
            }
        }
    };
    auto put = [&](const float4 (&r)[kDecPer], int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kDecPer; ++i) {
            const int f = t + i * kDecThreads, row = f >> kShift, c4 = f & (kPieces - 1);
            const bool in = c0 + row < seq;
            float4 x = r[i];
            if constexpr (kIndirect) {  // an entry that names no slab: the row reads as quiet NaNs (under the zeros)
                const float qn = __uint_as_float(0x7fc00000u);
                if ((int)own[min(c0 + row, seq - 1)] >= n_slabs) x = make_float4(qn, qn, qn, qn);
            }
            float4 v;
            v.x = in && 4 * c4 < dk ? x.x : 0.0f;
            v.y = in && 4 * c4 + 1 < dk ? x.y : 0.0f;
            v.z = in && 4 * c4 + 2 < dk ? x.z : 0.0f;
            v.w = in && 4 * c4 + 3 < dk ? x.w : 0.0f;
            *reinterpret_cast<float4 *>(KV + row * kDecStride + 4 * c4) = v;
        }
    };
    auto fetch_g = [&](float4 (&r)[kDecPer], int g) __attribute__((always_inline)) {
        if (g < nck) fetch(r, Kb, ldk, g * kDecChunk, vec_k);
        else if (g < nck + ncv) fetch(r, Vb, ldv, (g - nck) * kDecChunk, vec_v);
    };
    auto slabs_g = [&](int g) __attribute__((always_inline)) {
        if (g < nck) slabs_of(ko, g * kDecChunk);
        else if (g < nck + ncv) slabs_of(vo, (g - nck) * kDecChunk);
    };
    float4 pfa[kDecPer], pfb[kDecPer];
    if constexpr (kIndirect) slabs_g(0);
    fetch_g(pfa, 0);
    if constexpr (kIndirect) slabs_g(1);
    fetch_g(pfb, 1);
    // the block's query rows, zeros past d_k and in the rows of heads the block does not have
    for (int i = t; i < kDecGroupHeads * kW; i += kDecThreads) {
        const int hh = i / kW, c = i & (kW - 1);
        Qs[hh][c] = hh < nh && c < dk ? Qb[(int64_t)hh * dk + c] : 0.0f;
    }

    // ---- s_h[j] = Q_h[i] . K[j], j < L: thread t runs the chains of key t & 127 for heads 2 (t >> 7) and + 1 -- the K
    // row as b128 reads from LDS ONCE for both, the two query rows as broadcast reads.  Each chain is
    // attention_decode_kernel's `steps`.  A pair with no head of the block (nh <= 2, the upper pair) skips; the second
    // chain of a pair whose second head the block lacks runs on the zero query row into a score row nobody reads.
    const int key = t & (kDecChunk - 1), pair = wave >> 1;
    const bool more = dk > (kW == 64 ? 32 : 96);
    auto k_step = [&](float4 (&pf)[kDecPer], int c) __attribute__((always_inline)) {
        if constexpr (kIndirect) slabs_g(c + 2);
        if (c) __syncthreads();  // every thread is done with the previous chunk
        put(pf, c * kDecChunk);
        __syncthreads();
        fetch_g(pf, c + 2);
        const int j = c * kDecChunk + key;
        if (2 * pair < nh && j < L) {
            const float4 *kr = reinterpret_cast<const float4 *>(KV + key * kDecStride);
            const float4 *q0 = reinterpret_cast<const float4 *>(Qs[2 * pair]);
            const float4 *q1 = reinterpret_cast<const float4 *>(Qs[2 * pair + 1]);
            float res0 = 0.0f, res1 = 0.0f;
            auto steps = [&](int s0) __attribute__((always_inline)) {
#pragma unroll
                for (int s = s0; s < s0 + 8; ++s) {
                    const float4 b = kr[s], a0 = q0[s], a1 = q1[s];
                    res0 = fmaf(a0.x, b.x, res0);
                    res0 = fmaf(a0.y, b.y, res0);
                    res0 = fmaf(a0.z, b.z, res0);
                    res0 = fmaf(a0.w, b.w, res0);
                    res1 = fmaf(a1.x, b.x, res1);
                    res1 = fmaf(a1.y, b.y, res1);
                    res1 = fmaf(a1.z, b.z, res1);
                    res1 = fmaf(a1.w, b.w, res1);
                }
            };
            steps(0);
            if constexpr (kW == 128) {
                steps(8);
                steps(16);
            }
            if (more) steps(kPieces - 8);
            S[2 * pair][j] = res0;
            S[2 * pair + 1][j] = res1;
        }
    };
    for (int c = 0; c < nck; c += 2) {
        k_step(pfa, c);
        if (c + 1 < nck) k_step(pfb, c + 1);
    }
    __syncthreads();

    // ---- softmax of head `wave` over its first L columns, in place in its score row: everything is wave-local (no
    // cross-wave step for the maximum, no LDS for the sum); the barrier between the exps and the sum chain orders the
    // lanes' LDS writes before the other lanes' reads.
    float *row = S[wave];
    const bool mine = wave < nh;
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

    // ---- O_h[i] = p_h V over every key: lane = output column, the accumulators carried across the chunks in key order.
    // kW = 64: wave w carries head w.  kW = 128: wave w carries columns 64 (w & 1) .. + 63 of heads 2 (w >> 1) and + 1:
    // one V element from LDS feeds both heads' fmaf, P comes from two broadcast rows.  (A second head the block lacks:
    // its chain runs on a score row nobody wrote and is not stored.)
    const int hd = kW == 64 ? wave : 2 * pair;             // the (first) head this wave carries
    const bool pv = hd < nh, two = kW == 128 && hd + 1 < nh;
    const int col = kW == 64 ? lane : 64 * (wave & 1) + lane;
    float acc0 = 0.0f, acc1 = 0.0f;
    auto v_step = [&](float4 (&pf)[kDecPer], int c) __attribute__((always_inline)) {
        if constexpr (kIndirect) slabs_g(nck + c + 2);
        __syncthreads();  // P complete (c = 0) / the previous chunk consumed
        put(pf, c * kDecChunk);
        __syncthreads();
        fetch_g(pf, nck + c + 2);
        if (pv) {
            const int k0 = c * kDecChunk, kn = min(kDecChunk, seq - k0);
            const float *vcol = KV + col, *p0 = S[hd] + k0;
            const float *p1 = S[kW == 64 ? hd : hd + 1] + k0;
            int k = 0;
            for (; k + 8 <= kn; k += 8) {
                const float4 a0 = *reinterpret_cast<const float4 *>(p0 + k);
                const float4 a1 = *reinterpret_cast<const float4 *>(p0 + k + 4);
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = vcol[(k + u) * kDecStride];
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
                const float v = vcol[k * kDecStride];
                acc0 = fmaf(p0[k], v, acc0);
                if constexpr (kW == 128) acc1 = fmaf(p1[k], v, acc1);
            }
        }
    };
    // V chunk c is chunk nck + c of the stream: it sits in pfa when nck + c is even
    auto v_phase = [&](float4 (&first)[kDecPer], float4 (&second)[kDecPer]) __attribute__((always_inline)) {
        for (int c = 0; c < ncv; c += 2) {
            v_step(first, c);
            if (c + 1 < ncv) v_step(second, c + 1);
        }
    };
    if (nck & 1) v_phase(pfb, pfa);
    else v_phase(pfa, pfb);
    if (pv && col < dk) {
        if (seq & 31) {  // the zero-padded rest of the last 32-key tile: -0 becomes +0
            acc0 = __fadd_rn(acc0, 0.0f);
            acc1 = __fadd_rn(acc1, 0.0f);
        }
        float *o = O + qi * ldo + (int64_t)(h0 + hd) * dk + col;
        o[0] = acc0;
        if (two) o[dk] = acc1;
    }
}

// the instantiation a launch takes (the caller has tested that d_k lies in one of the two envelopes), on the grid
// (KV heads x blocks of a group, rows, sequences)
template <typename Seqs>
hipError_t gqa_launch(int rows, int n_seqs, bool causal, const float *Q, int64_t ldq, const float *K, int64_t ldk,
                      const float *V, int64_t ldv, float *O, int64_t ldo, int n_heads, int n_kv_heads, int dk,
                      float scale, const Seqs &seqs, hipStream_t stream) {
    auto *kernel = dk > kDecMaxDk ? (causal ? attention_decode_gqa_kernel<true, Seqs, kDecWideDk>
                                            : attention_decode_gqa_kernel<false, Seqs, kDecWideDk>)
                                  : (causal ? attention_decode_gqa_kernel<true, Seqs, kDecMaxDk>
                                            : attention_decode_gqa_kernel<false, Seqs, kDecMaxDk>);
    kernel<<<decode_group_grid(n_heads, n_kv_heads, rows, n_seqs), kDecThreads, 0, stream>>>(
        Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, n_heads / n_kv_heads, seqs);
    return hipGetLastError();
}

}  // namespace

// whole groups of 2 .. 16 heads inside either decode envelope
bool attention_decode_gqa_ok(int seq_q, int seq_kv, int dk, int n_heads, int n_kv_heads) {
    return attention_decode_any_ok(seq_q, seq_kv, dk) && groups_ok(n_heads, n_kv_heads, 2);
}

hipError_t launch_attention_decode_gqa(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V,
                                       int64_t ldv, float *O, int64_t ldo, int seq_q, int seq_kv, int n_heads,
                                       int n_kv_heads, int dk, float scale, int q_pos0, hipStream_t stream) {
    if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads || dk < 1 || seq_q < 0 || seq_kv < 1 || q_pos0 < kNoMask)
        return hipErrorInvalidValue;
    if (!attention_decode_gqa_ok(seq_q, seq_kv, dk, n_heads, n_kv_heads)) return hipErrorNotSupported;
    if (seq_q == 0) return hipSuccess;
    // past seq_kv - 1 the mask hides nothing: clamped, so the kernel's row limit cannot overflow
    const DecodeOne one{seq_kv, q_pos0 == kNoMask ? 0 : (q_pos0 < seq_kv ? q_pos0 : seq_kv)};
    return gqa_launch(seq_q, 1, q_pos0 != kNoMask, Q, ldq, K, ldk, V, ldv, O, ldo, n_heads, n_kv_heads, dk, scale, one,
                      stream);
}

// tab: checked and clamped by launch_attention_batched_gqa (attention_launch.hip); what sizes the kernel's LDS arrays
// and grid is tested again here (decode_table_ok), as in launch_attention_decode_batched
hipError_t launch_attention_decode_batched_gqa(const float *Q, int64_t ldq, const float *K, int64_t ldk,
                                               int64_t k_stride_seq, const float *V, int64_t ldv, int64_t v_stride_seq,
                                               float *O, int64_t ldo, int n_seqs, int rows_per_seq,
                                               const DecodeBatchTable &tab, bool causal, int n_heads, int n_kv_heads,
                                               int dk, float scale, hipStream_t stream) {
    if (!groups_ok(n_heads, n_kv_heads, 2) || !decode_table_ok(tab, n_seqs, rows_per_seq, dk, false, 0))
        return hipErrorInvalidValue;
    const DecodeMany many{k_stride_seq, v_stride_seq, rows_per_seq, tab};
    return gqa_launch(rows_per_seq, n_seqs, causal, Q, ldq, K, ldk, V, ldv, O, ldo, n_heads, n_kv_heads, dk, scale, many,
                      stream);
}

// ... and what keeps every table read inside the table, as in launch_attention_decode_indirect
hipError_t launch_attention_decode_indirect_gqa(const float *Q, int64_t ldq, const float *K, int64_t ldk,
                                                int64_t k_stride_seq, const float *V, int64_t ldv, int64_t v_stride_seq,
                                                float *O, int64_t ldo, int n_seqs, int rows_per_seq,
                                                const uint8_t *row_slab, int64_t row_slab_stride, int n_slabs,
                                                const DecodeBatchTable &tab, bool causal, int n_heads, int n_kv_heads,
                                                int dk, float scale, hipStream_t stream) {
    if (!groups_ok(n_heads, n_kv_heads, 2) || !row_slab || n_slabs < 1 || n_slabs > kDecodeMaxBatch ||
        !decode_table_ok(tab, n_seqs, rows_per_seq, dk, true, row_slab_stride))
        return hipErrorInvalidValue;
    const DecodeIndirect ind{k_stride_seq, v_stride_seq, rows_per_seq, n_slabs, row_slab, row_slab_stride, tab};
    return gqa_launch(rows_per_seq, n_seqs, causal, Q, ldq, K, ldk, V, ldv, O, ldo, n_heads, n_kv_heads, dk, scale, ind,
                      stream);
}

}  // namespace qgemm
