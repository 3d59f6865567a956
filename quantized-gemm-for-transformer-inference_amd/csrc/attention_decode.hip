// attention_decode.hip -- the attention core for a few query rows against a long key sequence: the self-attention of
// an incremental decoding step (1 .. 8 new rows against a key / value cache) and its cross-attention.
// attention_fused_kernel (attention.hip) gives such a call a 32-query tile, 1024 threads and 153 KiB of LDS per head
// and stops at 512 keys; here ONE WORKGROUP of 256 threads owns ONE (head, query row) pair, up to 4096 keys:
//   s[j] = Q_h[i] . K_h[j]          one thread per key of a 128-key chunk staged in LDS
//   p    = softmax(s * scale)       max / exp / divide across the threads, the sum as one chain in wave 0
//   O[i, h*d_k ..] = p V_h          one lane per output column (wave 0), V streamed through LDS in 128-key chunks
// The result is bit-identical to qgemm_mm_fp32 + qgemm_softmax_rows[_causal] + qgemm_mm_fp32 per head, the contract of
// attention_fused_kernel (its header comment):
//   * a score is the fmaf chain from +0 over k ascending, d_k zero-padded to 32: Q and K are staged with zeros past
//     d_k, so the padded steps are fmaf(+0, +0, res) = fl(res + 0) (the f32 MFMA of gemm_f32.hip computes this chain);
//   * softmax as softmax_rows_kernel: max and exp by the contract at softmax_row_max (qgemm_internal.h), ONE
//     sequential fp32 sum in column order (hopping lane to lane, 16 elements per lane, wrapping from lane 63 to lane 0
//     every 1024 elements), __fdiv_rn;
//   * P V is the fmaf chain from +0 over ALL seq_kv keys ascending, then fl(acc + 0) when seq_kv % 32 != 0 (the zero
//     padding of the reference's last 32-wide tile).
// Both serial chains (the row sum, each column's P V) run along the keys, so a row cannot be split across workgroups:
// the parallelism is heads x query rows outside the workgroup, keys (Q K^T, max, exp, divide) and d_k columns (P V)
// inside it.
// kCausal: row i sees keys 0 .. L - 1, L = min(seq_kv, i + q_pos0 + 1).  Scores are computed, and K is read, below L
// only; the softmax runs over L columns; P is +0 from L on and P V still runs over all of seq_kv, so a masked key
// contributes fmaf(+0, v, acc) (0 * inf = NaN, as DESIGN.md s15 defines).  kCausal = false: L = seq_kv.
// LDS: the score row (16 KiB) + one K / V chunk (34 KiB) + the query row: 50.3 KiB, room for three workgroups per CU;
// the two chunks held in registers (176 VGPRs) make it two.  A decoding step launches heads x rows <= 128 workgroups
// for 256 CUs, so a workgroup's own latency, not the occupancy, sets the launch time.
// The batched launch runs the same workgroup for up to 64 independent sequences (grid z = the
// sequence): each sequence has its own K / V slab, key count and mask offset, read from a table in the kernel
// arguments.  It is the SAME kernel template, instantiated with DecodeMany instead of DecodeOne: one text of the
// arithmetic.  (The body as a __device__ function inlined into two kernels was tried first: the compiler then
// transformed the chunk loops differently and the single-sequence launch measured 0.2 % slower at 4096 keys; as one
// kernel template the single-sequence instantiation compiles to the instruction stream it had before, register
// numbers aside.)
// The indirect launch is the batched one with a THIRD Seqs type, DecodeIndirect: every key position of
// a sequence names the slab that holds its K / V row, through a byte table in device memory (beam search's copy-free
// cache reorder).  The sequence's table row (<= 4096 bytes) is staged in LDS before the first fetch -- one 16-byte piece
// per thread, one exposed latency per WORKGROUP -- so the byte in front of a K / V address is an LDS read issued with
// the fetch, two chunks ahead of the data's use, not a second memory latency per chunk.  Only the address of a fetched
// row and a NaN select in `put` differ; the arithmetic below is the one text.
#include <type_traits>

#include "qgemm_internal.h"

namespace qgemm {

namespace {

constexpr int kAttnDecodeMaxQ = 8;  // query rows up to which launch_attention prefers this kernel
constexpr int kDecMaxSeq = 4096;  // the softmax row limit of the API
constexpr int kDecMaxDk = 64;
constexpr int kDecThreads = 256;
constexpr int kDecChunk = 128;    // keys per staged K / V chunk
constexpr int kDecStride = 68;    // chunk row stride (floats): a thread-per-key b128 read is conflict-free
constexpr int kDecPer = kDecChunk * 16 / kDecThreads;  // float4 pieces of a chunk per thread

// The sequences of a launch, the kernel's last argument (by value).  DecodeOne: the single-sequence launch, grid
// (heads, query rows).  DecodeMany: up to kDecodeMaxBatch independent sequences, grid (heads, rows per sequence,
// sequences): sequence b's query / output rows are b * rows_per_seq .. of Q / O, its K / V rows the slab at
// K / V + kv_slot[b] * k / v_stride_seq, with seq_kv[b] keys and mask offset q_pos0[b] (uniform per workgroup: scalar
// loads from the kernel arguments, nothing in device memory).
struct DecodeOne {
    int seq_kv, q_pos0;
};
struct DecodeMany {
    int64_t k_stride_seq, v_stride_seq;
    int rows_per_seq;
    DecodeBatchTable tab;
};
// DecodeIndirect: DecodeMany's grid; K / V row j of sequence b is row j of slab row_slab[tab.kv_slot[b] * row_slab_stride
// + j] (tab.kv_slot holds the sequence's TABLE ROW here), an entry >= n_slabs reads as a row of quiet NaNs.
struct DecodeIndirect {
    int64_t k_stride_seq, v_stride_seq;
    int rows_per_seq, n_slabs;
    const uint8_t *row_slab;
    int64_t row_slab_stride;
    DecodeBatchTable tab;
};

// ONE kernel text for both launches (the batched decode kernel of DESIGN.md s17 is
// attention_decode_kernel<kCausal, DecodeMany>): the sequence's parameters are resolved at the top, everything below
// is the work of one (head, query row) of one sequence.
template <bool kCausal, typename Seqs>
__global__ __launch_bounds__(kDecThreads) void attention_decode_kernel(
    const float *__restrict__ Q, int64_t ldq, const float *__restrict__ K, int64_t ldk, const float *__restrict__ V,
    int64_t ldv, float *__restrict__ O, int64_t ldo, int dk, float scale, Seqs seqs) {
    __shared__ __attribute__((aligned(16))) float S[kDecMaxSeq];
    __shared__ __attribute__((aligned(16))) float KV[kDecChunk * kDecStride];
    __shared__ __attribute__((aligned(16))) float Qs[kDecMaxDk];
    __shared__ float red[kDecThreads / 64 + 1];
    // grid (heads, query rows): with a multiple of 8 heads the rows of a head share an XCD and its L2
    const int h = blockIdx.x, qi = blockIdx.y;
    int seq_kv, q_pos0;
    constexpr bool kIndirect = std::is_same<Seqs, DecodeIndirect>::value;
    // DecodeIndirect alone: the sequence's table row in LDS (own[j] = the slab of key j), the slabs' offsets in K and V
    // in LDS (ko[e] / vo[e], e the table entry clamped to 63: an entry that names no slab gives the last slab's), the
    // slab strides and count
    const uint8_t *own = nullptr;
    const int64_t *ko = nullptr, *vo = nullptr;
    int64_t kss = 0, vss = 0;
    int n_slabs = 0;
    if constexpr (kIndirect) {
        // The row starts at any byte: the aligned 16-byte pieces that hold an entry of it are copied as they lie (a
        // piece that holds a byte of the row lies in that byte's page), and own points `off` bytes into the copy.
        // A slab's offset is a 64-bit product; 64 of them per matrix are made here once, so that a fetched row costs two
        // LDS reads in front of its address and no 64-bit multiply (as products per row the launch measured 20 % over
        // the batched one at 2048 keys with the identity table).
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
    const float *Qb = Q + qi * ldq + (int64_t)h * dk, *Kb = K + (int64_t)h * dk, *Vb = V + (int64_t)h * dk;
    const int seq = seq_kv;
    // the row's limit (q_pos0 <= seq_kv: the launcher clamps it, so the sum stays in int range)
    const int L = kCausal ? min(seq, qi + q_pos0 + 1) : seq;
    const int nck = (L + kDecChunk - 1) / kDecChunk;      // K chunks that hold a visible key
    const int ncv = (seq + kDecChunk - 1) / kDecChunk;    // V chunks: every key
    const int dk4 = (dk + 3) >> 2;                        // float4 columns of a row (the last one zero-padded)

    // A chunk as float4 pieces (16 threads per key row: coalesced) fetched into registers ahead of its use, then
    // written to KV [key][stride] with zeros past seq_kv and past d_k.  The fetch is BRANCH-FREE, so its loads stay in
    // flight under the arithmetic that follows: every address is clamped into the matrix (row to seq_kv - 1, column to
    // d_k - 1) and the zeros are selected in `put`, when the data is used.  (With attention_fused_kernel's per-piece
    // test -- a divergent vector-or-scalar branch writing the same registers -- the compiler waited for every load
    // right after issuing it, and the launch was bound by the exposed latency of each chunk: 139 us at 4096 keys.)
    // The 16-byte alignment test is made once per matrix: every row of a head is aligned when the head's first row is
    // and the row stride is a multiple of 4 floats; anything else (any stride, any d_k) takes the scalar loads.
    // (DecodeIndirect: ... and the slab stride is one too, every slab starting like the first)
    auto aligned = [&](const float *base, int64_t ld, int64_t ss) {
        return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && (ld & 3) == 0 && (dk & 3) == 0 && (ss & 3) == 0;
    };
    const bool vec_k = aligned(Kb, ldk, kss), vec_v = aligned(Vb, ldv, vss);  // workgroup-uniform
    // DecodeIndirect: nxo[i] = the offset of the slab that holds this thread's row i of the chunk the NEXT fetch
    // brings (so: the matrix's slab offsets), every table entry clamped into the slabs so that no entry forms an address
    // outside them; `put` selects the NaNs.  They are read from LDS into registers of their own BEFORE the buffer that
    // fetch refills is `put`: read inside the fetch, the compiler took the buffer's just-freed registers as the LDS
    // reads' temporaries and then waited, between a chunk's loads, for loads still in flight into the OTHER buffer
    // (s_waitcnt vmcnt(6) after the third load), which stalled every fetch on the chunk before it.
    int64_t nxo[kDecPer];
    auto slabs_of = [&](const int64_t *so, int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kDecPer; ++i) {
            const int row = (t + i * kDecThreads) >> 4;
            nxo[i] = so[min((int)own[min(c0 + row, seq - 1)], kDecodeMaxBatch - 1)];
        }
    };
    auto slab_at = [&](const float *src, const int64_t *so, int i) __attribute__((always_inline)) {
        if constexpr (kIndirect) src += nxo[i];
        return src;
    };
    auto fetch = [&](float4 (&r)[kDecPer], const float *src, int64_t ld, const int64_t *ss, int c0,
                     bool vec) __attribute__((always_inline)) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < kDecPer; ++i) {
                const int f = t + i * kDecThreads, row = f >> 4, c4 = f & 15;
                r[i] = *reinterpret_cast<const float4 *>(slab_at(src, ss, i) + min(c0 + row, seq - 1) * ld +
                                                         4 * min(c4, dk4 - 1));
            }
        } else {
#pragma unroll
            for (int i = 0; i < kDecPer; ++i) {
                const int f = t + i * kDecThreads, row = f >> 4, c4 = f & 15;
                const float *p = slab_at(src, ss, i) + min(c0 + row, seq - 1) * ld;
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
            const int f = t + i * kDecThreads, row = f >> 4, c4 = f & 15;
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

    // The K chunks and then the V chunks are ONE stream of nck + ncv chunks, chunk g of it fetched TWO chunks ahead
    // into pfa (g even) or pfb (g odd): a workgroup is bound by the latency of its own loads, so two chunks, 64 KiB per
    // workgroup, are in flight under every chunk's arithmetic, and the first two V chunks stream in under the softmax
    // and its sum chain
    auto fetch_g = [&](float4 (&r)[kDecPer], int g) __attribute__((always_inline)) {
        if (g < nck) fetch(r, Kb, ldk, ko, g * kDecChunk, vec_k);
        else if (g < nck + ncv) fetch(r, Vb, ldv, vo, (g - nck) * kDecChunk, vec_v);
    };
    // (DecodeIndirect) the slab offsets of chunk g of the stream into nxo
    auto slabs_g = [&](int g) __attribute__((always_inline)) {
        if (g < nck) slabs_of(ko, g * kDecChunk);
        else if (g < nck + ncv) slabs_of(vo, (g - nck) * kDecChunk);
    };
    float4 pfa[kDecPer], pfb[kDecPer];
    if constexpr (kIndirect) slabs_g(0);
    fetch_g(pfa, 0);
    if constexpr (kIndirect) slabs_g(1);
    fetch_g(pfb, 1);
    if (t < kDecMaxDk) Qs[t] = t < dk ? Qb[t] : 0.0f;

    // ---- s[j] = Q[i] . K[j], j < L: thread j of the chunk runs the whole chain of its key from LDS (K row as b128
    // reads, the query row as broadcast reads), over d_k zero-padded to 32
    const bool wide = dk > 32;
    auto k_step = [&](float4 (&pf)[kDecPer], int c) __attribute__((always_inline)) {
        if constexpr (kIndirect) slabs_g(c + 2);
        if (c) __syncthreads();  // every thread is done with the previous chunk
        put(pf, c * kDecChunk);
        __syncthreads();
        fetch_g(pf, c + 2);
        const int j = c * kDecChunk + t;
        if (t < kDecChunk && j < L) {
            const float4 *kr = reinterpret_cast<const float4 *>(KV + t * kDecStride);
            const float4 *qr = reinterpret_cast<const float4 *>(Qs);
            float res = 0.0f;
            auto steps = [&](int s0) __attribute__((always_inline)) {
#pragma unroll
                for (int s = s0; s < s0 + 8; ++s) {
                    const float4 a = qr[s], b = kr[s];
                    res = fmaf(a.x, b.x, res);
                    res = fmaf(a.y, b.y, res);
                    res = fmaf(a.z, b.z, res);
                    res = fmaf(a.w, b.w, res);
                }
            };
            steps(0);
            if (wide) steps(8);
            S[j] = res;
        }
    };
    for (int c = 0; c < nck; c += 2) {
        k_step(pfa, c);
        if (c + 1 < nck) k_step(pfb, c + 1);
    }
    __syncthreads();

    // ---- softmax of the row over its first L columns, in place in S
    const float seed = __fmul_rn(S[0], scale);
    float cand = softmax_row_max(S, t + 1, L, kDecThreads, scale);
    if (lane == 0) red[wave] = cand;
    __syncthreads();  // (also: every thread has read S[0] before the exps overwrite it)
#pragma unroll
    for (int w = 0; w < kDecThreads / 64; ++w) {
        const float o = red[w];
        cand = (o > cand) ? o : cand;
    }
    const float mx = (cand > seed) ? cand : seed;
    for (int c = t; c < L; c += kDecThreads) S[c] = softmax_exp(S[c], scale, mx);
    __syncthreads();
    // the ONE sequential sum, in wave 0: lane l holds elements 1024 p + 16 l .. + 15 of pass p in registers and the
    // running sum hops from lane to lane (hop_left); after step t of a pass the chain through lane t - 1's block
    // sits in that lane, and lane 0's first step of the next pass reads lane 63 (the rotation wraps), so the chain
    // goes on across passes.  Elements at or past L are -0.0f, which leaves any sum unchanged.
    if (wave == 0) {
        const int nl = (L + 15) >> 4;  // 16-element blocks that hold an element
        float s = 0.0f;
        for (int b0 = 0; b0 < nl; b0 += 64) {
            const int e0 = 16 * (b0 + lane);
            float e[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float4 v = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
                if (e0 + 4 * j < L) v = *reinterpret_cast<const float4 *>(S + e0 + 4 * j);
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
        if (lane == 0) red[kDecThreads / 64] = sum;
    }
    __syncthreads();
    const float sum = red[kDecThreads / 64];
    for (int c = t; c < L; c += kDecThreads) S[c] = __fdiv_rn(S[c], sum);
    if constexpr (kCausal)
        for (int c = L + t; c < seq; c += kDecThreads) S[c] = 0.0f;  // P = +0 at the masked keys

    // ---- O[i] = p V over every key: lane = output column, the accumulator carried across the chunks in key order
    float acc = 0.0f;
    auto v_step = [&](float4 (&pf)[kDecPer], int c) __attribute__((always_inline)) {
        if constexpr (kIndirect) slabs_g(nck + c + 2);
        __syncthreads();  // P complete (c = 0) / the previous chunk consumed
        put(pf, c * kDecChunk);
        __syncthreads();
        fetch_g(pf, nck + c + 2);
        if (wave == 0) {
            const int k0 = c * kDecChunk, kn = min(kDecChunk, seq - k0);
            const float *vcol = KV + lane, *prow = S + k0;
            // (reading group g + 1's operands under group g's fmafs, 16 keys a group, measured no faster: 117.5 against
            // 112.2 us at 4096 keys, and 254 VGPRs against 176)
            int k = 0;
            for (; k + 8 <= kn; k += 8) {
                const float4 p0 = *reinterpret_cast<const float4 *>(prow + k);
                const float4 p1 = *reinterpret_cast<const float4 *>(prow + k + 4);
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = vcol[(k + u) * kDecStride];
                acc = fmaf(p0.x, v[0], acc);
                acc = fmaf(p0.y, v[1], acc);
                acc = fmaf(p0.z, v[2], acc);
                acc = fmaf(p0.w, v[3], acc);
                acc = fmaf(p1.x, v[4], acc);
                acc = fmaf(p1.y, v[5], acc);
                acc = fmaf(p1.z, v[6], acc);
                acc = fmaf(p1.w, v[7], acc);
            }
            for (; k < kn; ++k) acc = fmaf(prow[k], vcol[k * kDecStride], acc);
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
    if (wave == 0 && lane < dk) {
        if (seq & 31) acc = __fadd_rn(acc, 0.0f);  // the zero-padded rest of the last 32-key tile: -0 becomes +0
        O[qi * ldo + (int64_t)h * dk + lane] = acc;
    }
}

}  // namespace

bool attention_decode_ok(int seq_q, int seq_kv, int dk) {
    return seq_q <= kAttnDecodeMaxQ && seq_kv <= kDecMaxSeq && dk <= kDecMaxDk;
}

hipError_t launch_attention_decode(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                                   float *O, int64_t ldo, int seq_q, int seq_kv, int n_heads, int dk, float scale,
                                   int q_pos0, hipStream_t stream) {
    if (n_heads < 1 || dk < 1 || seq_q < 0 || seq_kv < 1 || q_pos0 < kNoMask) return hipErrorInvalidValue;
    if (!attention_decode_ok(seq_q, seq_kv, dk)) return hipErrorNotSupported;
    if (seq_q == 0) return hipSuccess;
    const dim3 grid((unsigned)n_heads, (unsigned)seq_q);
    if (q_pos0 == kNoMask)
        attention_decode_kernel<false, DecodeOne><<<grid, kDecThreads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, O, ldo, dk,
                                                                                    scale, DecodeOne{seq_kv, 0});
    else  // past seq_kv - 1 the mask hides nothing: clamped, so the kernel's row limit cannot overflow
        attention_decode_kernel<true, DecodeOne><<<grid, kDecThreads, 0, stream>>>(
            Q, ldq, K, ldk, V, ldv, O, ldo, dk, scale, DecodeOne{seq_kv, q_pos0 < seq_kv ? q_pos0 : seq_kv});
    return hipGetLastError();
}

// tab: checked and clamped by launch_attention_batched (attention_launch.hip); the envelope is tested again here,
// where the kernel's LDS arrays and grid are sized
hipError_t launch_attention_decode_batched(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                           const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                           int n_seqs, int rows_per_seq, const DecodeBatchTable &tab, bool causal,
                                           int n_heads, int dk, float scale, hipStream_t stream) {
    if (n_seqs < 1 || n_seqs > kDecodeMaxBatch || rows_per_seq < 1 || rows_per_seq > kAttnDecodeMaxQ || dk < 1 ||
        dk > kDecMaxDk || n_heads < 1)
        return hipErrorInvalidValue;
    for (int b = 0; b < n_seqs; ++b)
        if (tab.seq_kv[b] < 1 || tab.seq_kv[b] > kDecMaxSeq || tab.kv_slot[b] < 0 || tab.q_pos0[b] < 0 ||
            tab.q_pos0[b] > tab.seq_kv[b])
            return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_heads, (unsigned)rows_per_seq, (unsigned)n_seqs);
    const DecodeMany many{k_stride_seq, v_stride_seq, rows_per_seq, tab};
    if (causal)
        attention_decode_kernel<true, DecodeMany><<<grid, kDecThreads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, O, ldo, dk,
                                                                                    scale, many);
    else
        attention_decode_kernel<false, DecodeMany><<<grid, kDecThreads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, O, ldo, dk,
                                                                                     scale, many);
    return hipGetLastError();
}

// tab (kv_slot = the table row) checked and clamped by launch_attention_indirect (attention_launch.hip); what sizes
// the kernel's LDS arrays and grid, and what keeps every table read inside the table, is tested again here
hipError_t launch_attention_decode_indirect(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                            const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                            int n_seqs, int rows_per_seq, const uint8_t *row_slab,
                                            int64_t row_slab_stride, int n_slabs, const DecodeBatchTable &tab,
                                            bool causal, int n_heads, int dk, float scale, hipStream_t stream) {
    if (n_seqs < 1 || n_seqs > kDecodeMaxBatch || rows_per_seq < 1 || rows_per_seq > kAttnDecodeMaxQ || dk < 1 ||
        dk > kDecMaxDk || n_heads < 1 || !row_slab || n_slabs < 1 || n_slabs > kDecodeMaxBatch)
        return hipErrorInvalidValue;
    for (int b = 0; b < n_seqs; ++b)
        if (tab.seq_kv[b] < 1 || tab.seq_kv[b] > kDecMaxSeq || tab.kv_slot[b] < 0 || tab.q_pos0[b] < 0 ||
            tab.q_pos0[b] > tab.seq_kv[b] || row_slab_stride < tab.seq_kv[b])
            return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_heads, (unsigned)rows_per_seq, (unsigned)n_seqs);
    const DecodeIndirect ind{k_stride_seq, v_stride_seq, rows_per_seq, n_slabs, row_slab, row_slab_stride, tab};
    if (causal)
        attention_decode_kernel<true, DecodeIndirect><<<grid, kDecThreads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, O, ldo,
                                                                                        dk, scale, ind);
    else
        attention_decode_kernel<false, DecodeIndirect><<<grid, kDecThreads, 0, stream>>>(Q, ldq, K, ldk, V, ldv, O, ldo,
                                                                                         dk, scale, ind);
    return hipGetLastError();
}

}  // namespace qgemm
