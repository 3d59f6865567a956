// qgemm_internal.h -- shared definitions of the gfx950 quantized-GEMM kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace qgemm {

// Packed operand geometry (include/qgemm.h): rows padded to the GEMM macro-tile, k to its k-step.
constexpr int kRowPad = 256;
constexpr int kKPad = 128;

__host__ __device__ inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// Column-absmax partials: pack_cols' pass 1 reduces chunks of kColChunk rows (k >= 1) and writes one
// partial per (chunk, column); pass 2 reduces the partials.  No atomics, nothing to zero per call.
constexpr int kColChunk = 256;
__host__ __device__ inline int64_t colmax_parts(int64_t k) { return k > 1 ? (k - 1 + kColChunk - 1) / kColChunk : 1; }

// Layout of one packed operand buffer:
//   [scale: rows_pad f32][scratch: parts x rows_pad u32][q: rows_pad x k_pad i8, FRAGMENT-MAJOR]
// The scratch holds pack_cols' column-absmax partials (pass 1 -> pass 2).
//
// q is stored fragment-major: 1-KiB blocks of 16 packed rows x 64 k-bytes, block (rg, kb) at byte
// (rg * (k_pad / 64) + kb) * 1024, and inside a block the bytes in the lane order of one
// v_mfma_i32_16x16x64_i8 operand: lane l = 16 kc + r holds row 16 rg + r, k = 64 kb + 16 kc .. +15.  So a
// GEMM wave loads a whole MFMA fragment as ONE contiguous 1-KiB buffer_load_dwordx4 (gemm_i8_f4), and
// an LDS-DMA piece is one block (no source swizzle, conflict-free fragment reads).  Any 4-byte group
// k .. k+3 with k % 4 == 0 (and any aligned 16-byte group) of one row stays contiguous.
__host__ __device__ inline int64_t fofs(int64_t row, int64_t k, int64_t k_pad) {
    return ((row >> 4) * (k_pad >> 6) + (k >> 6)) * 1024 + ((((k >> 4) & 3) << 4) + (row & 15)) * 16 + (k & 15);
}
struct PackedView {
    float *scale;       // rows_pad floats (Cx or Cw)
    uint32_t *scratch;  // parts x rows_pad words
    int8_t *q;          // rows_pad x k_pad
    int64_t rows_pad, k_pad, parts;
};

inline PackedView packed_view(const void *base, int rows, int k) {
    PackedView v;
    v.rows_pad = round_up(rows, kRowPad);
    v.k_pad = round_up(k, kKPad);
    v.parts = colmax_parts(k);
    char *p = static_cast<char *>(const_cast<void *>(base));
    v.scale = reinterpret_cast<float *>(p);
    v.scratch = reinterpret_cast<uint32_t *>(p + v.rows_pad * 4);
    v.q = reinterpret_cast<int8_t *>(p + round_up(v.rows_pad * 4 * (1 + v.parts), 256));
    return v;
}

inline size_t packed_bytes(int rows, int k) {
    const int64_t rp = round_up(rows, kRowPad);
    return (size_t)round_up(rp * 4 * (1 + colmax_parts(k)), 256) + (size_t)rp * round_up(k, kKPad);
}

// the dword of packed row `row` holding k .. k+3 (k % 4 == 0)
__device__ __forceinline__ uint32_t *qword(int8_t *q, int64_t row, int64_t k, int64_t k_pad) {
    return reinterpret_cast<uint32_t *>(q + fofs(row, k, k_pad));
}
// zero packed rows [r0, r0 + nrows) over all k_pad bytes, 16 B per thread-step (threads t of nt)
__device__ __forceinline__ void zero_packed_rows(int8_t *q, int64_t r0, int nrows, int64_t k_pad, int t, int nt) {
    const int64_t per = k_pad >> 4;
    for (int64_t i = t; i < (int64_t)nrows * per; i += nt)
        *reinterpret_cast<uint4 *>(q + fofs(r0 + i / per, (i % per) << 4, k_pad)) = make_uint4(0, 0, 0, 0);
}

// ---- the reference's per-element arithmetic, pinned to single IEEE operations ----------------

// AbsMaxFunc (op_reduction.cuh:11-24) on an element that is not the seed: |x|, skipping NaN.
// Returned as a candidate for a running maximum started at -inf; the caller combines candidates
// with strict ">" so NaN never enters.
__device__ __forceinline__ float absmax_candidate(float x) { return fabsf(x); }

// Final combine with the signed seed (the reduction kernels' first element, op_reduction.cuh:80/105):
// acc = seed; if (p > acc) acc = p.  A NaN seed sticks, exactly as in the sequential functor.
__device__ __forceinline__ float absmax_finish(float seed, float p) { return (p > seed) ? p : seed; }

// InvDivideConstFunc (op_elemwise.cuh:131-143): correctly rounded range / C.
__device__ __forceinline__ float inv_divide(float range, float c) { return __fdiv_rn(range, c); }

// MultiplyWithTypecastFunc<float,int8_t> (op_elemwise.cuh:106-114): static_cast<int8_t>(x*s),
// truncation toward zero; saturation and NaN->0 where C++ leaves the cast undefined.
// v_cvt_i32_f32 truncates toward zero, turns NaN into 0 and saturates out-of-range values, so
// after the clamp (v_med3_i32) this equals clamping the float first: 3 VALU per element.
__device__ __forceinline__ int quant_i8(float x, float s) {
    const float v = __fmul_rn(x, s);
    int i;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(i) : "v"(v));
    return min(max(i, -128), 127);
}

// op_mm(Cx, Cw) with K = 1 (op_mm.cuh:96-97): res = 0; res += Cx*Cw -> fl(Cx*Cw) + 0 (turns -0 into +0).
__device__ __forceinline__ float outer_product(float cx, float cw) { return __fadd_rn(__fmul_rn(cx, cw), 0.0f); }

// op_dequantize (DequantizeFunc, op_elemwise.cuh:93-103) then op_multiply(O, 1/(range*range))
// (op_mm.cuh:99): two separate launches in the reference, so two roundings, no contraction.
__device__ __forceinline__ float dequantize(int acc, float outer, float inv_r2) {
    return __fmul_rn(__fmul_rn((float)acc, outer), inv_r2);
}

// fl(1 / range) of the prepacked weight's dequantization: qgemm_linear_outlier takes weights packed with range 127
constexpr float kInvRange127 = 1.0f / 127.0f;
// Wd of one cached weight byte: two separate roundings (-ffp-contract=off)
__device__ __forceinline__ float dequant_w(int8_t q, float cw) {
    return __fmul_rn(__fmul_rn((float)(int)q, cw), kInvRange127);
}

// The running value of the lane to the LEFT (DPP wave_ror:1: lane l reads lane l - 1, lane 0 reads lane 63),
// for sequential fp32 sums that hop from lane to lane (encoder_ops.hip lane_chain_sum, attention.hip).  With
// old = 0 and bound_ctrl set, hipcc folds the move into the consuming v_add_f32 (v_add_f32_dpp).
__device__ __forceinline__ float hop_left(float s) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x13C /* wave_ror:1 */, 0xf, 0xf, true));
}

// The softmax's max and exp steps (op_multiply by `scale` + op_softmax, attention.cuh:65-68, op_softmax.cuh:13-24), the
// numerics contract of softmax_rows_kernel, attention_fused_kernel and attention_decode_kernel, whose results are
// bit-identical because they share it:
//   * every score enters as fl(s * scale);
//   * the maximum is seeded by element 0 and updated by "if (x > max) max = x" with a strict >, so a NaN never wins
//     and a NaN seed sticks;
//   * the exponential is the correctly rounded fp32 exp of fl(fl(s * scale) - max): fl32(exp((double)x)).
// softmax_row_max: this lane's candidates row[first], row[first + stride], .. below w, from -inf, reduced over the 64
// lanes of the wave.  `first` skips element 0: the caller combines the result with its seed fl(row[0] * scale),
// (cand > seed) ? cand : seed -- after combining the waves' results the same way where a row spans several.
__device__ __forceinline__ float softmax_row_max(const float *row, int first, int w, int stride, float scale) {
    float cand = -INFINITY;
    for (int c = first; c < w; c += stride) {
        const float x = __fmul_rn(row[c], scale);  // op_multiply(QK_T, scale_factor) (attention.cuh:65)
        cand = (x > cand) ? x : cand;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(cand, off, 64);
        cand = (o > cand) ? o : cand;
    }
    return cand;
}
__device__ __forceinline__ float softmax_exp(float s, float scale, float mx) {
    return (float)exp((double)__fsub_rn(__fmul_rn(s, scale), mx));
}

// Counter-based generator shared with oracle_uniform_at (oracle/qgemm_oracle.c).
__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// ---- bf16 activations (qgemm_*_dt, include/qgemm.h QGEMM_BF16) ------------------------------------
// A bf16 element as stored: the upper half of the fp32 with the same value.  Widening is exact (the bits shifted
// left by 16, subnormals included), so a bf16 X is packed as the fp32 chain packs the widened matrix.
struct bf16_t {
    uint16_t bits;
};
__host__ __device__ inline float widen(float x) { return x; }
__device__ __forceinline__ float widen(bf16_t x) { return __uint_as_float((uint32_t)x.bits << 16); }

// Two fp32 values -> one dword of two bf16 (`lo` in the low half), each rounded to nearest even: one
// v_cvt_pk_bf16_f32.  Past the bf16 maximum it gives +-inf; subnormals stay subnormal (the kernels run with
// denormals on), -0 stays -0 and NaN stays NaN (tests/test_gpu_bf16.py checks each on the device).
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// ---- the outlier column mask (outlier.hip writes it, pack.hip and outlier.hip read it) -------------
// outlier_colmask_kernel writes the mask as nparts partial masks (partial[p][w] for row split p, every word written
// each call, so no state lives on between calls; nparts = 2 at K = 4096): word w = OR over p, bit c of word w = feature
// column 32 w + c.  The partial words come from an earlier launch in the stream: plain loads.
struct OutlierMask {
    const uint32_t *partial;  // nparts x nwords partial mask words (bit 0 of word 0: column 0, the absmax seed)
    int nwords, nparts;
    int *idx;                 // out: [count][columns ascending]
    // mask words w[j] (0 where w[j] >= nwords): the ORs of their nparts partial words -- every load of split 0 issued
    // before any is waited for (nparts is 1 or 2 on the shapes the benchmarks run)
    template <int NW>
    __device__ __forceinline__ void words(const int (&w)[NW], uint32_t (&out)[NW]) const {
#pragma unroll
        for (int j = 0; j < NW; ++j) out[j] = w[j] < nwords ? partial[w[j]] : 0u;
        for (int p = 1; p < nparts; ++p)
#pragma unroll
            for (int j = 0; j < NW; ++j) out[j] |= w[j] < nwords ? partial[p * nwords + w[j]] : 0u;
    }
    __device__ __forceinline__ uint32_t word(int w) const {
        const int ws[1] = {w};
        uint32_t x[1];
        words(ws, x);
        return x[0];
    }
};
// The one list builder, run by ONE workgroup (workgroup 0 of the masked packs, or outlier_index_kernel): idx[0] = the
// number of outlier columns, idx[1 ..] = them ascending -- a wave scan of the words' popcounts + the wave sums in
// wsum (LDS, blockDim / 64 ints).  kAnyWords = false: nwords <= blockDim, one pass, nothing else written (the packs).
// kAnyWords = true: passes of blockDim words over a running base, and bits[w] = mask word w for every w < nwords.
template <bool kAnyWords = false>
__device__ __forceinline__ void outlier_column_list(const OutlierMask &om, int *wsum, uint32_t *bits = nullptr) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwave = blockDim.x >> 6;
    int w0 = 0, total = 0;  // uniform: every thread makes every pass (the barriers)
    do {
        const int w = w0 + t;
        const uint32_t word = w < om.nwords ? om.word(w) : 0u;
        const int pc = __popc(word);
        int x = pc;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(x, off, 64);
            if (lane >= off) x += v;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int below = x - pc, sum = 0;
        for (int j = 0; j < nwave; ++j) {
            below += j < wave ? wsum[j] : 0;
            sum += wsum[j];
        }
        if constexpr (kAnyWords) below += total;  // the columns of the passes before this one
        total += sum;
        int j = 0;
        for (uint32_t b = word; b; b &= b - 1, ++j) om.idx[1 + below + j] = 32 * w + __builtin_ctz(b);
        if constexpr (kAnyWords) {
            if (w < om.nwords) bits[w] = word;
            __syncthreads();  // wsum is rewritten by the next pass
        }
    } while (kAnyWords && (w0 += blockDim.x) < om.nwords);
    if (t == 0) om.idx[0] = total;
}

// ---- launchers (defined in the .hip files) ------------------------------------------------------
hipError_t launch_pack_rows(const float *src, int64_t sh, int64_t sw, int rows, int len, float range,
                            PackedView out, hipStream_t stream);
// the same from a bf16 source (strides in bf16 elements): its own alignment rule and length limits (pack.hip)
hipError_t launch_pack_rows(const bf16_t *src, int64_t sh, int64_t sw, int rows, int len, float range,
                            PackedView out, hipStream_t stream);
hipError_t launch_pack_cols(const float *src, int64_t sh, int len, int cols, float range, PackedView out,
                            hipStream_t stream);
// The two-pass pack of a row-major A and B (B's columns reduced in pass 1, quantized in pass 2; A's rows in one of
// the passes): long rows (4096 < K <= 16384) as a W-only pass 1 + pass 2 with A's rows at its end, shorter rows as
// launch_pack_rows_and_colmax + launch_pack_cols_pass2.  hipErrorNotSupported when the layouts do not allow it.
hipError_t launch_pack_two_pass(const float *a, int64_t ash, int m, int k, PackedView outa, const float *b, int64_t bsh,
                                int n, PackedView outb, float range, hipStream_t stream, uint32_t *zero_words = nullptr,
                                int nzero = 0);
// One launch: pack_rows of a row-major A (vector path) and pass 1 of pack_cols of a row-major B.
// Returns hipErrorNotSupported when the layouts do not allow it (caller falls back).
hipError_t launch_pack_rows_and_colmax(const float *a, int64_t ash, int m, int k, PackedView outa, const float *b,
                                       int64_t bsh, int n, PackedView outb, float range, hipStream_t stream,
                                       uint32_t *zero_words = nullptr, int nzero = 0);
// One launch, W read once: single-pass W strips (K <= 4096, n % 8 == 0: 8-column strips at two blocks
// per CU, or 16-column strips) + X rows.  hipErrorNotSupported when the shape/layout is outside that
// (caller falls back).
// zero_words/nzero: words zeroed by block 0 of the launch (the GEMM's split-K tickets)
hipError_t launch_pack_single_pass(const float *x, int64_t xsh, int m, int k, PackedView outx, const float *w,
                                   int64_t wsh, int n, PackedView outw, float range, hipStream_t stream,
                                   uint32_t *zero_words = nullptr, int nzero = 0);
// kind 8 / 16 forces the strip width (lab); 0 chooses.
hipError_t launch_pack_single_pass_kind(const float *x, int64_t xsh, int m, int k, PackedView outx, const float *w,
                                        int64_t wsh, int n, PackedView outw, float range, hipStream_t stream, int kind,
                                        uint32_t *zero_words = nullptr, int nzero = 0);
// The single-pass pack (8-column W strips) of the LLM.int8() decomposition's int8 part: outlier columns
// of X / rows of W packed as +0 (the mask = OR of the column-mask launch's nparts x nwords partial words partial[p][w],
// bit c of word w = column 32 w + c); workgroup 0 writes idx[0] = the outlier count, idx[1 ..] = the columns
// ascending.  hipErrorNotSupported outside the single pass's envelope (K % 4 == 0 too) or for nparts > 16 (nothing
// launched).
bool pack_single_pass_outlier_ok(const float *x, int64_t xsh, int m, int k, const float *w, int64_t wsh, int n);
hipError_t launch_pack_single_pass_outlier(const float *x, int64_t xsh, int m, int k, PackedView outx, const float *w,
                                           int64_t wsh, int n, PackedView outw, float range, const uint32_t *partial,
                                           int nparts, int nwords, int *idx, hipStream_t stream);
// The X role of that pack alone, for a weight packed beforehand (qgemm_linear_outlier): X's rows (row stride xsh)
// packed with the outlier columns as +0, the register-resident row kernel chosen by row length as launch_pack_rows
// does; workgroup 0 writes idx[0] = the outlier count, idx[1 ..] = the columns ascending.  Envelope: K % 4 == 0,
// K <= 4096, 16-B aligned rows, nwords <= 128, nparts <= 16; hipErrorNotSupported outside it (nothing launched).
bool pack_rows_outlier_ok(const float *x, int64_t xsh, int m, int k);
hipError_t launch_pack_rows_outlier(const float *x, int64_t xsh, int m, int k, PackedView outx, float range,
                                    const uint32_t *partial, int nparts, int nwords, int *idx, hipStream_t stream);
hipError_t launch_pack_cols_pass2(const float *src, int64_t sh, int len, int cols, float range, PackedView out,
                                  hipStream_t stream);
hipError_t launch_fill_uniform(float *dst, int64_t count, uint64_t seed, float lo, float hi, hipStream_t stream);
// Split-K for shapes with too few 256x256 tiles to fill the chip: gemm_splits() slices per tile and
// the scratch (tickets + int32 slabs) they need; 1 / 0 when the shape is not split.
int gemm_splits(int m, int n, int k);
// the plan's tile edge and kernel name (qgemm_gemm_plan); returns the splits
int gemm_plan_info(int m, int n, int k, int *tile, const char **kernel);
size_t gemm_scratch_bytes(int m, int n, int k);
// scratch: gemm_scratch_bytes(m, n, k) bytes, or nullptr (then no split: correct, slower)
// bias (n floats) != nullptr: y = fl(O + b[j]) (+ relu): the encoder's linear layers.
// tickets_zeroed: the split-K scratch is library-owned, zeroed once at allocation; the launch's
// reducers re-zero their tickets instead of a memset ahead of every launch.
// bytes at the start of the split-K scratch that must be zero before a split launch (0: no split)
size_t gemm_ticket_bytes(int m, int n, int k);
// c_bf16: C holds bf16 (csh / csw in bf16 elements): the fp32 value the epilogue would store, rounded once (pk_bf16)
hipError_t launch_gemm_dequant(const PackedView &a, const PackedView &b, void *C, int64_t csh, int64_t csw,
                               int m, int n, float inv_r2, void *scratch, size_t scratch_bytes, hipStream_t stream,
                               const float *bias = nullptr, bool relu = false, bool tickets_zeroed = false,
                               bool c_bf16 = false);
// The LLM.int8() decomposition's GEMM: int8 part + the outlier columns' fp32 products in the epilogue, read from
// X (m x k, row stride xsh) and W (k x n, row stride wsh) at the columns / rows ocols[0 .. *ocount) (ascending).
// Only where the plan is the 256-tile GEMM without split-K (gemm_outlier_ok); hipErrorNotSupported otherwise.
bool gemm_outlier_ok(int m, int n, int k);
hipError_t launch_gemm_dequant_outlier(const PackedView &a, const PackedView &b, float *C, int64_t csh, int m, int n,
                                       float inv_r2, const float *x, int64_t xsh, const float *w, int64_t wsh,
                                       const int *ocols, const int *ocount, hipStream_t stream);
// The same for a prepacked weight b: the chain's W operands are b's own bytes dequantized (fl(fl(q * Cw) * fl(1/127)),
// range 127), and bias (n floats, or nullptr) / relu follow the add of the chain.
hipError_t launch_gemm_dequant_outlier_q(const PackedView &a, const PackedView &b, float *C, int64_t csh, int m, int n,
                                         float inv_r2, const float *x, int64_t xsh, const int *ocols, const int *ocount,
                                         const float *bias, bool relu, hipStream_t stream);
hipError_t launch_gemm_i32(const PackedView &a, const PackedView &b, int32_t *Acc, int m, int n,
                           hipStream_t stream);
hipError_t launch_mm_f32(const float *A, int64_t ash, int64_t asw, const float *B, int64_t bsh, int64_t bsw, float *C,
                         int64_t csh, int64_t csw, int m, int n, int k, hipStream_t stream);
// The fp32 GEMM's kernel for one call (gemm_f32.hip): the family (LDS-DMA ring or register staging), for the ring
// whether B is k-contiguous, the block's tile, and the stable name qgemm_mm_fp32_plan reports.
struct MmF32Plan {
    bool dma, bkc;
    int tm, tn;
    const char *name;
};
inline bool mm_f32_al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// the one selection rule, read by the launch and by the query; a_al16 / b_al16: the bases are 16-byte aligned
MmF32Plan mm_f32_plan(int m, int n, int k, int batch, int64_t ash, int64_t asw, int64_t a_bs, bool a_al16, int64_t bsh,
                      int64_t bsw, int64_t b_bs, bool b_al16);
// whether plan p's 32-bit tile offsets hold these strides (the envelope at qgemm_mm_fp32, include/qgemm.h);
// launch_mm_f32_batched returns hipErrorInvalidValue before its launch where they do not
bool mm_f32_strides_ok(const MmF32Plan &p, int64_t ash, int64_t asw, int64_t bsh, int64_t bsw, int64_t csh,
                       int64_t csw, int m, int n, int k);
// batch of independent GEMMs (blockIdx.z), operand i at base + i * batch stride (attention heads)
hipError_t launch_mm_f32_batched(const float *A, int64_t ash, int64_t asw, int64_t a_bs, const float *B, int64_t bsh,
                                 int64_t bsw, int64_t b_bs, float *C, int64_t csh, int64_t csw, int64_t c_bs, int m,
                                 int n, int k, int batch, hipStream_t stream);
// Encoder row ops (encoder_ops.hip): the reference's op_softmax (after op_multiply by `scale`) and
// op_add + op_layernorm, one row per wave, sums in the reference's sequential order.
// S = QK^T, softmax(S * scale), O = PV for every head in one launch (S in LDS), bit-identical to
// the three separate kernels; hipErrorNotSupported outside attention_fused_ok (d_k <= 64, seq_kv <= 512).
// Q, O: seq_q rows; K, V: seq_kv rows; row strides ld* in floats, unit inner stride, head h at columns
// h*d_k .. of each matrix.  O must not overlap Q, K or V.
// q_pos0: kNoMask, or the key position of query row 0 for the causal mask (>= 0): row i sees keys
// 0 .. min(seq_kv, i + q_pos0 + 1) - 1, its softmax runs over those columns alone and P is +0 past them.
constexpr int kNoMask = -1;
bool attention_fused_ok(int seq_kv, int dk);
hipError_t launch_attention_fused(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                                  float *O, int64_t ldo, int seq_q, int seq_kv, int n_heads, int dk, float scale,
                                  int q_pos0, hipStream_t stream);
// The launch for a few query rows against up to 4096 keys (attention_decode.hip): one workgroup per (head, query
// row), the same bits; hipErrorNotSupported outside attention_decode_ok (seq_q <= 8, seq_kv <= 4096, d_k <= 64).
bool attention_decode_ok(int seq_q, int seq_kv, int dk);
hipError_t launch_attention_decode(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                                   float *O, int64_t ldo, int seq_q, int seq_kv, int n_heads, int dk, float scale,
                                   int q_pos0, hipStream_t stream);
// The decode launch for a batch of independent sequences (attention_decode_kernel<., DecodeMany>): grid
// (heads, rows per sequence, sequences); sequence b's query / output rows are b * rows_per_seq .., its K / V rows the
// slab at K / V + kv_slot[b] * k / v_stride_seq, seq_kv[b] keys, mask offset q_pos0[b].  The table is a kernel argument
// passed by value (768 bytes): filled on the host at enqueue time, never in device memory.
constexpr int kDecodeMaxBatch = 64;
struct DecodeBatchTable {
    int kv_slot[kDecodeMaxBatch], seq_kv[kDecodeMaxBatch], q_pos0[kDecodeMaxBatch];
};
// tab already checked and clamped (q_pos0[b] <= seq_kv[b]); causal = false ignores q_pos0
hipError_t launch_attention_decode_batched(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                           const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                           int n_seqs, int rows_per_seq, const DecodeBatchTable &tab, bool causal,
                                           int n_heads, int dk, float scale, hipStream_t stream);
// The batched launch through a per-row slab table (attention_decode_kernel<., DecodeIndirect>): K / V
// row j of sequence b is row j of slab row_slab[tab.kv_slot[b] * row_slab_stride + j] -- tab.kv_slot holds the
// sequence's table ROW here -- row_slab a uint8 array in device memory, any alignment; an entry >= n_slabs reads as a
// row of quiet NaNs and forms no address outside the slabs.  tab already checked and clamped.
hipError_t launch_attention_decode_indirect(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                            const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo,
                                            int n_seqs, int rows_per_seq, const uint8_t *row_slab,
                                            int64_t row_slab_stride, int n_slabs, const DecodeBatchTable &tab,
                                            bool causal, int n_heads, int dk, float scale, hipStream_t stream);
// The fused launch over a table of independent sequences of their own lengths (attention_fused_kernel<., FusedMany>,
// DESIGN.md s19): sequence b has seq_q[b] query / output rows from row q_row0[b] of Q / O, seq_kv[b] keys from row
// kv_row0[b] of K / V and mask offset q_pos0[b]; item0 is the work map, the first workgroup of each sequence, filled
// by launch_attention_fused_many.  A kernel argument passed by value (2056 bytes): filled on the host at enqueue time,
// never in device memory.
constexpr int kVarlenMaxSeqs = 64;
struct FusedSeqTable {
    int64_t q_row0[kVarlenMaxSeqs], kv_row0[kVarlenMaxSeqs];
    int seq_q[kVarlenMaxSeqs], seq_kv[kVarlenMaxSeqs], q_pos0[kVarlenMaxSeqs], item0[kVarlenMaxSeqs + 1];
};
// tab already checked and clamped (every seq_kv[b] <= 512, q_pos0[b] <= seq_kv[b]); causal = false ignores q_pos0;
// sequences with seq_q[b] == 0 get no workgroup
hipError_t launch_attention_fused_many(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V,
                                       int64_t ldv, float *O, int64_t ldo, int n_seqs, const FusedSeqTable &tab,
                                       bool causal, int n_heads, int dk, float scale, hipStream_t stream);
// Attention dispatch (attention_launch.hip).
// Many sequences of different lengths from host arrays of n_seqs entries (q_pos0 nullptr: no mask), read at enqueue
// time: ONE launch_attention_fused_many where d_k <= 64 and every seq_kv[b] <= 512, else launch_attention sequence by
// sequence in order through `scores` (the largest n_heads x seq_q[b] x seq_kv[b] floats of a sequence outside the
// fused envelope).  hipErrorInvalidValue before any launch outside 0 <= n_seqs <= 64, row offsets >= 0, seq_q[b] >= 0,
// 1 <= seq_kv[b] <= 4096, q_pos0[b] >= 0, n_heads, d_k >= 1.  Sequence b's rows of O are launch_attention's on its views.
const char *attention_varlen_plan_name(int n_seqs, const int *seq_kv, int dk);
hipError_t launch_attention_varlen(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                                   float *O, int64_t ldo, int n_seqs, const int64_t *q_row0, const int *seq_q,
                                   const int64_t *kv_row0, const int *seq_kv, const int *q_pos0, int n_heads, int dk,
                                   float scale, float *scores, hipStream_t stream);
// the batched decode launch from host arrays of n_seqs entries (kv_slot nullptr: 0, 1, 2, ..; q_pos0 nullptr: no mask):
// hipErrorInvalidValue before any launch outside n_seqs <= 64, 1 <= rows_per_seq <= 8, 1 <= d_k <= 64,
// 1 <= seq_kv[b] <= 4096, q_pos0[b] >= 0, kv_slot[b] >= 0; n_seqs == 0 launches nothing
hipError_t launch_attention_batched(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                    const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo, int n_seqs,
                                    int rows_per_seq, const int *kv_slot, const int *seq_kv, const int *q_pos0,
                                    int n_heads, int dk, float scale, hipStream_t stream);
// the indirect launch from host arrays (tab_row nullptr: 0, 1, 2, ..): launch_attention_batched's checks, and a null
// table, n_slabs < 1 or > 64, row_slab_stride < seq_kv[b], tab_row[b] < 0
hipError_t launch_attention_indirect(const float *Q, int64_t ldq, const float *K, int64_t ldk, int64_t k_stride_seq,
                                     const float *V, int64_t ldv, int64_t v_stride_seq, float *O, int64_t ldo, int n_seqs,
                                     int rows_per_seq, const uint8_t *row_slab, int64_t row_slab_stride, int n_slabs,
                                     const int *tab_row, const int *seq_kv, const int *q_pos0, int n_heads, int dk,
                                     float scale, hipStream_t stream);
// the kernel launch_attention takes for a shape (qgemm_attention_plan): a static string
const char *attention_plan_name(int seq_q, int seq_kv, int dk);
// whether a call of at most max_q query rows and max_kv keys can reach the three launches, and so needs `scores`
bool attention_needs_scores(int max_q, int max_kv, int dk);
// The decode launch for seq_q <= 8, else the fused launch where it fits, else launch_mm_f32_batched + launch_softmax_rows[_causal] + launch_mm_f32_batched
// through scores (n_heads x seq_q x seq_kv floats; may be nullptr inside the other two envelopes; seq_kv <= 4096).
hipError_t launch_attention(const float *Q, int64_t ldq, const float *K, int64_t ldk, const float *V, int64_t ldv,
                            float *O, int64_t ldo, int seq_q, int seq_kv, int n_heads, int dk, float scale, int q_pos0,
                            float *scores, hipStream_t stream);
hipError_t launch_softmax_rows(const float *S, float *P, int64_t rows, int w, float scale, hipStream_t stream);
// the same on a stack of rows / seq_q matrices under the causal mask: row r is query i = r % seq_q and its softmax
// runs over its first min(w, i + q_pos0 + 1) columns, +0 stored past them (P may be S)
hipError_t launch_softmax_rows_causal(const float *S, float *P, int64_t rows, int w, float scale, int seq_q,
                                      int q_pos0, hipStream_t stream);
hipError_t launch_add_layernorm_rows(const float *A, const float *B, float *Y, int64_t rows, int w,
                                     hipStream_t stream);
// the same, also writing Y's rows packed (Cx + int8) for the next quantized linear (pack_rows fused)
hipError_t launch_add_layernorm_rows_pack(const float *A, const float *B, float *Y, int64_t rows, int w, float range,
                                          PackedView out, hipStream_t stream);
// LLM.int8() outlier decomposition (outlier.hip).
// The scratch of a call with an fp32 W (qgemm_mm_outlier), and of one on a PREPACKED weight (qgemm_linear_outlier):
// the same without the W' slot.
size_t outlier_scratch_bytes(int m, int n, int k);
size_t outlier_linear_scratch_bytes(int m, int k);
int outlier_count_slot(const void *scratch, int *count_host);
// Fast paths into the packed views va / vb; hipErrorNotSupported (nothing launched) outside their envelopes.
// outlier_fast (row-major fp32 operands): column mask, masked single-pass pack, the 256-tile GEMM with the fp32 chain
// in its epilogue.  outlier_linear_fast: column mask, masked X-only pack into va, the 256-tile GEMM with the chain on
// vb's dequantized rows (+ bias / relu) in its epilogue.
hipError_t outlier_fast(const float *X, const float *W, float *O, int m, int n, int k, float t, void *scratch,
                        PackedView va, PackedView vb, float range, hipStream_t s);
hipError_t outlier_linear_fast(const float *X, int64_t xsh, int m, int n, int k, float t, void *scratch, PackedView va,
                               PackedView vb, const float *bias, bool relu, float *Y, int64_t ysh, hipStream_t s);
// Fallback: outlier_prepare (column mask, index, X' and -- where W != nullptr -- W' into the scratch; Wm may be
// nullptr without a W), the caller's plain chain on them without bias, then outlier_finish: the chain on W's rows
// (W != nullptr) or on the packed weight vb's dequantized rows added to O, then bias / relu.
hipError_t outlier_prepare(const float *X, int64_t xsh, const float *W, int64_t wsh, int m, int n, int k, float t,
                           void *scratch, float **Xm, float **Wm, hipStream_t s);
hipError_t outlier_finish(const float *X, int64_t xsh, const float *W, int64_t wsh, const PackedView *vb,
                          const float *bias, bool relu, int m, int n, int k, void *scratch, float *O, int64_t osh,
                          hipStream_t s);
// The transformer stack (transformer.hip): an encoder is a stack without cross-attention, a decoder one with it, a
// decoder-only stack (arch bit QGEMM_ARCH_DECODER_ONLY) a handle of the decoder family whose blocks
// are the encoder's.  encoder_forward refuses a handle of the decoder family and decoder_* an encoder
// (hipErrorInvalidValue).  stack_create's `decoder` names the family; without cross-attention enc_out is nullptr and
// enc_seq 0 in decoder_forward / decoder_begin_slot, and begin launches nothing.
struct Stack;
uint64_t encoder_weight_seed(uint64_t base, int block, int kind, int head);
float encoder_init_bound(int n);
// max_enc_seq, causal and kv_cache count only with cross; n_slots (1 .. kDecodeMaxBatch, > 1 only with kv_cache) is
// the number of sequences the caches hold; max_rows (0: none) raises the rows the scratch buffers hold
// for encoder_forward_batch / decoder_step_varlen, refused where a row-local index could leave int32
hipError_t stack_create(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq, uint64_t seed,
                        bool decoder, bool causal, bool kv_cache, Stack **out, int n_slots = 1, int max_rows = 0,
                        int arch = 0, int activation = 0, float ln_eps = 0.0f);
void stack_destroy(Stack *S);
hipError_t encoder_forward(Stack *S, const float *X, float *Y, int seq, hipStream_t s);
// begin / step of one cache slot (qgemm_decoder_begin / qgemm_decoder_step are slot 0's)
hipError_t decoder_begin_slot(Stack *S, int slot, const float *enc_out, int enc_seq, hipStream_t s);
hipError_t decoder_step_slot(Stack *S, int slot, const float *X, float *Y, int pos, int n, hipStream_t s);
// one step of n_seqs sequences, rows_per_seq rows each: rows b * r .. of X / Y at positions pos[b] .. of slot slots[b]
hipError_t decoder_step_batch(Stack *S, int n_seqs, const int *slots, const int *pos, int rows_per_seq, const float *X,
                              float *Y, hipStream_t s);
// n_seqs sequences of seq_lens[b] rows, packed one after another in X / Y: each one's rows are encoder_forward's
hipError_t encoder_forward_batch(Stack *S, const float *X, float *Y, int n_seqs, const int *seq_lens, hipStream_t s);
// step_batch with n_rows[b] >= 1 rows per sequence, rows packed one after another: each one's rows are step_slot's
hipError_t decoder_step_varlen(Stack *S, int n_seqs, const int *slots, const int *pos, const int *n_rows, const float *X,
                               float *Y, hipStream_t s);
hipError_t decoder_copy_slot(Stack *S, int dst, int src, hipStream_t s);
hipError_t decoder_slot_state(const Stack *S, int slot, int *enc_seq, int *filled);
// whether the slot's sequence was begun (begin_slot, copy_slot, beam_begin) and no set_weight came since
bool decoder_slot_begun(const Stack *S, int slot);
// a slot's self slab (max_seq x 3 d_model) / cross slab (max_enc_seq x 2 d_model) of one block, copied out in stream order
hipError_t decoder_read_slot(const Stack *S, int block, int slot, float *self_rows, float *cross_rows, hipStream_t s);
// what a caller that drives step_batch must know to check its arguments before the first launch (head.hip's generate):
// hipErrorInvalidValue for a stack without caches
hipError_t decoder_limits(const Stack *S, int *d_model, int *d_k, int *max_seq, int *n_slots);
hipError_t decoder_forward(Stack *S, const float *X, const float *enc_out, float *Y, int seq, int enc_seq,
                           hipStream_t s);
// draws a k x n fp32 weight into tmp (col_seeds[c] fills columns [c*cols_per_seed, (c+1)*cols_per_seed), one
// reference tensor each, uniform [-bound, bound)) and packs it as B into a fresh allocation; tmp holds
// k * n + k * cols_per_seed floats
hipError_t encoder_make_packed(int k, int n, const std::vector<uint64_t> &col_seeds, int cols_per_seed, float bound,
                               void **packed, float *tmp, hipStream_t s);
const char *gemm_config_name();
// Caller-supplied weights (weights.hip, transformer.hip; the contracts are at qgemm_pack_b_window and
// qgemm_model_set_weight in include/qgemm.h).  dtype: QGEMM_F32 = 0 / QGEMM_BF16 = 1; strides in elements.
// launch_pack_b_window: the k x ncols tensor B into packed rows col0 .. col0 + ncols - 1 of the packed k x n_total
// weight at packed_b, one launch, nothing else in its scale and q regions written; every check of pack_b_window_ok
// and a null destination before the launch.  pack_b_window_path: the source path's stable name.
bool pack_b_window_ok(const void *B, int dtype, int64_t sh, int64_t sw, int k, int n_total, int col0, int ncols);
const char *pack_b_window_path(const void *B, int dtype, int64_t sh, int64_t sw, int ncols);
hipError_t launch_pack_b_window(const void *B, int dtype, int64_t sh, int64_t sw, int k, int n_total, int col0,
                                int ncols, float range, void *packed_b, hipStream_t stream);
// dst[i] = src[i * sw] widened, i < n: a bias from a strided fp32 or bf16 row
hipError_t launch_copy_row(const void *src, int dtype, int64_t sw, int n, float *dst, hipStream_t stream);
// The stack's side (transformer.hip).  kind: 0 .. 7 and, with cross-attention, 8 .. 11 (encoder_weight_seed's);
// which: 0 .. 6 = wqkv, wo, w1, w2 and, with cross-attention, wq2, wkv2, wo2.
hipError_t stack_weight_shape(const Stack *S, int kind, int *rows, int *cols, int *heads);
hipError_t stack_set_weight(Stack *S, int block, int kind, int head, const void *W, int dtype, int64_t sh, int64_t sw,
                            hipStream_t s);
hipError_t stack_packed_weight(const Stack *S, int block, int which, const void **packed, int *n, int *k);
hipError_t stack_bias(const Stack *S, int block, int kind, const float **bias, int *n);
hipError_t stack_rope_tables(const Stack *S, const float **cos_t, const float **sin_t, int *rows, int *half);
// Rotary position embeddings (rope.hip; the contract is at qgemm_rope_rows in include/qgemm.h): every
// check before the one launch; row0 / n_rows / pos0 are host arrays of n_seqs <= kVarlenMaxSeqs entries
hipError_t launch_rope_rows(float *X, int64_t stride, int64_t rows, int groups, int dk, const float *cos_t,
                            const float *sin_t, int table_rows, int pos0, hipStream_t s);
hipError_t launch_rope_rows_varlen(float *X, int64_t stride, int groups, int dk, const float *cos_t, const float *sin_t,
                                   int table_rows, int n_seqs, const int64_t *row0, const int *n_rows, const int *pos0,
                                   hipStream_t s);
// Sampled token choice (sample.hip; the contract is at qgemm_sample_rows in include/qgemm.h).
// sample_plan: the parts a row is cut into and a part's columns, from rows, w and top_k alone; false outside
// rows >= 0, 1 <= w <= 2^24, 1 <= top_k <= 1024.  sample_check: every limit of the contract that needs no pointer.
// launch_sample_rows checks everything before its first launch; counters (host, <= 64 entries) travel by value.
bool sample_plan(int64_t rows, int w, int top_k, int *parts, int *chunk);
size_t sample_ws_bytes(int64_t rows, int w, int top_k);
hipError_t sample_check(int64_t rows, int w, int top_k, float top_p, float temperature, bool has_counters);
hipError_t launch_sample_rows(const float *S, int64_t stride, int64_t rows, int w, int top_k, float top_p,
                              float temperature, uint64_t seed, uint64_t counter0, const uint64_t *counters,
                              const int *prev, int eos, int *idx, int *top_idx, float *top_prob, int *n_kept, void *ws,
                              size_t ws_bytes, hipStream_t s);
// Beam search (beam.hip; the contracts are at qgemm_logsumexp_rows, qgemm_beam_step and
// qgemm_decoder_gather_slots in include/qgemm.h).  The plans need rows, w and beams alone; every launch_* checks
// everything before its first launch.
bool logsumexp_plan(int64_t rows, int w, int *parts, int *bpp);
size_t logsumexp_ws_bytes(int64_t rows, int w);
hipError_t launch_logsumexp_rows(const float *S, int64_t stride, int64_t rows, int w, float *mx, float *logz, void *ws,
                                 size_t ws_bytes, hipStream_t s);
bool beam_step_plan(int n_groups, int beams, int w, int *select_parts, int *lse_parts);
size_t beam_step_ws_bytes(int n_groups, int beams, int w);
hipError_t launch_beam_step(const float *S, int64_t stride, int n_groups, int beams, int w, const float *scores_in,
                            const int *prev, int eos, int *parents, int *tokens, float *scores_out, void *ws,
                            size_t ws_bytes, hipStream_t s);
// one cache (n_slabs slabs of slab_rows x 3 d floats): the [K | V] of rows 0 .. n_rows[g] - 1 of slab
// src_slots[g * beams + parents[g * beams + q]] into slab dst_slots[g * beams + q]; parents on the device, the rest host
hipError_t launch_gather_kv(float *cache, int64_t slab_rows, int n_slabs, int d, int n_groups, int beams,
                            const int *dst_slots, const int *src_slots, const int *n_rows, const int *parents,
                            hipStream_t s);
// the decoder's side of it (transformer.hip): the checks on the slots' state, one launch_gather_kv per block, filled
hipError_t decoder_gather_slots(Stack *S, int n_groups, int beams, const int *dst_slots, const int *src_slots,
                                const int *parents, const int *n_rows, hipStream_t s);
// Copy-free beam search (the contracts are at qgemm_beam_reindex and qgemm_decoder_beam_begin in
// include/qgemm.h).  The table kernels (beam.hip) work on a uint8 table of n_table_rows rows, `stride` bytes apart, and
// take their slots, values and counts from host arrays in the kernel arguments; each checks that every byte it touches
// lies in a named row's first `stride` bytes before its launch.
//   reindex: own[slots[g * beams + q]][j] = old own[slots[g * beams + parents[g * beams + q]]][j], j < n_rows[g], in place
//   fill:    own[slots[i]][first[i] .. first[i] + count[i] - 1] = value[i], i < n
hipError_t launch_beam_reindex(uint8_t *own, int64_t stride, int n_table_rows, int n_groups, int beams, const int *slots,
                               const int *parents, const int *n_rows, hipStream_t s);
hipError_t launch_beam_fill(uint8_t *own, int64_t stride, int n_table_rows, int n, const int *slots, const int *first,
                            const int *count, const int *value, hipStream_t s);
// the decoder's side (transformer.hip): the state checks, the launches, enc_seq / filled / the slots' indirect flag
hipError_t decoder_beam_begin(Stack *S, int n_groups, int beams, const int *slots, const int *src_slots, const int *pos,
                              hipStream_t s);
hipError_t decoder_step_batch_indirect(Stack *S, int n_seqs, const int *slots, const int *cross_slots, const int *pos,
                                       int rows_per_seq, const float *X, float *Y, hipStream_t s);
hipError_t decoder_beam_reindex(Stack *S, int n_groups, int beams, const int *slots, const int *parents,
                                const int *n_rows, hipStream_t s);
hipError_t decoder_read_beam_table(const Stack *S, uint8_t *out, hipStream_t s);
// whether the slot was begun by decoder_beam_begin (its slab does not hold its own sequence); false out of range
bool decoder_slot_indirect(const Stack *S, int slot);
// Quantization-error statistics on the device (error_stats.hip); scratch = error_stats_scratch_bytes().
size_t error_stats_scratch_bytes();
hipError_t launch_error_stats(const float *C, const float *O, int64_t n, bool reference_order, double *stats,
                              void *scratch, hipStream_t stream);

// Diagnostics: events to record exactly around the next GEMM kernel (hipExtLaunchKernelGGL), set
// through qgemm_set_gemm_events() and consumed by one launch.  Thread-local.
struct GemmEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
GemmEvents take_gemm_events();
void set_gemm_events(hipEvent_t start, hipEvent_t stop);
void set_gemm_event_mode(int mode);

// The standard post-LN block (the contracts are at qgemm_layernorm_rows, qgemm_gelu_rows and
// qgemm_model_create in include/qgemm.h).
// norm.hip: Y = LN(A + B) with gamma, beta and eps (B may be nullptr; Y may be A or B), one wave per row, w <= 4096;
// the pack variant also writes Y's rows packed, padding rows and columns included.  Every check before the launch.
hipError_t launch_layernorm_rows(const float *A, const float *B, const float *gamma, const float *beta, float eps,
                                 float *Y, int64_t rows, int w, hipStream_t stream);
hipError_t launch_layernorm_rows_pack(const float *A, const float *B, const float *gamma, const float *beta, float eps,
                                      float *Y, int64_t rows, int w, float range, PackedView out, hipStream_t stream);
// The pre-LN boundary (the contract is at qgemm_prenorm_pack_a in include/qgemm.h), the same kernel's
// norm-first form: S = A + B (B may be nullptr: S = A; S may be nullptr: not stored; S may be A or B), LN(S) written
// only packed.  launch_add_rows: S = A + B alone.
hipError_t launch_prenorm_pack(const float *A, const float *B, const float *gamma, const float *beta, float eps,
                               float *S, int64_t rows, int w, float range, PackedView out, hipStream_t stream);
hipError_t launch_add_rows(const float *A, const float *B, float *S, int64_t rows, int w, hipStream_t stream);
// gelu.hip: the tanh-form GELU elementwise (row strides in floats, unit inner stride), and fused into pack_rows of an
// m x k matrix, k <= 16384: the packed view of the GELU'd matrix, which is never written
hipError_t launch_gelu_rows(const float *X, int64_t xsh, float *Y, int64_t ysh, int64_t rows, int w, hipStream_t stream);
hipError_t launch_gelu_pack(const float *X, int64_t xsh, int m, int k, float range, PackedView out, hipStream_t stream);
// Llama-style blocks (the contracts are at qgemm_rmsnorm_rows and qgemm_glu_rows in include/qgemm.h).
// norm.hip: the RMS forms of the three launchers above -- no mean, no beta, the same kernel, rules and checks
hipError_t launch_rmsnorm_rows(const float *A, const float *B, const float *gamma, float eps, float *Y, int64_t rows,
                               int w, hipStream_t stream);
hipError_t launch_rmsnorm_rows_pack(const float *A, const float *B, const float *gamma, float eps, float *Y,
                                    int64_t rows, int w, float range, PackedView out, hipStream_t stream);
hipError_t launch_prenorm_rms_pack(const float *A, const float *B, const float *gamma, float eps, float *S,
                                   int64_t rows, int w, float range, PackedView out, hipStream_t stream);
// glu.hip: h = act(gate) * up on rows of [gate: w | up: w] floats (activation: QGEMM_ACT_*), elementwise and fused
// into pack_rows of the m x k product, k <= 16384, which is never written
hipError_t launch_glu_rows(const float *X, int64_t xsh, float *Y, int64_t ysh, int64_t rows, int w, int activation,
                           hipStream_t stream);
hipError_t launch_glu_pack(const float *X, int64_t xsh, int m, int k, int activation, float range, PackedView out,
                           hipStream_t stream);
// transformer.hip: the architecture of a stack (stack_create's arch: 0 the reference's block, 1 the standard one with
// its new tensors allocated and set, b_* = +0, gamma = 1, beta = +0; activation: 0 relu, 1 tanh GELU, arch 1 only;
// arch 0x101 the pre-LN block and 0x301 the pre-LN block with a final norm, QGEMM_ARCH_NORM_FIRST / _FINAL_NORM;
// 0x400 QGEMM_ARCH_DECODER_ONLY with cross alone, 0x800 QGEMM_ARCH_ROPE on the standard block alone; 0x2000
// QGEMM_ARCH_RMSNORM and 0x4000 QGEMM_ARCH_GATED_FFN on the standard block alone, activation 2, SiLU, with the gate
// alone); stack_activation_ok is the one check of arch and activation together;
// stack_describe reads back what creation was given.
bool stack_arch_ok(int arch, bool cross);
bool stack_activation_ok(int arch, int activation, int d_ff);
struct StackDesc {
    int cross, d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq;
    uint64_t seed;
    int flags, n_slots, max_rows, arch, activation;
    float ln_eps;
};
hipError_t stack_describe(const Stack *S, StackDesc *out);

}  // namespace qgemm
