/*
 * qgemm.h -- C-ABI of the MI355X-native (gfx950) int8 absmax quantized GEMM.
 *
 * Drop-in for the reference's quantized matrix multiply
 *     template<typename T> void op_quantized_mm(const Tensor<T>& X, const Tensor<T>& W,
 *                                               Tensor<T>& O, T range)
 *     (/root/reference/src/ops/op_mm.cuh:67-101, instantiated only at T = float,
 *      called from test_quantize.cu:78 and inlined in timing_quantize.cu:38-58)
 * as the flat C entry point the north star names, op_mm_quantize(A, B, C, M, N, K).
 *
 * Semantics (bit-exact with the reference chain, see DESIGN.md "Semantics"):
 *   Cx[i] = absmax of row i of A with the reference's signed-first-element seed
 *   Cw[j] = absmax of column j of B, same seed rule
 *   Aq = trunc_sat_i8(A * fl(range/Cx)), Bq = trunc_sat_i8(B * fl(range/Cw))
 *   C[i,j] = fl(fl(float(sum_k Aq[i,k]*Bq[k,j]) * (fl(Cx[i]*Cw[j]) + 0)) * fl(1/fl(range*range)))
 *
 * Conventions
 *   - All matrix pointers are DEVICE pointers (the reference asserts on_device, op_mm.cuh:72).
 *   - Return value: 0 on success, otherwise a hipError_t code (hipErrorInvalidValue = 1 for
 *     bad shapes / null pointers -- where the reference would assert(), op_mm.cuh:71-72).
 *   - Work is enqueued asynchronously; the plain entry point uses the null stream, like the
 *     reference's launches (legacy default stream).
 *   - No parameter is named N: the reference's op_elemwise.cuh:10 does "#define N 256".
 *   - The entry points without a workspace argument use a grow-only device buffer cached per
 *     (device, stream) -- per calling thread as well for hipStreamPerThread -- so calls on
 *     different streams never share it; the reference allocates per call (op_mm.cuh:76-93).
 *     Growing it allocates (not allowed inside a hipGraph capture) and waits for that stream;
 *     at most 8 such buffers are kept per device (the least recently used one is freed, after
 *     a device synchronisation, when a ninth stream arrives).  Pass an explicit workspace
 *     (op_mm_quantize_ws) for capture or to bound memory.
 */
#ifndef QGEMM_H_
#define QGEMM_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define QGEMM_API __attribute__((visibility("default")))
#else
#define QGEMM_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces op_quantized_mm<float>(X, W, O, 127.0f) (op_mm.cuh:67-101).
 * A = X: m x k, row-major fp32.  B = W: k x n, row-major fp32.  C = O: m x n, row-major fp32. */
QGEMM_API int op_mm_quantize(const float *A, const float *B, float *C, int m, int n, int k);

/* Strided form: element (r, c) of a matrix lives at ptr[r*stride_h + c*stride_w], exactly the
 * reference's Index() macro (tensor.cuh:14), so transposed views (tensor.cuh:121-133) work.
 * range is the reference's `range` argument (127 at every reference call site). stream is a
 * hipStream_t (NULL = null stream).
 * range, wherever an entry point takes it: a finite positive float, not checked.  It scales the operands by
 * fl(range / absmax) before the cast to int8, and the cast saturates, so with range > 127 every element past
 * 127 / range of its row's (column's) absmax becomes -128 or 127; the output is multiplied by
 * fl(1 / fl(range * range)), which is +0 once range * range overflows.  The GEMM must be given the range its
 * operands were packed with.  The prepacked drop-in and the linear entry points (op_mm_quantize_prepacked*,
 * qgemm_linear*) take no range: they are fixed at 127. */
QGEMM_API int op_mm_quantize_ex(const float *A, int64_t a_stride_h, int64_t a_stride_w,
                      const float *B, int64_t b_stride_h, int64_t b_stride_w,
                      float *C, int64_t c_stride_h, int64_t c_stride_w,
                      int m, int n, int k, float range, void *stream);

/* Same, with caller-owned device workspace (no allocation inside: safe for hipGraph capture and
 * for concurrent calls on different streams).  ws_bytes >= op_mm_quantize_workspace_size(m,n,k). */
QGEMM_API size_t op_mm_quantize_workspace_size(int m, int n, int k);
QGEMM_API int op_mm_quantize_ws(const float *A, int64_t a_stride_h, int64_t a_stride_w,
                      const float *B, int64_t b_stride_h, int64_t b_stride_w,
                      float *C, int64_t c_stride_h, int64_t c_stride_w,
                      int m, int n, int k, float range,
                      void *workspace, size_t ws_bytes, void *stream);

/* ---- The chain's stages (the reference's L2 primitives, fused MI355X-style) ----------------
 * Packed operand = the quantized operand in MFMA-ready form, in ONE device buffer:
 *   [ scale: rows_pad f32 ][ reserved: parts x rows_pad u32, padded to 256 B ][ q: rows_pad x k_pad int8,
 *     zero padded ]   with parts = max(1, ceil((k-1)/256))
 * The q region is OPAQUE to callers: it is stored FRAGMENT-MAJOR (1-KiB blocks of 16 packed rows x 64 k,
 * bytes in the lane order of one v_mfma_i32_16x16x64_i8 operand; csrc/qgemm_internal.h fofs), so the GEMM
 * loads each MFMA operand with one contiguous 1-KiB load.  Treat a packed buffer as a handle: produce it
 * with qgemm_pack_a / qgemm_pack_b, consume it with qgemm_mm_packed / qgemm_linear / the prepacked drop-in.
 * rows_pad = round_up(rows, 256), k_pad = round_up(k, 128).  For A, rows = m and the scale is
 * Cx (op_absmax(X,Cx), op_mm.cuh:76-77) and q = X_int8 (op_mm.cuh:86-87).  For B, rows = n
 * (B is stored transposed, k contiguous) and the scale is Cw (op_mm.cuh:78-79), q = W_int8^T.
 * Packing B once and reusing it is the LLM.int8() weight-cache pattern. */
QGEMM_API size_t qgemm_packed_size(int rows, int k);
QGEMM_API int qgemm_pack_a(const float *A, int64_t a_stride_h, int64_t a_stride_w, int m, int k, float range,
                 void *packed_a, void *stream);
QGEMM_API int qgemm_pack_b(const float *B, int64_t b_stride_h, int64_t b_stride_w, int k, int n, float range,
                 void *packed_b, void *stream);
/* int8 x int8 -> int32 MFMA GEMM with the fused dequantize epilogue (op_mm.cuh:92-99). */
QGEMM_API int qgemm_mm_packed(const void *packed_a, const void *packed_b, float *C, int64_t c_stride_h,
                    int64_t c_stride_w, int m, int n, int k, float range, void *stream);
/* The weight-cache form of the drop-in (op_mm_quantize_prepacked): B was packed once
 * with qgemm_pack_b(range 127); every call quantizes A (op_mm.cuh:76-77, 82-87) and runs the int8 GEMM
 * with the fused dequantize (op_mm.cuh:92-99) -- bit-identical to op_mm_quantize(A, B, C, m, n, k) on the
 * B that was packed.  A: m x k (row stride a_stride_h, unit column stride), C: m x n (row stride
 * c_stride_h).  The plain form uses the library's workspace and the null stream.
 * Range: A is quantized with range 127 and O dequantized with fl(1/127^2), as op_mm_quantize does, so
 * packed_b must come from qgemm_pack_b(..., range = 127, ...); a B packed with another range gives
 * results that differ from op_mm_quantize (the packed buffer does not record its range). */
QGEMM_API int op_mm_quantize_prepacked(const float *A, const void *packed_b, float *C, int m, int n, int k);
QGEMM_API size_t op_mm_quantize_prepacked_workspace_size(int m, int n, int k);
QGEMM_API int op_mm_quantize_prepacked_ws(const float *A, int64_t a_stride_h, const void *packed_b, float *C,
                                int64_t c_stride_h, int m, int n, int k, void *workspace, size_t ws_bytes,
                                void *stream);
/* Debug/parity view of the raw int32 accumulator (op_mm<int8_t,int>, op_mm.cuh:92-93):
 * Acc is m x n row-major int32. */
QGEMM_API int qgemm_mm_packed_i32(const void *packed_a, const void *packed_b, int32_t *Acc, int m, int n, int k,
                        void *stream);

/* The reference's UNQUANTIZED op_mm<float,float> (op_mm.cuh:49-65), bit-exact: sequential-k fmaf from +0.
 * Used for the reference's error metric (timing_quantize.cu:67-70) and its unquantized timing line.
 * Strides are in floats; row-major, column-major and transposed views of A, B and C all work.  The stride
 * envelope: the kernels reach an element of a block's tile (at most 128 x 128 outputs, 32 k) by a 32-bit byte
 * offset, so
 *   - the stride of every dimension longer than one element is >= 0, and
 *   - (R - 1) * stride_h + (W - 1) * stride_w < 2^29 - 1 floats (2^31 bytes) for the tile's extent R x W of each
 *     matrix: A min(m, TM) x min(k, 32), B min(k, 32) x min(n, TN), C min(m, TM) x min(n, TN), with TM x TN the
 *     tile of the kernel the call takes (qgemm_mm_fp32_plan names it: 128x128, 64x64, 32x64 or 16x32).
 * How many rows or k steps the matrices have beyond one tile does not matter: tiles start at 64-bit addresses.
 * hipErrorInvalidValue before any launch: a null pointer, m < 0, n < 0, k < 1, or strides outside that envelope
 * (C is then untouched; never zeros in place of products).  m == 0 or n == 0 returns 0. */
QGEMM_API int qgemm_mm_fp32(const float *A, int64_t a_stride_h, int64_t a_stride_w,
                  const float *B, int64_t b_stride_h, int64_t b_stride_w,
                  float *C, int64_t c_stride_h, int64_t c_stride_w, int m, int n, int k, void *stream);
/* Diagnostics: the kernel qgemm_mm_fp32 takes for a call, and each of the two batched GEMMs of qgemm_attention's
 * three launches (batch = heads; batch strides in floats).  It takes all the selection reads: the dimensions, the
 * batch, the strides of A and B and their batch strides, and A and B themselves for their 16-byte alignment only --
 * they are never dereferenced, and any integer with the same low four bits serves.  Returns 0 and, when kernel is
 * non-NULL, a static string in *kernel, one of
 *   mm_f32_dma_128x128_bkc  mm_f32_dma_64x64_bkc  mm_f32_dma_32x64_bkc    LDS-DMA ring, B k-contiguous (a B^T view)
 *   mm_f32_dma_128x128_bnc  mm_f32_dma_64x64_bnc  mm_f32_dma_32x64_bnc    LDS-DMA ring, B n-contiguous (row-major)
 *   mm_f32_mfma_128x128     mm_f32_mfma_64x64     mm_f32_mfma_16x32       register staging, any strides
 * (family, then the block's tile TM x TN).  The ring serves 16-byte aligned bases with k % 4 == 0, unit
 * a_stride_w, a_stride_h % 4 == 0, batch strides % 4 == 0 and B either k-contiguous with b_stride_w % 4 == 0 or
 * row-major with b_stride_h % 4 == 0 and n % 4 == 0; the tile is the largest that still fills the GPU.  Every kernel
 * gives the same bits.  The query does not judge the stride envelope above: the call does.
 * hipErrorInvalidValue: m, n, k or batch < 1.  Needs no GPU. */
QGEMM_API int qgemm_mm_fp32_plan(int m, int n, int k, int batch, const void *A, int64_t a_stride_h,
                       int64_t a_stride_w, int64_t a_batch_stride, const void *B, int64_t b_stride_h,
                       int64_t b_stride_w, int64_t b_batch_stride, const char **kernel);

/* ---- The encoder counterpart (transformer.cu:14-77, BASELINE config 5) ----------
 * Linear layer on the quantized path (linear.cuh:50-54): Y = quantized_mm(X, W) [+ b] [relu], where
 * W (k x n) was packed once with qgemm_pack_b.  X is m x k row-major (row stride x_stride_h), Y m x n
 * (row stride y_stride_h).  bias = NULL: no bias (relu requires a bias, as the reference's FFN).
 * y = fl(O + b[j]) then (y < 0 ? 0 : y) (op_add, op_relu: op_elemwise.cuh:57-65, 181-195). */
QGEMM_API size_t qgemm_linear_workspace_size(int m, int n, int k);
QGEMM_API int qgemm_linear(const float *X, int64_t x_stride_h, int m, int k, const void *packed_w, int n,
                 const float *bias, int relu, float *Y, int64_t y_stride_h, void *workspace, size_t ws_bytes,
                 void *stream);
/* ---- bf16 activations and outputs on the prepacked path -------------------------------------------
 * Element-type tags of the _dt entry points; strides are in elements of the tagged type.  The arithmetic
 * is the fp32 chain's, only its two ends change:
 *   bf16 input : every element is widened exactly (its bits shifted left by 16; subnormals stay subnormal),
 *                so Cx, Xq and the accumulators are bit-identical to the fp32 entry point on the widened matrix.
 *   bf16 output: the fp32 value the fp32 entry point would store (after dequantize, + bias, relu) is rounded
 *                once, to nearest even: past the bf16 maximum it becomes +-inf, subnormals stay subnormal, -0
 *                stays -0, NaN stays NaN.
 * bias stays fp32, and weights are packed from fp32 with qgemm_pack_b (a bf16 checkpoint goes in through
 * qgemm_pack_b_window below, which widens it exactly).  With every tag QGEMM_F32 a _dt entry point IS its fp32 counterpart (same
 * launches, bit-identical results); an unknown tag returns hipErrorInvalidValue before any launch.
 * qgemm_linear_dt takes the workspace of qgemm_linear_workspace_size (it does not depend on the types). */
enum { QGEMM_F32 = 0, QGEMM_BF16 = 1 };
QGEMM_API int qgemm_pack_a_dt(const void *A, int a_dtype, int64_t a_stride_h, int64_t a_stride_w, int m, int k,
                    float range, void *packed_a, void *stream);
QGEMM_API int qgemm_mm_packed_dt(const void *packed_a, const void *packed_b, void *C, int c_dtype, int64_t c_stride_h,
                       int64_t c_stride_w, int m, int n, int k, float range, void *stream);
QGEMM_API int qgemm_linear_dt(const void *X, int x_dtype, int64_t x_stride_h, int m, int k, const void *packed_w, int n,
                    const float *bias, int relu, void *Y, int y_dtype, int64_t y_stride_h,
                    void *workspace, size_t ws_bytes, void *stream);
/* op_multiply(S, scale) then op_softmax (attention.cuh:65-68, op_softmax.cuh:6-29), per row of w
 * contiguous floats (w <= 4096); P may equal S.  exp is the correctly rounded fp32 exp. */
QGEMM_API int qgemm_softmax_rows(const float *S, float *P, int64_t rows, int w, float scale, void *stream);
/* The same under the causal mask of qgemm_attention_causal: the rows are a stack of rows / seq_q score matrices of
 * seq_q rows each; row r is query i = r % seq_q and sees its first L_i = min(w, i + q_pos0 + 1) columns.  Its
 * result is qgemm_softmax_rows' on a row of width L_i (columns L_i .. w-1 are never read), then +0 in columns
 * L_i .. w-1.  P may equal S.  hipErrorInvalidValue: a null pointer, w < 1 or > 4096, rows < 0, seq_q < 1,
 * rows % seq_q != 0, q_pos0 < 0. */
QGEMM_API int qgemm_softmax_rows_causal(const float *S, float *P, int64_t rows, int w, float scale, int seq_q,
                              int q_pos0, void *stream);
/* op_add(A, B) then op_layernorm (transformer.cu:58-59, op_layernorm.cuh:6-33) as written:
 * (y - mean) / var, sums in column order, pow(d, 2) = fl32(d*d); rows of w <= 4096 floats. */
QGEMM_API int qgemm_add_layernorm_rows(const float *A, const float *B, float *Y, int64_t rows, int w, void *stream);
/* Encoder stack with seeded weights drawn once and packed (the weight cache, s8f f2).  X, Y: seq x
 * d_model row-major fp32 device arrays, seq <= max_seq <= 4096, d_model <= 4096, d_model % n_heads == 0.
 * Weight tensor t of block i is the qgemm_fill_uniform stream encoder_weight_seed(seed, i, kind, head)
 * = seed*1000003 + i*4099 + kind*131 + head, kind 0..7 = Wq, Wk, Wv, W_O, W1, b1, W2, b2, with the
 * reference's init bounds (DESIGN.md "Encoder"). */
QGEMM_API int qgemm_encoder_create(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, uint64_t seed,
                         void **encoder);
QGEMM_API int qgemm_encoder_forward(void *encoder, const float *X, float *Y, int seq, void *stream);
QGEMM_API int qgemm_encoder_destroy(void *encoder);

/* ---- Multi-head attention core, fp32 (attention.cuh:58-69), self- or cross-attention ------------------
 * For every head h = 0 .. n_heads-1, on columns h*d_k .. h*d_k + d_k - 1 of each matrix (d_v = d_k):
 *   S_h = Q_h K_h^T              op_mm<float> on the transposed view: the sequential-k fmaf chain from +0
 *   P_h = softmax(fl(S_h*scale)) op_multiply + op_softmax, as qgemm_softmax_rows
 *   O_h = P_h V_h                op_mm<float>, the chain over seq_kv
 * bit-identical to qgemm_mm_fp32 + qgemm_softmax_rows + qgemm_mm_fp32 per head.  Q and O have seq_q rows, K and V
 * seq_kv rows (the decoder's cross-attention: queries from one stream, keys and values from another, of another
 * length); each matrix has its own base pointer and row stride in floats (*_stride_h) and unit inner stride, so
 * column slices of wider buffers work (the encoder passes the thirds of one [Q | K | V] buffer).  No mask (qgemm_attention_causal has one).
 * O must not overlap Q, K or V (not checked).
 * One fused launch (the scores stay on chip) for d_k <= 64 and seq_kv <= 512, any seq_q; outside that three
 * launches through `workspace`, n_heads x seq_q x seq_kv floats of scores: qgemm_attention_workspace_size returns
 * that size in bytes, 0 inside the fused envelope (workspace may then be NULL) and 0 for invalid dimensions.
 * (seq_q <= 8 with d_k <= 64 takes a launch of its own, up to 4096 keys, which leaves the workspace untouched:
 * qgemm_attention_plan below.  The workspace rules do not change with it.)
 * The call allocates nothing and makes no host synchronization.
 * hipErrorInvalidValue before any launch: a null Q / K / V / O, seq_q < 0, seq_kv < 1, n_heads < 1, d_k < 1,
 * seq_kv > 4096 (qgemm_softmax_rows' row limit), a short workspace or, on the three launches only, a row stride
 * outside qgemm_mm_fp32's stride envelope (negative, or 127 rows of it reaching 2^31 bytes); seq_q == 0 returns 0. */
QGEMM_API size_t qgemm_attention_workspace_size(int seq_q, int seq_kv, int n_heads, int d_k);
QGEMM_API int qgemm_attention(const float *Q, int64_t q_stride_h, const float *K, int64_t k_stride_h,
                    const float *V, int64_t v_stride_h, float *O, int64_t o_stride_h,
                    int seq_q, int seq_kv, int n_heads, int d_k, float scale,
                    void *workspace, size_t ws_bytes, void *stream);
/* qgemm_attention under a causal mask.  q_pos0 >= 0 is the position of query row 0 in the key sequence: query row
 * i sees keys 0 .. L_i - 1, L_i = min(seq_kv, i + q_pos0 + 1) >= 1 (self-attention: q_pos0 = 0; queries appended
 * to a key / value cache: q_pos0 = seq_kv - seq_q).
 *   S_h as qgemm_attention's.
 *   P_h: row i is qgemm_softmax_rows' result on the first L_i columns of fl(S_h*scale) (seed the first element,
 *        strict >, correctly rounded exp, one sum in column order); columns L_i .. seq_kv-1 are +0.  No masked
 *        score reaches the result: a NaN or inf in a K row that no query of the call sees changes nothing.
 *   O_h = P_h V_h, the chain over ALL seq_kv keys as qgemm_attention's: a masked key contributes fmaf(+0, v, acc),
 *        so a non-finite V at a key masked for row i makes that row's column NaN (0 * inf), as an underflowed P does
 *        without a mask.
 * Bit-identical on every input to qgemm_mm_fp32 + qgemm_softmax_rows_causal + qgemm_mm_fp32 per head, on the fused
 * launch and on the three-launch path alike.  With q_pos0 >= seq_kv - 1 the mask hides nothing and the result is
 * qgemm_attention's bit for bit.  Where V is finite at the masked keys and no product underflows to -0, row i
 * equals row 0 of qgemm_attention(Q[i], K[:L_i], V[:L_i]).
 * Workspace, envelope and argument checks as qgemm_attention (qgemm_attention_workspace_size); also
 * hipErrorInvalidValue before any launch for q_pos0 < 0. */
QGEMM_API int qgemm_attention_causal(const float *Q, int64_t q_stride_h, const float *K, int64_t k_stride_h,
                           const float *V, int64_t v_stride_h, float *O, int64_t o_stride_h,
                           int seq_q, int seq_kv, int n_heads, int d_k, float scale, int q_pos0,
                           void *workspace, size_t ws_bytes, void *stream);
/* Diagnostics: the launch qgemm_attention / qgemm_attention_causal take for a shape, with or without a mask.  Returns
 * 0 and, when kernel is non-NULL, a static string in *kernel that begins "attention_decode" (seq_q <= 8, d_k <= 64:
 * one workgroup per (head, query row), up to 4096 keys -- a decoding step), "attention_fused" (d_k <= 64,
 * seq_kv <= 512) or "three_launches"; hipErrorInvalidValue for dimensions the calls refuse.  Every path gives the
 * same bits.  qgemm_attention_workspace_size does not depend on it: the decode launch leaves a workspace it is
 * handed untouched, and a shape outside the fused envelope still has to bring one.  Needs no GPU. */
QGEMM_API int qgemm_attention_plan(int seq_q, int seq_kv, int n_heads, int d_k, const char **kernel);

/* ---- The decoder counterpart (transformer.cu:79-168) --------------------------------------------------
 * Decoder stack with seeded weights drawn once and packed, like the encoder's.  X, Y: seq x d_model; enc_out:
 * enc_seq x d_model; all row-major contiguous fp32 device arrays; seq <= max_seq <= 4096, enc_seq <= max_enc_seq
 * <= 4096, d_model <= 4096, d_model % n_heads == 0.  Per block: self-attention on the block input (the encoder's
 * first half), cross-attention with queries from the decoder stream and keys / values from enc_out, then the FFN
 * whose residual is the cross-attention's multiHeadOut (DESIGN.md "Decoder").  No causal mask, as the reference
 * (qgemm_decoder_create_ex adds one).
 * Weight kinds 0..7 as qgemm_encoder_create; 8, 9, 10 = the cross-attention's Wq2, Wk2, Wv2 (one d_model x d_k
 * tensor per head, bound 1/sqrt(d_k)); 11 = its output projection W_O2 (head 0, U(-1, 1)). */
QGEMM_API int qgemm_decoder_create(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq,
                         uint64_t seed, void **decoder);
/* qgemm_decoder_create with flags (0: exactly qgemm_decoder_create).  QGEMM_DECODER_CAUSAL: every block's
 * SELF-attention runs under the causal mask with q_pos0 = 0 (row i sees rows 0 .. i); the cross-attention stays
 * unmasked.  Every other step is row-local, so row i of a forward then depends on rows 0 .. i of X and on enc_out
 * alone: forward(X[:n]) equals the first n rows of forward(X) bit for bit.  An unknown flag bit:
 * hipErrorInvalidValue.  Forward and destroy are the same calls. */
/* QGEMM_DECODER_KV_CACHE (only together with QGEMM_DECODER_CAUSAL, else hipErrorInvalidValue): every block also owns a
 * self-attention cache, its [Q | K | V] rows of max_seq x 3 d_model, and a cross cache [K2 | V2] of max_enc_seq x
 * 2 d_model, for qgemm_decoder_begin / qgemm_decoder_step below.  A decoder created without it allocates nothing
 * more and behaves as before; forward on a cached decoder still works and neither reads nor writes the caches.
 * (Its value is 8: flag bits 2 and 4 stay unknown bits, so flags == 3 and flags == 5 are still refused.) */
enum { QGEMM_DECODER_CAUSAL = 1, QGEMM_DECODER_KV_CACHE = 8 };
QGEMM_API int qgemm_decoder_create_ex(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq,
                            uint64_t seed, int flags, void **decoder);
QGEMM_API int qgemm_decoder_forward(void *decoder, const float *X, const float *enc_out, float *Y, int seq, int enc_seq,
                          void *stream);
/* Incremental decoding on a decoder created with QGEMM_DECODER_KV_CACHE.
 * qgemm_decoder_begin starts a sequence: it quantizes enc_out (enc_seq x d_model) once, runs every block's [K2 | V2]
 * projection into that block's cross cache, records enc_seq and sets the filled length to 0.  Calling it again
 * starts a new sequence.
 * qgemm_decoder_step takes X, the n x d_model contiguous decoder input rows at positions pos .. pos + n - 1, and
 * writes Y, their n output rows: per block the QKV projection of the n rows into cache rows pos .., the masked
 * attention of those rows against cache rows 0 .. pos + n - 1 (qgemm_attention_causal with q_pos0 = pos), and the
 * rest of forward's steps on n rows, the cross-attention reading the cross cache.  Y equals rows pos .. pos + n - 1
 * of the causal qgemm_decoder_forward on the whole prefix (the rows fed at positions 0 .. pos + n - 1) and the same
 * enc_out, BIT FOR BIT: every step but the attention is row-local, and the masked attention's row i depends on keys
 * and values 0 .. i alone where the cached V is finite and no P V accumulator is -0 (qgemm_attention_causal above).
 * pos is a host argument; the decoder keeps a host-side filled length, updated when the call is enqueued:
 * 0 <= pos <= filled is required and the call sets filled = pos + n, so stepping at an earlier pos rewinds
 * (speculative decoding, beam search), and a captured graph replays one position.
 * Neither call allocates or synchronizes; both use the decoder's scratch buffers in stream order, as forward does,
 * so one decoder does one thing at a time.
 * hipErrorInvalidValue before any launch: a decoder without the cache flag, a step without a begin, a null pointer,
 * n < 1, pos < 0, pos > filled, pos + n > max_seq, enc_seq < 1 or > max_enc_seq. */
QGEMM_API int qgemm_decoder_begin(void *decoder, const float *enc_out, int enc_seq, void *stream);
QGEMM_API int qgemm_decoder_step(void *decoder, const float *X, float *Y, int pos, int n, void *stream);
QGEMM_API int qgemm_decoder_destroy(void *decoder);

/* ---- Batched incremental decoding: many sequences per decoder step --------------------
 * qgemm_attention_decode_batched: the decode launch of qgemm_attention / qgemm_attention_causal for up to
 * QGEMM_DECODE_MAX_BATCH independent sequences in ONE launch.  Q and O hold n_seqs * rows_per_seq rows (row strides
 * q / o_stride_h, unit inner stride), rows b * rows_per_seq .. + rows_per_seq - 1 are sequence b's.  K and V are
 * stacks of slabs: sequence b reads rows 0 .. seq_kv[b] - 1 (row stride k / v_stride_h) of the slab that starts at
 * K + kv_slot[b] * k_stride_seq (V likewise; strides in floats).  kv_slot, seq_kv and q_pos0 are HOST arrays of n_seqs
 * ints, read when the call is enqueued: they travel in the kernel's arguments, so nothing is copied to the device,
 * allocated or synchronized, and a captured graph replays the values of the capture.  kv_slot == NULL means slabs
 * 0, 1, 2, ..; q_pos0 == NULL means no mask.
 * Contract: for every b, rows b * rows_per_seq .. of O are BIT FOR BIT what qgemm_attention (q_pos0 == NULL) or
 * qgemm_attention_causal with q_pos0[b] gives on those query rows and the seq_kv[b] rows of slab kv_slot[b].  Two
 * sequences may share a slab.  O must not overlap Q, K or V (not checked).
 * hipErrorInvalidValue before any launch: a null Q / K / V / O / seq_kv, n_seqs < 0 or > 64, rows_per_seq < 1 or > 8,
 * d_k < 1 or > 64, n_heads < 1, any seq_kv[b] < 1 or > 4096, any q_pos0[b] < 0, any kv_slot[b] < 0; n_seqs == 0
 * returns 0. */
enum { QGEMM_DECODE_MAX_BATCH = 64 };
QGEMM_API int qgemm_attention_decode_batched(const float *Q, int64_t q_stride_h,
                                   const float *K, int64_t k_stride_h, int64_t k_stride_seq,
                                   const float *V, int64_t v_stride_h, int64_t v_stride_seq,
                                   float *O, int64_t o_stride_h, int n_seqs, int rows_per_seq,
                                   const int *kv_slot, const int *seq_kv, const int *q_pos0,
                                   int n_heads, int d_k, float scale, void *stream);
/* Cache slots: ONE decoder (one copy of the packed weights) that holds n_slots (1 .. 64) independent sequences.
 * flags must be exactly QGEMM_DECODER_CAUSAL | QGEMM_DECODER_KV_CACHE.  Every block's self cache is one allocation of
 * n_slots x max_seq x 3 d_model floats ([Q | K | V] rows per slot, as before) and its cross cache one of n_slots x
 * max_enc_seq x 2 d_model; enc_seq and the filled length are host state per slot.  n_slots == 1 allocates and behaves
 * exactly as qgemm_decoder_create_ex with those flags, and every decoder created with the cache flag has slot 0:
 * qgemm_decoder_begin / qgemm_decoder_step ARE begin_slot(0) / step_slot(0).  With n_slots > 1 the decoder's scratch
 * buffers hold max(max_seq, 8 * n_slots) rows.
 *   begin_slot  qgemm_decoder_begin on one slot: the slot's cross cache, its enc_seq, filled = 0.
 *   step_slot   qgemm_decoder_step on one slot (the QKV GEMM writes the slot's cache rows directly).
 *   step_batch  one step of n_seqs (1 .. n_slots) DIFFERENT slots, rows_per_seq (1 .. 8) rows each.  X and Y are
 *               (n_seqs * rows_per_seq) x d_model, contiguous; rows b * r .. b * r + r - 1 are the new rows of slot
 *               slots[b] at positions pos[b] .. pos[b] + r - 1 (slots and pos: host arrays, read at enqueue time).
 *               Row for row Y is BIT FOR BIT what step_slot(slots[b], .., pos[b], r) gives for that sequence alone, and
 *               so the rows of the causal forward on that sequence's prefix: every step but the attention is row-local
 *               (per-row quantization scales, exact int32 accumulation, per-element dequantization, one-row layernorm),
 *               and the attention of all sequences is one qgemm_attention_decode_batched launch over the cache slabs.
 *               On success filled[slots[b]] = pos[b] + r; an earlier pos rewinds that sequence alone.  Needs
 *               d_model / n_heads <= 64.  The Q third of the cache rows it writes is unspecified.
 *   copy_slot   forks a sequence: rows 0 .. filled - 1 of every block's self cache and rows 0 .. enc_seq - 1 of its
 *               cross cache, device to device in stream order; dst takes src's enc_seq and filled length.
 *   slot_state  the host state of a slot (enc_seq 0: not begun); enc_seq / filled may be NULL.  No GPU call.
 * None of these allocates or synchronizes; they share the decoder's scratch in stream order with forward, so a decoder
 * still does one thing at a time.  forward on a slotted decoder touches no cache.
 * hipErrorInvalidValue before any launch and without moving any filled length: a decoder without the cache flag, a
 * null pointer, a slot out of range or not begun (begin_slot: out of range), the same slot twice in one step_batch,
 * pos[b] < 0, pos[b] > filled, pos[b] + r > max_seq, n_seqs or rows_per_seq out of range, d_k > 64 (step_batch);
 * copy_slot with dst == src or a source not begun; create_slots with other flags, n_slots < 1 or > 64 or a null
 * handle (the handle is left NULL). */
QGEMM_API int qgemm_decoder_create_slots(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq,
                               uint64_t seed, int flags, int n_slots, void **decoder);
QGEMM_API int qgemm_decoder_begin_slot(void *decoder, int slot, const float *enc_out, int enc_seq, void *stream);
QGEMM_API int qgemm_decoder_step_slot(void *decoder, int slot, const float *X, float *Y, int pos, int n, void *stream);
QGEMM_API int qgemm_decoder_step_batch(void *decoder, int n_seqs, const int *slots, const int *pos, int rows_per_seq,
                             const float *X, float *Y, void *stream);
QGEMM_API int qgemm_decoder_copy_slot(void *decoder, int dst_slot, int src_slot, void *stream);
QGEMM_API int qgemm_decoder_slot_state(void *decoder, int slot, int *enc_seq, int *filled);

/* ---- Batched variable-length forward: packed sequences in one attention launch ---------
 * qgemm_attention_varlen: qgemm_attention / qgemm_attention_causal for up to QGEMM_VARLEN_MAX_SEQS independent
 * sequences of DIFFERENT lengths in one call.  Sequence b has seq_q[b] query rows that start at row q_row0[b] of Q --
 * and its output rows at the same row q_row0[b] of O -- and seq_kv[b] keys that start at row kv_row0[b] of K and V
 * (row strides *_stride_h in floats, unit inner stride, head h at columns h*d_k ..).  q_pos0[b] is its mask offset;
 * q_pos0 == NULL means no mask for any sequence.  All five arrays are HOST arrays of n_seqs entries, read when the
 * call is enqueued: they travel in the kernel's arguments, so nothing is copied to the device, allocated or
 * synchronized, and a captured graph replays the values of the capture.
 * Where d_k <= 64 and EVERY seq_kv[b] <= 512 the call is ONE launch of the fused kernel over a table of sequences:
 * sum_b ceil(seq_q[b] / 32) * n_heads workgroups, none for a sequence with seq_q[b] == 0.  Otherwise it runs the
 * sequences one after another in order, each as qgemm_attention[_causal] would (decode, fused or three launches
 * through `workspace`).  qgemm_attention_varlen_plan names the path: "attention_fused_kernel<many>" or
 * "per_sequence"; it needs no GPU.  qgemm_attention_varlen_workspace_size is the largest
 * qgemm_attention_workspace_size over the sequences: 0 exactly when one table launch serves the call.
 * Contract: for every b, rows q_row0[b] .. q_row0[b] + seq_q[b] - 1 of O are BIT FOR BIT what
 * qgemm_attention (q_pos0 == NULL) or qgemm_attention_causal with q_pos0[b] gives on
 * (Q + q_row0[b] * q_stride_h, K + kv_row0[b] * k_stride_h, V + kv_row0[b] * v_stride_h, O + q_row0[b] * o_stride_h,
 * seq_q[b], seq_kv[b]); no other row of O is written.  Sequences may share rows of Q, K and V.  Output rows that two
 * sequences share are the caller's error and are not checked; O must not overlap Q, K or V (not checked).
 * hipErrorInvalidValue before any launch: a null Q / K / V / O / q_row0 / seq_q / kv_row0 / seq_kv, n_seqs < 0 or
 * > 64, a negative row offset, seq_q[b] < 0, seq_kv[b] < 1 or > 4096, q_pos0[b] < 0, n_heads < 1, d_k < 1, a workspace
 * smaller than qgemm_attention_varlen_workspace_size (which is 0 for arguments the call refuses); n_seqs == 0
 * returns 0 without a launch.  (On the three launches alone a row stride outside qgemm_mm_fp32's stride envelope is
 * refused when its sequence is reached, as by qgemm_attention.) */
enum { QGEMM_VARLEN_MAX_SEQS = 64 };
QGEMM_API size_t qgemm_attention_varlen_workspace_size(int n_seqs, const int *seq_q, const int *seq_kv, int n_heads,
                                             int d_k);
QGEMM_API int qgemm_attention_varlen(const float *Q, int64_t q_stride_h, const float *K, int64_t k_stride_h,
                           const float *V, int64_t v_stride_h, float *O, int64_t o_stride_h, int n_seqs,
                           const int64_t *q_row0, const int *seq_q, const int64_t *kv_row0, const int *seq_kv,
                           const int *q_pos0 /* NULL: no mask */, int n_heads, int d_k, float scale,
                           void *workspace, size_t ws_bytes, void *stream);
QGEMM_API int qgemm_attention_varlen_plan(int n_seqs, const int *seq_q, const int *seq_kv, int n_heads, int d_k,
                                const char **kernel);
/* The stacks on many sequences at once.  Every step of a block but the attention is row-local (per-row quantization
 * scales, exact int32 accumulation, per-element dequantization, one-row add + layernorm), so the rows of all
 * sequences run through one pass of the blocks as ONE matrix, and the attention goes through qgemm_attention_varlen.
 *   create_rows    qgemm_encoder_create / qgemm_decoder_create_slots with a ROW BUDGET: the scratch buffers, the packed
 *                  activations and the split-K scratch hold max(what those calls give, max_rows) rows (max_rows == 0:
 *                  exactly those calls).  The scores of the per-sequence path stay sized by max_seq.  Refused:
 *                  max_rows < 0, and a max_rows with round_up(max_rows, 256) * round_up(max(3 d_model, d_ff), 128)
 *                  > 2^31 - 1 -- below that no element index of a row-local kernel (pack, GEMM epilogue, add +
 *                  layernorm) on the widest activation buffer or its packed image leaves 32 bits.
 *   forward_batch  X, Y: the n_seqs (1 .. 64) sequences' rows packed one after another, sum seq_lens rows x d_model,
 *                  contiguous; 1 <= seq_lens[b] <= max_seq, sum <= the row budget.  Sequence b's rows of Y are BIT FOR
 *                  BIT qgemm_encoder_forward's on its rows of X alone.
 *   step_varlen    step_batch without its limits of 8 and of equal rows: sequence b appends n_rows[b] >= 1 rows (rows
 *                  sum_{b' < b} n_rows[b'] .. of X and Y) at positions pos[b] .. of slot slots[b] -- a prefill of many
 *                  slots in one pass, or prefills mixed with single decoding rows.  Row for row Y is BIT FOR BIT what
 *                  step_slot(slots[b], .., pos[b], n_rows[b]) gives for that sequence alone.  On success
 *                  filled[slots[b]] = pos[b] + n_rows[b].  Past 512 keys (or d_k > 64) the attention runs sequence by
 *                  sequence.  The Q third of the cache rows it writes is unspecified.
 * Neither allocates or synchronizes; seq_lens, slots, pos and n_rows are host arrays read at enqueue time.
 * hipErrorInvalidValue before any launch and without moving any filled length: a null pointer, n_seqs < 1 or > 64
 * (step_varlen: > n_slots), a length < 1 or > max_seq, more rows than the budget, an encoder handed to step_varlen or
 * a decoder to forward_batch; for step_varlen also step_batch's: a slot out of range, not begun or named twice,
 * pos[b] < 0, pos[b] > filled, pos[b] + n_rows[b] > max_seq. */
QGEMM_API int qgemm_encoder_create_rows(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_rows,
                              uint64_t seed, void **encoder);
QGEMM_API int qgemm_encoder_forward_batch(void *encoder, const float *X, float *Y, int n_seqs, const int *seq_lens,
                                void *stream);
QGEMM_API int qgemm_decoder_create_rows(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq,
                              uint64_t seed, int flags, int n_slots, int max_rows, void **decoder);
QGEMM_API int qgemm_decoder_step_varlen(void *decoder, int n_seqs, const int *slots, const int *pos, const int *n_rows,
                              const float *X, float *Y, void *stream);

/* ---- The output end: argmax, token embedding, vocabulary head, greedy generation --------
 * None of the entry points below allocates (qgemm_head_create / _destroy apart), synchronizes or copies anything to
 * the device: host arrays travel in kernel arguments, so each call can be captured in a graph, which then replays the
 * values of the capture.  Invalid arguments return hipErrorInvalidValue before any launch.
 *
 * qgemm_argmax_rows: row-wise argmax with the reference's op_argmax semantics for an [h x 1] index output
 * (op_reduction.cuh:41-54, 174-182).  S: rows of w floats, unit inner stride, row stride s_stride_h >= w floats;
 * idx: int32[rows]; val: float[rows] or NULL.  Per row the reference's chain:
 *   best = 0; for i = 1 .. w-1: if (S[i] > S[best]) best = i;     idx = best, val = the bits of S[best]
 * so among equal maxima the lowest index wins (+0 and -0 are equal), a NaN at i >= 1 never wins, and a NaN at column 0
 * is never beaten (idx 0, val that NaN).  The reference's functor also writes the running maximum back into its input;
 * here S is const and is not touched.  Nothing outside a row's w floats is read; 16-byte loads wherever base and
 * stride allow, a scalar head and tail otherwise.
 * With many rows it is one launch, one workgroup per row.  With fewer than 256 rows a wide row is split over `parts`
 * workgroups (each at least 4096 columns, about 512 workgroups in all, parts <= 64) whose partial winners go through
 * `workspace` to a second, combining launch; the result does not depend on the plan.  parts is chosen from rows and w
 * alone: qgemm_argmax_rows_plan reports it (parts == 1 for rows >= 256, else parts * rows < 768; needs no GPU; part p
 * covers columns p * chunk .. with chunk = ceil(w / parts) rounded up to a multiple of 4), and
 * qgemm_argmax_rows_workspace_size is 8 * rows * parts bytes, 0 for parts == 1 (workspace may then be NULL) and for
 * arguments the call refuses.
 * hipErrorInvalidValue: a null S / idx, rows < 0, w < 1 or > 2^24, s_stride_h < w, a short or null workspace with
 * parts > 1; rows == 0 returns 0 and touches nothing. */
QGEMM_API size_t qgemm_argmax_rows_workspace_size(int64_t rows, int w);
QGEMM_API int qgemm_argmax_rows_plan(int64_t rows, int w, int *parts);
QGEMM_API int qgemm_argmax_rows(const float *S, int64_t s_stride_h, int64_t rows, int w, int32_t *idx, float *val,
                      void *workspace, size_t ws_bytes, void *stream);
/* qgemm_embed_rows: Y[r] = E[tokens[r]], or fl(E[tokens[r]] + P[p_r]) -- one fp32 add -- with a position table P
 * (max_pos x d_model).  E: vocab x d_model; Y: (n_seqs * rows_per_seq) x d_model; E, P and Y have their own row
 * strides in floats (>= d_model) and unit inner stride.  tokens: int32[n_seqs * rows_per_seq] in DEVICE memory.
 * Positions follow step_batch's layout: row r belongs to sequence b = r / rows_per_seq and has position
 * p_r = pos[b] + r % rows_per_seq; pos is a HOST array of n_seqs <= 64 ints, read at enqueue time (not read when
 * P == NULL, and may then be NULL).
 * A token outside [0, vocab) cannot be seen by the host: its row of Y is d_model quiet NaNs (0x7fc00000), nothing of E
 * or P is read for it, and every other row stays right -- the error shows downstream and nothing faults.
 * hipErrorInvalidValue: a null E / tokens / Y, vocab < 1, d_model < 1, a row stride below d_model, n_seqs < 0 or > 64,
 * rows_per_seq < 1; with P: a null pos, max_pos < 1, pos[b] < 0 or pos[b] + rows_per_seq > max_pos.  n_seqs == 0
 * returns 0. */
QGEMM_API int qgemm_embed_rows(const float *E, int64_t e_stride_h, int vocab, int d_model, const int32_t *tokens,
                     const float *P, int64_t p_stride_h, int max_pos, const int *pos, int n_seqs, int rows_per_seq,
                     float *Y, int64_t y_stride_h, void *stream);
/* The head object.  It BORROWS (the caller keeps them alive): packed_w, a d_model x vocab weight packed by
 * qgemm_pack_b with range 127 (a tied head is the pack of E's transposed view: the pack takes strided views); bias
 * (vocab floats) or NULL; E (vocab x d_model) or NULL; P (max_pos x d_model) or NULL (P needs E).  It OWNS, allocated at
 * creation: a logits buffer of max_rows x vocab floats, two blocks of max_rows x d_model rows, and the workspaces of
 * qgemm_linear and qgemm_argmax_rows for every row count up to max_rows.  One head does one thing at a time (its
 * buffers are used in stream order).
 *   logits       qgemm_linear(H, packed_w, bias, no relu) into the caller's `logits` (rows x vocab, row stride
 *                l_stride_h), bit for bit.  H: rows x d_model, row stride h_stride_h, rows <= max_rows.
 *   next_tokens  logits into the owned buffer, then qgemm_argmax_rows over the vocabulary: tokens int32[rows], device.
 *   embed        qgemm_embed_rows on the head's tables (needs E).
 * hipErrorInvalidValue: a null handle or pointer, d_model / vocab / max_rows < 1, vocab > 2^24, a row stride below its
 * row, rows < 0 or > max_rows, embed on a head without E, and what qgemm_embed_rows refuses. */
QGEMM_API int qgemm_head_create(const void *packed_w, int d_model, int vocab, const float *bias, const float *E,
                      int64_t e_stride_h, const float *P, int64_t p_stride_h, int max_pos, int max_rows, void **head);
QGEMM_API int qgemm_head_logits(void *head, const float *H, int64_t h_stride_h, int rows, float *logits,
                      int64_t l_stride_h, void *stream);
QGEMM_API int qgemm_head_next_tokens(void *head, const float *H, int64_t h_stride_h, int rows, int32_t *tokens,
                           void *stream);
QGEMM_API int qgemm_head_embed(void *head, const int32_t *tokens, const int *pos, int n_seqs, int rows_per_seq, float *Y,
                     int64_t y_stride_h, void *stream);
QGEMM_API int qgemm_head_destroy(void *head);
/* Greedy decoding of n_seqs cache slots for n_new tokens, enqueued in ONE call with no host round trip.  With
 * tok_0 = tokens_in (int32[n_seqs], device), for t = 0 .. n_new - 1:
 *   X = head embed(tok_t, pos + t);  H = step_batch(slots, X, pos + t);  tok_{t+1} = head next_tokens(H)
 * tok_{t+1} is row t of tokens_out (int32[n_new x n_seqs], device), and step t + 1's embed reads that row on the
 * device.  So the tokens are, bit for bit, those of the same loop driven through qgemm_head_embed,
 * qgemm_decoder_step_batch and qgemm_head_next_tokens.  pos: a host array of n_seqs ints, or NULL for the slots' filled
 * lengths; an earlier pos rewinds, as in step_batch.  On success filled[slots[b]] = pos[b] + n_new.  It does not stop
 * at an end token: the caller trims the output.  The head's row buffers and the decoder's scratch are used in stream
 * order.
 * hipErrorInvalidValue before any launch and without moving any filled length: a null pointer, a decoder without
 * caches, a head without E or of another d_model, n_seqs < 1, > n_slots or > the head's max_rows, n_new < 0, a slot out
 * of range, not begun or named twice, pos[b] < 0, pos[b] > filled, pos[b] + n_new > max_seq (or > the head's max_pos
 * with a P), d_model / n_heads > 64 (step_batch).  n_new == 0 returns 0. */
QGEMM_API int qgemm_decoder_generate(void *decoder, void *head, int n_seqs, const int *slots, const int32_t *tokens_in,
                           int n_new, const int *pos, int32_t *tokens_out, void *stream);

/* ---- Sampled token choice: top-k / top-p at a temperature, seeded draws, end-token hold ----
 * Like the entry points above, none of these allocates, synchronizes or copies anything to the device, and each can be
 * captured; invalid arguments return hipErrorInvalidValue before any launch.
 *
 * qgemm_sample_rows draws one column per row of S (rows of w floats, unit inner stride, row stride s_stride_h >= w;
 * S is const and untouched, nothing outside a row's w floats is read).  The rules for one row, every step one IEEE
 * fp32 operation, so that a restatement predicts each token exactly:
 *  1. Candidates are the columns with S[i] > -inf: a NaN or a -inf is never one (-inf is how a caller bans a token).
 *     Their order is the argmax's: greater value first, among == values (+0 equals -0) the lower index first.
 *     k' = min(top_k, candidates); the list t_0 .. t_{k'-1} holds the first k' columns in that order, v_j = S[t_j]
 *     (own bits).  k' == 0: the token is 0 (what qgemm_argmax_rows gives such a row) and n_kept = 0.
 *  2. temperature == 0 means greedy: top_k is taken as 1 and inv_t = 1.  Otherwise inv_t = 1.0f / temperature, one fp32
 *     division on the host.
 *  3. p_0 .. p_{k'-1} is qgemm_softmax_rows on the row v_0 .. v_{k'-1} with scale = inv_t, bit for bit: fl(v * inv_t),
 *     a maximum seeded by element 0 and moved by a strict >, the correctly rounded exp of fl(x - max), one sum from +0
 *     in list order, one division.
 *  4. c_j = fl(c_{j-1} + p_j) with c_{-1} = +0, one after another in list order.
 *  5. Nucleus: thr = fl(top_p * c_{k'-1}); n = 1 + the first j with c_j >= thr; n = k' where no j qualifies (NaNs).
 *     top_p acts inside the top_k list.
 *  6. Draw: u = (z >> 40) * 2^-24 with key = mix64(seed + G), z = mix64(key + (counter + 1) * G), G = 0x9E3779B97F4A7C15
 *     and mix64 the generator of qgemm_fill_uniform (element `counter` of its [0, 1) fill with this seed);
 *     r = fl(u * c_{n-1}); the token is t_j for the first j < n with c_j > r, j = 0 where there is none.  On finite rows
 *     there always is one (u <= 1 - 2^-24); a row holding +inf has every p NaN and gives its lowest-index +inf.
 *  7. Hold: with prev != NULL and eos >= 0, a row with prev[r] == eos gets the token eos whatever was drawn.
 * So top_k = 1 (or temperature 0) gives qgemm_argmax_rows' index on every row whose column 0 is not a NaN.
 * Row r's counter is counters[r] where counters != NULL -- a HOST array of rows <= 64 entries, read at enqueue time and
 * passed in the kernel arguments -- else counter0 + ((uint64_t)r << 32).  A captured call replays the counters of
 * its capture, and with them its draws: a device-resident counter is out of scope.
 * idx: int32[rows], the tokens.  top_idx (int32) and top_prob (float), both or neither, rows x top_k: the list and the
 * bits of its p, -1 and +0 at and past position k'.  n_kept: int32[rows] or NULL, n (0 where k' == 0).  prev:
 * int32[rows] on the device or NULL.
 * Few, wide rows are split as the argmax splits them: `parts` column ranges of at least 4096 columns per row (parts
 * from rows, w and top_k alone, at most 64; qgemm_sample_rows_plan reports it and needs no GPU), whose top_k best go
 * through `workspace` (qgemm_sample_rows_workspace_size: 8 * rows * parts * top_k bytes, 8-byte aligned; 0 for
 * parts == 1, where workspace may be NULL, and for arguments the call refuses) to a second launch.  The result does not
 * depend on the plan.
 * hipErrorInvalidValue: a null S / idx, rows < 0, w < 1 or > 2^24, s_stride_h < w, top_k < 1 or > 1024, top_p outside
 * (0, 1] or NaN, temperature < 0, infinite or NaN, one of top_idx / top_prob without the other, counters with
 * rows > 64, a short, misaligned or null workspace with parts > 1; rows == 0 returns 0 and touches nothing. */
QGEMM_API int qgemm_sample_rows_plan(int64_t rows, int w, int top_k, int *parts);
QGEMM_API size_t qgemm_sample_rows_workspace_size(int64_t rows, int w, int top_k);
QGEMM_API int qgemm_sample_rows(const float *S, int64_t s_stride_h, int64_t rows, int w, int top_k, float top_p,
                      float temperature, uint64_t seed, uint64_t counter0, const uint64_t *counters,
                      const int32_t *prev, int eos, int32_t *idx, int32_t *top_idx, float *top_prob, int32_t *n_kept,
                      void *workspace, size_t ws_bytes, void *stream);
/* qgemm_head_next_tokens with qgemm_sample_rows in the argmax's place: logits into the head's buffer, then one draw per
 * row from them (the sampling arguments as above) into tokens, int32[rows] on the device.  The head owns a sampling
 * workspace for top_k = 1024 and every row count up to max_rows.  Refused before the logits are launched: what
 * qgemm_head_next_tokens and qgemm_sample_rows refuse. */
QGEMM_API int qgemm_head_sample_tokens(void *head, const float *H, int64_t h_stride_h, int rows, int top_k, float top_p,
                             float temperature, uint64_t seed, uint64_t counter0, const uint64_t *counters,
                             const int32_t *prev, int eos, int32_t *tokens, void *stream);
/* qgemm_decoder_generate with qgemm_head_sample_tokens in qgemm_head_next_tokens' place.  Sequence b draws at step t
 * with the counter ((uint64_t)stream_b << 32) + pos[b] + t, stream_b = streams ? streams[b] : slots[b] (streams: a HOST
 * array of n_seqs uint32, or NULL), and prev is the row of tokens fed at that step.  Because the counter is the
 * position, a sequence's tokens depend neither on its batch neighbours nor on how n_new is split over calls, and a
 * rewind (or a replayed graph) repeats its draws.  With eos >= 0 a sequence that has produced eos keeps producing it;
 * its steps still run, so filled[slots[b]] = pos[b] + n_new as in the greedy call.  eos < 0: no end token.
 * hipErrorInvalidValue before any launch: what qgemm_decoder_generate and qgemm_sample_rows refuse. */
QGEMM_API int qgemm_decoder_generate_sampled(void *decoder, void *head, int n_seqs, const int *slots,
                                   const int32_t *tokens_in, int n_new, const int *pos, int top_k, float top_p,
                                   float temperature, uint64_t seed, const uint32_t *streams, int eos,
                                   int32_t *tokens_out, void *stream);

/* ---- Beam search: log-sum-exp rows, beam step, cache gather, device loop -----------------
 * Like the entry points above, none of these allocates, synchronizes or copies anything to the device, and each can be
 * captured; host arrays travel in kernel arguments; invalid arguments return hipErrorInvalidValue before any launch and
 * without moving host state.
 *
 * qgemm_logsumexp_rows: mx[r], logz[r] (float[rows], device) for every row of S (rows of w floats, unit inner stride,
 * row stride s_stride_h >= w, 1 <= w <= 2^24; S is const, nothing outside a row's w floats is read).  The rules for one
 * row, every step one IEEE fp32 operation:
 *  1. Candidates are the columns with S[i] > -inf (qgemm_sample_rows' rule 1: never a NaN or a -inf).
 *  2. m is the greatest candidate in the argmax's order (among == values the lowest index); mx[r] holds its bits.
 *  3. e_i = fl32(exp((double)fl(S[i] - m))) for a candidate (qgemm_softmax_rows' exp at scale 1), +0 for any other column.
 *  4. The sum: e padded with +0 to P, the least power of two >= max(w, 1024); y_i = fl(x_2i + x_2i+1) level by level;
 *     the sum is the root of that perfect binary tree.  (fl(x + +0) == x for every e, so all-padding subtrees are
 *     identities; the tree does not depend on the launch plan.)
 *  5. logz[r] = fl32(log((double)sum)).
 * A row without a candidate gives mx = logz = -inf; a row holding +inf gives logz = NaN (fl(inf - inf)).  The
 * log-probability of column i is then fl(fl(S[i] - mx) - logz).
 * With fewer than 256 rows a wide row is split by whole 1024-column blocks over `parts` workgroups (each at least 4
 * blocks, about 512 workgroups in all, parts <= 64: qgemm_logsumexp_rows_plan reports it, from rows and w alone, no GPU
 * needed) whose maxima and block sums go through `workspace` (qgemm_logsumexp_rows_workspace_size:
 * 8 * rows * parts + 4 * rows * ceil(w / 1024) bytes, 8-byte aligned; 0 for parts == 1, where workspace may be NULL, and
 * for arguments the call refuses) to a finishing launch; the result does not depend on the plan.
 * hipErrorInvalidValue: a null S / mx / logz, rows < 0, w < 1 or > 2^24, s_stride_h < w, a short, misaligned or null
 * workspace with parts > 1; rows == 0 returns 0 and touches nothing. */
QGEMM_API int qgemm_logsumexp_rows_plan(int64_t rows, int w, int *parts);
QGEMM_API size_t qgemm_logsumexp_rows_workspace_size(int64_t rows, int w);
QGEMM_API int qgemm_logsumexp_rows(const float *S, int64_t s_stride_h, int64_t rows, int w, float *mx, float *logz,
                         void *workspace, size_t ws_bytes, void *stream);
/* qgemm_beam_step: one step of beam search on the logits S, rows = n_groups * beams rows (row g * beams + b is beam b of
 * group g; 1 <= beams <= 8, rows <= 64).  scores_in: float[rows] on the device, or NULL for the start (beam 0 of every
 * group has +0, the others are dead); prev: int32[rows] on the device or NULL; eos < 0: no end token.
 *  1. A beam whose score is not > -inf is dead and contributes no candidate.
 *  2. A beam with eos >= 0, prev != NULL and prev[r] == eos is finished: it contributes exactly one candidate, token
 *     eos at rank j = 0 with its score unchanged; its logits are not used.
 *  3. Any other beam is live: its first k' = min(beams, candidates) columns t_j in the argmax's order (qgemm_sample_rows'
 *     rule 1), v_j = S[t_j], lp_j = fl(fl(v_j - mx_r) - logz_r) with qgemm_logsumexp_rows' (mx_r, logz_r), and
 *     c_j = fl(scores_in[r] + lp_j).
 *  4. Of a group's candidates those with c > -inf are ordered by greater c first, among == values (+0 equals -0) the
 *     lower b * beams + j first.  Place i < beams of the group gets parents[g * beams + i] = b (the index inside the
 *     group), tokens[g * beams + i] = t and scores_out[g * beams + i] = the bits of c.
 *  5. Places past the number of candidates get parent i, token 0 and score -inf: dead beams.
 * Every fl step is monotone in v, so this is the selection over all beams * w columns of the group under that tie rule;
 * beams == 1 gives qgemm_argmax_rows' index on every row whose column 0 is not a NaN.  parents / tokens: int32[rows],
 * scores_out: float[rows], device.  The workspace (qgemm_beam_step_workspace_size, 8-byte aligned) holds the row lists
 * of a split selection (qgemm_sample_rows' plan at top_k = beams), the log-sum-exp's workspace, mx, logz and the
 * candidates; qgemm_beam_step_plan reports the parts of the selection and of the log-sum-exp (either pointer may be
 * NULL) and needs no GPU.  The result does not depend on the plan.
 * hipErrorInvalidValue: a null S / parents / tokens / scores_out, n_groups < 0, beams < 1 or > 8, n_groups * beams > 64,
 * w < 1 or > 2^24, s_stride_h < w, a short, misaligned or null workspace; n_groups == 0 returns 0. */
QGEMM_API int qgemm_beam_step_plan(int n_groups, int beams, int w, int *select_parts, int *lse_parts);
QGEMM_API size_t qgemm_beam_step_workspace_size(int n_groups, int beams, int w);
QGEMM_API int qgemm_beam_step(const float *S, int64_t s_stride_h, int n_groups, int beams, int w, const float *scores_in,
                    const int32_t *prev, int eos, int32_t *parents, int32_t *tokens, float *scores_out, void *workspace,
                    size_t ws_bytes, void *stream);
/* qgemm_head_next_tokens with qgemm_beam_step in the argmax's place: logits of the n_groups * beams rows of H into the
 * head's buffer, then the step on them.  The head owns a beam workspace for every beams <= 8 and every row count up to
 * max_rows.  Refused before the logits are launched: what qgemm_head_next_tokens and qgemm_beam_step refuse. */
QGEMM_API int qgemm_head_beam_step(void *head, const float *H, int64_t h_stride_h, int n_groups, int beams,
                         const float *scores_in, const int32_t *prev, int eos, int32_t *parents, int32_t *tokens,
                         float *scores_out, void *stream);
/* qgemm_decoder_gather_slots reorders KV caches by a permutation that exists only on the device: destination slot
 * dst_slots[g * beams + i] takes, for every block, the K and V thirds (the 2 d_model contiguous floats at offset d_model
 * of each 3 d_model row) of self-cache rows 0 .. n_rows[g] - 1 of slot src_slots[g * beams + parents[g * beams + i]].
 * dst_slots, src_slots (n_groups * beams entries) and n_rows (n_groups) are HOST arrays read at enqueue time; parents is
 * int32[n_groups * beams] on the DEVICE, read by the kernel.  The Q third, rows at or past n_rows[g], the cross caches
 * and every other slot are not written.  On success filled[dst] = n_rows[g].  A parent outside [0, beams) cannot be
 * seen by the host: that destination's rows get quiet NaNs (0x7fc00000), nothing is read through the bad index and
 * nothing faults (qgemm_embed_rows' convention).  A copy into a second set of slots is the design: a source may be named
 * by many destinations, never a destination.
 * hipErrorInvalidValue: a decoder without caches, a null pointer, n_groups < 1, beams < 1 or > 8, n_groups * beams > 64,
 * a slot out of range or not begun, a destination named twice, a slot in both lists, n_rows[g] < 0, above max_seq or
 * above the filled length of any source slot of the group, enc_seq differing among a group's slots. */
QGEMM_API int qgemm_decoder_gather_slots(void *decoder, int n_groups, int beams, const int *dst_slots,
                               const int *src_slots, const int32_t *parents, const int *n_rows, void *stream);
/* A cache slot as it is, for inspection: block `block`'s self slab of slot `slot` (max_seq x 3 d_model floats, rows
 * [Q | K | V]) into self_rows and its cross slab (max_enc_seq x 2 d_model, rows [K2 | V2]) into cross_rows, device to
 * device in stream order; either may be NULL.  Rows at or past the filled length / enc_seq, and the Q thirds that
 * step_batch and gather_slots do not write, hold whatever was there.  hipErrorInvalidValue: a decoder without caches,
 * a block or slot out of range. */
QGEMM_API int qgemm_decoder_read_slot(void *decoder, int block, int slot, float *self_rows, float *cross_rows,
                            void *stream);
/* Beam search of n_groups sequences with `beams` beams each for n_new tokens, enqueued in ONE call with no host round
 * trip.  Two sets of rows = n_groups * beams distinct cache slots, slots_a and slots_b (rows <= 32, rows <= the head's
 * max_rows): every slot begun, slots_b[r] with the enc_seq of slots_a[r], equal inside a group, and the cross caches of
 * a group's slots equal (the caller's job: qgemm_decoder_copy_slot).  The beams' self caches are in set A.  With
 * tok_0 = tokens_in (int32[rows], device), sc_0 = scores_in (float[rows], device, or NULL for the start) and
 * cur = A for even t, B for odd t:
 *   X = head embed(tok_t, pos + t);  H = step_batch(cur, X, pos + t);
 *   (par_t, tok_{t+1}, sc_{t+1}) = head beam_step(H, sc_t, prev = tok_t, eos);
 *   gather_slots(other <- cur, par_t, pos + t + 1)                       -- after the last step too
 * par_t, tok_{t+1} and sc_{t+1} are row t of parents_out, tokens_out and scores_out ([n_new x rows], device).  pos: a
 * host array of n_groups ints, or NULL for the filled length of the group's first set-A slot.  Afterwards the beams'
 * caches are in set A for an even n_new and in set B for an odd one, and both sets report filled = pos + n_new.  A
 * second call that passes the sets in their new roles, the last row of tokens_out as tokens_in and the last row of
 * scores_out as scores_in continues the search: together they give, bit for bit, what one call gives.
 * hipErrorInvalidValue before any launch and without moving any filled length: what qgemm_decoder_generate,
 * qgemm_head_beam_step and qgemm_decoder_gather_slots refuse, rows > 32, 2 * rows > n_slots, a slot named twice in or
 * across the sets, enc_seq differing between slots_a[r] and slots_b[r] or inside a group, pos[g] < 0 or above the
 * filled length of any set-A slot of the group.  n_new == 0 returns 0. */
QGEMM_API int qgemm_decoder_generate_beam(void *decoder, void *head, int n_groups, int beams, const int *slots_a,
                                const int *slots_b, const int32_t *tokens_in, int n_new, const int *pos,
                                const float *scores_in, int eos, int32_t *tokens_out, int32_t *parents_out,
                                float *scores_out, void *stream);

/* ---- Copy-free beam search: per-row KV cache indirection in decode attention ---------------
 * A row table `row_slab` is a uint8 array in DEVICE memory, one row per sequence place, row stride row_slab_stride
 * bytes (any stride that covers the entries read, any alignment): entry [s][j] names the slab whose row j holds the K
 * and V of position j of the sequence at place s.  255 is the invalid entry (slabs <= 64).
 *
 * qgemm_attention_decode_indirect: qgemm_attention_decode_batched reading through such a table.  Same envelope and the
 * same host arrays; tab_row[b] (NULL: b) is sequence b's table row, n_slabs the slabs K and V hold.
 * Contract: BIT FOR BIT qgemm_attention_decode_batched on slabs in which row j of sequence b's slab is row j of slab
 * row_slab[tab_row[b]][j], for j < seq_kv[b]; an entry >= n_slabs stands for a row of quiet NaNs (0x7fc00000) in the
 * d_k columns of every head: nothing is loaded through such an entry, the kernel forms no address outside the
 * n_slabs slabs whatever the table holds, and the call returns normally (qgemm_decoder_gather_slots' convention).
 * Two sequences may share a table row.  Of the table the kernel reads the aligned 16-byte pieces that hold an entry
 * 0 .. seq_kv[b] - 1 of a named row.  Nothing is copied to the device, allocated or synchronized.
 * hipErrorInvalidValue before any launch: what qgemm_attention_decode_batched refuses, a null row_slab, n_slabs < 1 or
 * > 64, row_slab_stride < any seq_kv[b], any tab_row[b] < 0; n_seqs == 0 returns 0. */
QGEMM_API int qgemm_attention_decode_indirect(const float *Q, int64_t q_stride_h,
                                    const float *K, int64_t k_stride_h, int64_t k_stride_seq,
                                    const float *V, int64_t v_stride_h, int64_t v_stride_seq,
                                    float *O, int64_t o_stride_h, int n_seqs, int rows_per_seq,
                                    const uint8_t *row_slab, int64_t row_slab_stride, int n_slabs,
                                    const int *tab_row, const int *seq_kv, const int *q_pos0,
                                    int n_heads, int d_k, float scale, void *stream);
/* qgemm_beam_reindex: beam search's reorder on any row table, IN PLACE:
 *   row_slab[slots[g * beams + q]][j] = old row_slab[slots[g * beams + parents[g * beams + q]]][j],  j < n_rows[g].
 * slots (n_groups * beams table rows) and n_rows (n_groups) are HOST arrays read at enqueue time; parents is
 * int32[n_groups * beams] on the DEVICE.  The reorder is column-local (column j of a group's new rows depends on column
 * j of its old rows alone), so one thread reads a column's `beams` entries and then writes them: one table, no
 * barrier.  A parent outside [0, beams) gives that destination 255 in entries 0 .. n_rows[g] - 1.  Entries at or past
 * n_rows[g] and every other row are not written.
 * hipErrorInvalidValue before the launch: a null pointer, row_slab_stride < 1, n_groups < 1, beams < 1 or > 8,
 * n_groups * beams > 64, a slot < 0 or > 63, a slot named twice, n_rows[g] < 0 or > row_slab_stride. */
QGEMM_API int qgemm_beam_reindex(uint8_t *row_slab, int64_t row_slab_stride, int n_groups, int beams, const int *slots,
                       const int32_t *parents, const int *n_rows, void *stream);
/* The decoder's row table.  A decoder with n_slots > 1 owns ONE table of n_slots x max_seq bytes for all its blocks,
 * allocated at creation (never in a step) and filled with the identity, own[s][j] = s.  The row index inside a slab is
 * always the position: a sequence writes the row of position p into its OWN slab once, and only its descendants read
 * it afterwards.  Per slot the decoder keeps a host flag, set by beam_begin and cleared by qgemm_decoder_begin_slot: the
 * slot's slab does not hold its own sequence.  On a flagged slot qgemm_decoder_step_slot / _step_batch / _step_varlen,
 * qgemm_decoder_copy_slot and qgemm_decoder_gather_slots as source and qgemm_decoder_generate* return
 * hipErrorInvalidValue before any launch; no other call sequence sets the flag.
 *   beam_begin          for every group g the slots slots[g * beams + q] get entries 0 .. pos[g] - 1 = src_slots[g], the
 *                       slot that holds the group's prompt; their enc_seq becomes src's, filled = pos[g], the flag is
 *                       set.  They need not have been begun.  No K / V row and no cross cache is copied: one launch.
 *                       slots[g * beams] may be src_slots[g] itself.
 *   step_batch_indirect qgemm_decoder_step_batch on flagged slots with the append: the new [K | V] into slot slots[b]'s
 *                       own slab at rows pos[b] .. pos[b] + r - 1, own[slots[b]][those] = slots[b], the self-attention
 *                       over own[slots[b]][0 .. pos[b] + r - 1] through qgemm_attention_decode_indirect, the
 *                       cross-attention on the cross cache of slot cross_slots[b] (a group's beams share their prompt's;
 *                       it may be named by many).  Row for row Y is BIT FOR BIT what step_batch gives on slots whose
 *                       slabs hold the rows the table names: the same values in the same key order through one kernel text.
 *   beam_reindex        qgemm_beam_reindex on the table rows of flagged slots; filled of group g's slots = n_rows[g].
 *   read_beam_table     the table as it is, n_slots x max_seq bytes into `out` (device), in stream order: read_slot's sibling.
 * None allocates or synchronizes; slots, src_slots, cross_slots, pos and n_rows are host arrays read at enqueue time.
 * hipErrorInvalidValue before any launch and without moving any state: a decoder without a table (n_slots == 1, no
 * caches), a null pointer, n_groups < 1, beams < 1 or > 8, n_groups * beams > 64, a slot out of range or named twice;
 * beam_begin: a source not begun, pos[g] < 0 or above the rows of the source's slab that hold its own sequence (its
 * filled length; for a flagged source, which can only be one that was place 0 of its own group, the pos of that begin,
 * less what a step at an earlier position overwrote -- so the same begin may be enqueued again), a slot that is a source
 * other than place 0 of a group whose source no other group names; step_batch_indirect: what step_batch refuses, a
 * slot without the flag, a cross slot out of range, not begun or of another enc_seq; beam_reindex: a slot without the
 * flag, n_rows[g] < 0 or above the filled length of any slot of the group. */
QGEMM_API int qgemm_decoder_beam_begin(void *decoder, int n_groups, int beams, const int *slots, const int *src_slots,
                             const int *pos, void *stream);
QGEMM_API int qgemm_decoder_step_batch_indirect(void *decoder, int n_seqs, const int *slots, const int *cross_slots,
                                      const int *pos, int rows_per_seq, const float *X, float *Y, void *stream);
QGEMM_API int qgemm_decoder_beam_reindex(void *decoder, int n_groups, int beams, const int *slots,
                               const int32_t *parents, const int *n_rows, void *stream);
QGEMM_API int qgemm_decoder_read_beam_table(void *decoder, uint8_t *out, void *stream);
/* qgemm_decoder_generate_beam's loop over ONE slot set, no K / V row copied.  slots: rows = n_groups * beams distinct
 * slots begun by qgemm_decoder_beam_begin from src_slots (n_groups prompt slots, begun; they lend their cross caches).
 * rows <= the head's max_rows and the decoder's slots, so up to 64.  Per step t:
 *   X = head embed(tok_t, pos + t);  H = step_batch_indirect(slots, cross = the groups' src_slots, X, pos + t);
 *   (par_t, tok_{t+1}, sc_{t+1}) = head beam_step(H, sc_t, prev = tok_t, eos);
 *   beam_reindex(slots, par_t, n_rows = pos + t + 1)                      -- after the last step too
 * Outputs, pos (NULL: the filled length of the group's first slot) and the continuation rule are
 * qgemm_decoder_generate_beam's: every token, parent and score is BIT FOR BIT that call's, and a second call with the
 * last row of tokens_out and scores_out continues bit for bit -- without another beam_begin.  It allocates nothing and
 * does not synchronize, so it can be captured; a replay starts from the table of the capture's start only if
 * beam_begin is enqueued again before it or captured with it (a search leaves the table reordered).
 * hipErrorInvalidValue before any launch and without moving any filled length: what qgemm_decoder_generate_beam refuses
 * where it applies, rows > max_rows or > n_slots, a slot named twice or without the flag, a prompt slot not begun or of
 * another enc_seq, pos[g] < 0 or above the filled length of a slot of the group.  n_new == 0 returns 0. */
QGEMM_API int qgemm_decoder_generate_beam_indirect(void *decoder, void *head, int n_groups, int beams, const int *slots,
                                         const int *src_slots, const int32_t *tokens_in, int n_new, const int *pos,
                                         const float *scores_in, int eos, int32_t *tokens_out, int32_t *parents_out,
                                         float *scores_out, void *stream);

/* ---- Caller-supplied weights -----------------------------------------------------------
 * qgemm_pack_b_window packs B, a logical k x ncols tensor of QGEMM_F32 or QGEMM_BF16 elements with element strides
 * b_stride_h (along k) and b_stride_w (along the columns) -- an [out, in] checkpoint tensor is passed as
 * b_stride_h = 1, b_stride_w = k --, into columns col0 .. col0 + ncols - 1 of packed_b, a buffer of
 * qgemm_packed_size(n_total, k) bytes that already holds a packed k x n_total weight.  Afterwards scale[col0 ..
 * col0 + ncols - 1] and the q bytes of packed rows col0 .. col0 + ncols - 1 over all of k_pad are BIT FOR BIT what
 * qgemm_pack_b writes for those columns of any k x n_total fp32 matrix whose columns col0 .. are B (bf16 widened
 * exactly, as qgemm_pack_a_dt widens): the quantization of B is column-local.  No other byte of the scale and q
 * regions changes, and the reserved region is left alone, so windows that cover 0 .. n_total - 1 reproduce
 * qgemm_pack_b of the assembled matrix.  One launch in stream order; no allocation, no synchronization, no workspace.
 * Windows need not be multiples of 16.  The source path follows from the layout: 16-byte loads along k where
 * b_stride_h == 1 and the base and every column are 16-byte aligned, neighbouring columns side by side where
 * b_stride_w == 1, element by element through both strides otherwise; qgemm_pack_b_window_plan names it (a static
 * string; it launches nothing).
 * hipErrorInvalidValue before any launch: a null pointer, an unknown dtype, a negative stride, k < 1 or > 16384,
 * col0 < 0, ncols < 1, col0 + ncols > n_total. */
QGEMM_API int qgemm_pack_b_window(const void *B, int b_dtype, int64_t b_stride_h, int64_t b_stride_w, int k, int n_total,
                        int col0, int ncols, float range, void *packed_b, void *stream);
QGEMM_API int qgemm_pack_b_window_plan(const void *B, int b_dtype, int64_t b_stride_h, int64_t b_stride_w, int k,
                             int n_total, int col0, int ncols, const char **kernel);
/* The weights of an encoder or decoder handle (`model`), one tensor at a time.  kind is the weight kind of
 * qgemm_encoder_create / qgemm_decoder_create: 0, 1, 2 (Wq, Wk, Wv) and on a decoder 8, 9, 10 (Wq2, Wk2, Wv2) are one
 * d_model x d_k tensor per head; 3 (W_O) and on a decoder 11 (W_O2) d_model x d_model, head 0; 4 (W1) d_model x d_ff;
 * 6 (W2) d_ff x d_model; 5 and 7 the biases b1 and b2 as 1 x d_ff and 1 x d_model.  A tensor is rows x cols with y = x W:
 * rows = in features.
 * qgemm_model_weight_shape reports rows, cols and the number of heads that have such a tensor (each may be NULL); no
 * GPU call.
 * qgemm_model_set_weight loads W (element strides stride_h along the rows, stride_w along the columns; an [out, in]
 * tensor: stride_h = 1, stride_w = rows) as tensor (block, kind, head): ONE qgemm_pack_b_window launch with range 127
 * into the block's packed weight at the tensor's column offset (kind 1 of head h: column d_model + h * d_k of
 * [Wq | Wk | Wv]); a bias is a strided copy, a bf16 one widened.  Afterwards the model behaves, bit for bit, as one whose
 * seeded draw had produced those values: forward, forward_batch, step*, generate* and the beam calls keep their
 * contracts with "the weights" meaning the current ones.  It allocates nothing and does not synchronize; it runs in
 * stream order with the model's other work.  On a decoder with caches the cached keys and values are stale after it,
 * so when it is enqueued EVERY slot goes back to "not begun" (enc_seq 0, filled length 0, the beam search's flag
 * cleared): a step is refused until the slot's next begin.
 * hipErrorInvalidValue before any launch and without touching a slot: a null pointer, a kind the model lacks (8 .. 11
 * on an encoder), block or head out of range (head != 0 for a kind without heads), an unknown dtype, a negative stride.
 * qgemm_model_packed_weight / qgemm_model_bias give READ-ONLY access for tests and tools: the packed buffer of block's
 * weight `which` = 0 .. 6 (wqkv, wo, w1, w2 and on a decoder wq2, wkv2, wo2) with its n packed rows and k, and bias 5
 * or 7 with its n floats -- device pointers owned by the model. */
QGEMM_API int qgemm_model_weight_shape(void *model, int kind, int *rows, int *cols, int *heads);
QGEMM_API int qgemm_model_set_weight(void *model, int block, int kind, int head, const void *W, int dtype, int64_t stride_h,
                           int64_t stride_w, void *stream);
QGEMM_API int qgemm_model_packed_weight(void *model, int block, int which, const void **packed, int *n, int *k);
QGEMM_API int qgemm_model_bias(void *model, int block, int kind, const float **bias, int *n);

/* ---- LLM.int8() outlier decomposition ------------------------------------------
 * Feature columns k of A (= rows of B) holding an element with NOT(|x| <= threshold) (the reference's
 * AbsCompareLTEConstFunc, op_elemwise.cuh:293-306; NaN counts as an outlier) are multiplied in fp32,
 * the rest by the int8 chain, so outliers no longer set the absmax scales:
 *   C = fl( op_quantized_mm(A', B') + fmaf-chain over the outlier columns in ascending k )
 * with A' / B' = A / B with those columns / rows zeroed (no outlier column: the plain op_mm_quantize).
 * A: m x k, B: k x n, C: m x n, row-major contiguous, device pointers.  threshold: 6.0 in LLM.int8(). */
QGEMM_API size_t qgemm_mm_outlier_workspace_size(int m, int n, int k);
QGEMM_API int qgemm_mm_outlier(const float *A, const float *B, float *C, int m, int n, int k, float threshold,
                     void *workspace, size_t ws_bytes, void *stream);
/* number of outlier columns found by the last qgemm_mm_outlier / qgemm_linear_outlier on this workspace
 * (synchronizes) */
QGEMM_API int qgemm_outlier_count(int k, const void *workspace, int *count);

/* ---- LLM.int8() outlier decomposition on a CACHED weight ------------------------------------------
 * Y = linear_outlier(X, packed W, threshold [, bias] [, relu]): the decomposition for a weight quantized once by
 * qgemm_pack_b(range 127) -- int8 values Wq (k x n), scales Cw -- as LLM.int8() inference runs it: the outlier
 * columns of the activations are found per call and multiplied against the matching weight rows DEQUANTIZED FROM THE
 * CACHED int8, so no fp32 weight is read or kept.  X: m x k fp32, unit inner stride, row stride x_stride_h.
 *   outlier column k : some X[i,k] with NOT(|x| <= threshold), as qgemm_mm_outlier (NaN counts)
 *   X'               : X with those columns as +0
 *   O8               = op_quantized_mm(X', W) on the cached Wq / Cw: X' is zero in the outlier columns, so Wq's outlier
 *                      rows contribute nothing and are not zeroed, and Cw is the full column's scale
 *   Wd[k,j]          = fl( fl( float(Wq[k,j]) * Cw[j] ) * fl(1/127) ), outlier rows k only: two IEEE roundings
 *   Co               = fmaf chain from +0 over the outlier columns in ascending k of X[i,k] * Wd[k,j]
 *   O                = fl(O8 + Co); with no outlier column O = O8 with NO add (an O8 of -0 stays -0)
 *   Y                = O, then fl(O + bias[j]) when bias != NULL, then (y < 0 ? 0 : y) when relu (relu needs a bias)
 * With no outlier column Y is bit-identical to qgemm_linear.  qgemm_mm_outlier differs: it takes an fp32 B, defines
 * the int8 part on B' (outlier rows zeroed, so Cw depends on the activations) and multiplies the fp32 rows.
 * workspace: qgemm_linear_outlier_workspace_size(m, n, k) bytes, used in stream order; the call allocates nothing,
 * makes no host synchronization and keeps no state between calls (it can be captured in a HIP graph);
 * qgemm_outlier_count(k, workspace, &count) reads the count of the last call on that workspace.
 * hipErrorInvalidValue: a null X / packed_w / Y, m < 0, n < 0, k < 1, NOT(threshold >= 0), relu without bias, or a
 * short workspace; m == 0 || n == 0 returns 0.  The workspace size is 0 for invalid dims. */
QGEMM_API size_t qgemm_linear_outlier_workspace_size(int m, int n, int k);
QGEMM_API int qgemm_linear_outlier(const float *X, int64_t x_stride_h, int m, int k, const void *packed_w, int n,
                         const float *bias, int relu, float threshold, float *Y, int64_t y_stride_h,
                         void *workspace, size_t ws_bytes, void *stream);

/* The reference's quantization-error metric on the device: E = fl(C - O) per
 * element (op_subtract, op_elemwise.cuh:531-542), C = the unquantized product, O = the quantized one;
 * count elements, contiguous.  stats = DEVICE array of 5 doubles:
 *   [0] the reference's "Mean Quantization error" (tensor.cuh:201-211: signed, summed sequentially in
 *       fp32, / (float)count) -- computed only when reference_order != 0 (one lane, slow), else NaN
 *   [1] signed mean (fp64)  [2] mean |E|  [3] max |E|  [4] mean |C|   (relative error = [2] / [4])
 * Deterministic (fixed reduction tree for a given count). */
QGEMM_API int qgemm_error_stats(const float *C, const float *O, int64_t count, int reference_order, double *stats,
                      void *stream);

/* Deterministic U[lo,hi) fill, bit-identical to oracle_fill_uniform (stands in for the
 * reference's cuRAND op_uniform_init, op_elemwise.cuh:728-744). */
QGEMM_API int qgemm_fill_uniform(float *dst, int64_t count, uint64_t seed, float lo, float hi, void *stream);

/* Diagnostics: record hipEvent_t start_event / stop_event exactly at the start and end of the GEMM
 * kernel of the NEXT op_mm_quantize* / qgemm_mm_packed call made by this thread (then cleared).
 * Used by bench.py to time the dominant kernel inside its timed region.  NULL, NULL = off. */
QGEMM_API int qgemm_set_gemm_events(void *start_event, void *stop_event);
/* How those events are taken: 0 = hipExtLaunchKernel start/stop (default), 1 = hipEventRecord on the
 * stream right before / after the GEMM launch. */
QGEMM_API int qgemm_set_event_mode(int mode);

/* Diagnostics: the int8 GEMM launch plan op_mm_quantize* / qgemm_mm_packed use for an m x n x k call:
 * returns the number of K slices (1 = no split-K; < 0 on invalid sizes) and, when non-NULL, the
 * macro-tile edge (256, 64 or 32) and a static string naming the kernel. */
QGEMM_API int qgemm_gemm_plan(int m, int n, int k, int *tile, const char **kernel);

/* Library identification: "qgemm <version> gfx950 <kernel config>". */
QGEMM_API const char *qgemm_version(void);

/* ---- The standard post-LN transformer block ---------------------------------------------
 * The reference's block normalises with (y - mean) / var, adds the attention's multiHeadOut as every residual, has no
 * projection biases and only relu.  QGEMM_ARCH_STANDARD is the block of "Attention Is All You Need" and of
 * torch.nn.TransformerEncoderLayer / TransformerDecoderLayer with norm_first=False, every linear on the int8 path:
 *   x1 = LN1(x  + SelfAttn(x) W_O + b_O)
 *   x2 = LN2(x1 + CrossAttn(x1, enc) W_O2 + b_O2)        (decoder)
 *   y  = LN3(x2 + act(x2 W1 + b1) W2 + b2)               act: relu or tanh-form GELU
 *
 * qgemm_layernorm_rows: Y = LN(A + B) on rows x w floats, contiguous rows, w <= 4096; B may be NULL (Y = LN(A)).
 * gamma, beta: w floats.  Every step is ONE IEEE fp32 operation, no contraction and no fma:
 *   v[c]  = fl(A[c] + B[c])                        (B == NULL: v[c] = A[c])
 *   mean  = fl(rowsum(v) / fl32(w))
 *   d[c]  = fl(v[c] - mean)
 *   var   = fl(rowsum(fl(d[c] d[c])) / fl32(w))
 *   rstd  = fl(1 / fl(sqrt(fl(var + eps))))
 *   Y[c]  = fl(fl(fl(d[c] rstd) gamma[c]) + beta[c])
 * rowsum -- the order is part of the contract, and it is NOT the reference's sequential chain (nothing pins it here,
 * and that chain is what the reference architecture's add + layernorm spends its time on):
 *   partial p[l], l = 0 .. 63, starts at +0 and adds, in increasing c, the elements whose float4 column c / 4 is
 *   congruent to l modulo 64 (lane l reads float4 columns l, l + 64, ..);
 *   then six butterfly steps p[l] = fl(p[l] + p[l ^ off]), off = 32, 16, 8, 4, 2, 1 (for every l at once: an fp32 add
 *   is commutative, so the two lanes of a pair hold the same bits); every p[l] ends as the same value, the sum.
 * The order depends on w alone: not on rows, not on the launch a shape takes -- 16-byte aligned rows of w % 4 == 0
 * floats stay in registers through float4 loads, any other w or alignment fills the same registers float by float and
 * gives the same bits.  eps is any float; with eps = 0 a constant row gives d = 0, rstd = inf, 0 inf = NaN.
 * Y may be the same buffer as A or as B (the same rows): a row belongs to one wave, which reads all of it before it
 * writes.  For that reason A, B and Y are not restrict-qualified inside the library; gamma and beta must not overlap Y.
 * qgemm_layernorm_pack_a: the same, and Y's rows are also written packed into packed_a (qgemm_packed_size(rows, w)
 * bytes) with the operations of qgemm_pack_a: the scale and q regions equal qgemm_pack_a(Y, range) byte for byte,
 * padding rows and columns included.  Workspace-free: one launch, no allocation, no synchronization.
 * hipErrorInvalidValue before any launch: a null A / gamma / beta / Y (/ packed_a), w < 1 or > 4096, rows < 0;
 * rows == 0 returns 0. */
QGEMM_API int qgemm_layernorm_rows(const float *A, const float *B_or_null, const float *gamma, const float *beta, float eps,
                         float *Y, int64_t rows, int w, void *stream);
QGEMM_API int qgemm_layernorm_pack_a(const float *A, const float *B_or_null, const float *gamma, const float *beta,
                           float eps, float *Y, int64_t rows, int w, float range, void *packed_a, void *stream);

/* qgemm_gelu_rows: the tanh-form GELU, elementwise on rows x w floats (unit inner stride, row strides in floats),
 * written as x sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3) -- algebraically 0.5 x (1 + tanh(u)) -- so that it needs
 * only the correctly rounded exp the softmax uses; every other step ONE IEEE fp32 operation:
 *   t = fl(x C1)                         C1 = fl32(2 sqrt(2/pi)) = 0x3FCC422A
 *   q = fl(fl(fl(x x) 0.044715f) + 1.0f)
 *   z = fl(t q)
 *   e = fl32(exp((double)(-z)))
 *   g = fl(x / fl(1.0f + e))
 * NaN and +-inf give what these operations give (-inf: NaN; a very negative x: x / inf = -0).  The erf form is not
 * offered: its bits would hang on a library's double erf, and it differs from this form by at most 4.7e-4 absolute,
 * far below one int8 step of a row whose absmax is of order 1.
 * qgemm_gelu_pack_a: packed_a (qgemm_packed_size(m, k) bytes) = qgemm_pack_a(gelu_rows(X), range) byte for byte over the
 * scale and q regions, the GELU'd matrix never written: the hidden layer of a GELU FFN is written once by the W1 GEMM
 * and read once by this pack.  The signed first element of the GELU'd row seeds its absmax, as in qgemm_pack_a.
 * k <= 16384; one launch, no workspace, no allocation, no synchronization.
 * hipErrorInvalidValue before any launch: a null pointer, a negative stride, w < 1 / k < 1 or k > 16384, rows < 0 /
 * m < 0; rows == 0 / m == 0 returns 0. */
QGEMM_API int qgemm_gelu_rows(const float *X, int64_t x_stride_h, float *Y, int64_t y_stride_h, int64_t rows, int w,
                    void *stream);
QGEMM_API int qgemm_gelu_pack_a(const float *X, int64_t x_stride_h, int m, int k, float range, void *packed_a, void *stream);

/* qgemm_model_create: the one creator that knows architectures.  desc->size = sizeof(qgemm_model_desc).
 * arch = QGEMM_ARCH_REFERENCE creates exactly what the matching older creator creates -- cross = 0:
 * qgemm_encoder_create_rows (flags, n_slots and max_enc_seq must be 0 / 0 or 1 / anything); cross = 1:
 * qgemm_decoder_create_rows where n_slots > 1 or max_rows > 0 (flags must then be CAUSAL | KV_CACHE), else
 * qgemm_decoder_create_ex -- with the same argument checks and the same seeded weights.  n_slots = 0 means 1.
 * arch = QGEMM_ARCH_STANDARD: the block above.  The twelve matrices and b1, b2 are drawn exactly as on the reference
 * architecture (same seeds, kinds and bounds); the new tensors are set to b = +0, gamma = 1, beta = +0:
 *   kind 12, 13, 14  b_q, b_k, b_v     1 x d_model each (all heads side by side)
 *   kind 15          b_o               1 x d_model
 *   kind 16, 17      gamma1, beta1     1 x d_model        LN1
 *   kind 18, 19      gamma3, beta3     1 x d_model        LN3, the FFN's
 *   kind 20, 21, 22  b_q2, b_k2, b_v2  1 x d_model each   decoder
 *   kind 23          b_o2              1 x d_model        decoder
 *   kind 24, 25      gamma2, beta2     1 x d_model        decoder, LN2
 * qgemm_model_set_weight, qgemm_model_weight_shape and qgemm_model_bias take them on a standard model (head 0; the
 * strided widening row copy of kinds 5 and 7) and refuse them on a reference model as kinds the model lacks; 20 .. 25
 * are refused on an encoder.  The fused biases live as one 3 d_model vector beside [Wq | Wk | Wv], one d_model vector
 * beside Wq2 and one 2 d_model vector beside [Wk2 | Wv2], so the GEMM epilogue adds them with no launch of their own.
 * activation = QGEMM_ACT_GELU_TANH (standard only): W1 runs without relu and the pack in front of W2 is
 * qgemm_gelu_pack_a's.  ln_eps: the epsilon of every LN.
 * The handle works with every qgemm_encoder_* (cross = 0) / qgemm_decoder_* (cross = 1) / qgemm_model_* call and with
 * that family's destroy.  Every contract of those calls that rests on row-locality carries over: the new steps are
 * row-local.  hipErrorInvalidValue: a null pointer, a wrong size, an unknown arch or activation, GELU on the reference
 * architecture, GELU with d_ff > 16384 (qgemm_gelu_pack_a's limit), a negative or NaN ln_eps, and whatever the older
 * creators refuse.  arch also takes the pre-LN modifier bits QGEMM_ARCH_NORM_FIRST / QGEMM_ARCH_FINAL_NORM (below).
 * qgemm_model_info reads the descriptor back (n_slots as created, 1 for 0). */
#define QGEMM_ARCH_REFERENCE 0
#define QGEMM_ARCH_STANDARD 1
#define QGEMM_ACT_RELU 0
#define QGEMM_ACT_GELU_TANH 1
typedef struct {
    uint32_t size; /* sizeof(qgemm_model_desc), for later growth */
    int cross;     /* 0 encoder, 1 decoder */
    int d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq;
    uint64_t seed;
    int flags;             /* QGEMM_DECODER_* */
    int n_slots, max_rows; /* 0: the defaults of the older creators */
    int arch;              /* QGEMM_ARCH_* */
    int activation;        /* QGEMM_ACT_* (standard only) */
    float ln_eps;
} qgemm_model_desc;
QGEMM_API int qgemm_model_create(const qgemm_model_desc *desc, void **model);
QGEMM_API int qgemm_model_info(void *model, qgemm_model_desc *desc);

/* ---- Pre-LN blocks: norm-first stacks, a final norm, fused add + LN + pack -----------------
 * The block of GPT-2, Whisper, mBART, ViT and torch.nn.Transformer*Layer(norm_first=True): every sub-layer normalises
 * its own input and adds its output to the un-normalised residual stream (an encoder lacks the middle line):
 *   x = x + SelfAttn(LN1(x)) W_O + b_O
 *   x = x + CrossAttn(LN2(x), enc) W_O2 + b_O2
 *   x = x + act(LN3(x) W1 + b1) W2 + b2
 *   after the last block:  y = LNf(x)  (QGEMM_ARCH_FINAL_NORM)   or   y = x
 * It is QGEMM_ARCH_STANDARD with two modifier bits on qgemm_model_desc.arch, which does not grow:
 *   arch = QGEMM_ARCH_STANDARD | QGEMM_ARCH_NORM_FIRST [| QGEMM_ARCH_FINAL_NORM]
 * hipErrorInvalidValue: any other bit above the low byte, NORM_FIRST on the reference architecture, FINAL_NORM without
 * NORM_FIRST.  qgemm_model_info returns arch as given.  Kinds 12 .. 25 keep their meaning: gamma1 / beta1 belong to the
 * LN in front of the self-attention, gamma2 / beta2 to the one in front of the cross-attention, gamma3 / beta3 to the
 * one in front of the FFN.  A FINAL_NORM model has two more vectors, addressed with block = 0, head = 0:
 *   kind 26, 27      gamma_f, beta_f   1 x d_model        LNf; created as gamma = 1, beta = +0
 * with the copy path of kinds 5 and 7; every other model refuses them, and so does any other block index.  Setting
 * them resets the cache slots as every kind does.  Cross keys and values come from enc_out as given.  Each sub-layer
 * boundary is ONE launch of qgemm_prenorm_pack_a's kernel (block 0 begins with LN1 of X, which is never written), so a
 * pre-LN block has the launch count of the post-LN block; the last boundary is qgemm_layernorm_rows with gamma_f,
 * beta_f, or qgemm_add_rows.  Every new step is row-local, so every contract of the cached, batched, varlen and
 * generate calls that rests on row-locality carries over.
 *
 * qgemm_prenorm_pack_a: the norm-first form of qgemm_layernorm_pack_a's kernel.  On rows x w floats, contiguous rows:
 *   S[c] = v[c] = fl(A[c] + B[c])      one fp32 add; B == NULL: S[c] = A[c]; S == NULL: the store is skipped
 *   packed_a    = the scale and q regions qgemm_layernorm_pack_a writes for the same A, B, gamma, beta, eps and range,
 *                 byte for byte, padding rows and columns included: the pack of LN(v) by qgemm_layernorm_rows'
 *                 contract (every arithmetic step and both sums' order); the normalised fp32 row is never stored.
 * S may be A or B (the same rows): a wave reads its whole row before it writes, and A, B and S are not restrict-
 * qualified inside the library; gamma and beta must not overlap S.  w <= 4096.  16-byte aligned base pointers (S
 * included) with w % 4 == 0 stay in registers through float4 loads and stores, anything else goes float by float and
 * gives the same bits.  One launch, no workspace, no allocation, no synchronization.
 * hipErrorInvalidValue before any launch: a null A / gamma / beta / packed_a, w < 1 or > 4096, rows < 0; rows == 0
 * returns 0.
 * qgemm_add_rows: S = fl(A + B) alone, the same rows, paths and aliasing rules; a null A / B / S is refused. */
#define QGEMM_ARCH_NORM_FIRST 0x100 /* with QGEMM_ARCH_STANDARD only */
#define QGEMM_ARCH_FINAL_NORM 0x200 /* with QGEMM_ARCH_NORM_FIRST only */
QGEMM_API int qgemm_prenorm_pack_a(const float *A, const float *B_or_null, const float *gamma, const float *beta, float eps,
                         float *S_or_null, int64_t rows, int w, float range, void *packed_a, void *stream);
QGEMM_API int qgemm_add_rows(const float *A, const float *B, float *S, int64_t rows, int w, void *stream);

/* ---- Decoder-only stacks and rotary position embeddings -------------------------------------
 * Two more modifier bits on qgemm_model_desc.arch, which does not grow; any bit above them is refused.
 *
 * QGEMM_ARCH_DECODER_ONLY: a model of the decoder family (cross = 1 only; with cross = 0 it is refused) whose blocks
 * lack the cross-attention third -- self-attention, the boundary, FFN, the boundary: the encoder's block, under the
 * decoder's causal mask and with its caches (GPT-2, OPT).  Valid on every base architecture.  max_enc_seq must be 0;
 * every other check of the decoder creators applies (flags, n_slots, max_rows).  The weights are the ENCODER's: the
 * same kinds, heads, bounds and seeds, so with flags = 0 qgemm_decoder_forward gives, bit for bit, qgemm_encoder_forward
 * of an encoder with the same sizes, seed and arch bits; kinds 8 .. 11 and 20 .. 25 are refused as on an encoder, and
 * a pre-LN block's second norm is gamma3 / beta3.  No cross weights, scratch or slabs exist.  The handle takes every
 * qgemm_decoder_* and qgemm_model_* call and the decoder's destroy:
 *   qgemm_decoder_forward              enc_out must be NULL and enc_seq 0 (anything else: hipErrorInvalidValue)
 *   qgemm_decoder_begin / begin_slot   the same arguments; NO launch: the slot becomes "begun" with filled = 0 and
 *                                      its indirect flag cleared
 *   step, step_slot, step_batch, step_varlen, generate, generate_sampled, generate_beam, generate_beam_indirect,
 *   beam_begin, beam_reindex           the same contracts, without the cross launches
 *   copy_slot, gather_slots            the self slabs only
 *   step_batch_indirect                cross_slots is checked as before (in range, begun) and otherwise unused
 *   read_slot                          cross_rows must be NULL
 *   slot_state                         *enc_seq is 0 whether or not the slot is begun: ask qgemm_decoder_slot_begun
 * qgemm_decoder_slot_begun (any decoder with caches): *begun = 1 between the slot's begin (or a copy / beam_begin that
 * made it a sequence) and the next qgemm_model_set_weight, else 0; with cross-attention that is enc_seq >= 1.
 *
 * QGEMM_ARCH_ROPE: rotary position embeddings on the self-attention's Q and K (GPT-NeoX, Llama: the half-split
 * "rotate_half" pairing, not the interleaved one).  Valid on QGEMM_ARCH_STANDARD only (post-LN or pre-LN; encoder,
 * decoder or decoder-only) and where d_k = d_model / n_heads is even.  The model owns two tables, addressed with
 * block = 0, head = 0, which exist on ROPE models only (every other model refuses the kinds):
 *   kind 28, 29      rope_cos, rope_sin   max_seq x d_k / 2 each
 * filled at creation on the host in double precision,
 *   inv_i = pow(10000.0, -2.0 i / d_k),  cos[p][i] = (float)cos((double)p inv_i),  sin[p][i] = (float)sin((double)p inv_i)
 * qgemm_model_set_weight replaces a table (another theta, a scaled table) by the strided widening copy of the bias
 * kinds, one copy per table row, and resets the cache slots as every kind does; qgemm_model_weight_shape reports
 * max_seq x d_k / 2; qgemm_model_bias refuses the kinds, qgemm_model_rope_tables returns non-owning device pointers
 * (rows = max_seq, half = d_k / 2; rows / half may be NULL).  In every block ONE qgemm_rope_rows[_varlen] launch
 * follows the QKV GEMM: the Q and K thirds of the call's new rows (2 n_heads groups of d_k at stride 3 d_model), each
 * row at its absolute position -- 0 .. for a forward and for every sequence of a batched forward, pos .. for a step.
 * V is not touched, the caches hold rotated K, and the cross-attention is never rotated.  The rotation is row-local
 * and depends on the row's own position alone, so every contract that rests on row-locality and the prefix property
 * carries over.
 *
 * qgemm_rope_rows: in place on `rows` rows of `groups` consecutive groups of d_k floats, rows stride_h floats apart;
 * row r stands at position p = pos0 + r.  With h = d_k / 2, c = cos[p h + i], s = sin[p h + i], i < h, per group:
 *   a = x[i], b = x[i + h]               both read before either is written
 *   x[i]     = fl(fl(a c) - fl(b s))
 *   x[i + h] = fl(fl(b c) + fl(a s))
 * Every step is ONE IEEE fp32 operation: no contraction, no fma.  NaN and +-inf give what these operations give.  No
 * trigonometry runs on the device: cos and sin are the caller's tables of table_rows x h floats.  Where d_k % 8 == 0
 * and X, stride_h and both tables are 16-byte aligned a thread moves one float4 of the low half and the matching one
 * of the high half, else one pair; both give the same bits.  One launch, no workspace, no allocation, no
 * synchronization; capturable.
 * qgemm_rope_rows_varlen: n_seqs <= 64 sequences in one launch; sequence b is rows row0[b] .. row0[b] + n_rows[b] - 1
 * of X at positions pos0[b] ..; the three arrays are HOST arrays read at enqueue time (they travel in the kernel
 * arguments).  Rows between the sequences are not touched; sequences must not overlap.
 * hipErrorInvalidValue before any launch: a null pointer; d_k odd or < 2; groups < 1; stride_h < groups d_k (a
 * negative one included) or groups d_k past int32; rows < 0 or n_rows[b] < 0; row0[b] < 0; n_seqs < 1 or > 64; table_rows < 1; any position
 * < 0 or >= table_rows (pos0 itself, and pos0 + rows - 1).  rows == 0 (every n_rows[b] == 0) returns 0. */
#define QGEMM_ARCH_DECODER_ONLY 0x400 /* with cross = 1 only; max_enc_seq = 0 */
#define QGEMM_ARCH_ROPE 0x800         /* with QGEMM_ARCH_STANDARD only; d_model / n_heads even */
QGEMM_API int qgemm_decoder_slot_begun(void *decoder, int slot, int *begun);
QGEMM_API int qgemm_model_rope_tables(void *model, const float **cos, const float **sin, int *rows, int *half);
QGEMM_API int qgemm_rope_rows(float *X, int64_t stride_h, int64_t rows, int groups, int d_k, const float *cos,
                    const float *sin, int table_rows, int pos0, void *stream);
QGEMM_API int qgemm_rope_rows_varlen(float *X, int64_t stride_h, int groups, int d_k, const float *cos, const float *sin,
                           int table_rows, int n_seqs, const int64_t *row0, const int *n_rows, const int *pos0,
                           void *stream);

/* ---- Llama-style blocks: RMSNorm and the gated FFN -------------------------------------------
 * Two more modifier bits on qgemm_model_desc.arch, which does not grow, valid on QGEMM_ARCH_STANDARD only; either
 * combines with post-LN or pre-LN, with an encoder, a decoder or a decoder-only model, and with or without ROPE.  Bit
 * 0x1000 is NOT a bit of arch and stays refused, as does every bit from 0x8000 up.  Grouped-query attention is not
 * part of this: n_kv_heads = n_heads (the Llama-1 / Llama-2 7B and 13B shape).
 *
 * QGEMM_ARCH_RMSNORM: every norm of the model -- LN1, LN2, LN3 and the final norm -- is the root-mean-square norm of
 * Llama, Mistral, Qwen, Gemma and T5, with gamma alone.  The beta kinds 17, 19, 25 and 27 do not exist on such a model:
 * qgemm_model_set_weight, qgemm_model_weight_shape and qgemm_model_bias refuse them.  The gamma kinds keep their
 * numbers and meaning; ln_eps is the norm's epsilon.  The launch counts do not change: every boundary is the same ONE
 * launch, of the RMS form below.
 *
 * QGEMM_ARCH_GATED_FFN: the block's FFN is
 *   t = (act(x W1 + b1) * (x W3 + b3)) W2 + b2          act: relu (ReGLU), tanh-form GELU (GEGLU) or SiLU (SwiGLU)
 * with two more tensors per block, which every other model refuses as kinds it lacks:
 *   kind 30          W3                d_model x d_ff     head 0; the UP projection.  Kind 4, W1, is the GATE, the
 *                                                         activated one, and kind 6, W2, is down: Meta's w1 / w3 / w2,
 *                                                         Hugging Face's gate_proj / up_proj / down_proj
 *   kind 31          b3                1 x d_ff           created +0, with the copy path of kinds 5 and 7
 * W3 is drawn at creation as the stream encoder_weight_seed(seed, block, 30, 0) with W1's bound.  The block's packed W1
 * is [W1 | W3], d_model x 2 d_ff, and [b1 | b3] sits beside it, as [Wq | Wk | Wv] and its bias do: ONE GEMM produces
 * gate and up, qgemm_model_set_weight(kind 30) is one qgemm_pack_b_window launch at column d_ff, and
 * qgemm_model_packed_weight(block, 2) reports n = 2 d_ff.  Setting either kind resets the cache slots as every kind
 * does.  The FFN stays three launches: the W1 GEMM, qgemm_glu_pack_a's kernel, the W2 GEMM; no fp32 matrix of the
 * product is written.  d_ff <= 16384 (qgemm_glu_pack_a's limit); where the older creators bound max_rows by d_ff, a
 * gated model is bound by 2 d_ff.
 * QGEMM_ACT_SILU is valid together with QGEMM_ARCH_GATED_FFN only: an ungated SiLU FFN is no known model's.
 * Every new step is row-local, so every contract of the cached, batched, varlen, generate and beam calls that rests
 * on row-locality carries over.  qgemm_model_info returns arch and activation as given.
 *
 * qgemm_rmsnorm_rows: on rows x w floats, contiguous rows, w <= 4096, with the aliasing and alignment rules of
 * qgemm_layernorm_rows.  Every step is ONE IEEE fp32 operation, no contraction and no fma:
 *   v[c] = fl(A[c] + B[c])                      (B == NULL: v[c] = A[c])
 *   ms   = fl(rowsum(fl(v[c] v[c])) / fl32(w))
 *   r    = fl(1 / fl(sqrt(fl(ms + eps))))
 *   Y[c] = fl(fl(v[c] r) gamma[c])
 * rowsum is EXACTLY qgemm_layernorm_rows': lane l's partial over float4 columns l, l + 64, .. from +0, then six butterfly
 * steps; the order depends on w alone, positions past the row do not change the sum, and the float-by-float path
 * gives the float4 path's bits.  This is the order of Hugging Face's LlamaRMSNorm / T5LayerNorm: scale by the
 * reciprocal root first, then by the weight.  With eps = 0 a zero row gives r = inf, 0 inf = NaN.
 * qgemm_rmsnorm_pack_a: the same, and Y's rows also written packed: the scale and q regions equal qgemm_pack_a(Y, range)
 * byte for byte, padding rows and columns included.
 * qgemm_prenorm_rms_pack_a: the norm-first form, S = v stored before normalising (S == NULL: not stored; S may be A or
 * B), the normalised row written only packed, byte for byte qgemm_rmsnorm_pack_a's.
 * qgemm_add_rows serves an RMS model unchanged.  One launch each, no workspace, no allocation, no synchronization.
 * hipErrorInvalidValue before any launch: a null A / gamma (/ Y / packed_a), w < 1 or > 4096, rows < 0; rows == 0
 * returns 0.
 *
 * qgemm_glu_rows: a row of X holds 2w floats, the gate in columns 0 .. w - 1 and up in w .. 2w - 1 (unit inner stride,
 * row strides in floats); Y is rows x w:
 *   a    = act(X[c])        QGEMM_ACT_RELU:      (g < 0 ? 0 : g), the GEMM epilogue's relu
 *                           QGEMM_ACT_GELU_TANH: qgemm_gelu_rows' five steps
 *                           QGEMM_ACT_SILU:      e = fl32(exp((double)(-g))),  a = fl(g / fl(1.0f + e))
 *   Y[c] = fl(a * X[w + c])
 * NaN, +-inf and -0 give what these operations give; silu(-inf) is NaN.
 * qgemm_glu_pack_a: packed_a (qgemm_packed_size(m, k) bytes) = qgemm_pack_a(glu_rows(X), range) byte for byte over the
 * scale and q regions, the signed first element of the product row seeding its absmax as in qgemm_pack_a, padding rows
 * and columns zeroed; the product matrix is never written.  k <= 16384; one launch, no workspace, no allocation, no
 * synchronization; capturable.  16-byte aligned X with k % 4 == 0 and x_stride_h % 4 == 0 (or m == 1) loads float4s,
 * anything else goes float by float and gives the same bits.
 * hipErrorInvalidValue before any launch: a null pointer, an unknown activation, a negative stride, x_stride_h < 2k
 * (2w) or y_stride_h < w with more than one row, w < 1 / k < 1 or k > 16384, rows < 0 / m < 0; rows == 0 / m == 0
 * returns 0. */
#define QGEMM_ARCH_RMSNORM 0x2000   /* with QGEMM_ARCH_STANDARD only */
#define QGEMM_ARCH_GATED_FFN 0x4000 /* with QGEMM_ARCH_STANDARD only; d_ff <= 16384 */
#define QGEMM_ACT_SILU 2            /* with QGEMM_ARCH_GATED_FFN only */
QGEMM_API int qgemm_rmsnorm_rows(const float *A, const float *B_or_null, const float *gamma, float eps, float *Y,
                       int64_t rows, int w, void *stream);
QGEMM_API int qgemm_rmsnorm_pack_a(const float *A, const float *B_or_null, const float *gamma, float eps, float *Y,
                         int64_t rows, int w, float range, void *packed_a, void *stream);
QGEMM_API int qgemm_prenorm_rms_pack_a(const float *A, const float *B_or_null, const float *gamma, float eps,
                             float *S_or_null, int64_t rows, int w, float range, void *packed_a, void *stream);
QGEMM_API int qgemm_glu_rows(const float *X, int64_t x_stride_h, float *Y, int64_t y_stride_h, int64_t rows, int w,
                   int activation, void *stream);
QGEMM_API int qgemm_glu_pack_a(const float *X, int64_t x_stride_h, int m, int k, int activation, float range,
                     void *packed_a, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QGEMM_H_ */
