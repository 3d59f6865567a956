// transformer.hip -- the counterparts of the reference's Encoder (transformer.cu:14-77; SURVEY.md s8f f1, BASELINE
// config 5) and Decoder (transformer.cu:79-168) with their GEMM call sites on the int8 quantized path: ONE stack of
// blocks, an encoder without and a decoder with the cross-attention third (DESIGN.md "Encoder", "Decoder").  One
// function, run_blocks, makes every pass over the blocks; what kind of pass it is and which architecture the blocks
// have are each decided in one place.  Softmax and add + layernorm: encoder_ops.hip.  LayerNorm with gamma and beta
// and the norm-first form: norm.hip.  The GELU pack: gelu.hip.  The attention launches: attention_launch.hip.
// A decoder-only stack (QGEMM_ARCH_DECODER_ONLY) is a handle of the decoder family (S->decoder: what
// the entry points' guards ask) whose blocks lack the cross-attention third (S->cross: what run_blocks, the weights and
// the allocations ask): the encoder's blocks with the decoder's mask, caches and calls.  QGEMM_ARCH_ROPE adds ONE
// launch per block, rope.hip's rotation of Q and K behind the QKV GEMM (rotate_qk).
//
// THE BLOCK, once and in order (run_blocks).  Every linear is pack_rows + the int8 GEMM with bias (and relu) in its
// epilogue; a boundary packs its own output, so the linear behind it quantizes nothing itself.
//   [Q | K | V] = in @ [Wq | Wk | Wv]    attention.cuh:54-56 -- ONE GEMM over all heads (per-column absmax makes this
//                                        bit-identical to per-head GEMMs); where it writes: qkv_rows
//   heads = attention(Q, K, V)           attention.cuh:58-69 -- fp32 (activation x activation): bit-exact op_mm<float>
//                                        (sequential-k fmaf), batched over heads: self_attention
//   t = heads @ W_O                      transformer.cu:52-59
//   boundary after W_O
//   decoder:  Q2 = x @ Wq2, [K2 | V2] = enc_out @ [Wk2 | Wv2], heads2 = attention(Q2, K2, V2) with the rows as queries
//             and enc_seq keys, unmasked: cross_attention; t = heads2 @ W_O2          transformer.cu:128-150
//             boundary after W_O2
//   t = act(x W1 + b1) W2 + b2           transformer.cu:62-75 / :152-167, linear.cuh:50-54.  relu in W1's epilogue; with
//                                        GELU W1 runs without relu and the pack in front of W2 is gelu.hip's fused one
//   gated (QGEMM_ARCH_GATED_FFN):  t = (act(x W1 + b1) * (x W3 + b3)) W2 + b2 -- the block's packed W1 is
//                                        [W1 | W3], so ONE GEMM writes gate | up, and the pack in front of W2 is
//                                        glu.hip's: activate the gate, multiply by up, quantize; the same three launches
//   boundary after W2
//
// THE BOUNDARIES.  The architecture (qgemm_model_create's arch) is what stands between the
// sub-layers, ONE launch each; every other launch above is the same for all three.
//                    reference                       post-LN (STANDARD)                pre-LN (STANDARD | NORM_FIRST)
//   after W_O        x = LN(t + heads), packed       x = LN1(in + t), packed           stream += t; LN2 (encoder: LN3), packed
//   after W_O2       x = LN(t + heads2), packed      x = LN2(x + t), in place, packed  stream += t; LN3, packed
//   after W2         out = LN(t + mho), packed       out = LN3(x + t), packed          stream += t; next block's LN1, packed
//   after W2, last   Y = LN(t + mho)                 Y = LN3(x + t)                    Y = LNf(stream + t), or stream + t
//   reference: the LN without gamma and beta, the residual the last attention's multiHeadOut as in the reference (:58,
//     :74) -- mho = heads2 in a decoder, heads in an encoder; no projection has a bias (nullptr: the reference's call);
//   post-LN: the textbook block, x1 = LN1(x + heads W_O + b_O), x2 = LN2(x1 + heads2 W_O2 + b_O2), y = LN3(x2 + FFN(x2)).
//     The projections' biases ride in the GEMM epilogue ([b_q | b_k | b_v] beside [Wq | Wk | Wv], ..): no launch; the
//     cross caches carry b_k2 | b_v2;
//   pre-LN: x += SelfAttn(LN1(x)) W_O + b_O, x += CrossAttn(LN2(x), enc) W_O2 + b_O2, x += act(LN3(x) W1 + b1) W2 + b2
//     and y = LNf(x) [FINAL_NORM] or y = x.  Every boundary is norm.hip's norm-first form: stream += t, the NEXT
//     sub-layer's LN, its pack; the normalised rows exist only packed, the stream lives in S->x (the caller's X is read,
//     never written).  Block 0 begins with LN1 + pack of X in place of pack_rows(X) (run_blocks' prologue); the last
//     boundary is the post-LN kernel with gamma_f, beta_f (kinds 26, 27, the stack's own allocation) or
//     launch_add_rows.  enc_out enters the cross-attention as given.
//   QGEMM_ARCH_RMSNORM: every LN above, post-LN or pre-LN, is the RMS norm with gamma alone -- the same
//     launches on norm.hip's RMS instantiations (norm_rows, norm_rows_pack, prenorm_pack below pick them).
//
// Decisions where the reference cannot run as written:
//   * arity (transformer.cu:37 calls forward(X, X, out); attention.cuh:47 takes (X, out)): self attention on the block
//     input.  The decoder's attn.forward(output, enc_output, out) (:132): its first argument is read as the source of
//     the queries, its second as the source of the keys and values -- the only reading in which enc_output is used;
//   * d_ff (transformer.cu:62 sizes ffnOut {h, d_model}): the FFN hidden is {seq, d_ff};
//   * weights are drawn ONCE per stack (the reference re-draws them on every call, :34, :53, :63): they are packed
//     once (the LLM.int8() weight cache, s8f f2) -- seeded, reproducible.  W_O is redrawn at :144, so the
//     cross-attention's output projection W_O2 is a tensor of its own;
//   * heads are written straight into their column slice of multiHeadOut (no host round trip, :43-50); the residual
//     adds multiHeadOut, as the reference does (:58, :74);
//   * enc_out is quantized ONCE per forward and its packed form serves every block's [K2 | V2] projection: its
//     per-row absmax scales do not depend on the weight, so this is bit-identical to quantizing it per block.
//
// PASS KINDS.  The entry point says in a Pass which of five kinds its call is; qkv_rows, self_attention and
// cross_attention alone read the kind.  Caches (QGEMM_DECODER_KV_CACHE with QGEMM_DECODER_CAUSAL):
// every block owns n_slots self slabs of max_seq x 3 d_model ([Q | K | V] rows) and n_slots cross slabs of max_enc_seq
// x 2 d_model ([K2 | V2]); enc_seq and the filled length are kept per slot on the host; the weights exist once.
// decoder_begin_slot packs enc_out once, runs every block's [K2 | V2] projection into the slot's cross slab, records
// enc_seq and sets filled to 0: no step runs a [K2 | V2] GEMM or an enc_out pack.
//   Forward        encoder_forward, decoder_forward: the rows are a whole sequence.  [Q | K | V] and [K2 | V2] live in
//                  the stack's scratch, [K2 | V2] is projected from the packed enc_out; the mask is the stack's causal
//                  flag.  On a cached decoder it neither reads nor writes the caches.
//   Slot           decoder_step_slot (qgemm_decoder_step: slot 0): n rows at positions pos .. pos + n - 1.  The QKV GEMM
//                  writes cache rows pos .. of the slot's slab itself; those n query rows attend, masked with q_pos0 =
//                  pos, to cache rows 0 .. pos + n - 1; the cross-attention reads the slot's cross slab.
//   Batch          decoder_step_batch: r = 1 .. 8 rows of each of n_seqs different slots, M = n_seqs * r rows.  The QKV
//                  GEMM of all rows into the qkv scratch, scatter_kv_kernel copies each row's [K | V] into row pos[b] + i
//                  of its slot's slab, the batched decode launch (attention_decode.hip) reads Q from the scratch and K / V
//                  from the slabs with seq_kv[b] = pos[b] + r and q_pos0[b] = pos[b]; the batched launch again, unmasked,
//                  on the cross slabs with seq_kv[b] = the slot's enc_seq.
//   BatchIndirect  decoder_step_batch_indirect (the copy-free beam search): Batch, the self-attention
//                  reading row j of a sequence from slab own[slot][j] of the stack's row table, the cross-attention the
//                  slab of cross_slots[b].
//   Varlen         n_seqs sequences of their own lengths packed one after another (qgemm_*_create_rows);
//                  both attentions go through launch_attention_varlen (attention_launch.hip): one launch of the fused
//                  kernel over a table of sequences where every one has at most 512 keys, else sequence by sequence.
//                  encoder_forward_batch: keys and queries in the qkv scratch.  decoder_step_varlen: Batch with n_rows[b]
//                  >= 1 rows per sequence (a prefill of many slots, or prefills mixed with decoding rows): the scatter
//                  takes per-sequence row counts, keys in the slabs.
// Why every kind gives the same bits:
//   (1) row-locality.  Every step but the attention is row-local -- the pack's scales are per row, the int8 GEMM
//       accumulates exactly and dequantizes per element, every boundary of every architecture and the GELU pack work on
//       one row -- so a row gets the same bits whatever other rows share the launch, and a cache row holds what forward
//       computes for that row, whichever call wrote it;
//   (2) the prefix property.  The masked attention's row i reads K rows below its limit alone, and the V rows past it
//       enter as fmaf(+0, v, acc), which changes nothing WHILE THE CACHED V IS FINITE and no P V accumulator is -0
//       (the conditions of forward(X[:n]) == forward(X)[:n] itself; a step's key sequence ends at its
//       own last row, so there is no V row past the last limit at all).  A non-finite V row written by an earlier,
//       longer sequence is never read either: rows pos + n .. are outside the call's seq_kv.
//   Slot: by (1) and (2) the result is rows pos .. pos + n - 1 of the causal forward on the whole prefix, bit for bit.
//   Batch: row b * r + i is, bit for bit, row i of decoder_step_slot(slots[b], pos[b], r) alone: by (1) every step but
//     the attention gives a row the same bits with M = n_seqs * r or M = r, and the batched attention launch runs, per
//     (head, row, sequence), the single launch's workgroup on the same operands -- the K / V rows of the slab are the
//     same values whether a GEMM or the scatter stored them.
//   BatchIndirect: the same workgroup again, its K / V rows the same values read from the slabs the table names.
//   Varlen: by (1) the rows of B sequences run through the blocks as ONE matrix; the attention alone must know where a
//     sequence ends.  Each sequence's rows are forward's / step_slot's on it alone, bit for bit.
// pos is a host argument; the filled length is updated at enqueue time: 0 <= pos <= filled, then filled = pos + n (an
// earlier pos rewinds: speculative decoding, beam search).  The step entry points share one admission check per slot
// (admit), and every check comes before the first launch.  begin and the steps allocate nothing and do not
// synchronize; they share the stack's scratch buffers with forward, so a stack does one thing at a time.  The scratch
// buffers, the packed activations and the split-K scratch hold max(max_seq, 8 * n_slots with more than one slot,
// max_rows) rows; the scores stay sized by max_seq (the per-sequence varlen path runs one sequence at a time).
// decoder_copy_slot forks a sequence with stream-ordered device-to-device copies of the rows in use.
//
// Caller-supplied weights (qgemm_model_set_weight).  The seeded draw stays what creation does; afterwards
// stack_set_weight replaces one tensor at a time: launch_pack_b_window (weights.hip) packs it into its column window of
// the block's packed weight, a bias is copied.  Every call above then runs on the current weights.
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "qgemm_internal.h"

namespace qgemm {

namespace {

// every tensor of a block its own seed stream; 8 .. 11 are the cross-attention's
enum WeightKind { kWq = 0, kWk = 1, kWv = 2, kWo = 3, kW1 = 4, kB1 = 5, kW2 = 6, kB2 = 7,
                  kWq2 = 8, kWk2 = 9, kWv2 = 10, kWo2 = 11,
                  // the standard architecture's, 1 x d_model each; 20 .. 25 are the cross-attention's
                  kBq = 12, kBk = 13, kBv = 14, kBo = 15, kG1 = 16, kBe1 = 17, kG3 = 18, kBe3 = 19,
                  kBq2 = 20, kBk2 = 21, kBv2 = 22, kBo2 = 23, kG2 = 24, kBe2 = 25,
                  // the final norm of a pre-LN stack, 1 x d_model each, block 0's
                  kGf = 26, kBef = 27,
                  // the rotary tables of a ROPE stack, max_seq x d_k / 2 each, block 0's
                  kRopeCos = 28, kRopeSin = 29,
                  // the gated FFN's up projection and its bias: d_model x d_ff and 1 x d_ff, every block's
                  kW3 = 30, kB3 = 31 };

// QGEMM_ARCH_NORM_FIRST / _FINAL_NORM / _DECODER_ONLY / _ROPE (include/qgemm.h): modifier bits above the
// architecture's low byte; _RMSNORM / _GATED_FFN above a hole: 0x1000 is no bit of arch
constexpr int kArchNormFirst = 0x100, kArchFinalNorm = 0x200, kArchDecoderOnly = 0x400, kArchRope = 0x800;
constexpr int kArchRms = 0x2000, kArchGated = 0x4000;
constexpr int kActRelu = 0, kActGelu = 1, kActSilu = 2;  // QGEMM_ACT_*

}  // namespace

// arch as qgemm_model_create takes it: the reference's block or the standard one in the low byte; above it NORM_FIRST
// ROPE, RMSNORM and GATED_FFN on the standard block alone, FINAL_NORM with NORM_FIRST alone, DECODER_ONLY on a
// descriptor of the decoder family (cross = 1) alone, and no other bit
bool stack_arch_ok(int arch, bool cross) {
    const int base = arch & 0xff, mods = arch & ~0xff;
    if ((base != 0 && base != 1) ||
        (mods & ~(kArchNormFirst | kArchFinalNorm | kArchDecoderOnly | kArchRope | kArchRms | kArchGated)))
        return false;
    if ((mods & (kArchNormFirst | kArchRope | kArchRms | kArchGated)) && base != 1) return false;
    if ((mods & kArchDecoderOnly) && !cross) return false;
    return !(mods & kArchFinalNorm) || (mods & kArchNormFirst);
}

// activation as qgemm_model_create takes it, beside a valid arch: relu anywhere, the tanh GELU on the standard block,
// SiLU with the gate alone; the GELU pack and the gated pack hold rows of at most 16384 floats
bool stack_activation_ok(int arch, int activation, int d_ff) {
    const bool gated = (arch & kArchGated) != 0;
    if (activation < kActRelu || activation > kActSilu) return false;
    if ((arch & 0xff) == 0 && activation != kActRelu) return false;
    if (activation == kActSilu && !gated) return false;
    return !(gated || activation == kActGelu) || d_ff <= 16384;
}

// Seed of one weight tensor: every tensor its own counter stream (documented for the oracle).
uint64_t encoder_weight_seed(uint64_t base, int block, int kind, int head) {
    return base * 1000003ULL + (uint64_t)block * 4099ULL + (uint64_t)kind * 131ULL + (uint64_t)head;
}

// fl32(1 / sqrt(n)): the reference's "float max = 1.0f / std::sqrt(n)" with an int n (double sqrt).
float encoder_init_bound(int n) { return (float)(1.0 / std::sqrt((double)n)); }

struct Block {
    // packed (W^T int8 + Cw); on a gated stack w1 is [W1 | W3], d_model x 2 d_ff, gate and up in ONE GEMM
    void *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;
    void *wq2 = nullptr, *wkv2 = nullptr, *wo2 = nullptr;               // cross
    float *b1 = nullptr, *b2 = nullptr;  // (gated: b1 is [b1 | b3], 2 d_ff floats)
    // the standard architecture's vectors, ONE allocation `sp` (nullptr on a reference stack, and so is every pointer
    // into it: a nullptr bias is the reference's GEMM call): [bqkv: 3d][bo][g1][be1][g3][be3] and with cross-attention
    // [bq2][bkv2: 2d][bo2][g2][be2] -- the order of kinds 12 .. 25, the fused biases side by side as their fused
    // weights' columns are
    float *sp = nullptr, *bqkv = nullptr, *bo = nullptr, *g1 = nullptr, *be1 = nullptr, *g3 = nullptr, *be3 = nullptr;
    float *bq2 = nullptr, *bkv2 = nullptr, *bo2 = nullptr, *g2 = nullptr, *be2 = nullptr;
    // kv_cache: n_slots slabs of max_seq x 3d ([Q | K | V] rows) and n_slots slabs of max_enc_seq x 2d ([K2 | V2])
    float *qkv_cache = nullptr, *kv2_cache = nullptr;
};

struct Stack {
    int d_model = 0, n_heads = 0, d_ff = 0, n_blocks = 0, max_seq = 0, max_enc_seq = 0;
    bool decoder = false;   // the decoder family: the handle the decoder_* entry points take, with or without cross
    bool cross = false;     // the blocks have the cross-attention third (a decoder-only stack: decoder without cross)
    bool rope = false;      // Q and K are rotated by their rows' positions behind the QKV GEMM
    float *rope_t = nullptr;  // rope: [cos: max_seq x d_k / 2][sin: the same], kinds 28 and 29
    bool causal = false;    // the self-attention masks keys past the query's own row (QGEMM_DECODER_CAUSAL)
    bool kv_cache = false;  // the blocks own caches for decoder_begin / decoder_step (QGEMM_DECODER_KV_CACHE)
    int n_slots = 1;        // sequences the caches hold side by side (qgemm_decoder_create_slots)
    bool standard = false;  // the post-LN block with biases, block-input residuals and a real LayerNorm
    bool gelu = false;      // standard: the FFN's activation is the tanh-form GELU, fused into the pack in front of W2
    // standard: every norm is the RMS one, gamma alone; the FFN is (act(x W1 + b1) * (x W3 + b3)) W2 + b2,
    // act the stack's activation, applied by glu.hip's pack in front of W2 (gelu is false on a gated stack)
    bool rms = false, gated = false;
    int activation = 0;     // as created: QGEMM_ACT_*
    float ln_eps = 0.0f;    // standard: every LN's epsilon
    // standard: the pre-LN block -- every sub-layer normalises its own input and adds its output to
    // the un-normalised stream -- and whether LNf follows the last block; fn = [gamma_f][beta_f], final_norm only
    bool norm_first = false, final_norm = false;
    int arch = 0;           // as created, for stack_describe
    float *fn = nullptr;
    uint64_t seed = 0;      // as created, for stack_describe
    int max_rows = 0;
    int scratch_rows = 0;   // rows the scratch buffers hold: max_seq, 8 rows of every slot or max_rows, the largest
    // per slot, host side, updated at enqueue time: whether a sequence was begun, its enc_seq (0 without cross) and the
    // filled length (cache rows 0 .. filled - 1 hold the sequence so far)
    std::vector<char> begun;
    std::vector<int> enc_seq, filled;
    // the copy-free beam search, n_slots > 1 only: ONE row table for all blocks, n_slots x max_seq bytes
    // on the device, own[s][j] = the slot whose self slab holds row j of the sequence in slot s (the identity at
    // creation), and per slot the host flag that beam_begin sets and begin_slot clears: the slot's slab does not hold
    // its own sequence, so the plain calls refuse it.  own_rows (flagged slots): the leading rows of the slot's slab that
    // still hold the plain sequence it had -- what beam_begin may name as a prompt again (a slot that is place 0 of its
    // own group keeps its prompt rows: begin copies nothing and a step writes at or past its position)
    uint8_t *own = nullptr;
    std::vector<char> indirect;
    std::vector<int> own_rows;
    std::vector<Block> blocks;
    float *qkv = nullptr, *scores = nullptr, *heads = nullptr, *t = nullptr, *ffn = nullptr, *x = nullptr;
    float *xa = nullptr, *xb = nullptr;
    float *q2 = nullptr, *kv2 = nullptr, *heads2 = nullptr;  // cross
    char *ws = nullptr;  // [split-K scratch][packed activations][cross: packed enc_out]
    size_t scratch_bytes = 0, act_bytes = 0;
};

namespace {

hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 16); }

template <typename T>
hipError_t alloc_f(T **p, size_t count) {
    return alloc(reinterpret_cast<void **>(p), count * sizeof(T));
}

}  // namespace

// draw a K x N fp32 weight (uniform [-bound, bound), reference init formula) and pack it as B
hipError_t encoder_make_packed(int k, int n, const std::vector<uint64_t> &col_seeds, int cols_per_seed, float bound,
                               void **packed, float *tmp, hipStream_t s) {
    // col_seeds[c] fills columns [c*cols_per_seed, (c+1)*cols_per_seed) -- one reference tensor each
    hipError_t e;
    float *one = tmp + (size_t)k * n;  // k x cols_per_seed staging
    for (size_t c = 0; c < col_seeds.size(); ++c) {
        if ((e = launch_fill_uniform(one, (int64_t)k * cols_per_seed, col_seeds[c], -bound, bound, s)) != hipSuccess)
            return e;
        if ((e = hipMemcpy2DAsync(tmp + c * cols_per_seed, sizeof(float) * n, one, sizeof(float) * cols_per_seed,
                                  sizeof(float) * cols_per_seed, k, hipMemcpyDeviceToDevice, s)) != hipSuccess)
            return e;
    }
    if ((e = alloc(packed, packed_bytes(n, k))) != hipSuccess) return e;
    // B = W (k x n, row-major): reduction vectors are its columns -> pack_cols path
    return launch_pack_cols(tmp, n, k, n, 127.0f, packed_view(*packed, n, k), s);
}

namespace {

// the packed activations of the next linear (one buffer, reused by every linear in stream order) ...
PackedView act_view(Stack &S, int seq, int k) { return packed_view(S.ws + S.scratch_bytes, seq, k); }
// ... and the packed encoder output, written once per forward or begin and read by every block
PackedView enc_view(Stack &S, int enc_seq) {
    return packed_view(S.ws + S.scratch_bytes + S.act_bytes, enc_seq, S.d_model);
}

// y = quantized_mm(packed rows va, packed weight) [+ bias] [relu]
hipError_t gemm(Stack &S, const PackedView &va, int rows, int k, const void *wpacked, int n, float *y,
                const float *bias, bool relu, hipStream_t s) {
    const float inv_r2 = 1.0f / (127.0f * 127.0f);
    return launch_gemm_dequant(va, packed_view(wpacked, n, k), y, n, 1, rows, n, inv_r2, S.ws, S.scratch_bytes, s, bias,
                               relu, /*tickets_zeroed=*/true);
}

// x == nullptr: the activations are already packed in act_view (by the add+layernorm that made them)
hipError_t linear(Stack &S, const float *x, int seq, int k, const void *wpacked, int n, float *y, const float *bias,
                  bool relu, hipStream_t s) {
    // pack the activations (Cx per row: op_absmax(X), X_int8), then the GEMM with the fused epilogue
    const PackedView va = act_view(S, seq, k);
    const hipError_t e = x ? launch_pack_rows(x, k, 1, seq, k, 127.0f, va, s) : hipSuccess;
    if (e != hipSuccess) return e;
    return gemm(S, va, seq, k, wpacked, n, y, bias, relu, s);
}

}  // namespace

void stack_destroy(Stack *S) {
    if (!S) return;
    for (auto &b : S->blocks)
        for (void *p : {b.wqkv, b.wo, b.wq2, b.wkv2, b.wo2, b.w1, b.w2, (void *)b.b1, (void *)b.b2, (void *)b.sp,
                        (void *)b.qkv_cache, (void *)b.kv2_cache})
            (void)hipFree(p);
    for (void *p : {(void *)S->qkv, (void *)S->scores, (void *)S->heads, (void *)S->t, (void *)S->ffn, (void *)S->x,
                    (void *)S->q2, (void *)S->kv2, (void *)S->heads2, (void *)S->xa, (void *)S->xb, (void *)S->ws,
                    (void *)S->own, (void *)S->fn, (void *)S->rope_t})
        (void)hipFree(p);
    delete S;
}

hipError_t stack_create(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq, uint64_t seed,
                        bool decoder, bool causal, bool kv_cache, Stack **out, int n_slots, int max_rows, int arch,
                        int activation, float ln_eps) {
    *out = nullptr;
    // decoder: the family the handle belongs to; cross: whether its blocks have the cross-attention third.  A
    // decoder-only stack is of the decoder family, has the encoder's blocks and no encoder output to size anything by
    const bool cross = decoder && !(arch & kArchDecoderOnly);
    if (decoder && !cross && max_enc_seq != 0) return hipErrorInvalidValue;
    if ((arch & kArchRope) && (n_heads < 1 || d_model % n_heads || (d_model / n_heads) % 2)) return hipErrorInvalidValue;
    if (!stack_arch_ok(arch, decoder) || !stack_activation_ok(arch, activation, d_ff) || !(ln_eps >= 0.0f))
        return hipErrorInvalidValue;
    // what the W1 GEMM writes per row: d_ff floats, on a gated stack gate and up side by side
    const bool gated = (arch & kArchGated) != 0;
    const int64_t ffw = gated ? 2 * (int64_t)d_ff : d_ff;
    // max_rows: the row-local kernels (pack, GEMM epilogue, add + layernorm) address an activation buffer of
    // scratch_rows x 3 d_model or x ffw floats and its packed image of rows padded to 256 x columns padded to 128;
    // with that padded product inside int32 no element index leaves its type, whichever type a kernel forms it in
    if (max_rows < 0) return hipErrorInvalidValue;
    if (max_rows > 0 && d_model >= 2 && d_ff >= 2 &&
        (((int64_t)max_rows + 255) & ~(int64_t)255) * ((std::max(3 * (int64_t)d_model, ffw) + 127) & ~(int64_t)127) > INT32_MAX)
        return hipErrorInvalidValue;
    if (kv_cache && !causal) return hipErrorInvalidValue;
    if (n_slots < 1 || n_slots > kDecodeMaxBatch || (n_slots > 1 && !(decoder && kv_cache))) return hipErrorInvalidValue;
    if (d_model < 2 || n_heads < 1 || d_model % n_heads || d_ff < 2 || n_blocks < 1 || max_seq < 1 || max_seq > 4096 ||
        (cross && (max_enc_seq < 1 || max_enc_seq > 4096)) || d_model > 4096)
        return hipErrorInvalidValue;
    Stack *S = new (std::nothrow) Stack;
    if (!S) return hipErrorOutOfMemory;
    S->d_model = d_model;
    S->n_heads = n_heads;
    S->d_ff = d_ff;
    S->n_blocks = n_blocks;
    S->max_seq = max_seq;
    S->max_enc_seq = cross ? max_enc_seq : 0;
    S->decoder = decoder;
    S->cross = cross;
    S->rope = (arch & kArchRope) != 0;
    S->causal = causal;
    S->kv_cache = kv_cache;
    S->n_slots = n_slots;
    S->standard = (arch & 0xff) == 1;
    S->norm_first = (arch & kArchNormFirst) != 0;
    S->final_norm = (arch & kArchFinalNorm) != 0;
    S->arch = arch;
    S->rms = (arch & kArchRms) != 0;
    S->gated = gated;
    S->activation = activation;
    S->gelu = activation == kActGelu && !gated;
    S->ln_eps = ln_eps;
    S->seed = seed;
    S->max_rows = max_rows;
    // a batched step runs up to 8 rows of every slot through the scratch buffers (one slot: a step's rows fit max_seq)
    // and a batched forward or a varlen step its row budget (qgemm_*_create_rows)
    S->scratch_rows = std::max(n_slots > 1 ? std::max(max_seq, 8 * n_slots) : max_seq, max_rows);
    S->enc_seq.assign(n_slots, 0);
    S->begun.assign(n_slots, 0);
    S->filled.assign(n_slots, 0);
    S->indirect.assign(n_slots, 0);
    S->own_rows.assign(n_slots, 0);
    S->blocks.resize(n_blocks);
    const int d = d_model, dk = d_model / n_heads;
    const int rows = S->scratch_rows;
    const size_t Sq = (size_t)rows, Se = (size_t)S->max_enc_seq;
    hipError_t e = hipSuccess;
    auto fail = [&](hipError_t err) {
        stack_destroy(S);
        return err;
    };
    // scores only where some forward or step can reach the three launches (both attentions share them); else they
    // stay nullptr, which launch_attention refuses on that path
    const int max_kv = std::max(max_seq, S->max_enc_seq);
    if (attention_needs_scores(max_seq, max_kv, dk) &&
        (e = alloc_f(&S->scores, (size_t)n_heads * (size_t)max_seq * (size_t)max_kv)))
        return fail(e);
    if ((e = alloc_f(&S->qkv, Sq * 3 * d)) || (e = alloc_f(&S->heads, Sq * d)) ||
        (e = alloc_f(&S->t, Sq * d)) || (e = alloc_f(&S->ffn, Sq * (size_t)ffw)) || (e = alloc_f(&S->x, Sq * d)) ||
        (e = alloc_f(&S->xa, Sq * d)) || (e = alloc_f(&S->xb, Sq * d)))
        return fail(e);
    if (cross && ((e = alloc_f(&S->q2, Sq * d)) || (e = alloc_f(&S->kv2, Se * 2 * d)) || (e = alloc_f(&S->heads2, Sq * d))))
        return fail(e);
    // workspace: split-K scratch for the largest of the linear shapes + the packed activations (+ the packed enc_out)
    const int shapes[5][3] = {{rows, 3 * d, d}, {rows, d, d}, {rows, (int)ffw, d}, {rows, d, d_ff},
                              {S->max_enc_seq, 2 * d, d}};  // (m, n, k); the last one exists only with cross
    size_t scratch = 0;
    for (int i = 0; i < (cross ? 5 : 4); ++i)
        scratch = std::max(scratch, gemm_scratch_bytes(shapes[i][0], shapes[i][1], shapes[i][2]));
    const size_t act = std::max(packed_bytes(rows, d), packed_bytes(rows, d_ff));
    S->scratch_bytes = (scratch + 255) & ~(size_t)255;
    S->act_bytes = (act + 255) & ~(size_t)255;
    const size_t ws_bytes = S->scratch_bytes + S->act_bytes + (cross ? packed_bytes(max_enc_seq, d) : 0);
    if ((e = alloc(reinterpret_cast<void **>(&S->ws), ws_bytes))) return fail(e);
    if ((e = hipMemset(S->ws, 0, S->scratch_bytes))) return fail(e);  // split-K tickets start at zero
    if (n_slots > 1) {  // the row table, allocated here and never in a step: the identity
        std::vector<uint8_t> ident((size_t)n_slots * max_seq);
        for (int sl = 0; sl < n_slots; ++sl) std::fill_n(ident.begin() + (size_t)sl * max_seq, max_seq, (uint8_t)sl);
        if ((e = alloc(reinterpret_cast<void **>(&S->own), ident.size())) ||
            (e = hipMemcpy(S->own, ident.data(), ident.size(), hipMemcpyHostToDevice)))
            return fail(e);
    }

    // weights, drawn once with the reference's init bounds (attention.cuh:37-41, linear.cuh:34-39,
    // transformer.cu:53, :120, :144) and packed
    const size_t maxk = std::max(d, d_ff), maxn = std::max<size_t>(3 * d, ffw);
    float *tmp = nullptr;
    if ((e = alloc_f(&tmp, maxk * maxn + maxk * maxn))) return fail(e);
    hipStream_t s = nullptr;
    for (int i = 0; i < n_blocks && e == hipSuccess; ++i) {
        Block &B = S->blocks[i];
        auto head_seeds = [&](int first, int last) {
            std::vector<uint64_t> v;
            for (int kind = first; kind <= last; ++kind)
                for (int h = 0; h < n_heads; ++h) v.push_back(encoder_weight_seed(seed, i, kind, h));
            return v;
        };
        const float bk = encoder_init_bound(dk), bd = encoder_init_bound(d), bf = encoder_init_bound(d_ff);
        if ((e = encoder_make_packed(d, 3 * d, head_seeds(kWq, kWv), dk, bk, &B.wqkv, tmp, s))) break;
        if ((e = encoder_make_packed(d, d, {encoder_weight_seed(seed, i, kWo, 0)}, d, 1.0f, &B.wo, tmp, s))) break;
        if (cross) {
            if ((e = encoder_make_packed(d, d, head_seeds(kWq2, kWq2), dk, bk, &B.wq2, tmp, s))) break;
            if ((e = encoder_make_packed(d, 2 * d, head_seeds(kWk2, kWv2), dk, bk, &B.wkv2, tmp, s))) break;
            if ((e = encoder_make_packed(d, d, {encoder_weight_seed(seed, i, kWo2, 0)}, d, 1.0f, &B.wo2, tmp, s))) break;
        }
        // gated: [W1 | W3], the up projection W3 drawn as a tensor of its own with W1's bound; b3 = +0
        std::vector<uint64_t> w1_seeds = {encoder_weight_seed(seed, i, kW1, 0)};
        if (gated) w1_seeds.push_back(encoder_weight_seed(seed, i, kW3, 0));
        if ((e = encoder_make_packed(d, (int)ffw, w1_seeds, d_ff, bd, &B.w1, tmp, s))) break;
        if ((e = encoder_make_packed(d_ff, d, {encoder_weight_seed(seed, i, kW2, 0)}, d, bf, &B.w2, tmp, s))) break;
        if ((e = alloc_f(&B.b1, (size_t)ffw)) || (e = alloc_f(&B.b2, d))) break;
        if (gated && (e = hipMemsetAsync(B.b1 + d_ff, 0, sizeof(float) * d_ff, s))) break;
        if (kv_cache && ((e = alloc_f(&B.qkv_cache, (size_t)n_slots * max_seq * 3 * d)) ||
                         (cross && (e = alloc_f(&B.kv2_cache, (size_t)n_slots * Se * 2 * d)))))
            break;
        if ((e = launch_fill_uniform(B.b1, d_ff, encoder_weight_seed(seed, i, kB1, 0), -bd, bd, s))) break;
        if ((e = launch_fill_uniform(B.b2, d, encoder_weight_seed(seed, i, kB2, 0), -bf, bf, s))) break;
        if (S->standard) {  // b = +0, gamma = 1, beta = +0: nothing drawn, so no new generator contract
            const size_t nd = cross ? 16 : 8;  // vectors of d floats
            if ((e = alloc_f(&B.sp, nd * d))) break;
            float *p = B.sp;
            auto take = [&](int n) { float *r = p; p += (size_t)n * d; return r; };
            B.bqkv = take(3), B.bo = take(1), B.g1 = take(1), B.be1 = take(1), B.g3 = take(1), B.be3 = take(1);
            if (cross) B.bq2 = take(1), B.bkv2 = take(2), B.bo2 = take(1), B.g2 = take(1), B.be2 = take(1);
            std::vector<float> host(nd * d, 0.0f);
            for (float *g : {B.g1, B.g3, B.g2})
                if (g) std::fill_n(host.begin() + (g - B.sp), d, 1.0f);
            if ((e = hipMemcpy(B.sp, host.data(), sizeof(float) * host.size(), hipMemcpyHostToDevice))) break;
        }
    }
    if (e == hipSuccess && S->final_norm) {  // gamma_f = 1, beta_f = +0
        std::vector<float> host(2 * (size_t)d, 0.0f);
        std::fill_n(host.begin(), d, 1.0f);
        if (!(e = alloc_f(&S->fn, host.size())))
            e = hipMemcpy(S->fn, host.data(), sizeof(float) * host.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && S->rope) {  // theta = 10000, in double on the host; set_weight brings any other table
        const int h = dk / 2;
        std::vector<float> host(2 * (size_t)max_seq * h);
        float *c = host.data(), *sn = c + (size_t)max_seq * h;
        for (int i = 0; i < h; ++i) {
            const double inv = std::pow(10000.0, -2.0 * i / dk);
            for (int p = 0; p < max_seq; ++p) {
                c[(size_t)p * h + i] = (float)std::cos((double)p * inv);
                sn[(size_t)p * h + i] = (float)std::sin((double)p * inv);
            }
        }
        if (!(e = alloc_f(&S->rope_t, host.size())))
            e = hipMemcpy(S->rope_t, host.data(), sizeof(float) * host.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(e);
    *out = S;
    return hipSuccess;
}

namespace {

// The new [K | V] of a batched or varlen step into the caches: block (i, b) with i < tab.n_rows[b] copies columns
// d .. 3d - 1 of row tab.row0[b] + i of the step's [Q | K | V] scratch into row tab.pos[b] + i of slab tab.slot[b], as
// float4 where d % 4 == 0 (then every row and third of both buffers is 16-byte aligned), else float by float.  The Q
// third of those cache rows is not written.  The grid's x extent is the largest row count; a batched step has the same
// count for every sequence, so no block of it is idle.
struct ScatterTable {
    int slot[kDecodeMaxBatch], pos[kDecodeMaxBatch], row0[kDecodeMaxBatch], n_rows[kDecodeMaxBatch];
};

__global__ __launch_bounds__(256) void scatter_kv_kernel(const float *__restrict__ qkv, float *__restrict__ cache,
                                                         int64_t slab_rows, int d, ScatterTable tab) {
    const int i = blockIdx.x, b = blockIdx.y;
    if (i >= tab.n_rows[b]) return;
    const float *src = qkv + ((int64_t)tab.row0[b] + i) * 3 * d + d;
    float *dst = cache + ((int64_t)tab.slot[b] * slab_rows + tab.pos[b] + i) * 3 * d + d;
    if ((d & 3) == 0) {
        for (int c = threadIdx.x; c < d / 2; c += blockDim.x)
            reinterpret_cast<float4 *>(dst)[c] = reinterpret_cast<const float4 *>(src)[c];
    } else {
        for (int c = threadIdx.x; c < 2 * d; c += blockDim.x) dst[c] = src[c];
    }
}

// slab_rows: rows of one slab of `cache`, n_slabs of them; scratch_rows: rows of `qkv`.  Every source row is checked
// to lie inside the scratch and every destination row inside its slab
hipError_t launch_scatter_kv(const float *qkv, int64_t scratch_rows, float *cache, int64_t slab_rows, int n_slabs, int d,
                             int n_seqs, const ScatterTable &tab, hipStream_t s) {
    if (!qkv || !cache || d < 1 || n_seqs < 1 || n_seqs > kDecodeMaxBatch) return hipErrorInvalidValue;
    int max_n = 0;
    for (int b = 0; b < n_seqs; ++b) {
        if (tab.slot[b] < 0 || tab.slot[b] >= n_slabs || tab.n_rows[b] < 1 || tab.pos[b] < 0 ||
            tab.pos[b] > slab_rows - tab.n_rows[b] || tab.row0[b] < 0 || tab.row0[b] > scratch_rows - tab.n_rows[b])
            return hipErrorInvalidValue;
        max_n = std::max(max_n, tab.n_rows[b]);
    }
    scatter_kv_kernel<<<dim3((unsigned)max_n, (unsigned)n_seqs), 256, 0, s>>>(qkv, cache, slab_rows, d, tab);
    return hipGetLastError();
}

// ---- one pass over the blocks ----------------------------------------------------------------------------------------
// Which pass this is (the header's "Pass kinds") and the tables that kind reads.  The entry point builds it, after its
// checks, by aggregate initialisation, and the block loop only reads it.  What the entry point does not name is zero,
// and must be: the launchers check whole table entries, and e.g. a cross table's q_pos0 is never set.
//   Forward        the rows are ONE whole sequence; [Q | K | V] and [K2 | V2] live in the stack's scratch
//   Slot           the rows sit at positions pos .. of ONE cache slot
//   Batch          rows_per_seq rows of each of n_seqs slots
//   BatchIndirect  Batch, the self-attention reading through the row table
//   Varlen         n_seqs sequences of their own row counts, packed one after another
enum class PassKind { Forward, Slot, Batch, BatchIndirect, Varlen };

struct Pass {
    PassKind kind;
    int rows;                  // rows of X and Y, all sequences together
    int n_seqs, rows_per_seq;  // (rows_per_seq: 0 in a Varlen pass)
    int enc_seq;               // Forward (decoder), Slot: the cross-attention's keys
    int slot, pos;             // Slot
    // Batch, BatchIndirect -- self: kv_slot = the slot (indirect: its table row), seq_kv = pos + rows_per_seq, q_pos0 =
    // pos; cross: kv_slot = the slot (indirect: cross_slots[b]), seq_kv = that slot's enc_seq, no mask
    DecodeBatchTable self, cross;
    ScatterTable scatter;      // the kinds whose new [K | V] go from the scratch into the slabs: slot, pos, row0, n_rows
    // Varlen: sequence b's rows are row0[b] .. row0[b] + n_rows[b] - 1 of every row buffer (prefix sums).
    // A batched forward: its keys are its own rows of the [Q | K | V] scratch (self_kv_row0 = row0, self_seq_kv =
    // n_rows, self_pos0 = 0).  A step (kv_in_slabs): its keys are rows 0 .. pos + n - 1 of its slot's slab (self_kv_row0
    // = slot * max_seq, self_pos0 = pos), the cross keys the slot's cross slab (cross_kv_row0 = slot * max_enc_seq,
    // cross_seq_kv = its enc_seq)
    bool kv_in_slabs;
    int64_t row0[kVarlenMaxSeqs], self_kv_row0[kVarlenMaxSeqs], cross_kv_row0[kVarlenMaxSeqs];
    int n_rows[kVarlenMaxSeqs], self_seq_kv[kVarlenMaxSeqs], self_pos0[kVarlenMaxSeqs], cross_seq_kv[kVarlenMaxSeqs];
};

// 1 / sqrt(d_k), attention.cuh:64
float attention_scale(const Stack &S) { return (float)(1.0 / std::sqrt((double)(S.d_model / S.n_heads))); }

// Where the QKV GEMM writes the pass's rows: a single-slot step projects straight into cache rows pos .. of the slot's
// slab, every other kind into the [Q | K | V] scratch
float *qkv_rows(const Stack &S, const Block &B, const Pass &p) {
    return p.kind == PassKind::Slot ? B.qkv_cache + ((int64_t)p.slot * S.max_seq + p.pos) * 3 * S.d_model : S.qkv;
}

// sequence b's rows see its slot's cache rows 0 .. pos[b] + n - 1, the last n of them copied here from the scratch
hipError_t scatter_new_kv(Stack &S, const Block &B, const Pass &p, hipStream_t s) {
    return launch_scatter_kv(S.qkv, S.scratch_rows, B.qkv_cache, S.max_seq, S.n_slots, S.d_model, p.n_seqs, p.scatter, s);
}

// RoPE (rope.hip): the Q and K thirds of the pass's new rows, where the QKV GEMM wrote them, rotated in
// place by each row's absolute position -- ONE launch: the thirds are adjacent, so a row is 2 n_heads groups of d_k
// floats at stride 3 d_model; V is not touched.  Row-local and a function of the row's own position alone, so the
// header's argument for the pass kinds carries over.  A forward's sequence starts at position 0, and so does every
// sequence of a batched forward (self_pos0 = 0 there); a step's rows stand at pos ..
hipError_t rotate_qk(Stack &S, const Block &B, const Pass &p, hipStream_t s) {
    const int d = S.d_model, H = S.n_heads, dk = d / H;
    const float *cos_t = S.rope_t, *sin_t = S.rope_t + (size_t)S.max_seq * (dk / 2);
    float *rows = qkv_rows(S, B, p);
    int64_t row0[kDecodeMaxBatch];
    int n_rows[kDecodeMaxBatch];
    switch (p.kind) {
        case PassKind::Forward:
        case PassKind::Slot:
            return launch_rope_rows(rows, 3 * d, p.rows, 2 * H, dk, cos_t, sin_t, S.max_seq,
                                    p.kind == PassKind::Slot ? p.pos : 0, s);
        case PassKind::Batch:
        case PassKind::BatchIndirect:
            for (int b = 0; b < p.n_seqs; ++b) row0[b] = (int64_t)b * p.rows_per_seq, n_rows[b] = p.rows_per_seq;
            return launch_rope_rows_varlen(rows, 3 * d, 2 * H, dk, cos_t, sin_t, S.max_seq, p.n_seqs, row0, n_rows,
                                           p.self.q_pos0, s);
        case PassKind::Varlen:
            return launch_rope_rows_varlen(rows, 3 * d, 2 * H, dk, cos_t, sin_t, S.max_seq, p.n_seqs, p.row0, p.n_rows,
                                           p.self_pos0, s);
    }
    return hipErrorInvalidValue;
}

// S_h = Q_h K_h^T, P_h = softmax(S_h * 1/sqrt(d_k)), heads[:, h*d_v..] = P_h V_h, Q, K and V the thirds of the rows that
// the QKV GEMM wrote (causal: row i sees rows 0 .. i, so row i of the forward depends on rows 0 .. i of X alone)
hipError_t self_attention(Stack &S, const Block &B, const Pass &p, hipStream_t s) {
    const int d = S.d_model, H = S.n_heads, dk = d / H;
    const int64_t slab = (int64_t)S.max_seq * 3 * d;  // floats
    const float scale = attention_scale(S);
    const float *cache = B.qkv_cache;  // [Q | K | V] rows of slab 0 (the step kinds)
    if (S.rope)  // before the scatter: the caches hold rotated K
        if (const hipError_t e = rotate_qk(S, B, p, s)) return e;
    switch (p.kind) {
        case PassKind::Forward:
            return launch_attention(S.qkv, 3 * d, S.qkv + d, 3 * d, S.qkv + 2 * d, 3 * d, S.heads, d, p.rows, p.rows, H, dk,
                                    scale, S.causal ? 0 : kNoMask, S.scores, s);
        case PassKind::Slot:  // the rows at pos .. against the slot's rows 0 .. pos + rows - 1
            cache += p.slot * slab;
            return launch_attention(qkv_rows(S, B, p), 3 * d, cache + d, 3 * d, cache + 2 * d, 3 * d, S.heads, d, p.rows,
                                    p.pos + p.rows, H, dk, scale, p.pos, S.scores, s);
        case PassKind::Batch:
            if (const hipError_t e = scatter_new_kv(S, B, p, s)) return e;
            return launch_attention_decode_batched(S.qkv, 3 * d, cache + d, 3 * d, slab, cache + 2 * d, 3 * d, slab, S.heads,
                                                   d, p.n_seqs, p.rows_per_seq, p.self, /*causal=*/true, H, dk, scale, s);
        case PassKind::BatchIndirect:  // row j of the sequence is row j of slab own[slot][j], the new rows its own slab's
            if (const hipError_t e = scatter_new_kv(S, B, p, s)) return e;
            return launch_attention_decode_indirect(S.qkv, 3 * d, cache + d, 3 * d, slab, cache + 2 * d, 3 * d, slab, S.heads,
                                                    d, p.n_seqs, p.rows_per_seq, S.own, S.max_seq, S.n_slots, p.self,
                                                    /*causal=*/true, H, dk, scale, s);
        case PassKind::Varlen:  // a step's keys are in the slabs, a forward's its own rows of the scratch
            if (!p.kv_in_slabs) cache = S.qkv;
            else if (const hipError_t e = scatter_new_kv(S, B, p, s)) return e;
            return launch_attention_varlen(S.qkv, 3 * d, cache + d, 3 * d, cache + 2 * d, 3 * d, S.heads, d, p.n_seqs, p.row0,
                                           p.n_rows, p.self_kv_row0, p.self_seq_kv,
                                           p.kv_in_slabs || S.causal ? p.self_pos0 : nullptr, H, dk, scale, S.scores, s);
    }
    return hipErrorInvalidValue;
}

// heads2 = attention(Q2, K2, V2), unmasked: the queries in S.q2, [K2 | V2] projected here from the packed enc_out for a
// forward, the slots' cross slabs (filled by begin) for every step
hipError_t cross_attention(Stack &S, const Block &B, const Pass &p, hipStream_t s) {
    const int d = S.d_model, H = S.n_heads, dk = d / H;
    const int64_t slab = (int64_t)S.max_enc_seq * 2 * d;  // floats
    const float scale = attention_scale(S);
    const float *kv2 = B.kv2_cache;  // slab 0 (the step kinds)
    switch (p.kind) {
        case PassKind::Forward:
            if (const hipError_t e = gemm(S, enc_view(S, p.enc_seq), p.enc_seq, d, B.wkv2, 2 * d, S.kv2, B.bkv2, false, s))
                return e;
            return launch_attention(S.q2, d, S.kv2, 2 * d, S.kv2 + d, 2 * d, S.heads2, d, p.rows, p.enc_seq, H, dk, scale,
                                    kNoMask, S.scores, s);
        case PassKind::Slot:
            kv2 += p.slot * slab;
            return launch_attention(S.q2, d, kv2, 2 * d, kv2 + d, 2 * d, S.heads2, d, p.rows, p.enc_seq, H, dk, scale,
                                    kNoMask, S.scores, s);
        case PassKind::Batch:
        case PassKind::BatchIndirect:
            return launch_attention_decode_batched(S.q2, d, kv2, 2 * d, slab, kv2 + d, 2 * d, slab, S.heads2, d, p.n_seqs,
                                                   p.rows_per_seq, p.cross, /*causal=*/false, H, dk, scale, s);
        case PassKind::Varlen:
            return launch_attention_varlen(S.q2, d, kv2, 2 * d, kv2 + d, 2 * d, S.heads2, d, p.n_seqs, p.row0, p.n_rows,
                                           p.cross_kv_row0, p.cross_seq_kv, nullptr, H, dk, scale, S.scores, s);
    }
    return hipErrorInvalidValue;
}

// ---- the sub-layer boundaries: the residual, the LayerNorm and the pack in front of the next linear, ONE launch each,
// per architecture (the header's table).  t = S.t is the sub-layer's output, what W_O, W_O2 or W2 just wrote
enum Boundary { kAfterWo, kAfterWo2, kAfterW2 };

// What the block loop carries: the fp32 rows the next QKV linear reads (a post-LN block's LN1 adds them too), or that
// they are packed in act_view already.  res is the pre-LN boundary's own: the residual stream -- the caller's X, never
// written, until the first boundary stores S.x, then S.x in place
struct Carry { const float *in; bool packed; const float *res; };

// where a reference or post-LN block's last boundary writes, and what that makes of the carry: Y unpacked behind the
// last block, else xa / xb in turn, packed for the next block
float *block_out(Stack &S, int i, float *Y, Carry &c) {
    c.packed = i != S.n_blocks - 1;
    float *out = c.packed ? (i % 2 ? S.xb : S.xa) : Y;
    c.in = out;
    return out;
}

// the reference block: x = LN(t + multiHeadOut), multiHeadOut the last attention's -- heads2 in a decoder, also behind W2
hipError_t boundary_reference(Stack &S, int i, Boundary where, int rows, Carry &c, float *Y, hipStream_t s) {
    const int d = S.d_model;
    const float *mho = where == kAfterWo || !S.cross ? S.heads : S.heads2;
    if (where != kAfterW2) return launch_add_layernorm_rows_pack(S.t, mho, S.x, rows, d, 127.0f, act_view(S, rows, d), s);
    float *out = block_out(S, i, Y, c);
    return c.packed ? launch_add_layernorm_rows_pack(S.t, mho, out, rows, d, 127.0f, act_view(S, rows, d), s)
                    : launch_add_layernorm_rows(S.t, mho, out, rows, d, s);
}

// The stack's norm in its three forms, ONE launch each: the LayerNorm with gamma and beta, or on an RMSNORM stack
//  the RMS norm with gamma alone -- the same kernel's other instantiation, beta never read
hipError_t norm_rows(Stack &S, const float *A, const float *B, const float *g, const float *be, float *Y, int rows,
                     hipStream_t s) {
    return S.rms ? launch_rmsnorm_rows(A, B, g, S.ln_eps, Y, rows, S.d_model, s)
                 : launch_layernorm_rows(A, B, g, be, S.ln_eps, Y, rows, S.d_model, s);
}
hipError_t norm_rows_pack(Stack &S, const float *A, const float *B, const float *g, const float *be, float *Y, int rows,
                          const PackedView &va, hipStream_t s) {
    return S.rms ? launch_rmsnorm_rows_pack(A, B, g, S.ln_eps, Y, rows, S.d_model, 127.0f, va, s)
                 : launch_layernorm_rows_pack(A, B, g, be, S.ln_eps, Y, rows, S.d_model, 127.0f, va, s);
}
hipError_t prenorm_pack(Stack &S, const float *A, const float *B, const float *g, const float *be, float *res, int rows,
                        hipStream_t s) {
    const PackedView va = act_view(S, rows, S.d_model);
    return S.rms ? launch_prenorm_rms_pack(A, B, g, S.ln_eps, res, rows, S.d_model, 127.0f, va, s)
                 : launch_prenorm_pack(A, B, g, be, S.ln_eps, res, rows, S.d_model, 127.0f, va, s);
}

// post-LN: x1 = LN1(in + t), x2 = LN2(x1 + t) in place over x1, y = LN3(x + t) with x the FFN's own input
hipError_t boundary_post_ln(Stack &S, int i, Boundary where, int rows, Carry &c, float *Y, hipStream_t s) {
    const int d = S.d_model;
    const Block &B = S.blocks[i];
    const PackedView va = act_view(S, rows, d);
    if (where == kAfterWo) return norm_rows_pack(S, S.t, c.in, B.g1, B.be1, S.x, rows, va, s);
    if (where == kAfterWo2) return norm_rows_pack(S, S.t, S.x, B.g2, B.be2, S.x, rows, va, s);
    float *out = block_out(S, i, Y, c);
    return c.packed ? norm_rows_pack(S, S.t, S.x, B.g3, B.be3, out, rows, va, s)
                    : norm_rows(S, S.t, S.x, B.g3, B.be3, out, rows, s);
}

// pre-LN: stream += t, the LN in front of the NEXT sub-layer -- LN2, LN3 (after W_O too in an encoder),
// the next block's LN1 -- and its pack.  The normalised rows exist only packed: the QKV, Wq2 and W1 GEMMs read them from
// act_view.  Behind the last block Y = LNf(stream + t), the post-LN kernel as it is, or Y = stream + t
hipError_t boundary_pre_ln(Stack &S, int i, Boundary where, int rows, Carry &c, float *Y, hipStream_t s) {
    const int d = S.d_model;
    const float *res = c.res;
    if (where == kAfterW2 && i == S.n_blocks - 1)
        return S.final_norm ? norm_rows(S, res, S.t, S.fn, S.fn + d, Y, rows, s) : launch_add_rows(res, S.t, Y, rows, d, s);
    const Block &B = S.blocks[where == kAfterW2 ? i + 1 : i];
    const bool ln2 = where == kAfterWo && S.cross;
    const float *g = where == kAfterW2 ? B.g1 : ln2 ? B.g2 : B.g3, *be = where == kAfterW2 ? B.be1 : ln2 ? B.be2 : B.be3;
    c.res = S.x;
    return prenorm_pack(S, res, S.t, g, be, S.x, rows, s);
}

// One pass over the blocks on the p.rows rows of X into Y: the block of the header, once and in order.  The pass kind is
// the attention helpers' and qkv_rows' business, the architecture the boundaries'; every other launch is row-local and
// the same for all of them.  (B.bqkv and every other standard-only pointer is nullptr on a reference stack: the
// reference's GEMM call)
hipError_t run_blocks(Stack *S, const Pass &p, const float *X, float *Y, hipStream_t s) {
    const int d = S->d_model, rows = p.rows;
    const auto boundary = S->norm_first ? boundary_pre_ln : S->standard ? boundary_post_ln : boundary_reference;
    Carry c = {X, false, X};
    hipError_t e;
    if (S->norm_first) {  // LN1 of block 0 on X as it is: no add, nothing to store
        if ((e = prenorm_pack(*S, X, nullptr, S->blocks[0].g1, S->blocks[0].be1, nullptr, rows, s))) return e;
        c.packed = true;
    }
    for (int i = 0; i < S->n_blocks; ++i) {
        const Block &B = S->blocks[i];
        // ---- self-attention on the block input: [Q | K | V] = in @ [Wq | Wk | Wv] over all heads, t = heads @ W_O
        if ((e = linear(*S, c.packed ? nullptr : c.in, rows, d, B.wqkv, 3 * d, qkv_rows(*S, B, p), B.bqkv, false, s)))
            return e;
        if ((e = self_attention(*S, B, p, s))) return e;
        if ((e = linear(*S, S->heads, rows, d, B.wo, d, S->t, B.bo, false, s))) return e;
        if ((e = boundary(*S, i, kAfterWo, rows, c, Y, s))) return e;
        if (S->cross) {
            // ---- cross-attention: queries from the boundary's packed rows, keys and values from enc_out
            if ((e = linear(*S, nullptr, rows, d, B.wq2, d, S->q2, B.bq2, false, s))) return e;
            if ((e = cross_attention(*S, B, p, s))) return e;
            if ((e = linear(*S, S->heads2, rows, d, B.wo2, d, S->t, B.bo2, false, s))) return e;
            if ((e = boundary(*S, i, kAfterWo2, rows, c, Y, s))) return e;
        }
        // ---- FFN: t = act(x W1 + b1) W2 + b2, bias and relu fused into the GEMMs.  GELU: W1 without relu, and the pack
        // in front of W2 applies GELU as it quantizes -- the launch count is the relu path's
        // Gated: ONE GEMM on [W1 | W3] writes gate | up, glu.hip's pack activates the gate, multiplies
        // by up and quantizes -- the same three launches, the product never written
        const int ffw = S->gated ? 2 * S->d_ff : S->d_ff;
        if ((e = linear(*S, nullptr, rows, d, B.w1, ffw, S->ffn, B.b1, !S->gelu && !S->gated, s))) return e;
        if (S->gated || S->gelu) {
            const PackedView va = act_view(*S, rows, S->d_ff);
            if ((e = S->gated ? launch_glu_pack(S->ffn, ffw, rows, S->d_ff, S->activation, 127.0f, va, s)
                              : launch_gelu_pack(S->ffn, S->d_ff, rows, S->d_ff, 127.0f, va, s)))
                return e;
            if ((e = gemm(*S, va, rows, S->d_ff, B.w2, d, S->t, B.b2, false, s))) return e;
        } else if ((e = linear(*S, S->ffn, rows, S->d_ff, B.w2, d, S->t, B.b2, false, s))) {
            return e;
        }
        if ((e = boundary(*S, i, kAfterW2, rows, c, Y, s))) return e;
    }
    return hipSuccess;
}

// Cx and the int8 rows of enc_out, once for every block's [K2 | V2] projection
hipError_t pack_enc(Stack *S, const float *enc_out, int enc_seq, hipStream_t s) {
    return launch_pack_rows(enc_out, S->d_model, 1, enc_seq, S->d_model, 127.0f, enc_view(*S, enc_seq), s);
}

// the encoder output a forward or a begin is given: enc_seq rows with cross-attention, nothing at all without it
bool enc_out_ok(const Stack *S, const float *enc_out, int enc_seq) {
    return S->cross ? enc_out && enc_seq >= 1 && enc_seq <= S->max_enc_seq : !enc_out && enc_seq == 0;
}

// ---- what the step entry points share --------------------------------------------------------------------------------
// May slot sl take n rows at pos in this step?  In range, begun, its slab its own sequence's or (indirect) a beam's as
// the call needs it, not named before in this call (seen, a bit per slot: n_slots <= 64), 0 <= pos <= filled, and room
// for the rows.  Every entry point runs it for all its sequences before its first launch
bool admit(const Stack *S, int sl, bool indirect, uint64_t &seen, int pos, int n) {
    if (sl < 0 || sl >= S->n_slots || !S->begun[sl] || (S->indirect[sl] != 0) != indirect || (seen >> sl & 1) ||
        n < 1 || pos < 0 || pos > S->filled[sl] || n > S->max_seq - pos)
        return false;
    seen |= (uint64_t)1 << sl;
    return true;
}

// sequence b's n new [K | V] rows: from rows row0 .. of the scratch to rows pos .. of slab sl
void scatter_entry(ScatterTable &t, int b, int sl, int pos, int row0, int n) {
    t.slot[b] = sl, t.pos[b] = pos, t.row0[b] = row0, t.n_rows[b] = n;
}

// the filled lengths behind an enqueued step: every sequence's pos + its rows (an earlier pos rewinds)
void set_filled(Stack *S, int n_seqs, const ScatterTable &t) {
    for (int b = 0; b < n_seqs; ++b) S->filled[t.slot[b]] = t.pos[b] + t.n_rows[b];
}

}  // namespace

hipError_t encoder_forward(Stack *S, const float *X, float *Y, int seq, hipStream_t s) {
    if (!S || S->decoder || !X || !Y || seq < 1 || seq > S->max_seq) return hipErrorInvalidValue;
    return run_blocks(S, Pass{PassKind::Forward, seq, 1, seq}, X, Y, s);
}

// X and Y: the sequences' rows packed one after another.  Every row-local step of run_blocks sees one matrix of
// sum seq_lens rows; the self-attention alone knows where a sequence ends
hipError_t encoder_forward_batch(Stack *S, const float *X, float *Y, int n_seqs, const int *seq_lens, hipStream_t s) {
    if (!S || S->decoder || !X || !Y || !seq_lens || n_seqs < 1 || n_seqs > kVarlenMaxSeqs) return hipErrorInvalidValue;
    Pass p = {PassKind::Varlen, 0, n_seqs};  // (kv_in_slabs = false: a sequence's keys are its own rows of the scratch)
    int64_t rows = 0;
    for (int b = 0; b < n_seqs; ++b) {
        if (seq_lens[b] < 1 || seq_lens[b] > S->max_seq) return hipErrorInvalidValue;
        p.row0[b] = p.self_kv_row0[b] = rows;
        p.n_rows[b] = p.self_seq_kv[b] = seq_lens[b];
        rows += seq_lens[b];
    }
    if (rows > S->scratch_rows) return hipErrorInvalidValue;
    p.rows = (int)rows;
    return run_blocks(S, p, X, Y, s);
}

hipError_t decoder_forward(Stack *S, const float *X, const float *enc_out, float *Y, int seq, int enc_seq,
                           hipStream_t s) {
    if (!S || !S->decoder || !X || !Y || seq < 1 || seq > S->max_seq || !enc_out_ok(S, enc_out, enc_seq))
        return hipErrorInvalidValue;
    if (S->cross)
        if (const hipError_t e = pack_enc(S, enc_out, enc_seq, s)) return e;
    return run_blocks(S, Pass{PassKind::Forward, seq, 1, seq, enc_seq}, X, Y, s);
}

// (a decoder-only stack: no launch -- the slot is begun, empty and its own)
hipError_t decoder_begin_slot(Stack *S, int slot, const float *enc_out, int enc_seq, hipStream_t s) {
    if (!S || !S->decoder || !S->kv_cache || slot < 0 || slot >= S->n_slots || !enc_out_ok(S, enc_out, enc_seq))
        return hipErrorInvalidValue;
    const int d = S->d_model;
    hipError_t e = S->cross ? pack_enc(S, enc_out, enc_seq, s) : hipSuccess;
    if (e) return e;
    for (const Block &B : S->blocks)
        if (S->cross && (e = gemm(*S, enc_view(*S, enc_seq), enc_seq, d, B.wkv2, 2 * d,
                                  B.kv2_cache + (int64_t)slot * S->max_enc_seq * 2 * d, B.bkv2, false, s)))
            return e;
    S->begun[slot] = 1;
    S->enc_seq[slot] = enc_seq;
    S->filled[slot] = 0;
    S->indirect[slot] = 0;  // the slab is the slot's own again (rows 0 .. filled - 1: none)
    return hipSuccess;
}

hipError_t decoder_step_slot(Stack *S, int slot, const float *X, float *Y, int pos, int n, hipStream_t s) {
    uint64_t seen = 0;
    if (!S || !S->decoder || !S->kv_cache || !X || !Y || !admit(S, slot, /*indirect=*/false, seen, pos, n))
        return hipErrorInvalidValue;
    const hipError_t e = run_blocks(S, Pass{PassKind::Slot, n, 1, n, S->enc_seq[slot], slot, pos}, X, Y, s);
    if (e) return e;
    S->filled[slot] = pos + n;
    return hipSuccess;
}

hipError_t decoder_step_batch(Stack *S, int n_seqs, const int *slots, const int *pos, int rows_per_seq, const float *X,
                              float *Y, hipStream_t s) {
    if (!S || !S->decoder || !S->kv_cache || !slots || !pos || !X || !Y || n_seqs < 1 || n_seqs > S->n_slots ||
        rows_per_seq < 1 || rows_per_seq > 8)
        return hipErrorInvalidValue;
    const int r = rows_per_seq;
    if (!attention_decode_ok(r, 1, S->d_model / S->n_heads)) return hipErrorInvalidValue;  // d_k > 64: no batched launch
    // (n_seqs * r <= scratch_rows: n_seqs <= n_slots, and r <= max_seq with one slot)
    Pass p = {PassKind::Batch, n_seqs * r, n_seqs, r};
    uint64_t seen = 0;
    for (int b = 0; b < n_seqs; ++b) {
        const int sl = slots[b];
        if (!admit(S, sl, /*indirect=*/false, seen, pos[b], r)) return hipErrorInvalidValue;
        p.self.kv_slot[b] = p.cross.kv_slot[b] = sl;
        p.self.seq_kv[b] = pos[b] + r;
        p.self.q_pos0[b] = pos[b];
        p.cross.seq_kv[b] = S->enc_seq[sl];
        scatter_entry(p.scatter, b, sl, pos[b], b * r, r);
    }
    const hipError_t e = run_blocks(S, p, X, Y, s);
    if (e) return e;
    set_filled(S, n_seqs, p.scatter);
    return hipSuccess;
}

// step_batch without its 8-row, equal-rows limits: sequence b appends n_rows[b] rows (rows sum_{b' < b} n_rows[b'] ..
// of X / Y) at pos[b] of slot slots[b].  Every check comes before the first launch; `filled` is updated at enqueue.
hipError_t decoder_step_varlen(Stack *S, int n_seqs, const int *slots, const int *pos, const int *n_rows, const float *X,
                               float *Y, hipStream_t s) {
    if (!S || !S->decoder || !S->kv_cache || !slots || !pos || !n_rows || !X || !Y || n_seqs < 1 || n_seqs > S->n_slots)
        return hipErrorInvalidValue;
    Pass p = {PassKind::Varlen, 0, n_seqs};
    p.kv_in_slabs = true;
    uint64_t seen = 0;
    int64_t rows = 0;
    for (int b = 0; b < n_seqs; ++b) {
        const int sl = slots[b], n = n_rows[b];
        if (!admit(S, sl, /*indirect=*/false, seen, pos[b], n)) return hipErrorInvalidValue;
        p.row0[b] = rows;
        p.n_rows[b] = n;
        p.self_kv_row0[b] = (int64_t)sl * S->max_seq;
        p.self_seq_kv[b] = pos[b] + n;
        p.self_pos0[b] = pos[b];
        p.cross_kv_row0[b] = (int64_t)sl * S->max_enc_seq;
        p.cross_seq_kv[b] = S->enc_seq[sl];
        scatter_entry(p.scatter, b, sl, pos[b], (int)rows, n);
        rows += n;
        if (rows > S->scratch_rows) return hipErrorInvalidValue;
    }
    p.rows = (int)rows;
    const hipError_t e = run_blocks(S, p, X, Y, s);
    if (e) return e;
    set_filled(S, n_seqs, p.scatter);
    return hipSuccess;
}

// rows 0 .. filled - 1 of every block's self cache and rows 0 .. enc_seq - 1 of its cross cache, device to device in
// stream order: dst then continues src's sequence on its own (beam search)
hipError_t decoder_copy_slot(Stack *S, int dst, int src, hipStream_t s) {
    if (!S || !S->decoder || !S->kv_cache || dst < 0 || dst >= S->n_slots || src < 0 || src >= S->n_slots || dst == src ||
        !S->begun[src] || S->indirect[src])
        return hipErrorInvalidValue;
    const int64_t d = S->d_model, self_slab = S->max_seq * 3 * d, cross_slab = S->max_enc_seq * 2 * d;
    const size_t self_bytes = sizeof(float) * (size_t)S->filled[src] * 3 * d;
    const size_t cross_bytes = sizeof(float) * (size_t)S->enc_seq[src] * 2 * d;
    hipError_t e;
    for (const Block &B : S->blocks) {
        if (self_bytes && (e = hipMemcpyAsync(B.qkv_cache + dst * self_slab, B.qkv_cache + src * self_slab, self_bytes,
                                              hipMemcpyDeviceToDevice, s)))
            return e;
        if (S->cross && (e = hipMemcpyAsync(B.kv2_cache + dst * cross_slab, B.kv2_cache + src * cross_slab, cross_bytes,
                                            hipMemcpyDeviceToDevice, s)))
            return e;
    }
    S->enc_seq[dst] = S->enc_seq[src];
    S->begun[dst] = 1;
    S->filled[dst] = S->filled[src];
    return hipSuccess;
}

// Beam search's reorder: destination dst_slots[g * beams + q] takes the [K | V] of self-cache rows
// 0 .. n_rows[g] - 1 of source src_slots[g * beams + parents[g * beams + q]], parents read on the device by the copy
// kernel (beam.hip), one launch per block.  Every check comes before the first launch; `filled` moves at enqueue.
hipError_t decoder_gather_slots(Stack *S, int n_groups, int beams, const int *dst_slots, const int *src_slots,
                                const int *parents, const int *n_rows, hipStream_t s) {
    if (!S || !S->decoder || !S->kv_cache || !dst_slots || !src_slots || !parents || !n_rows || n_groups < 1 ||
        beams < 1 || beams > 8 || (int64_t)n_groups * beams > kDecodeMaxBatch)
        return hipErrorInvalidValue;
    uint64_t is_dst = 0, is_src = 0;  // n_slots <= 64
    for (int g = 0; g < n_groups; ++g) {
        if (n_rows[g] < 0 || n_rows[g] > S->max_seq) return hipErrorInvalidValue;
        for (int q = 0; q < beams; ++q) {
            const int ds = dst_slots[g * beams + q], ss = src_slots[g * beams + q];
            if (ds < 0 || ds >= S->n_slots || ss < 0 || ss >= S->n_slots || !S->begun[ds] || !S->begun[ss] ||
                S->indirect[ss] || (is_dst >> ds & 1) || n_rows[g] > S->filled[ss] ||
                S->enc_seq[ds] != S->enc_seq[src_slots[g * beams]] || S->enc_seq[ss] != S->enc_seq[src_slots[g * beams]])
                return hipErrorInvalidValue;
            is_dst |= (uint64_t)1 << ds;
            is_src |= (uint64_t)1 << ss;
        }
    }
    if (is_dst & is_src) return hipErrorInvalidValue;
    hipError_t e;
    for (const Block &B : S->blocks)
        if ((e = launch_gather_kv(B.qkv_cache, S->max_seq, S->n_slots, S->d_model, n_groups, beams, dst_slots, src_slots,
                                  n_rows, parents, s)))
            return e;
    for (int g = 0; g < n_groups; ++g)
        for (int q = 0; q < beams; ++q) S->filled[dst_slots[g * beams + q]] = n_rows[g];
    return hipSuccess;
}

// ---- the copy-free beam search: the row table's three operations ----------------------------------
namespace {

bool has_table(const Stack *S) { return S && S->decoder && S->kv_cache && S->own; }

// rows = n_groups * beams places in all, within the table kernels' 64
bool beam_places_ok(int n_groups, int beams) {
    return n_groups >= 1 && beams >= 1 && beams <= 8 && (int64_t)n_groups * beams <= kDecodeMaxBatch;
}

// the leading rows of the slot's own slab that hold a plain sequence: what a prompt may lend
int plain_rows(const Stack *S, int slot) { return S->indirect[slot] ? S->own_rows[slot] : S->filled[slot]; }

}  // namespace

// begin: entries 0 .. pos[g] - 1 of every slot of group g name src_slots[g], the slot that holds the group's prompt; no
// K / V row and no cross cache is copied.  A destination may be its own group's source (place 0 only, and then no
// other group may name that source): any other overlap of the lists would let a search write into a prompt.  Such a
// slot keeps its prompt rows, so the same begin may be enqueued again (a captured search, a second search).
hipError_t decoder_beam_begin(Stack *S, int n_groups, int beams, const int *slots, const int *src_slots, const int *pos,
                              hipStream_t s) {
    if (!has_table(S) || !slots || !src_slots || !pos || !beam_places_ok(n_groups, beams)) return hipErrorInvalidValue;
    const int rows = n_groups * beams;
    int first[kDecodeMaxBatch], count[kDecodeMaxBatch], value[kDecodeMaxBatch];
    uint64_t seen = 0;  // n_slots <= 64
    for (int g = 0; g < n_groups; ++g) {
        const int src = src_slots[g];
        if (src < 0 || src >= S->n_slots || !S->begun[src] || pos[g] < 0 || pos[g] > plain_rows(S, src))
            return hipErrorInvalidValue;
        for (int q = 0; q < beams; ++q) {
            const int i = g * beams + q, sl = slots[i];
            if (sl < 0 || sl >= S->n_slots || (seen >> sl & 1)) return hipErrorInvalidValue;
            seen |= (uint64_t)1 << sl;
            for (int g2 = 0; g2 < n_groups; ++g2)
                if (sl == src_slots[g2] && !(g2 == g && q == 0)) return hipErrorInvalidValue;
            first[i] = 0;
            count[i] = pos[g];
            value[i] = src;
        }
    }
    const hipError_t e = launch_beam_fill(S->own, S->max_seq, S->n_slots, rows, slots, first, count, value, s);
    if (e) return e;
    for (int g = 0; g < n_groups; ++g)
        for (int q = 0; q < beams; ++q) {
            const int sl = slots[g * beams + q];
            S->own_rows[sl] = sl == src_slots[g] ? pos[g] : 0;  // (rows at or past pos: the search's to overwrite)
            S->enc_seq[sl] = S->enc_seq[src_slots[g]];
            S->begun[sl] = 1;
            S->filled[sl] = pos[g];
            S->indirect[sl] = 1;
        }
    return hipSuccess;
}

// step_batch on slots begun by beam_begin, with the append: the new [K | V] into the slot's own slab (the scatter),
// own[slot][pos .. pos + r - 1] = slot (ONE launch per step: the table serves every block), the self-attention through
// the table, the cross-attention on the slab of cross_slots[b] (a group's beams share their prompt's cross cache).
hipError_t decoder_step_batch_indirect(Stack *S, int n_seqs, const int *slots, const int *cross_slots, const int *pos,
                                       int rows_per_seq, const float *X, float *Y, hipStream_t s) {
    if (!has_table(S) || !slots || !cross_slots || !pos || !X || !Y || n_seqs < 1 || n_seqs > S->n_slots ||
        rows_per_seq < 1 || rows_per_seq > 8)
        return hipErrorInvalidValue;
    const int r = rows_per_seq;
    if (!attention_decode_ok(r, 1, S->d_model / S->n_heads)) return hipErrorInvalidValue;
    Pass p = {PassKind::BatchIndirect, n_seqs * r, n_seqs, r};
    uint64_t seen = 0;
    for (int b = 0; b < n_seqs; ++b) {
        const int sl = slots[b], cs = cross_slots[b];
        // (a beam's slot carries its prompt's enc_seq, so "begun" is the cross slot's: begun, and the same enc_seq)
        if (!admit(S, sl, /*indirect=*/true, seen, pos[b], r) || cs < 0 || cs >= S->n_slots || !S->begun[cs] ||
            S->enc_seq[cs] != S->enc_seq[sl])
            return hipErrorInvalidValue;
        p.self.kv_slot[b] = sl;
        p.self.seq_kv[b] = pos[b] + r;
        p.self.q_pos0[b] = pos[b];
        p.cross.kv_slot[b] = cs;
        p.cross.seq_kv[b] = S->enc_seq[cs];
        scatter_entry(p.scatter, b, sl, pos[b], b * r, r);
    }
    hipError_t e = launch_beam_fill(S->own, S->max_seq, S->n_slots, n_seqs, slots, pos, p.scatter.n_rows, slots, s);
    if (e) return e;
    if ((e = run_blocks(S, p, X, Y, s))) return e;
    set_filled(S, n_seqs, p.scatter);
    for (int b = 0; b < n_seqs; ++b)
        S->own_rows[slots[b]] = std::min(S->own_rows[slots[b]], pos[b]);  // a rewind into the prompt overwrites it
    return hipSuccess;
}

// reindex: the table rows of a group's slots reordered in place by the parents on the device (beam.hip)
hipError_t decoder_beam_reindex(Stack *S, int n_groups, int beams, const int *slots, const int *parents,
                                const int *n_rows, hipStream_t s) {
    if (!has_table(S) || !slots || !parents || !n_rows || !beam_places_ok(n_groups, beams)) return hipErrorInvalidValue;
    for (int g = 0; g < n_groups; ++g)
        for (int q = 0; q < beams; ++q) {
            const int sl = slots[g * beams + q];
            // (any slot of the group may be a parent: the columns moved must be filled in all of them)
            if (sl < 0 || sl >= S->n_slots || !S->indirect[sl] || n_rows[g] < 0 || n_rows[g] > S->filled[sl])
                return hipErrorInvalidValue;
        }
    const hipError_t e = launch_beam_reindex(S->own, S->max_seq, S->n_slots, n_groups, beams, slots, parents, n_rows, s);
    if (e) return e;  // (a slot named twice: refused there, before its launch)
    for (int g = 0; g < n_groups; ++g)
        for (int q = 0; q < beams; ++q) S->filled[slots[g * beams + q]] = n_rows[g];
    return hipSuccess;
}

// the table as it is (n_slots x max_seq bytes), device to device in stream order: read_slot's sibling
hipError_t decoder_read_beam_table(const Stack *S, uint8_t *out, hipStream_t s) {
    if (!has_table(S) || !out) return hipErrorInvalidValue;
    return hipMemcpyAsync(out, S->own, (size_t)S->n_slots * S->max_seq, hipMemcpyDeviceToDevice, s);
}

bool decoder_slot_indirect(const Stack *S, int slot) {
    return S && slot >= 0 && slot < S->n_slots && slot < (int)S->indirect.size() && S->indirect[slot];
}

hipError_t decoder_slot_state(const Stack *S, int slot, int *enc_seq, int *filled) {
    if (!S || !S->decoder || !S->kv_cache || slot < 0 || slot >= S->n_slots) return hipErrorInvalidValue;
    if (enc_seq) *enc_seq = S->enc_seq[slot];
    if (filled) *filled = S->filled[slot];
    return hipSuccess;
}

// whether the slot's sequence was begun (with cross-attention: enc_seq >= 1); false out of range
bool decoder_slot_begun(const Stack *S, int slot) {
    return S && S->decoder && S->kv_cache && slot >= 0 && slot < S->n_slots && S->begun[slot];
}

// a slot's slabs as they are, device to device in stream order: block `block`'s self slab (max_seq x 3 d_model) into
// self_rows and its cross slab (max_enc_seq x 2 d_model) into cross_rows, either may be nullptr.  For inspection:
// what a reorder wrote and what it left alone cannot be seen through step's output alone.
hipError_t decoder_read_slot(const Stack *S, int block, int slot, float *self_rows, float *cross_rows, hipStream_t s) {
    if (!S || !S->decoder || !S->kv_cache || block < 0 || block >= S->n_blocks || slot < 0 || slot >= S->n_slots ||
        (cross_rows && !S->cross))
        return hipErrorInvalidValue;
    const int64_t d = S->d_model, self_slab = S->max_seq * 3 * d, cross_slab = S->max_enc_seq * 2 * d;
    const Block &B = S->blocks[block];
    hipError_t e;
    if (self_rows && (e = hipMemcpyAsync(self_rows, B.qkv_cache + slot * self_slab, sizeof(float) * self_slab,
                                         hipMemcpyDeviceToDevice, s)))
        return e;
    if (cross_rows && (e = hipMemcpyAsync(cross_rows, B.kv2_cache + slot * cross_slab, sizeof(float) * cross_slab,
                                          hipMemcpyDeviceToDevice, s)))
        return e;
    return hipSuccess;
}

hipError_t decoder_limits(const Stack *S, int *d_model, int *d_k, int *max_seq, int *n_slots) {
    if (!S || !S->decoder || !S->kv_cache) return hipErrorInvalidValue;
    *d_model = S->d_model;
    *d_k = S->d_model / S->n_heads;
    *max_seq = S->max_seq;
    *n_slots = S->n_slots;
    return hipSuccess;
}

// ---- caller-supplied weights -------------------------------------------------------------------------
namespace {

// Where weight tensor (kind, head) lives: the packed buffer of the block that holds it (k x n_total), its column
// window there, or the bias it is.  false: a kind the stack lacks or a head out of range.
struct WeightPlace {
    void *packed = nullptr;
    float *bias = nullptr;
    int k = 0, n_total = 0, col0 = 0, ncols = 0;
};

bool weight_kind_ok(const Stack *S, int kind) {
    if (kind >= kW3) return S->gated && kind <= kB3;  // the up projection and its bias of a gated stack
    if (S->rms && (kind == kBe1 || kind == kBe2 || kind == kBe3 || kind == kBef)) return false;  // an RMS norm has no beta
    if (kind >= kRopeCos) return S->rope && kind <= kRopeSin;  // the rotary tables of a stack that has them
    if (kind >= kGf) return S->final_norm && kind <= kBef;  // the final norm of a pre-LN stack that has one
    if (kind >= kBq) return S->standard && kind <= (S->cross ? kBe2 : kBe3);  // a reference stack lacks them
    return kind >= kWq && kind <= (S->cross ? kWo2 : kB2);
}
bool weight_per_head(int kind) { return (kind >= kWq && kind <= kWv) || (kind >= kWq2 && kind <= kWv2); }

bool weight_place(const Stack *S, const Block &B, int kind, int head, WeightPlace *p) {
    const int d = S->d_model, dk = d / S->n_heads, ff = S->d_ff, ffw = S->gated ? 2 * ff : ff;
    if (!weight_kind_ok(S, kind) || head < 0 || head >= (weight_per_head(kind) ? S->n_heads : 1)) return false;
    switch (kind) {
        case kWq: case kWk: case kWv: *p = {B.wqkv, nullptr, d, 3 * d, (kind - kWq) * d + head * dk, dk}; break;
        case kWo: *p = {B.wo, nullptr, d, d, 0, d}; break;
        case kW1: *p = {B.w1, nullptr, d, ffw, 0, ff}; break;  // (gated: the gate, the left half of [W1 | W3])
        case kW3: *p = {B.w1, nullptr, d, ffw, ff, ff}; break;
        case kB3: *p = {nullptr, B.b1 + ff, 1, ff, 0, ff}; break;
        case kB1: *p = {nullptr, B.b1, 1, ff, 0, ff}; break;
        case kW2: *p = {B.w2, nullptr, ff, d, 0, d}; break;
        case kB2: *p = {nullptr, B.b2, 1, d, 0, d}; break;
        case kWq2: *p = {B.wq2, nullptr, d, d, head * dk, dk}; break;
        case kWk2: case kWv2: *p = {B.wkv2, nullptr, d, 2 * d, (kind - kWk2) * d + head * dk, dk}; break;
        case kWo2: *p = {B.wo2, nullptr, d, d, 0, d}; break;
        case kGf: case kBef: *p = {nullptr, S->fn + (size_t)(kind - kGf) * d, 1, d, 0, d}; break;  // the stack's own
        case kRopeCos: case kRopeSin:  // max_seq rows of d_k / 2 floats, row after row
            *p = {nullptr, S->rope_t + (size_t)(kind - kRopeCos) * S->max_seq * (dk / 2), S->max_seq, dk / 2, 0, dk / 2};
            break;
        // the standard architecture's vectors, 1 x d_model each: B.sp holds them in the order of their kinds
        default: *p = {nullptr, B.sp + (size_t)(kind - kBq) * d, 1, d, 0, d}; break;
    }
    return true;
}

}  // namespace

// the logical shape of one tensor of `kind` and the heads that have one; no GPU call
hipError_t stack_weight_shape(const Stack *S, int kind, int *rows, int *cols, int *heads) {
    WeightPlace p;
    if (!S || !weight_place(S, S->blocks[0], kind, 0, &p)) return hipErrorInvalidValue;
    if (rows) *rows = p.k;
    if (cols) *cols = p.ncols;
    if (heads) *heads = weight_per_head(kind) ? S->n_heads : 1;
    return hipSuccess;
}

// One tensor of the caller's into the block's packed weight (ONE launch_pack_b_window at its column window) or bias (a
// strided, widening copy), in stream order with the stack's other work; nothing allocated, no synchronization.  The
// result is the packed weight the seeded draw would have made had it drawn these values: the pack is column-local.
// Cached keys and values were projected with the old weights, so on a stack with caches every slot goes back to "not
// begun" when the call is enqueued: a step is refused until the slot's next begin.
hipError_t stack_set_weight(Stack *S, int block, int kind, int head, const void *W, int dtype, int64_t sh, int64_t sw,
                            hipStream_t s) {
    WeightPlace p;
    if (!S || block < 0 || block >= S->n_blocks || !W || (dtype != 0 && dtype != 1) || sh < 0 || sw < 0 ||
        (kind >= kGf && kind <= kRopeSin && block != 0) || !weight_place(S, S->blocks[block], kind, head, &p))
        return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (p.bias) {  // a bias is one row; a rotary table max_seq of them, one copy each
        const int64_t row_bytes = sh * (dtype == 1 ? 2 : 4);
        for (int r = 0; r < p.k && !e; ++r)
            e = launch_copy_row(static_cast<const char *>(W) + r * row_bytes, dtype, sw, p.ncols,
                                p.bias + (size_t)r * p.ncols, s);
    } else {
        e = launch_pack_b_window(W, dtype, sh, sw, p.k, p.n_total, p.col0, p.ncols, 127.0f, p.packed, s);
    }
    if (e) return e;
    if (S->kv_cache) {
        S->enc_seq.assign(S->n_slots, 0);
        S->begun.assign(S->n_slots, 0);
        S->filled.assign(S->n_slots, 0);
        S->indirect.assign(S->n_slots, 0);
        S->own_rows.assign(S->n_slots, 0);
    }
    return hipSuccess;
}

// read-only views for tests and tools: a block's packed weight (n packed rows of k) ...
hipError_t stack_packed_weight(const Stack *S, int block, int which, const void **packed, int *n, int *k) {
    if (!S || block < 0 || block >= S->n_blocks || which < 0 || which > (S->cross ? 6 : 3) || !packed)
        return hipErrorInvalidValue;
    const Block &B = S->blocks[block];
    const int d = S->d_model, ff = S->d_ff, ffw = S->gated ? 2 * ff : ff;  // (gated: which = 2 is [W1 | W3])
    const struct {
        const void *p;
        int n, k;
    } w[7] = {{B.wqkv, 3 * d, d}, {B.wo, d, d}, {B.w1, ffw, d}, {B.w2, d, ff}, {B.wq2, d, d}, {B.wkv2, 2 * d, d}, {B.wo2, d, d}};
    *packed = w[which].p;
    if (n) *n = w[which].n;
    if (k) *k = w[which].k;
    return hipSuccess;
}

// ... and a bias (kind 5 or 7) or a vector of the standard architecture (kinds 12 ..; the final norm's 26, 27 are
// block 0's), n floats on the device
hipError_t stack_bias(const Stack *S, int block, int kind, const float **bias, int *n) {
    WeightPlace p;
    if (!S || block < 0 || block >= S->n_blocks || !bias || (kind >= kGf && kind <= kBef && block != 0) ||
        kind == kRopeCos || kind == kRopeSin ||
        !weight_place(S, S->blocks[block], kind, 0, &p) || !p.bias)
        return hipErrorInvalidValue;
    *bias = p.bias;
    if (n) *n = p.ncols;
    return hipSuccess;
}

// ... and the rotary tables (kinds 28, 29) of a ROPE stack: rows x half floats each, on the device
hipError_t stack_rope_tables(const Stack *S, const float **cos_t, const float **sin_t, int *rows, int *half) {
    if (!S || !S->rope || !cos_t || !sin_t) return hipErrorInvalidValue;
    const int h = S->d_model / S->n_heads / 2;
    *cos_t = S->rope_t;
    *sin_t = S->rope_t + (size_t)S->max_seq * h;
    if (rows) *rows = S->max_seq;
    if (half) *half = h;
    return hipSuccess;
}

hipError_t stack_describe(const Stack *S, StackDesc *out) {
    if (!S || !out) return hipErrorInvalidValue;
    // (QGEMM_DECODER_CAUSAL = 1, QGEMM_DECODER_KV_CACHE = 8, include/qgemm.h)
    *out = StackDesc{S->decoder, S->d_model, S->n_heads, S->d_ff, S->n_blocks, S->max_seq, S->max_enc_seq, S->seed,
                     (S->causal ? 1 : 0) | (S->kv_cache ? 8 : 0), S->n_slots, S->max_rows, S->arch,
                     S->activation, S->ln_eps};
    return hipSuccess;
}

}  // namespace qgemm
