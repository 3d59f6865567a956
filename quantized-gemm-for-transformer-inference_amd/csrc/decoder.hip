// decoder.hip -- the decoder counterpart of the reference's transformer.cu:79-168 with its GEMM call sites on
// the int8 quantized path, built from the encoder's pieces (encoder.hip, DESIGN.md "Decoder"):
//   1. self-attention on the block input            transformer.cu:93-126 -- exactly the encoder's first half:
//      [Q | K | V] = quantized_mm(in, [Wq | Wk | Wv]), heads = attention(Q, K, V),
//      t = quantized_mm(heads, W_O), x1 = LN(t + heads)
//   2. cross-attention                              transformer.cu:128-150:
//      Q2 = quantized_mm(x1, Wq2), [K2 | V2] = quantized_mm(enc_out, [Wk2 | Wv2]),
//      heads2 = attention(Q2, K2, V2) with seq queries and enc_seq keys, t = quantized_mm(heads2, W_O2),
//      x2 = LN(t + heads2)
//   3. FFN                                          transformer.cu:152-167:
//      out = LN(relu(x2 W1 + b1) W2 + b2 + heads2)
// Decisions beyond the encoder's (which carry over: d_ff, weights drawn once and packed, heads written in place):
//   * the reference's attn.forward(output, enc_output, out) (:132) does not match attention.cuh:47's
//     two-argument form: its first argument is read as the source of the queries, its second as the source of
//     the keys and values -- the only reading in which enc_output is used;
//   * W_O is redrawn at :144, so the cross-attention's output projection W_O2 is a tensor of its own;
//   * enc_out is quantized ONCE per forward and its packed form serves every block's [K2 | V2] projection: its
//     per-row absmax scales do not depend on the weight, so this is bit-identical to quantizing it per block.
//
// Incremental decoding (QGEMM_DECODER_KV_CACHE with QGEMM_DECODER_CAUSAL).  Every block owns a
// self-attention cache -- its own [Q | K | V] buffer of max_seq x 3 d_model, so the QKV GEMM of a step writes rows
// pos .. straight into it -- and a cross cache [K2 | V2] of max_enc_seq x 2 d_model.
//   decoder_begin  packs enc_out once, runs every block's [K2 | V2] projection into its cross cache, records enc_seq
//                  and sets the filled length to 0;
//   decoder_step   forward's steps and helpers on the n rows at positions pos .. pos + n - 1: the QKV projection into
//                  cache rows pos .., the masked attention of those n query rows against cache rows 0 .. pos + n - 1
//                  (q_pos0 = pos), W_O, add + layernorm, Wq2, the unmasked attention on the cross cache, W_O2, add +
//                  layernorm, the FFN.  No [K2 | V2] GEMM and no enc_out pack.
// The result is rows pos .. pos + n - 1 of the causal forward on the whole prefix, bit for bit.  The argument: (1)
// every step but the attention is row-local -- the pack's scales are per row, the int8 GEMM accumulates exactly and
// dequantizes per element, add + layernorm works on one row -- so a cache row holds what forward computes for that
// row, whichever call wrote it; (2) the masked attention has the prefix property: row i reads K rows below its limit
// alone, and the V rows past it enter as fmaf(+0, v, acc), which changes nothing WHILE THE CACHED V IS FINITE and no
// P V accumulator is -0 (the conditions of forward(X[:n]) == forward(X)[:n] itself; a step's key
// sequence ends at its own last row, so there is no V row past the last limit at all).  A non-finite V
// row written by an earlier, longer sequence is never read either: rows pos + n .. are outside the call's seq_kv.
// pos is a host argument; the decoder keeps a host-side filled length, updated at enqueue time: 0 <= pos <= filled,
// then filled = pos + n (an earlier pos rewinds: speculative decoding, beam search).  begin and step allocate nothing
// and do not synchronize; they share the decoder's scratch buffers with forward, so a decoder does one thing at a time.
// forward on a cached decoder neither reads nor writes the caches.
#include <cmath>
#include <new>
#include <vector>

#include "qgemm_internal.h"

namespace qgemm {

namespace {

// kinds 0..7 as the encoder's; the cross-attention's tensors follow
enum WeightKind { kWq = 0, kWk = 1, kWv = 2, kWo = 3, kW1 = 4, kB1 = 5, kW2 = 6, kB2 = 7,
                  kWq2 = 8, kWk2 = 9, kWv2 = 10, kWo2 = 11 };

}  // namespace

struct DecoderBlock {
    void *wqkv = nullptr, *wo = nullptr, *wq2 = nullptr, *wkv2 = nullptr, *wo2 = nullptr, *w1 = nullptr, *w2 = nullptr;
    float *b1 = nullptr, *b2 = nullptr;
    float *qkv_cache = nullptr, *kv2_cache = nullptr;  // QGEMM_DECODER_KV_CACHE: max_seq x 3d and max_enc_seq x 2d
};

struct Decoder {
    int d_model = 0, n_heads = 0, d_ff = 0, n_blocks = 0, max_seq = 0, max_enc_seq = 0;
    bool causal = false;  // the self-attention masks keys past the query's own row (QGEMM_DECODER_CAUSAL)
    bool kv_cache = false;  // the blocks own caches for decoder_begin / decoder_step (QGEMM_DECODER_KV_CACHE)
    int enc_seq = 0;        // of the sequence begun (0: no decoder_begin yet)
    int filled = 0;         // cache rows 0 .. filled - 1 hold the sequence so far (host side, at enqueue time)
    std::vector<DecoderBlock> blocks;
    float *qkv = nullptr, *scores = nullptr, *heads = nullptr, *t = nullptr, *ffn = nullptr, *x = nullptr;
    float *q2 = nullptr, *kv2 = nullptr, *heads2 = nullptr, *xa = nullptr, *xb = nullptr;
    char *ws = nullptr;  // [split-K scratch][packed activations][packed enc_out]
    size_t scratch_bytes = 0, act_bytes = 0, ws_bytes = 0;
};

namespace {

hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 16); }

template <typename T>
hipError_t alloc_f(T **p, size_t count) {
    return alloc(reinterpret_cast<void **>(p), count * sizeof(T));
}

// the packed activations of the next linear on the decoder stream (reused in stream order) ...
PackedView act_view(Decoder &D, int seq, int k) { return packed_view(D.ws + D.scratch_bytes, seq, k); }
// ... and the packed encoder output, written once per forward and read by every block
PackedView enc_view(Decoder &D, int enc_seq) {
    return packed_view(D.ws + D.scratch_bytes + D.act_bytes, enc_seq, D.d_model);
}

// y = quantized_mm(packed rows va, packed weight) [+ bias] [relu]
hipError_t gemm(Decoder &D, const PackedView &va, int rows, int k, const void *wpacked, int n, float *y,
                const float *bias, bool relu, hipStream_t s) {
    const float inv_r2 = 1.0f / (127.0f * 127.0f);
    return launch_gemm_dequant(va, packed_view(wpacked, n, k), y, n, 1, rows, n, inv_r2, D.ws, D.scratch_bytes, s, bias,
                               relu, /*tickets_zeroed=*/true);
}

// x == nullptr: the activations are already packed in act_view (by the add+layernorm that made them)
hipError_t linear(Decoder &D, const float *x, int seq, int k, const void *wpacked, int n, float *y, const float *bias,
                  bool relu, hipStream_t s) {
    const PackedView va = act_view(D, seq, k);
    const hipError_t e = x ? launch_pack_rows(x, k, 1, seq, k, 127.0f, va, s) : hipSuccess;
    if (e != hipSuccess) return e;
    return gemm(D, va, seq, k, wpacked, n, y, bias, relu, s);
}

}  // namespace

void decoder_destroy(Decoder *D) {
    if (!D) return;
    for (auto &b : D->blocks)
        for (void *p : {b.wqkv, b.wo, b.wq2, b.wkv2, b.wo2, b.w1, b.w2, (void *)b.b1, (void *)b.b2,
                        (void *)b.qkv_cache, (void *)b.kv2_cache})
            (void)hipFree(p);
    for (void *p : {(void *)D->qkv, (void *)D->scores, (void *)D->heads, (void *)D->t, (void *)D->ffn, (void *)D->x,
                    (void *)D->q2, (void *)D->kv2, (void *)D->heads2, (void *)D->xa, (void *)D->xb, (void *)D->ws})
        (void)hipFree(p);
    delete D;
}

hipError_t decoder_create(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq, uint64_t seed,
                          bool causal, bool kv_cache, Decoder **out) {
    *out = nullptr;
    if (kv_cache && !causal) return hipErrorInvalidValue;
    if (d_model < 2 || n_heads < 1 || d_model % n_heads || d_ff < 2 || n_blocks < 1 || max_seq < 1 || max_seq > 4096 ||
        max_enc_seq < 1 || max_enc_seq > 4096 || d_model > 4096)
        return hipErrorInvalidValue;
    Decoder *D = new (std::nothrow) Decoder;
    if (!D) return hipErrorOutOfMemory;
    D->d_model = d_model;
    D->n_heads = n_heads;
    D->d_ff = d_ff;
    D->n_blocks = n_blocks;
    D->max_seq = max_seq;
    D->max_enc_seq = max_enc_seq;
    D->causal = causal;
    D->kv_cache = kv_cache;
    D->blocks.resize(n_blocks);
    const int d = d_model, dk = d_model / n_heads;
    const size_t S = (size_t)max_seq, Se = (size_t)max_enc_seq;
    hipError_t e = hipSuccess;
    auto fail = [&](hipError_t err) {
        decoder_destroy(D);
        return err;
    };
    // scores only where some forward or step can reach the three launches (both attentions share them): never inside
    // the fused envelope, and never with at most kAttnDecodeMaxQ query rows (a step of n <= 8 needs none either way)
    const int max_kv = std::max(max_seq, max_enc_seq);
    const bool no_scores = attention_fused_ok(max_kv, dk) || attention_decode_ok(max_seq, max_kv, dk);
    const size_t nscores = no_scores ? 0 : (size_t)n_heads * S * (size_t)max_kv;
    if ((e = alloc_f(&D->qkv, S * 3 * d)) || (e = alloc_f(&D->scores, nscores)) || (e = alloc_f(&D->heads, S * d)) ||
        (e = alloc_f(&D->t, S * d)) || (e = alloc_f(&D->ffn, S * d_ff)) || (e = alloc_f(&D->x, S * d)) ||
        (e = alloc_f(&D->q2, S * d)) || (e = alloc_f(&D->kv2, Se * 2 * d)) || (e = alloc_f(&D->heads2, S * d)) ||
        (e = alloc_f(&D->xa, S * d)) || (e = alloc_f(&D->xb, S * d)))
        return fail(e);
    // workspace: split-K scratch for the largest of the linear shapes + the two packed activations
    const int shapes[5][3] = {{max_seq, 3 * d, d}, {max_seq, d, d}, {max_enc_seq, 2 * d, d}, {max_seq, d_ff, d},
                              {max_seq, d, d_ff}};  // (m, n, k)
    size_t scratch = 0;
    for (auto &sh : shapes) scratch = std::max(scratch, gemm_scratch_bytes(sh[0], sh[1], sh[2]));
    const size_t act = std::max(packed_bytes(max_seq, d), packed_bytes(max_seq, d_ff));
    D->scratch_bytes = (scratch + 255) & ~(size_t)255;
    D->act_bytes = (act + 255) & ~(size_t)255;
    D->ws_bytes = D->scratch_bytes + D->act_bytes + packed_bytes(max_enc_seq, d);
    if ((e = alloc(reinterpret_cast<void **>(&D->ws), D->ws_bytes))) return fail(e);
    if ((e = hipMemset(D->ws, 0, D->scratch_bytes))) return fail(e);  // split-K tickets start at zero

    // weights, drawn once with the reference's init bounds (attention.cuh:37-41, linear.cuh:34-39,
    // transformer.cu:120, :144) and packed
    const size_t maxk = std::max(d, d_ff), maxn = std::max(3 * d, d_ff);
    float *tmp = nullptr;
    if ((e = alloc_f(&tmp, maxk * maxn + maxk * maxn))) return fail(e);
    hipStream_t s = nullptr;
    for (int i = 0; i < n_blocks && e == hipSuccess; ++i) {
        DecoderBlock &B = D->blocks[i];
        auto head_seeds = [&](int first, int last) {
            std::vector<uint64_t> v;
            for (int kind = first; kind <= last; ++kind)
                for (int h = 0; h < n_heads; ++h) v.push_back(encoder_weight_seed(seed, i, kind, h));
            return v;
        };
        const float bk = encoder_init_bound(dk), bd = encoder_init_bound(d), bf = encoder_init_bound(d_ff);
        if ((e = encoder_make_packed(d, 3 * d, head_seeds(kWq, kWv), dk, bk, &B.wqkv, tmp, s))) break;
        if ((e = encoder_make_packed(d, d, {encoder_weight_seed(seed, i, kWo, 0)}, d, 1.0f, &B.wo, tmp, s))) break;
        if ((e = encoder_make_packed(d, d, head_seeds(kWq2, kWq2), dk, bk, &B.wq2, tmp, s))) break;
        if ((e = encoder_make_packed(d, 2 * d, head_seeds(kWk2, kWv2), dk, bk, &B.wkv2, tmp, s))) break;
        if ((e = encoder_make_packed(d, d, {encoder_weight_seed(seed, i, kWo2, 0)}, d, 1.0f, &B.wo2, tmp, s))) break;
        if ((e = encoder_make_packed(d, d_ff, {encoder_weight_seed(seed, i, kW1, 0)}, d_ff, bd, &B.w1, tmp, s))) break;
        if ((e = encoder_make_packed(d_ff, d, {encoder_weight_seed(seed, i, kW2, 0)}, d, bf, &B.w2, tmp, s))) break;
        if ((e = alloc_f(&B.b1, d_ff)) || (e = alloc_f(&B.b2, d))) break;
        if (kv_cache && ((e = alloc_f(&B.qkv_cache, S * 3 * d)) || (e = alloc_f(&B.kv2_cache, Se * 2 * d)))) break;
        if ((e = launch_fill_uniform(B.b1, d_ff, encoder_weight_seed(seed, i, kB1, 0), -bd, bd, s))) break;
        if ((e = launch_fill_uniform(B.b2, d, encoder_weight_seed(seed, i, kB2, 0), -bf, bf, s))) break;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(e);
    *out = D;
    return hipSuccess;
}

namespace {

// One pass over the blocks on `rows` rows of the decoder stream, for forward (cached = false: the rows are the whole
// sequence, [Q | K | V] and [K2 | V2] live in the decoder's scratch buffers, [K2 | V2] is projected here from the
// packed enc_out) and for a step (cached = true: the rows sit at positions pos .., [Q | K | V] rows pos .. are written
// into the block's cache and attend to cache rows 0 .. pos + rows - 1, [K2 | V2] is the block's cross cache).
hipError_t run_blocks(Decoder *D, const float *X, float *Y, int rows, int enc_seq, bool cached, int pos, hipStream_t s) {
    const int d = D->d_model, H = D->n_heads, dk = d / H;
    const int seq = rows;
    const float scale = (float)(1.0 / std::sqrt((double)dk));  // attention.cuh:64
    const float *in = X;
    bool in_packed = false;  // the previous block's last add+layernorm packed its output already
    hipError_t e;
    const PackedView venc = enc_view(*D, enc_seq);
    for (int i = 0; i < D->n_blocks; ++i) {
        const DecoderBlock &B = D->blocks[i];
        const bool last = i == D->n_blocks - 1;
        float *out = last ? Y : (i % 2 ? D->xb : D->xa);
        // ---- self-attention on the block input (transformer.cu:93-126): the encoder's first half
        float *qkv = cached ? B.qkv_cache : D->qkv;           // row 0 of [Q | K | V]
        float *qrows = qkv + (size_t)(cached ? pos : 0) * 3 * d;  // the rows this call projects
        if ((e = linear(*D, in_packed ? nullptr : in, seq, d, B.wqkv, 3 * d, qrows, nullptr, false, s))) return e;
        // (causal: row i sees rows 0 .. i, so row i of the forward depends on rows 0 .. i of X alone)
        if ((e = launch_attention(qrows, 3 * d, qkv + d, 3 * d, qkv + 2 * d, 3 * d, D->heads, d, seq,
                                  cached ? pos + seq : seq, H, dk, scale, cached ? pos : (D->causal ? 0 : kNoMask),
                                  D->scores, s)))
            return e;
        if ((e = linear(*D, D->heads, seq, d, B.wo, d, D->t, nullptr, false, s))) return e;
        // x1 = LN(t + heads), packed by the same launch for the query projection
        if ((e = launch_add_layernorm_rows_pack(D->t, D->heads, D->x, seq, d, 127.0f, act_view(*D, seq, d), s)))
            return e;
        // ---- cross-attention (transformer.cu:128-150): queries from x1, keys and values from enc_out
        if ((e = linear(*D, nullptr, seq, d, B.wq2, d, D->q2, nullptr, false, s))) return e;
        float *kv2 = cached ? B.kv2_cache : D->kv2;
        if (!cached && (e = gemm(*D, venc, enc_seq, d, B.wkv2, 2 * d, kv2, nullptr, false, s))) return e;
        if ((e = launch_attention(D->q2, d, kv2, 2 * d, kv2 + d, 2 * d, D->heads2, d, seq, enc_seq, H, dk, scale,
                                  kNoMask, D->scores, s)))
            return e;
        if ((e = linear(*D, D->heads2, seq, d, B.wo2, d, D->t, nullptr, false, s))) return e;
        // x2 = LN(t + heads2), packed for the FFN's first linear
        if ((e = launch_add_layernorm_rows_pack(D->t, D->heads2, D->x, seq, d, 127.0f, act_view(*D, seq, d), s)))
            return e;
        // ---- FFN: relu(x2 W1 + b1) W2 + b2; LN(ffn + the cross-attention's multiHeadOut)  (transformer.cu:152-167)
        if ((e = linear(*D, nullptr, seq, d, B.w1, D->d_ff, D->ffn, B.b1, true, s))) return e;
        if ((e = linear(*D, D->ffn, seq, D->d_ff, B.w2, d, D->t, B.b2, false, s))) return e;
        e = last ? launch_add_layernorm_rows(D->t, D->heads2, out, seq, d, s)
                 : launch_add_layernorm_rows_pack(D->t, D->heads2, out, seq, d, 127.0f, act_view(*D, seq, d), s);
        if (e) return e;
        in = out;
        in_packed = !last;
    }
    return hipSuccess;
}

}  // namespace

hipError_t decoder_forward(Decoder *D, const float *X, const float *enc_out, float *Y, int seq, int enc_seq,
                           hipStream_t s) {
    if (!D || !X || !enc_out || !Y || seq < 1 || seq > D->max_seq || enc_seq < 1 || enc_seq > D->max_enc_seq)
        return hipErrorInvalidValue;
    // Cx and the int8 rows of enc_out, once for every block's [K2 | V2] projection
    const hipError_t e = launch_pack_rows(enc_out, D->d_model, 1, enc_seq, D->d_model, 127.0f, enc_view(*D, enc_seq), s);
    if (e) return e;
    return run_blocks(D, X, Y, seq, enc_seq, /*cached=*/false, 0, s);
}

hipError_t decoder_begin(Decoder *D, const float *enc_out, int enc_seq, hipStream_t s) {
    if (!D || !D->kv_cache || !enc_out || enc_seq < 1 || enc_seq > D->max_enc_seq) return hipErrorInvalidValue;
    const int d = D->d_model;
    const PackedView venc = enc_view(*D, enc_seq);
    hipError_t e = launch_pack_rows(enc_out, d, 1, enc_seq, d, 127.0f, venc, s);
    if (e) return e;
    for (const DecoderBlock &B : D->blocks)
        if ((e = gemm(*D, venc, enc_seq, d, B.wkv2, 2 * d, B.kv2_cache, nullptr, false, s))) return e;
    D->enc_seq = enc_seq;
    D->filled = 0;
    return hipSuccess;
}

hipError_t decoder_step(Decoder *D, const float *X, float *Y, int pos, int n, hipStream_t s) {
    if (!D || !D->kv_cache || D->enc_seq < 1 || !X || !Y || n < 1 || pos < 0 || pos > D->filled ||
        n > D->max_seq - pos)
        return hipErrorInvalidValue;
    const hipError_t e = run_blocks(D, X, Y, n, D->enc_seq, /*cached=*/true, pos, s);
    if (e) return e;
    D->filled = pos + n;
    return hipSuccess;
}

}  // namespace qgemm
