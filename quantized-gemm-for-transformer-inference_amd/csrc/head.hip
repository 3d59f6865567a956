// head.hip -- the output end of the model: row-wise argmax over fp32 rows of any width, the token
// embedding gather, the vocabulary head object (logits = qgemm_linear, next token = argmax of the logits) and the
// greedy generation loop over a slotted decoder, enqueued in one call with the tokens staying on the device -- and the
// sampled counterparts of the last two (s21): the token chosen by launch_sample_rows (sample.hip) in argmax's place --
// and beam search (s22): the head's beam step (logits, then launch_beam_step, beam.hip) and the loop that alternates
// two sets of cache slots, the caches reordered by decoder_gather_slots (transformer.hip) after every step.
//
// The reference stops before this point (transformer.cu ends at "TODO:: MLP & op_softmax"); its op_argmax
// (op_reduction.cuh:41-54, 174-182: MaxAccumFunc over the columns of a row) fixes the selection's semantics:
//   best = 0; for i = 1 .. w-1: if (S[i] > S[best]) best = i;
// so the lowest index among equal maxima wins (+0 == -0), a NaN at i >= 1 never wins, and a NaN at column 0 is never
// beaten.  argmax_rows_kernel reproduces that chain with a parallel reduction of (value, index) pairs:
//   * a thread visits its elements in ascending index order from (-inf, INT_MAX) with the chain's own strict ">", so it
//     keeps the lowest index of its maximum and skips every NaN (x > best is false for a NaN x);
//   * two candidates combine by value, then by lower index (better()).  Over NaN-free candidates with distinct indices
//     that is the maximum of a total order, so lanes, waves and workgroups may combine in any grouping;
//   * column 0 is read again at the end: a NaN there wins outright, otherwise the reduction's winner replaces index 0
//     only where its value is strictly greater -- which also covers rows of -inf and NaN alone, whose candidates never
//     left (-inf, INT_MAX).
// val is the winner's own bits: they travel with the index through every combine.
// Everything here is a C-ABI entry point's body: argument checks first, then launches only -- no allocation, no
// synchronization, nothing copied to the device (positions travel in kernel arguments), so each can be captured.
#include <algorithm>
#include <climits>
#include <new>

#include "../../include/qgemm.h"
#include "qgemm_internal.h"

namespace qgemm {

namespace {

// ---- row-wise argmax ------------------------------------------------------------------------------------------
constexpr int kArgmaxThreads = 256;
constexpr int kArgmaxMaxW = 1 << 24;
// The split rule (argmax_plan): with fewer than kArgmaxManyRows rows, a row is cut into parts of at least
// kArgmaxMinChunk floats (16 KiB: four 16-byte loads per thread) until about kArgmaxTargetGroups workgroups -- two per
// CU of the MI355X -- are in flight, at most kArgmaxMaxParts (one wave combines a row's partials).
constexpr int kArgmaxManyRows = 256;
constexpr int kArgmaxMinChunk = 4096;
constexpr int kArgmaxTargetGroups = 512;
constexpr int kArgmaxMaxParts = 64;

struct Cand {
    float v;
    int i;
};

// the winner of two NaN-free candidates: the greater value, the lower index among equal values (+0 == -0)
__device__ __forceinline__ Cand better(Cand a, Cand b) {
    const bool take_b = (b.v > a.v) || (b.v == a.v && b.i < a.i);
    return take_b ? b : a;
}

__device__ __forceinline__ void visit(float x, int i, Cand &c) {
    if (x > c.v) {  // the chain's strict ">" (MaxAccumFunc): ascending i keeps the lowest index, a NaN never enters
        c.v = x;
        c.i = i;
    }
}

__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Cand o;
        o.v = __shfl_xor(c.v, off, 64);
        o.i = __shfl_xor(c.i, off, 64);
        c = better(c, o);
    }
    return c;
}

// the chain's end: column 0 against the winner of the whole row
__device__ __forceinline__ void argmax_finish(float s0, Cand c, int *idx, float *val, int64_t row) {
    const bool moved = !(s0 != s0) && c.v > s0;  // a NaN at column 0 is never beaten
    idx[row] = moved ? c.i : 0;
    if (val) val[row] = moved ? c.v : s0;
}

// One workgroup per (row, part): columns [part * chunk, min(w, (part + 1) * chunk)) of row blockIdx.x / parts.
// 16-byte loads between a scalar head (up to the first 16-byte aligned element) and a scalar tail; nothing outside
// the row's w floats is read.  parts == 1 writes idx / val, otherwise the workgroup's candidate goes to `partial`.
__global__ __launch_bounds__(kArgmaxThreads) void argmax_rows_kernel(const float *__restrict__ S, int64_t stride, int w,
                                                                     int chunk, int parts, int *__restrict__ idx,
                                                                     float *__restrict__ val,
                                                                     Cand *__restrict__ partial) {
    __shared__ Cand wave_c[kArgmaxThreads / 64];
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / parts;
    const int part = blockIdx.x % parts;
    const int c0 = part * chunk, c1 = min(w, c0 + chunk), n = c1 - c0;
    const float *p = S + row * stride;
    Cand c = {-INFINITY, INT_MAX};
    const int head = min(n, (int)((4 - ((reinterpret_cast<uintptr_t>(p + c0) >> 2) & 3)) & 3));
    const int nvec = (n - head) >> 2;
    const int v0 = c0 + head, t0 = v0 + 4 * nvec;
    if (t < head) visit(p[c0 + t], c0 + t, c);
    const float4 *pv = reinterpret_cast<const float4 *>(p + v0);
#pragma unroll 4
    for (int v = t; v < nvec; v += kArgmaxThreads) {
        const float4 q = pv[v];
        const int i = v0 + 4 * v;
        visit(q.x, i, c);
        visit(q.y, i + 1, c);
        visit(q.z, i + 2, c);
        visit(q.w, i + 3, c);
    }
    if (t < c1 - t0) visit(p[t0 + t], t0 + t, c);
    c = wave_best(c);
    if ((t & 63) == 0) wave_c[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int j = 1; j < kArgmaxThreads / 64; ++j) c = better(c, wave_c[j]);
        if (parts == 1)
            argmax_finish(p[0], c, idx, val, row);
        else
            partial[blockIdx.x] = c;
    }
}

// one wave per row: the row's parts (<= 64) combined, then the chain's end
__global__ __launch_bounds__(64) void argmax_combine_kernel(const float *__restrict__ S, int64_t stride, int parts,
                                                            const Cand *__restrict__ partial, int *__restrict__ idx,
                                                            float *__restrict__ val) {
    const int64_t row = blockIdx.x;
    const int t = threadIdx.x;
    Cand c = {-INFINITY, INT_MAX};
    if (t < parts) c = partial[row * parts + t];
    c = wave_best(c);
    if (t == 0) argmax_finish(S[row * stride], c, idx, val, row);
}

// the plan from rows and w alone: parts per row and the columns of a part, chunk = ceil(w / parts) rounded up to a
// multiple of 4 (parts * chunk >= w and every part holds at least one column)
bool argmax_plan(int64_t rows, int w, int *parts, int *chunk) {
    if (rows < 0 || w < 1 || w > kArgmaxMaxW) return false;
    int p = 1;
    if (rows > 0 && rows < kArgmaxManyRows) {
        const int by_width = w / kArgmaxMinChunk;  // every part at least kArgmaxMinChunk columns
        const int by_rows = (int)((kArgmaxTargetGroups + rows - 1) / rows);
        p = std::max(1, std::min(std::min(by_width, by_rows), kArgmaxMaxParts));
    }
    for (;;) {  // until chunk = round_up(ceil(w / parts), 4) leaves no part empty: parts only ever shrinks
        const int ch = (int)round_up((w + p - 1) / p, 4), q = (w + ch - 1) / ch;
        *chunk = ch;
        *parts = q;
        if (q == p) return true;
        p = q;
    }
}

size_t argmax_ws_bytes(int64_t rows, int w) {
    int parts, chunk;
    if (!argmax_plan(rows, w, &parts, &chunk) || parts == 1) return 0;
    return sizeof(Cand) * (size_t)rows * parts;
}

hipError_t launch_argmax_rows(const float *S, int64_t stride, int64_t rows, int w, int *idx, float *val, void *ws,
                              size_t ws_bytes, hipStream_t s) {
    int parts, chunk;
    if (!S || !idx || !argmax_plan(rows, w, &parts, &chunk) || stride < w) return hipErrorInvalidValue;
    if (rows * parts > INT_MAX) return hipErrorInvalidValue;
    if (parts > 1 && (!ws || ws_bytes < sizeof(Cand) * (size_t)rows * parts)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    Cand *partial = static_cast<Cand *>(ws);
    argmax_rows_kernel<<<(unsigned)(rows * parts), kArgmaxThreads, 0, s>>>(S, stride, w, chunk, parts, idx, val,
                                                                           partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || parts == 1) return e;
    argmax_combine_kernel<<<(unsigned)rows, 64, 0, s>>>(S, stride, parts, partial, idx, val);
    return hipGetLastError();
}

// ---- token embedding ------------------------------------------------------------------------------------------
constexpr int kEmbedMaxSeqs = 64;
constexpr int kEmbedThreads = 128;
constexpr uint32_t kQuietNaN = 0x7fc00000u;  // the row of a token outside [0, vocab)

// the first position of every sequence: a kernel argument passed by value (256 bytes), filled on the host at enqueue
struct EmbedPos {
    int pos[kEmbedMaxSeqs];
};

// One workgroup per output row: Y[r] = E[tokens[r]] (+ P[pos[r / rows_per_seq] + r % rows_per_seq], one fp32 add).
// V = float4 where every base and stride allows 16-byte accesses, else float.
template <typename V>
__global__ __launch_bounds__(kEmbedThreads) void embed_rows_kernel(const float *__restrict__ E, int64_t es, int vocab,
                                                                   int d, const int *__restrict__ tokens,
                                                                   const float *__restrict__ P, int64_t ps,
                                                                   EmbedPos tab, int rows_per_seq,
                                                                   float *__restrict__ Y, int64_t ys) {
    constexpr int kPer = sizeof(V) / sizeof(float);
    const int row = blockIdx.x;
    const int tok = tokens[row];
    V *y = reinterpret_cast<V *>(Y + row * ys);
    const int nv = d / kPer;
    if (tok < 0 || tok >= vocab) {  // nothing of E is read
        const float q = __uint_as_float(kQuietNaN);
        for (int c = threadIdx.x; c < nv; c += kEmbedThreads) {
            if constexpr (kPer == 4)
                y[c] = make_float4(q, q, q, q);
            else
                y[c] = q;
        }
        return;
    }
    const V *e = reinterpret_cast<const V *>(E + (int64_t)tok * es);
    if (!P) {
        for (int c = threadIdx.x; c < nv; c += kEmbedThreads) y[c] = e[c];
        return;
    }
    const V *p = reinterpret_cast<const V *>(P + (int64_t)(tab.pos[row / rows_per_seq] + row % rows_per_seq) * ps);
    for (int c = threadIdx.x; c < nv; c += kEmbedThreads) {
        const V a = e[c], b = p[c];
        if constexpr (kPer == 4)
            y[c] = make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
        else
            y[c] = __fadd_rn(a, b);
    }
}

bool al16(const void *p, int64_t stride) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && stride % 4 == 0; }

// pos: n_seqs host ints, read only with a P (then checked against max_pos)
hipError_t launch_embed_rows(const float *E, int64_t es, int vocab, int d, const int *tokens, const float *P, int64_t ps,
                             int max_pos, const int *pos, int n_seqs, int rows_per_seq, float *Y, int64_t ys,
                             hipStream_t s) {
    if (!E || !tokens || !Y || vocab < 1 || d < 1 || es < d || ys < d || n_seqs < 0 || n_seqs > kEmbedMaxSeqs ||
        rows_per_seq < 1 || (int64_t)n_seqs * rows_per_seq > INT_MAX)
        return hipErrorInvalidValue;
    EmbedPos tab = {};
    if (P) {
        if (!pos || ps < d || max_pos < 1) return hipErrorInvalidValue;
        for (int b = 0; b < n_seqs; ++b) {
            if (pos[b] < 0 || pos[b] > max_pos - rows_per_seq) return hipErrorInvalidValue;
            tab.pos[b] = pos[b];
        }
    }
    if (n_seqs == 0) return hipSuccess;
    const unsigned rows = (unsigned)(n_seqs * rows_per_seq);
    if (d % 4 == 0 && al16(E, es) && al16(Y, ys) && (!P || al16(P, ps)))
        embed_rows_kernel<float4><<<rows, kEmbedThreads, 0, s>>>(E, es, vocab, d, tokens, P, ps, tab, rows_per_seq, Y,
                                                                 ys);
    else
        embed_rows_kernel<float><<<rows, kEmbedThreads, 0, s>>>(E, es, vocab, d, tokens, P, ps, tab, rows_per_seq, Y,
                                                                ys);
    return hipGetLastError();
}

// ---- the head object ------------------------------------------------------------------------------------------
// Borrowed: the packed weight, the bias and the tables.  Owned: the logits, two blocks of max_rows x d_model rows
// (generate's input and hidden rows) and the workspaces of qgemm_linear, the argmax, the sampling (top_k = 1024) and
// the beam step (every beams <= 8), sized at creation for every row count up to max_rows.
struct Head {
    int d_model = 0, vocab = 0, max_pos = 0, max_rows = 0;
    const void *pw = nullptr;
    const float *bias = nullptr, *E = nullptr, *P = nullptr;
    int64_t es = 0, ps = 0;
    float *logits = nullptr, *rows = nullptr;
    void *lin_ws = nullptr, *arg_ws = nullptr, *smp_ws = nullptr, *beam_ws = nullptr;
    size_t lin_bytes = 0, arg_bytes = 0, smp_bytes = 0, beam_bytes = 0;
};

void head_free(Head *h) {
    if (!h) return;
    (void)hipFree(h->logits);
    (void)hipFree(h->rows);
    (void)hipFree(h->lin_ws);
    (void)hipFree(h->arg_ws);
    (void)hipFree(h->smp_ws);
    (void)hipFree(h->beam_ws);
    delete h;
}

hipError_t head_logits(Head *h, const float *H, int64_t hs, int rows, float *out, int64_t os, hipStream_t s) {
    if (!h || !H || !out || rows < 0 || rows > h->max_rows || hs < h->d_model || os < h->vocab)
        return hipErrorInvalidValue;
    return (hipError_t)qgemm_linear(H, hs, rows, h->d_model, h->pw, h->vocab, h->bias, 0, out, os, h->lin_ws,
                                    h->lin_bytes, s);
}

hipError_t head_next_tokens(Head *h, const float *H, int64_t hs, int rows, int *tokens, hipStream_t s) {
    if (!tokens) return hipErrorInvalidValue;
    const hipError_t e = head_logits(h, H, hs, rows, h ? h->logits : nullptr, h ? h->vocab : 0, s);
    if (e != hipSuccess) return e;
    return launch_argmax_rows(h->logits, h->vocab, rows, h->vocab, tokens, nullptr, h->arg_ws, h->arg_bytes, s);
}

// the sampling arguments of qgemm_sample_rows, checked before the logits are launched
struct SampleArgs {
    int top_k;
    float top_p, temperature;
    uint64_t seed, counter0;
    const uint64_t *counters;
    const int *prev;
    int eos;
};

hipError_t head_sample_check(const Head *h, int rows, const SampleArgs &a) {
    if (!h || rows < 0 || rows > h->max_rows) return hipErrorInvalidValue;
    return sample_check(rows, h->vocab, a.top_k, a.top_p, a.temperature, a.counters != nullptr);
}

hipError_t head_sample_tokens(Head *h, const float *H, int64_t hs, int rows, const SampleArgs &a, int *tokens,
                              hipStream_t s) {
    if (!tokens || head_sample_check(h, rows, a) != hipSuccess) return hipErrorInvalidValue;
    const hipError_t e = head_logits(h, H, hs, rows, h->logits, h->vocab, s);
    if (e != hipSuccess) return e;
    return launch_sample_rows(h->logits, h->vocab, rows, h->vocab, a.top_k, a.top_p, a.temperature, a.seed, a.counter0,
                              a.counters, a.prev, a.eos, tokens, nullptr, nullptr, nullptr, h->smp_ws, h->smp_bytes, s);
}

// what qgemm_beam_step refuses without looking at a pointer, and the head's row limit
hipError_t head_beam_check(const Head *h, int n_groups, int beams) {
    int sp, lp;
    if (!h || !beam_step_plan(n_groups, beams, h->vocab, &sp, &lp) || n_groups * beams > h->max_rows)
        return hipErrorInvalidValue;
    return hipSuccess;
}

// logits into the owned buffer, then the beam step on them
hipError_t head_beam_step(Head *h, const float *H, int64_t hs, int n_groups, int beams, const float *scores_in,
                          const int *prev, int eos, int *parents, int *tokens, float *scores_out, hipStream_t s) {
    if (!parents || !tokens || !scores_out || head_beam_check(h, n_groups, beams) != hipSuccess)
        return hipErrorInvalidValue;
    const hipError_t e = head_logits(h, H, hs, n_groups * beams, h->logits, h->vocab, s);
    if (e != hipSuccess) return e;
    return launch_beam_step(h->logits, h->vocab, n_groups, beams, h->vocab, scores_in, prev, eos, parents, tokens,
                            scores_out, h->beam_ws, h->beam_bytes, s);
}

hipError_t head_embed(Head *h, const int *tokens, const int *pos, int n_seqs, int rows_per_seq, float *Y, int64_t ys,
                      hipStream_t s) {
    if (!h || !h->E) return hipErrorInvalidValue;
    return launch_embed_rows(h->E, h->es, h->vocab, h->d_model, tokens, h->P, h->ps, h->max_pos, pos, n_seqs,
                             rows_per_seq, Y, ys, s);
}

// Decoding, greedy (sample == nullptr) or sampled: every check first, then n_new x (embed, step_batch, logits, token
// choice) on the stream.  Step t + 1's embed reads row t of tokens_out on the device; the host only advances the
// positions it passes along.  Sampled, sequence b draws at step t with the counter (stream_b << 32) + pos_b + t, filled
// on the host into the sample launch's arguments, and prev is the row of tokens fed at that step: a sequence that has
// produced eos keeps producing it while its steps run on.
int generate_steps(void *decoder, void *head, int n_seqs, const int *slots, const int32_t *tokens_in, int n_new,
                   const int *pos, const SampleArgs *sample, const uint32_t *streams, int32_t *tokens_out,
                   void *stream) {
    Stack *S = static_cast<Stack *>(decoder);
    Head *h = static_cast<Head *>(head);
    int d_model, d_k, max_seq, n_slots;
    if (!h || !h->E || !slots || !tokens_in || n_new < 0 || decoder_limits(S, &d_model, &d_k, &max_seq, &n_slots))
        return (int)hipErrorInvalidValue;
    if (n_seqs < 1 || n_seqs > n_slots || n_seqs > h->max_rows || n_seqs > kEmbedMaxSeqs || d_model != h->d_model ||
        d_k > 64 || (n_new > 0 && !tokens_out))
        return (int)hipErrorInvalidValue;
    uint64_t counters[kEmbedMaxSeqs];
    SampleArgs a = {};
    if (sample) {
        a = *sample;
        a.counters = counters;
        if (head_sample_check(h, n_seqs, a) != hipSuccess) return (int)hipErrorInvalidValue;
    }
    int at[kEmbedMaxSeqs];
    uint64_t seen = 0;  // n_slots <= 64
    for (int b = 0; b < n_seqs; ++b) {
        int filled;
        if (decoder_slot_state(S, slots[b], nullptr, &filled) || !decoder_slot_begun(S, slots[b]) ||
            decoder_slot_indirect(S, slots[b]) ||
            (seen >> slots[b] & 1))
            return (int)hipErrorInvalidValue;
        seen |= (uint64_t)1 << slots[b];
        at[b] = pos ? pos[b] : filled;
        if (at[b] < 0 || at[b] > filled || n_new > max_seq - at[b] || (h->P && n_new > h->max_pos - at[b]))
            return (int)hipErrorInvalidValue;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *X = h->rows, *Y = h->rows + (size_t)h->max_rows * h->d_model;
    const int32_t *tok = tokens_in;
    for (int t = 0; t < n_new; ++t) {
        int32_t *next = tokens_out + (size_t)t * n_seqs;
        hipError_t e;
        if ((e = head_embed(h, tok, at, n_seqs, 1, X, d_model, s)) != hipSuccess ||
            (e = decoder_step_batch(S, n_seqs, slots, at, 1, X, Y, s)) != hipSuccess)
            return (int)e;
        if (sample) {
            for (int b = 0; b < n_seqs; ++b)
                counters[b] = ((uint64_t)(streams ? streams[b] : (uint32_t)slots[b]) << 32) + (uint64_t)at[b];
            a.prev = tok;
            e = head_sample_tokens(h, Y, d_model, n_seqs, a, next, s);
        } else {
            e = head_next_tokens(h, Y, d_model, n_seqs, next, s);
        }
        if (e != hipSuccess) return (int)e;
        tok = next;
        for (int b = 0; b < n_seqs; ++b) ++at[b];
    }
    return 0;
}

// Beam search over two sets of rows = n_groups * beams cache slots: every check first, then n_new x
// (embed, step_batch on the set that holds the beams, the head's beam step, gather_slots into the other set by the
// parents just chosen) on the stream.  Step t + 1 reads row t of the three outputs on the device; the host only
// advances positions and swaps the sets' roles.
constexpr int kBeamGenerateMaxRows = 32;  // two sets share the decoder's 64 slots

int generate_beam_steps(void *decoder, void *head, int n_groups, int beams, const int *slots_a, const int *slots_b,
                        const int32_t *tokens_in, int n_new, const int *pos, const float *scores_in, int eos,
                        int32_t *tokens_out, int32_t *parents_out, float *scores_out, void *stream) {
    Stack *S = static_cast<Stack *>(decoder);
    Head *h = static_cast<Head *>(head);
    int d_model, d_k, max_seq, n_slots;
    if (!h || !h->E || !slots_a || !slots_b || !tokens_in || n_new < 0 ||
        decoder_limits(S, &d_model, &d_k, &max_seq, &n_slots))
        return (int)hipErrorInvalidValue;
    if (n_groups < 1 || head_beam_check(h, n_groups, beams) != hipSuccess ||
        n_groups * beams > kBeamGenerateMaxRows || 2 * n_groups * beams > n_slots || d_model != h->d_model ||
        d_k > 64 || (n_new > 0 && (!tokens_out || !parents_out || !scores_out)))
        return (int)hipErrorInvalidValue;
    const int rows = n_groups * beams;
    int at[kBeamGenerateMaxRows], next_rows[kBeamGenerateMaxRows];  // per row / per group
    uint64_t seen = 0;                                              // n_slots <= 64
    for (int g = 0; g < n_groups; ++g) {
        int enc0 = 0, start = 0;
        for (int q = 0; q < beams; ++q) {
            const int r = g * beams + q;
            int enc_a, enc_b, filled_a, filled_b;
            if (decoder_slot_state(S, slots_a[r], &enc_a, &filled_a) ||
                decoder_slot_state(S, slots_b[r], &enc_b, &filled_b) || !decoder_slot_begun(S, slots_a[r]) ||
                !decoder_slot_begun(S, slots_b[r]) || enc_b != enc_a ||
                slots_a[r] == slots_b[r] || (seen >> slots_a[r] & 1) || (seen >> slots_b[r] & 1) ||
                decoder_slot_indirect(S, slots_a[r]) || decoder_slot_indirect(S, slots_b[r]))
                return (int)hipErrorInvalidValue;
            seen |= (uint64_t)1 << slots_a[r] | (uint64_t)1 << slots_b[r];
            if (q == 0) {
                enc0 = enc_a;
                start = pos ? pos[g] : filled_a;
            }
            if (enc_a != enc0 || start < 0 || start > filled_a || n_new > max_seq - start ||
                (h->P && n_new > h->max_pos - start))
                return (int)hipErrorInvalidValue;
            at[r] = start;
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *X = h->rows, *Y = h->rows + (size_t)h->max_rows * h->d_model;
    const int32_t *tok = tokens_in;
    const float *sc = scores_in;
    const int *cur = slots_a, *other = slots_b;
    for (int t = 0; t < n_new; ++t) {
        int32_t *next = tokens_out + (size_t)t * rows, *par = parents_out + (size_t)t * rows;
        float *nsc = scores_out + (size_t)t * rows;
        for (int g = 0; g < n_groups; ++g) next_rows[g] = at[g * beams] + 1;
        hipError_t e;
        if ((e = head_embed(h, tok, at, rows, 1, X, d_model, s)) != hipSuccess ||
            (e = decoder_step_batch(S, rows, cur, at, 1, X, Y, s)) != hipSuccess ||
            (e = head_beam_step(h, Y, d_model, n_groups, beams, sc, tok, eos, par, next, nsc, s)) != hipSuccess ||
            (e = decoder_gather_slots(S, n_groups, beams, other, cur, par, next_rows, s)) != hipSuccess)
            return (int)e;
        tok = next;
        sc = nsc;
        std::swap(cur, other);
        for (int r = 0; r < rows; ++r) ++at[r];
    }
    return 0;
}

// Beam search over ONE set of rows = n_groups * beams cache slots: every check first, then n_new x
// (embed, step_batch_indirect with the groups' prompt slots as cross slots, the head's beam step, the in-place reindex
// of the row table by the parents just chosen) on the stream.  No K / V row is copied; rows may fill the decoder's
// slots and the head's max_rows (the copy path's cap of 32 belonged to its two sets).  What step_batch_indirect and
// beam_reindex would refuse at step t is refused here, before the first launch.
int generate_beam_indirect_steps(void *decoder, void *head, int n_groups, int beams, const int *slots,
                                 const int *src_slots, const int32_t *tokens_in, int n_new, const int *pos,
                                 const float *scores_in, int eos, int32_t *tokens_out, int32_t *parents_out,
                                 float *scores_out, void *stream) {
    Stack *S = static_cast<Stack *>(decoder);
    Head *h = static_cast<Head *>(head);
    int d_model, d_k, max_seq, n_slots;
    if (!h || !h->E || !slots || !src_slots || !tokens_in || n_new < 0 ||
        decoder_limits(S, &d_model, &d_k, &max_seq, &n_slots))
        return (int)hipErrorInvalidValue;
    if (n_groups < 1 || head_beam_check(h, n_groups, beams) != hipSuccess || n_groups * beams > kEmbedMaxSeqs ||
        n_groups * beams > n_slots || d_model != h->d_model || d_k > 64 ||
        (n_new > 0 && (!tokens_out || !parents_out || !scores_out)))
        return (int)hipErrorInvalidValue;
    const int rows = n_groups * beams;
    int at[kEmbedMaxSeqs], cross[kEmbedMaxSeqs], next_rows[kEmbedMaxSeqs];  // per row, per row, per group
    uint64_t seen = 0;                                                      // n_slots <= 64
    for (int g = 0; g < n_groups; ++g) {
        int enc_src, filled_src, start = 0;
        if (decoder_slot_state(S, src_slots[g], &enc_src, &filled_src) || !decoder_slot_begun(S, src_slots[g]))
            return (int)hipErrorInvalidValue;
        for (int q = 0; q < beams; ++q) {
            const int r = g * beams + q;
            int enc, filled;
            if (decoder_slot_state(S, slots[r], &enc, &filled) || !decoder_slot_indirect(S, slots[r]) ||
                enc != enc_src || (seen >> slots[r] & 1))
                return (int)hipErrorInvalidValue;
            seen |= (uint64_t)1 << slots[r];
            if (q == 0) start = pos ? pos[g] : filled;
            if (start < 0 || start > filled || n_new > max_seq - start || (h->P && n_new > h->max_pos - start))
                return (int)hipErrorInvalidValue;
            at[r] = start;
            cross[r] = src_slots[g];
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *X = h->rows, *Y = h->rows + (size_t)h->max_rows * h->d_model;
    const int32_t *tok = tokens_in;
    const float *sc = scores_in;
    for (int t = 0; t < n_new; ++t) {
        int32_t *next = tokens_out + (size_t)t * rows, *par = parents_out + (size_t)t * rows;
        float *nsc = scores_out + (size_t)t * rows;
        for (int g = 0; g < n_groups; ++g) next_rows[g] = at[g * beams] + 1;
        hipError_t e;
        if ((e = head_embed(h, tok, at, rows, 1, X, d_model, s)) != hipSuccess ||
            (e = decoder_step_batch_indirect(S, rows, slots, cross, at, 1, X, Y, s)) != hipSuccess ||
            (e = head_beam_step(h, Y, d_model, n_groups, beams, sc, tok, eos, par, next, nsc, s)) != hipSuccess ||
            (e = decoder_beam_reindex(S, n_groups, beams, slots, par, next_rows, s)) != hipSuccess)
            return (int)e;
        tok = next;
        sc = nsc;
        for (int r = 0; r < rows; ++r) ++at[r];
    }
    return 0;
}

}  // namespace

}  // namespace qgemm

using namespace qgemm;

extern "C" {

int qgemm_argmax_rows_plan(int64_t rows, int w, int *parts) {
    int p, chunk;
    if (!argmax_plan(rows, w, &p, &chunk)) return (int)hipErrorInvalidValue;
    if (parts) *parts = p;
    return 0;
}

size_t qgemm_argmax_rows_workspace_size(int64_t rows, int w) { return argmax_ws_bytes(rows, w); }

int qgemm_argmax_rows(const float *S, int64_t s_stride_h, int64_t rows, int w, int32_t *idx, float *val,
                      void *workspace, size_t ws_bytes, void *stream) {
    return (int)launch_argmax_rows(S, s_stride_h, rows, w, idx, val, workspace, ws_bytes,
                                   static_cast<hipStream_t>(stream));
}

int qgemm_embed_rows(const float *E, int64_t e_stride_h, int vocab, int d_model, const int32_t *tokens, const float *P,
                     int64_t p_stride_h, int max_pos, const int *pos, int n_seqs, int rows_per_seq, float *Y,
                     int64_t y_stride_h, void *stream) {
    return (int)launch_embed_rows(E, e_stride_h, vocab, d_model, tokens, P, p_stride_h, max_pos, pos, n_seqs,
                                  rows_per_seq, Y, y_stride_h, static_cast<hipStream_t>(stream));
}

int qgemm_head_create(const void *packed_w, int d_model, int vocab, const float *bias, const float *E,
                      int64_t e_stride_h, const float *P, int64_t p_stride_h, int max_pos, int max_rows, void **head) {
    if (!head) return (int)hipErrorInvalidValue;
    *head = nullptr;
    if (!packed_w || d_model < 1 || vocab < 1 || vocab > kArgmaxMaxW || max_rows < 1 || (E && e_stride_h < d_model) ||
        (P && (!E || p_stride_h < d_model || max_pos < 1)))
        return (int)hipErrorInvalidValue;
    Head *h = new (std::nothrow) Head();
    if (!h) return (int)hipErrorOutOfMemory;
    h->d_model = d_model;
    h->vocab = vocab;
    h->max_pos = P ? max_pos : 0;
    h->max_rows = max_rows;
    h->pw = packed_w;
    h->bias = bias;
    h->E = E;
    h->P = P;
    h->es = e_stride_h;
    h->ps = p_stride_h;
    for (int m = 1; m <= max_rows; ++m) {  // neither size is monotonic in the row count
        h->lin_bytes = std::max(h->lin_bytes, qgemm_linear_workspace_size(m, vocab, d_model));
        h->arg_bytes = std::max(h->arg_bytes, argmax_ws_bytes(m, vocab));
        h->smp_bytes = std::max(h->smp_bytes, sample_ws_bytes(m, vocab, 1024));
    }
    for (int beams = 1; beams <= 8; ++beams)
        for (int groups = 1; groups * beams <= std::min(max_rows, 64); ++groups)
            h->beam_bytes = std::max(h->beam_bytes, beam_step_ws_bytes(groups, beams, vocab));
    hipError_t e;
    if ((e = hipMalloc(&h->logits, sizeof(float) * (size_t)max_rows * vocab)) != hipSuccess ||
        (e = hipMalloc(&h->rows, sizeof(float) * 2 * (size_t)max_rows * d_model)) != hipSuccess ||
        (e = hipMalloc(&h->lin_ws, std::max<size_t>(h->lin_bytes, 16))) != hipSuccess ||
        (e = hipMalloc(&h->arg_ws, std::max<size_t>(h->arg_bytes, 16))) != hipSuccess ||
        (e = hipMalloc(&h->smp_ws, std::max<size_t>(h->smp_bytes, 16))) != hipSuccess ||
        (e = hipMalloc(&h->beam_ws, std::max<size_t>(h->beam_bytes, 16))) != hipSuccess) {
        head_free(h);
        return (int)e;
    }
    *head = h;
    return 0;
}

int qgemm_head_destroy(void *head) {
    head_free(static_cast<Head *>(head));
    return 0;
}

int qgemm_head_logits(void *head, const float *H, int64_t h_stride_h, int rows, float *logits, int64_t l_stride_h,
                      void *stream) {
    return (int)head_logits(static_cast<Head *>(head), H, h_stride_h, rows, logits, l_stride_h,
                            static_cast<hipStream_t>(stream));
}

int qgemm_head_next_tokens(void *head, const float *H, int64_t h_stride_h, int rows, int32_t *tokens, void *stream) {
    return (int)head_next_tokens(static_cast<Head *>(head), H, h_stride_h, rows, tokens,
                                 static_cast<hipStream_t>(stream));
}

int qgemm_head_sample_tokens(void *head, const float *H, int64_t h_stride_h, int rows, int top_k, float top_p,
                             float temperature, uint64_t seed, uint64_t counter0, const uint64_t *counters,
                             const int32_t *prev, int eos, int32_t *tokens, void *stream) {
    const SampleArgs a = {top_k, top_p, temperature, seed, counter0, counters, prev, eos};
    return (int)head_sample_tokens(static_cast<Head *>(head), H, h_stride_h, rows, a, tokens,
                                   static_cast<hipStream_t>(stream));
}

int qgemm_head_embed(void *head, const int32_t *tokens, const int *pos, int n_seqs, int rows_per_seq, float *Y,
                     int64_t y_stride_h, void *stream) {
    return (int)head_embed(static_cast<Head *>(head), tokens, pos, n_seqs, rows_per_seq, Y, y_stride_h,
                           static_cast<hipStream_t>(stream));
}

int qgemm_decoder_generate(void *decoder, void *head, int n_seqs, const int *slots, const int32_t *tokens_in,
                           int n_new, const int *pos, int32_t *tokens_out, void *stream) {
    return generate_steps(decoder, head, n_seqs, slots, tokens_in, n_new, pos, nullptr, nullptr, tokens_out, stream);
}

int qgemm_decoder_generate_sampled(void *decoder, void *head, int n_seqs, const int *slots, const int32_t *tokens_in,
                                   int n_new, const int *pos, int top_k, float top_p, float temperature, uint64_t seed,
                                   const uint32_t *streams, int eos, int32_t *tokens_out, void *stream) {
    const SampleArgs a = {top_k, top_p, temperature, seed, 0, nullptr, nullptr, eos};
    return generate_steps(decoder, head, n_seqs, slots, tokens_in, n_new, pos, &a, streams, tokens_out, stream);
}

int qgemm_head_beam_step(void *head, const float *H, int64_t h_stride_h, int n_groups, int beams,
                         const float *scores_in, const int32_t *prev, int eos, int32_t *parents, int32_t *tokens,
                         float *scores_out, void *stream) {
    return (int)head_beam_step(static_cast<Head *>(head), H, h_stride_h, n_groups, beams, scores_in, prev, eos, parents,
                               tokens, scores_out, static_cast<hipStream_t>(stream));
}

int qgemm_decoder_generate_beam(void *decoder, void *head, int n_groups, int beams, const int *slots_a,
                                const int *slots_b, const int32_t *tokens_in, int n_new, const int *pos,
                                const float *scores_in, int eos, int32_t *tokens_out, int32_t *parents_out,
                                float *scores_out, void *stream) {
    return generate_beam_steps(decoder, head, n_groups, beams, slots_a, slots_b, tokens_in, n_new, pos, scores_in, eos,
                               tokens_out, parents_out, scores_out, stream);
}

int qgemm_decoder_generate_beam_indirect(void *decoder, void *head, int n_groups, int beams, const int *slots,
                                         const int *src_slots, const int32_t *tokens_in, int n_new, const int *pos,
                                         const float *scores_in, int eos, int32_t *tokens_out, int32_t *parents_out,
                                         float *scores_out, void *stream) {
    return generate_beam_indirect_steps(decoder, head, n_groups, beams, slots, src_slots, tokens_in, n_new, pos,
                                        scores_in, eos, tokens_out, parents_out, scores_out, stream);
}

}  // extern "C"
