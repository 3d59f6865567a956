// sample.hip -- sampled token choice: the top_k best columns of every fp32 row in argmax's order, their
// softmax at a temperature, the nucleus cut top_p inside that list, one seeded draw, and the end-token hold.  The
// arithmetic is defined step by step at qgemm_sample_rows (include/qgemm.h), so a numpy restatement predicts every
// token (tests/sample_oracle.py); the softmax is the chain of qgemm_softmax_rows (softmax_exp, qgemm_internal.h) and
// the draw is the counter generator of qgemm_fill_uniform (mix64).
//
// Selection.  Every candidate column (S[i] > -inf: no NaN, no -inf) gets the 56-bit composite
//   (key(S[i]) << 24) | (w - 1 - i),   key = the order-preserving 32-bit image of the float with -0 folded onto +0,
// so "greater value first, lower index first among equal values" (head.hip better()) is the plain order of distinct
// integers, and 0 stands for "no candidate".  The k greatest of a set of distinct integers do not depend on how the set
// is grouped: a row may be cut into parts, each part's k best merged later.  radix_select finds the k-th greatest
// composite by 8-bit digits from the top: an LDS histogram of the digit over the elements that match the digits fixed
// so far, then the bucket in which the count from the top reaches k.  It stops as soon as a bucket closes the count
// exactly, which on distinct values happens once the key's own 32 bits are fixed; equal values go on into the index
// digits, and there only the lowest indices pass.  A thread adds a run of equal digits with one LDS atomic, so a row
// whose values share their top digit does not serialize on one counter.
//
// Launches.  parts == 1: one workgroup per row does everything.  parts > 1 (few, wide rows, the split rule of the
// argmax): launch 1 gives every (row, part) a workgroup that writes the part's k best composites into the workspace
// (0 in unused places), launch 2 runs the same select over a row's parts * k composites and finishes.  Workgroups meet
// only through the workspace between launches.  Argument checks first, then launches only.
#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/qgemm.h"
#include "qgemm_internal.h"

namespace qgemm {

namespace {

constexpr int kSampleThreads = 256;
constexpr int kSampleMaxW = 1 << 24;  // w - 1 - i fits the composite's 24 index bits
constexpr int kSampleMaxTopK = 1024;
constexpr int kSampleMaxCounters = 64;
constexpr int kPerLane = kSampleMaxTopK / 64;  // list elements per lane of the wave that runs the sequential chains
constexpr int kBatch = 4;                      // 16-byte loads a thread issues before it uses the first (the sources)
// the split rule: as argmax_plan (head.hip)
constexpr int kSampleManyRows = 256;
constexpr int kSampleMinChunk = 4096;
constexpr int kSampleTargetGroups = 512;
constexpr int kSampleMaxParts = 64;
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ULL;

// per-row counters: a kernel argument passed by value (512 bytes), filled on the host at enqueue
struct SampleCounters {
    uint64_t c[kSampleMaxCounters];
};

__device__ __forceinline__ uint64_t composite(float x, int i, int w) {
    if (!(x > -INFINITY)) return 0;  // NaN and -inf are no candidates
    uint32_t b = __float_as_uint(x);
    b = (b == 0x80000000u) ? 0u : b;  // -0 == +0
    const uint32_t key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)key << 24) | (uint32_t)(w - 1 - i);
}

// A source hands every composite of its elements to f, each thread its share, in no particular order; it may also
// hand over 0 (no candidate), which every f ignores.
// columns [c0, c1) of the row at p: 16-byte loads between a scalar head and a scalar tail, as argmax_rows_kernel
struct RowSource {
    const float *p;
    int c0, c1, w;
    template <class F>
    __device__ __forceinline__ void each(F &&f) const {
        const int t = threadIdx.x, n = c1 - c0;
        const int head = min(n, (int)((4 - ((reinterpret_cast<uintptr_t>(p + c0) >> 2) & 3)) & 3));
        const int nvec = (n - head) >> 2;
        const int v0 = c0 + head, t0 = v0 + 4 * nvec;
        if (t < head) f(composite(p[c0 + t], c0 + t, w));
        const float4 *pv = reinterpret_cast<const float4 *>(p + v0);
        // kBatch loads in flight before the first is used: f branches and adds to LDS, so the compiler does not
        // overlap one iteration's load with the next, and a lone workgroup has nothing else to hide the latency
        // behind.  Places past the end take -inf, which is no candidate.
        for (int v = t; v < nvec; v += kBatch * kSampleThreads) {
            float4 q[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const int u = v + j * kSampleThreads;
                q[j] = u < nvec ? pv[u] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const int i = v0 + 4 * (v + j * kSampleThreads);
                f(composite(q[j].x, i, w));
                f(composite(q[j].y, i + 1, w));
                f(composite(q[j].z, i + 2, w));
                f(composite(q[j].w, i + 3, w));
            }
        }
        if (t < c1 - t0) f(composite(p[t0 + t], t0 + t, w));
    }
};

// n composites written by sample_part_kernel (an earlier launch): plain loads
struct ListSource {
    const uint64_t *c;
    int n;
    template <class F>
    __device__ __forceinline__ void each(F &&f) const {
        for (int i = threadIdx.x; i < n; i += 2 * kBatch * kSampleThreads) {  // batched as RowSource::each
            uint64_t v[2 * kBatch];
#pragma unroll
            for (int j = 0; j < 2 * kBatch; ++j) {
                const int u = i + j * kSampleThreads;
                v[j] = u < n ? c[u] : 0;
            }
#pragma unroll
            for (int j = 0; j < 2 * kBatch; ++j) f(v[j]);
        }
    }
};

// the kept elements are the composites c != 0 with c >= thr, `kept` of them
struct Select {
    uint64_t thr;
    int kept;
};

// The min(k, candidates) greatest composites of src, by the whole workgroup.  hist: 256 ints, pick: 4 ints (LDS).
template <class Src>
__device__ __forceinline__ Select radix_select(const Src &src, int k, int *hist, int *pick) {
    const int t = threadIdx.x;
    uint64_t prefix = 0;  // the digits fixed so far
    int need = k;         // how many of the elements that match them are still to be taken
    for (int shift = 48; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        int run_d = 0, run_n = 0;
        src.each([&](uint64_t c) {
            if (c == 0 || (c >> (shift + 8)) != (prefix >> (shift + 8))) return;
            const int d = (int)(c >> shift) & 255;
            if (d != run_d && run_n) {
                atomicAdd(&hist[run_d], run_n);
                run_n = 0;
            }
            run_d = d;
            ++run_n;
        });
        if (run_n) atomicAdd(&hist[run_d], run_n);
        __syncthreads();
        if (t < 64) {  // wave 0: lane t owns buckets 255 - 4 t .. 252 - 4 t, from the top
            int h[4], sum = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) sum += h[i] = hist[255 - 4 * t - i];
            int inc = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_up(inc, off, 64);
                if (t >= off) inc += v;
            }
            int above = inc - sum;
            if (t == 63) pick[3] = inc;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (above < need && need <= above + h[i]) {
                    pick[0] = 255 - 4 * t - i;
                    pick[1] = above;
                    pick[2] = h[i];
                }
                above += h[i];
            }
        }
        __syncthreads();
        if (pick[3] < need) return {1, pick[3]};  // first pass only: fewer candidates than k, all of them kept
        prefix |= (uint64_t)pick[0] << shift;
        if (pick[1] + pick[2] == need) return {prefix, k};  // the bucket closes the count: everything >= prefix
        need -= pick[1];
    }
    return {prefix, k};  // not reached: distinct composites close the count at the last digit at the latest
}

// Launch 1 of a split row: the k best composites of part blockIdx.x % parts of row blockIdx.x / parts, in no
// particular order, at ws[blockIdx.x * k ..], 0 in the places a part with fewer candidates leaves.
__global__ __launch_bounds__(kSampleThreads) void sample_part_kernel(const float *__restrict__ S, int64_t stride, int w,
                                                                     int chunk, int parts, int k,
                                                                     uint64_t *__restrict__ ws) {
    __shared__ int hist[256];
    __shared__ int pick[4];
    __shared__ int count;
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / parts;
    const int part = blockIdx.x % parts;
    const int c0 = part * chunk;
    const RowSource src = {S + row * stride, c0, min(w, c0 + chunk), w};
    if (t == 0) count = 0;
    const Select sel = radix_select(src, k, hist, pick);
    uint64_t *out = ws + (int64_t)blockIdx.x * k;
    src.each([&](uint64_t c) {
        if (c == 0 || c < sel.thr) return;
        const int at = atomicAdd(&count, 1);
        if (at < k) out[at] = c;
    });
    for (int j = sel.kept + t; j < k; j += kSampleThreads) out[j] = 0;
}

// A sequential fp32 sum over the list in wave 0: lane l holds elements kPerLane l .. kPerLane l + kPerLane - 1 in x and
// ends with the running sums through each of them in cc.  The running value hops from lane to lane (hop_left, as
// encoder_ops.hip lane_block_sum): every lane runs every step, lane l's step l starts from its left neighbour's last
// sum (lane 0's from +0) and is the one it keeps.  nl = the lanes that hold elements; elements past the list must be
// -0.0f (x + -0 == x for every x), so the last lane's sums past the list repeat the list's last one.
__device__ __forceinline__ void lane_chain(const float (&x)[kPerLane], int nl, float (&cc)[kPerLane]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) cc[i] = 0.0f;
    for (int step = 0; step < nl; ++step) {
        float r = hop_left(cc[kPerLane - 1]);
        const bool live = step <= lane;
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) {
            r = __fadd_rn(r, x[i]);
            cc[i] = live ? r : cc[i];
        }
    }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

// One workgroup per row: the select (over the row itself, or with kList over the n_list composites its parts left in
// the workspace), a bitonic sort of the kept composites in LDS, the softmax of their values, the two sequential chains
// in wave 0, the nucleus cut, the draw, the hold and the stores.  k: the list's length (top_k, or 1 for temperature 0);
// k_out: the row length of top_idx / top_prob.
template <bool kList>
__global__ __launch_bounds__(kSampleThreads) void sample_finish_kernel(
    const float *__restrict__ S, int64_t stride, int w, int k, int k_out, int n_list, const uint64_t *__restrict__ ws,
    float top_p, float inv_t, uint64_t seed, uint64_t counter0, SampleCounters ctr, bool has_ctr,
    const int *__restrict__ prev, int eos, int *__restrict__ idx, int *__restrict__ top_idx,
    float *__restrict__ top_prob, int *__restrict__ n_kept) {
    __shared__ uint64_t list[kSampleMaxTopK];
    __shared__ int col[kSampleMaxTopK];
    __shared__ float val[kSampleMaxTopK], ev[kSampleMaxTopK], pv[kSampleMaxTopK], cv[kSampleMaxTopK];
    __shared__ int hist[256];
    __shared__ int pick[4];
    __shared__ float wave_m[kSampleThreads / 64];
    __shared__ int count, n_sh, j_sh;
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x;
    const float *p = S + row * stride;
    if (t == 0) count = 0;
    Select sel;
    if constexpr (kList) {
        const ListSource src = {ws + row * n_list, n_list};
        sel = radix_select(src, k, hist, pick);
        src.each([&](uint64_t c) {
            if (c == 0 || c < sel.thr) return;
            const int at = atomicAdd(&count, 1);
            if (at < kSampleMaxTopK) list[at] = c;
        });
    } else {
        const RowSource src = {p, 0, w, w};
        sel = radix_select(src, k, hist, pick);
        src.each([&](uint64_t c) {
            if (c == 0 || c < sel.thr) return;
            const int at = atomicAdd(&count, 1);
            if (at < kSampleMaxTopK) list[at] = c;
        });
    }
    const int kk = sel.kept;  // k' of the contract
    const bool hold = prev && eos >= 0 && prev[row] == eos;
    if (kk == 0) {  // no candidate: argmax_rows' answer for such a row
        if (t == 0) {
            idx[row] = hold ? eos : 0;
            if (n_kept) n_kept[row] = 0;
        }
        if (top_idx)
            for (int j = t; j < k_out; j += kSampleThreads) {
                top_idx[row * k_out + j] = -1;
                top_prob[row * k_out + j] = 0.0f;
            }
        return;
    }
    int n2 = 1;
    while (n2 < kk) n2 <<= 1;
    for (int j = kk + t; j < n2; j += kSampleThreads) list[j] = 0;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)  // bitonic sort, greatest first
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = t; i < n2; i += kSampleThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t a = list[i], b = list[l];
                    if ((i & size) == 0 ? a < b : a > b) {
                        list[i] = b;
                        list[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    // the list's columns and their values (own bits, read from the row)
    for (int j = t; j < kk; j += kSampleThreads) {
        const int c = w - 1 - (int)(list[j] & 0xffffffu);
        col[j] = c;
        val[j] = p[c];
    }
    __syncthreads();
    // qgemm_softmax_rows on the list with scale = inv_t: the contract at softmax_row_max (qgemm_internal.h)
    float cand = -INFINITY;
    for (int j = t ? t : kSampleThreads; j < kk; j += kSampleThreads) {  // element 0 is the seed
        const float x = __fmul_rn(val[j], inv_t);
        cand = (x > cand) ? x : cand;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(cand, off, 64);
        cand = (o > cand) ? o : cand;
    }
    if ((t & 63) == 0) wave_m[t >> 6] = cand;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSampleThreads / 64; ++j) cand = (wave_m[j] > cand) ? wave_m[j] : cand;
    const float x0 = __fmul_rn(val[0], inv_t);
    const float mx = (cand > x0) ? cand : x0;
    for (int j = t; j < kSampleMaxTopK; j += kSampleThreads) ev[j] = j < kk ? softmax_exp(val[j], inv_t, mx) : -0.0f;
    __syncthreads();
    // wave 0: the sum in list order, p = e / sum, the cumulative sums in list order, the nucleus cut
    const int nl = (kk + kPerLane - 1) / kPerLane;
    float x[kPerLane], cc[kPerLane];
    if (t < 64) {
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) x[i] = ev[kPerLane * t + i];
        lane_chain(x, nl, cc);
        const float sum = __shfl(cc[kPerLane - 1], nl - 1, 64);
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) {
            x[i] = kPerLane * t + i < kk ? __fdiv_rn(x[i], sum) : -0.0f;
            pv[kPerLane * t + i] = x[i];
        }
        lane_chain(x, nl, cc);
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) cv[kPerLane * t + i] = cc[i];
        const float thr = __fmul_rn(top_p, __shfl(cc[kPerLane - 1], nl - 1, 64));
        int first = INT_MAX;
#pragma unroll
        for (int i = kPerLane - 1; i >= 0; --i)
            if (kPerLane * t + i < kk && cc[i] >= thr) first = kPerLane * t + i;
        first = wave_min(first);
        if (t == 0) n_sh = first == INT_MAX ? kk : first + 1;
    }
    __syncthreads();
    const int n = n_sh;
    if (t < 64) {  // the draw: r = fl(u c_{n-1}), the first j < n with c_j > r
        const uint64_t counter = has_ctr ? ctr.c[row] : counter0 + ((uint64_t)row << 32);
        const uint64_t z = mix64(mix64(seed + kGolden) + (counter + 1) * kGolden);
        const float u = __fmul_rn((float)(uint32_t)(z >> 40), 1.0f / 16777216.0f);
        const float r = __fmul_rn(u, cv[n - 1]);
        int first = INT_MAX;
#pragma unroll
        for (int i = kPerLane - 1; i >= 0; --i)
            if (kPerLane * t + i < n && cc[i] > r) first = kPerLane * t + i;
        first = wave_min(first);
        if (t == 0) j_sh = first == INT_MAX ? 0 : first;
    }
    __syncthreads();
    if (t == 0) {
        idx[row] = hold ? eos : col[j_sh];
        if (n_kept) n_kept[row] = n;
    }
    if (top_idx)
        for (int j = t; j < k_out; j += kSampleThreads) {
            top_idx[row * k_out + j] = j < kk ? col[j] : -1;
            top_prob[row * k_out + j] = j < kk ? pv[j] : 0.0f;
        }
}

}  // namespace

// the plan from rows, w and top_k alone: argmax_plan's rule (every part at least kSampleMinChunk columns, so a part
// always holds more columns than top_k and the merge reads less than the row)
bool sample_plan(int64_t rows, int w, int top_k, int *parts, int *chunk) {
    if (rows < 0 || w < 1 || w > kSampleMaxW || top_k < 1 || top_k > kSampleMaxTopK) return false;
    int p = 1;
    if (rows > 0 && rows < kSampleManyRows) {
        const int by_width = w / kSampleMinChunk;
        const int by_rows = (int)((kSampleTargetGroups + rows - 1) / rows);
        p = std::max(1, std::min(std::min(by_width, by_rows), kSampleMaxParts));
    }
    for (;;) {  // until chunk = round_up(ceil(w / parts), 4) leaves no part empty: parts only ever shrinks
        const int ch = (int)round_up((w + p - 1) / p, 4), q = (w + ch - 1) / ch;
        *chunk = ch;
        *parts = q;
        if (q == p) return true;
        p = q;
    }
}

size_t sample_ws_bytes(int64_t rows, int w, int top_k) {
    int parts, chunk;
    if (!sample_plan(rows, w, top_k, &parts, &chunk) || parts == 1) return 0;
    return sizeof(uint64_t) * (size_t)rows * parts * top_k;
}

// the limits of the contract (include/qgemm.h), on the host before any launch; a NaN fails either comparison
hipError_t sample_check(int64_t rows, int w, int top_k, float top_p, float temperature, bool has_counters) {
    int parts, chunk;
    if (!sample_plan(rows, w, top_k, &parts, &chunk) || !(top_p > 0.0f && top_p <= 1.0f) ||
        !(temperature >= 0.0f && temperature < INFINITY) || (has_counters && rows > kSampleMaxCounters) ||
        rows * parts > INT_MAX)
        return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t launch_sample_rows(const float *S, int64_t stride, int64_t rows, int w, int top_k, float top_p,
                              float temperature, uint64_t seed, uint64_t counter0, const uint64_t *counters,
                              const int *prev, int eos, int *idx, int *top_idx, float *top_prob, int *n_kept, void *ws,
                              size_t ws_bytes, hipStream_t s) {
    int parts, chunk;
    if (!S || !idx || stride < w || (top_idx == nullptr) != (top_prob == nullptr) ||
        sample_check(rows, w, top_k, top_p, temperature, counters != nullptr) != hipSuccess)
        return hipErrorInvalidValue;
    sample_plan(rows, w, top_k, &parts, &chunk);
    if (parts > 1 && (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) ||
                      ws_bytes < sizeof(uint64_t) * (size_t)rows * parts * top_k))
        return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    const bool greedy = temperature == 0.0f;
    const int k = greedy ? 1 : top_k;
    const float inv_t = greedy ? 1.0f : 1.0f / temperature;  // one fp32 division
    SampleCounters ctr = {};
    if (counters)
        for (int64_t r = 0; r < rows; ++r) ctr.c[r] = counters[r];
    uint64_t *list = static_cast<uint64_t *>(ws);
    if (parts == 1) {
        sample_finish_kernel<false><<<(unsigned)rows, kSampleThreads, 0, s>>>(
            S, stride, w, k, top_k, 0, nullptr, top_p, inv_t, seed, counter0, ctr, counters != nullptr, prev, eos, idx,
            top_idx, top_prob, n_kept);
        return hipGetLastError();
    }
    sample_part_kernel<<<(unsigned)(rows * parts), kSampleThreads, 0, s>>>(S, stride, w, chunk, parts, k, list);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    sample_finish_kernel<true><<<(unsigned)rows, kSampleThreads, 0, s>>>(
        S, stride, w, k, top_k, parts * k, list, top_p, inv_t, seed, counter0, ctr, counters != nullptr, prev, eos, idx,
        top_idx, top_prob, n_kept);
    return hipGetLastError();
}

}  // namespace qgemm

using namespace qgemm;

extern "C" {

int qgemm_sample_rows_plan(int64_t rows, int w, int top_k, int *parts) {
    int p, chunk;
    if (!sample_plan(rows, w, top_k, &p, &chunk)) return (int)hipErrorInvalidValue;
    if (parts) *parts = p;
    return 0;
}

size_t qgemm_sample_rows_workspace_size(int64_t rows, int w, int top_k) { return sample_ws_bytes(rows, w, top_k); }

int qgemm_sample_rows(const float *S, int64_t s_stride_h, int64_t rows, int w, int top_k, float top_p,
                      float temperature, uint64_t seed, uint64_t counter0, const uint64_t *counters,
                      const int32_t *prev, int eos, int32_t *idx, int32_t *top_idx, float *top_prob, int32_t *n_kept,
                      void *workspace, size_t ws_bytes, void *stream) {
    return (int)launch_sample_rows(S, s_stride_h, rows, w, top_k, top_p, temperature, seed, counter0, counters, prev,
                                   eos, idx, top_idx, top_prob, n_kept, workspace, ws_bytes,
                                   static_cast<hipStream_t>(stream));
}

}  // extern "C"
