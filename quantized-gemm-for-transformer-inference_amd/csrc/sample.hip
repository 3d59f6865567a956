// sample.hip -- sampled token choice: the top_k best columns of every fp32 row in argmax's order, their
// softmax at a temperature, the nucleus cut top_p inside that list, one seeded draw, and the end-token hold.  The
// arithmetic is defined step by step at qgemm_sample_rows (include/qgemm.h), so a numpy restatement predicts every
// token (tests/sample_oracle.py); the softmax is the chain of qgemm_softmax_rows (softmax_exp, qgemm_internal.h) and
// the draw is the counter generator of qgemm_fill_uniform (mix64).
//
// Selection.  The composites, their sources and radix_select are topk_select.h's (shared with beam.hip).
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
#include "topk_select.h"

namespace qgemm {

namespace {

constexpr int kSampleMaxTopK = 1024;
constexpr int kSampleMaxCounters = 64;
constexpr int kPerLane = kSampleMaxTopK / 64;  // list elements per lane of the wave that runs the sequential chains
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

// Launch 1 of a split row: the k best composites of part blockIdx.x % parts of row blockIdx.x / parts, in no
// particular order, at ws[blockIdx.x * k ..], 0 in the places a part with fewer candidates leaves.
__global__ __launch_bounds__(kSampleThreads) void sample_part_kernel(const float *__restrict__ S, int64_t stride, int w,
                                                                     int chunk, int parts, int k,
                                                                     uint64_t *__restrict__ ws) {
    __shared__ int hist[256];
    __shared__ int pick[4];
    __shared__ int count;
    const int64_t row = blockIdx.x / parts;
    const int part = blockIdx.x % parts;
    const int c0 = part * chunk;
    const RowSource src = {S + row * stride, c0, min(w, c0 + chunk), w};
    select_part(src, k, ws + (int64_t)blockIdx.x * k, hist, pick, &count);
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
