// topk_select.h -- the k best columns of an fp32 row in argmax's order, shared by sample.hip and
// beam.hip (s22): the 56-bit composites, their sources and the radix select.  Device code only; every kernel that uses
// it runs kSampleThreads threads.
//
// Every candidate column (S[i] > -inf: no NaN, no -inf) gets the 56-bit composite
//   (key(S[i]) << 24) | (w - 1 - i),   key = the order-preserving 32-bit image of the float with -0 folded onto +0,
// so "greater value first, lower index first among equal values" (head.hip better()) is the plain order of distinct
// integers, and 0 stands for "no candidate".  The k greatest of a set of distinct integers do not depend on how the set
// is grouped: a row may be cut into parts, each part's k best merged later.  radix_select finds the k-th greatest
// composite by 8-bit digits from the top: an LDS histogram of the digit over the elements that match the digits fixed
// so far, then the bucket in which the count from the top reaches k.  It stops as soon as a bucket closes the count
// exactly, which on distinct values happens once the key's own 32 bits are fixed; equal values go on into the index
// digits, and there only the lowest indices pass.  A thread adds a run of equal digits with one LDS atomic, so a row
// whose values share their top digit does not serialize on one counter.
#pragma once

#include "qgemm_internal.h"

namespace qgemm {

constexpr int kSampleThreads = 256;
constexpr int kSampleMaxW = 1 << 24;  // w - 1 - i fits the composite's 24 index bits
constexpr int kBatch = 4;             // 16-byte loads a thread issues before it uses the first (the sources)

__device__ __forceinline__ uint64_t composite(float x, int i, int w) {
    if (!(x > -INFINITY)) return 0;  // NaN and -inf are no candidates
    uint32_t b = __float_as_uint(x);
    b = (b == 0x80000000u) ? 0u : b;  // -0 == +0
    const uint32_t key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)key << 24) | (uint32_t)(w - 1 - i);
}

// the column a composite (!= 0) stands for
__device__ __forceinline__ int composite_column(uint64_t c, int w) { return w - 1 - (int)(c & 0xffffffu); }

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

// n composites written by an earlier launch (select_part): plain loads
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

// Launch 1 of a split row, the body of a workgroup that owns columns [src.c0, src.c1): the part's k best composites
// to out[0 .. k), in no particular order, 0 in the places a part with fewer candidates leaves.  count: one int (LDS).
__device__ __forceinline__ void select_part(const RowSource &src, int k, uint64_t *out, int *hist, int *pick,
                                            int *count) {
    const int t = threadIdx.x;
    if (t == 0) *count = 0;
    const Select sel = radix_select(src, k, hist, pick);
    src.each([&](uint64_t c) {
        if (c == 0 || c < sel.thr) return;
        const int at = atomicAdd(count, 1);
        if (at < k) out[at] = c;
    });
    for (int j = sel.kept + t; j < k; j += kSampleThreads) out[j] = 0;
}

}  // namespace qgemm
