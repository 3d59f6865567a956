// rope.hip -- rotary position embeddings (the contract is at qgemm_rope_rows in include/qgemm.h): the
// half-split rotation of every d_k-wide group of a row by the row's position, in place, from caller-supplied cos / sin
// tables.  No trigonometry on the device.
//   y[i]     = fl(fl(x[i]     c) - fl(x[i + h] s))        h = d_k / 2, c = cos[p h + i], s = sin[p h + i]
//   y[i + h] = fl(fl(x[i + h] c) + fl(x[i]     s))
// Every step ONE IEEE fp32 operation (__fmul_rn / __fsub_rn / __fadd_rn: never contracted into an fma, whatever the
// compiler's flags).  A thread owns both elements of a pair and reads them before it writes either.
//
// ONE kernel, one launch: block (r, chunk, b) works on row r of sequence b -- row tab.row0[b] + r of X at position
// tab.pos0[b] + r -- and its threads on consecutive work items of that row: a float4 of a group's low half and the
// matching float4 of its high half where d_k % 8 == 0 and X, its row stride and both tables are 16-byte aligned, else
// one pair.  Both forms run the same operations on the same values, so they give the same bits.  The table of sequences
// travels in the kernel arguments (as ScatterTable does); qgemm_rope_rows is the table of one sequence.  Bandwidth- and
// launch-bound: a row is read once and written once, the tables' rows are shared by a row's groups through the cache.
#include <cstdint>

#include "qgemm_internal.h"

namespace qgemm {

namespace {

struct RopeTable {
    int64_t row0[kVarlenMaxSeqs];
    int n_rows[kVarlenMaxSeqs], pos0[kVarlenMaxSeqs];
};

__device__ __forceinline__ void rotate(float &lo, float &hi, float c, float s) {
    const float a = lo, b = hi;
    lo = __fsub_rn(__fmul_rn(a, c), __fmul_rn(b, s));
    hi = __fadd_rn(__fmul_rn(b, c), __fmul_rn(a, s));
}

// per: work items of one group -- h / 4 float4 pairs (kVec) or h pairs
template <bool kVec>
__global__ __launch_bounds__(256) void rope_rows_kernel(float *__restrict__ X, int64_t stride, int groups, int h,
                                                        const float *__restrict__ cos_t, const float *__restrict__ sin_t,
                                                        RopeTable tab) {
    const int r = blockIdx.x, b = blockIdx.z;
    if (r >= tab.n_rows[b]) return;
    const int per = kVec ? h >> 2 : h;
    const int item = blockIdx.y * 256 + threadIdx.x;
    if (item >= groups * per) return;
    const int g = item / per, i = item - g * per;
    float *lo = X + (tab.row0[b] + r) * stride + (int64_t)g * 2 * h;
    const int64_t t = ((int64_t)tab.pos0[b] + r) * h;
    if constexpr (kVec) {
        float4 *plo = reinterpret_cast<float4 *>(lo) + i, *phi = reinterpret_cast<float4 *>(lo + h) + i;
        const float4 c = reinterpret_cast<const float4 *>(cos_t + t)[i], s = reinterpret_cast<const float4 *>(sin_t + t)[i];
        float4 a = *plo, d = *phi;
        rotate(a.x, d.x, c.x, s.x);
        rotate(a.y, d.y, c.y, s.y);
        rotate(a.z, d.z, c.z, s.z);
        rotate(a.w, d.w, c.w, s.w);
        *plo = a;
        *phi = d;
    } else {
        float a = lo[i], d = lo[i + h];
        rotate(a, d, cos_t[t + i], sin_t[t + i]);
        lo[i] = a;
        lo[i + h] = d;
    }
}

bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what both entry points check before anything else
bool rope_args_ok(const float *X, int64_t stride, int groups, int dk, const float *cos_t, const float *sin_t,
                  int table_rows) {
    return X && cos_t && sin_t && dk >= 2 && !(dk & 1) && groups >= 1 && table_rows >= 1 &&
           (int64_t)groups * dk <= INT32_MAX && stride >= (int64_t)groups * dk;
}

hipError_t launch(float *X, int64_t stride, int groups, int dk, const float *cos_t, const float *sin_t, int n_seqs,
                  int max_rows, const RopeTable &tab, hipStream_t s) {
    const int h = dk / 2;
    const bool vec = dk % 8 == 0 && stride % 4 == 0 && al16(X) && al16(cos_t) && al16(sin_t);
    const int64_t items = (int64_t)groups * (vec ? h / 4 : h);
    const dim3 grid((unsigned)max_rows, (unsigned)((items + 255) / 256), (unsigned)n_seqs);
    if (grid.y > 65535) return hipErrorInvalidValue;
    if (vec)
        hipLaunchKernelGGL(rope_rows_kernel<true>, grid, dim3(256), 0, s, X, stride, groups, h, cos_t, sin_t, tab);
    else
        hipLaunchKernelGGL(rope_rows_kernel<false>, grid, dim3(256), 0, s, X, stride, groups, h, cos_t, sin_t, tab);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rope_rows(float *X, int64_t stride, int64_t rows, int groups, int dk, const float *cos_t,
                            const float *sin_t, int table_rows, int pos0, hipStream_t s) {
    if (!rope_args_ok(X, stride, groups, dk, cos_t, sin_t, table_rows) || rows < 0 || pos0 < 0 || pos0 >= table_rows ||
        rows > (int64_t)table_rows - pos0)
        return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    RopeTable tab = {};
    tab.n_rows[0] = (int)rows;
    tab.pos0[0] = pos0;
    return launch(X, stride, groups, dk, cos_t, sin_t, 1, (int)rows, tab, s);
}

hipError_t launch_rope_rows_varlen(float *X, int64_t stride, int groups, int dk, const float *cos_t, const float *sin_t,
                                   int table_rows, int n_seqs, const int64_t *row0, const int *n_rows, const int *pos0,
                                   hipStream_t s) {
    if (!rope_args_ok(X, stride, groups, dk, cos_t, sin_t, table_rows) || !row0 || !n_rows || !pos0 || n_seqs < 1 ||
        n_seqs > kVarlenMaxSeqs)
        return hipErrorInvalidValue;
    RopeTable tab = {};
    int max_rows = 0;
    for (int b = 0; b < n_seqs; ++b) {
        if (row0[b] < 0 || n_rows[b] < 0 || pos0[b] < 0 || pos0[b] >= table_rows || n_rows[b] > table_rows - pos0[b])
            return hipErrorInvalidValue;
        tab.row0[b] = row0[b], tab.n_rows[b] = n_rows[b], tab.pos0[b] = pos0[b];
        max_rows = n_rows[b] > max_rows ? n_rows[b] : max_rows;
    }
    if (max_rows == 0) return hipSuccess;
    return launch(X, stride, groups, dk, cos_t, sin_t, n_seqs, max_rows, tab, s);
}

}  // namespace qgemm
