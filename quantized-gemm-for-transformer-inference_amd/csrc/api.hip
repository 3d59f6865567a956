// api.hip -- the C-ABI of include/qgemm.h: argument checks, layout dispatch, workspace, stream order.
//
// op_quantized_mm (/root/reference/src/ops/op_mm.cuh:67-101) runs ten launches and allocates eight
// temporaries per call.  Here a call is two or three stream-ordered launches on caller memory plus a
// grow-only workspace cached per (device, stream):
//   pack A  (Cx + X_int8)          -- op_mm.cuh:76-77, 82-83, 86-87
//   pack B  (Cw + W_int8^T)        -- op_mm.cuh:78-79, 84-85, 88-89
//   MFMA GEMM + dequant epilogue   -- op_mm.cuh:92-99
#include <algorithm>
#include <map>
#include <mutex>
#include <thread>
#include <stdio.h>

#include "../../include/qgemm.h"
#include "qgemm_internal.h"

using namespace qgemm;

namespace {

constexpr float kDefaultRange = 127.0f;  // `range` at every reference call site (test_quantize.cu:76)

int err(hipError_t e) { return (int)e; }

bool dims_ok(int m, int n, int k) { return m >= 0 && n >= 0 && k >= 1; }

// Which packing pass serves a matrix whose reduction vectors are its rows (row_stride, elem_stride)?
//   elem_stride == 1       : the vectors are contiguous        -> pack_rows (vector path)
//   row_stride  == 1       : the vectors are columns of a row-major image -> pack_cols
//   anything else          : pack_rows generic (scalar, strided)
hipError_t pack_vectors(const float *src, int64_t row_stride, int64_t elem_stride, int rows, int len, float range,
                        PackedView out, hipStream_t stream) {
    if (elem_stride == 1) return launch_pack_rows(src, row_stride, 1, rows, len, range, out, stream);
    if (row_stride == 1 && len > 1) return launch_pack_cols(src, elem_stride, len, rows, range, out, stream);
    return launch_pack_rows(src, row_stride, elem_stride, rows, len, range, out, stream);
}

// A bf16 matrix (qgemm_pack_a_dt): contiguous rows take pack_rows' vector kernels where they are 16-B aligned, and
// every other layout -- columns of a row-major image included -- its generic strided kernel.
hipError_t pack_vectors(const bf16_t *src, int64_t row_stride, int64_t elem_stride, int rows, int len, float range,
                        PackedView out, hipStream_t stream) {
    return launch_pack_rows(src, row_stride, elem_stride, rows, len, range, out, stream);
}

bool dtype_ok(int t) { return t == QGEMM_F32 || t == QGEMM_BF16; }

// the same for a matrix given by pointer and dtype tag (dtype_ok)
hipError_t pack_vectors(const void *src, int dtype, int64_t row_stride, int64_t elem_stride, int rows, int len,
                        float range, PackedView out, hipStream_t stream) {
    return dtype == QGEMM_BF16
               ? pack_vectors(static_cast<const bf16_t *>(src), row_stride, elem_stride, rows, len, range, out, stream)
               : pack_vectors(static_cast<const float *>(src), row_stride, elem_stride, rows, len, range, out, stream);
}

// Grow-only cached buffers for the entry points without an explicit workspace, one per (device, stream, use): a
// buffer is only reused in its stream's order, so calls on different streams never share packed operands or split-K
// tickets (the reference allocates its temporaries per call, op_mm.cuh:76-93).  hipStreamPerThread names a different
// stream in every host thread, so it is keyed by the calling thread as well.  Growth waits for the owning stream only.
// At most kMaxCachedStreams buffers per (device, use): a process that cycles through many streams does not keep one
// workspace per stream it ever used -- the least recently used buffer is freed after a device synchronisation (its
// stream may no longer exist), which only happens when a new stream arrives.
enum CacheUse { kUseWorkspace = 0, kUseSplitK = 1, kUseErrorStats = 2 };  // never shared: split-K tickets stay zero
constexpr int kMaxCachedStreams = 8;
struct CacheKey {
    int dev;
    hipStream_t stream;
    std::thread::id thread;
    int use;
    bool operator<(const CacheKey &o) const {
        if (dev != o.dev) return dev < o.dev;
        if (stream != o.stream) return stream < o.stream;
        if (thread != o.thread) return thread < o.thread;
        return use < o.use;
    }
};
struct CachedBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    uint64_t last_use = 0;
};
std::mutex g_cache_mu;
std::map<CacheKey, CachedBuf> g_cache;
uint64_t g_cache_clock = 0;

// frees the least recently used buffer of (dev, use) other than `keep` once there are more than kMaxCachedStreams
hipError_t evict_cached(int dev, int use, const CacheKey &keep) {
    int n = 0;
    auto victim = g_cache.end();
    for (auto it = g_cache.begin(); it != g_cache.end(); ++it) {
        if (it->first.dev != dev || it->first.use != use) continue;
        ++n;
        if (!(it->first < keep) && !(keep < it->first)) continue;
        if (victim == g_cache.end() || it->second.last_use < victim->second.last_use) victim = it;
    }
    if (n <= kMaxCachedStreams || victim == g_cache.end()) return hipSuccess;
    hipError_t e = hipSuccess;
    if (victim->second.ptr) {
        if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
        e = hipFree(victim->second.ptr);
    }
    g_cache.erase(victim);
    return e;
}

// zero_new: the buffer is zeroed when (re)allocated (split-K tickets start at zero; the launches re-zero them)
hipError_t cached_buffer(size_t need, hipStream_t stream, int use, bool zero_new, size_t headroom, void **out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const std::thread::id th = stream == hipStreamPerThread ? std::this_thread::get_id() : std::thread::id();
    std::lock_guard<std::mutex> lk(g_cache_mu);
    const CacheKey key{dev, stream, th, use};
    const bool fresh = g_cache.find(key) == g_cache.end();
    CachedBuf &w = g_cache[key];
    w.last_use = ++g_cache_clock;
    if (fresh && (e = evict_cached(dev, use, key)) != hipSuccess) return e;
    if (w.bytes < need) {
        if (w.ptr) {
            // earlier calls on this stream may still be using it
            if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
            if ((e = hipFree(w.ptr)) != hipSuccess) return e;
            w.ptr = nullptr;
            w.bytes = 0;
        }
        const size_t grow = need + headroom;
        if ((e = hipMalloc(&w.ptr, grow)) != hipSuccess) return e;
        if (zero_new && (e = hipMemset(w.ptr, 0, grow)) != hipSuccess) return e;
        w.bytes = grow;
    }
    *out = w.ptr;
    return hipSuccess;
}

hipError_t cached_workspace(size_t need, hipStream_t stream, void **out) {
    return cached_buffer(need, stream, kUseWorkspace, false, need / 8 /* headroom for nearby shapes */, out);
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// One chain's workspace: [split-K scratch (0 unless the shape has too few tiles)][packed A][packed B], each part
// 256-B aligned.  The prepacked-weight chain (qgemm_linear) ends after packed A.
struct ChainWorkspace {
    size_t scratch_bytes;  // the split-K scratch, at offset 0 (its tickets first)
    size_t a, b;           // offsets of packed A and packed B
    size_t end;            // bytes with packed B; `b` bytes without
    ChainWorkspace(int m, int n, int k)
        : scratch_bytes(gemm_scratch_bytes(m, n, k)),
          a(align256(scratch_bytes)),
          b(a + align256(packed_bytes(m, k))),
          end(b + align256(packed_bytes(n, k))) {}
};

// Split-K scratch of qgemm_mm_packed and the error-statistics scratch (no workspace argument): zeroed at allocation.
hipError_t cached_scratch(size_t need, hipStream_t stream, int use, void **out) {
    return cached_buffer(need, stream, use, true, 0, out);
}

hipError_t mm_packed_impl(const void *packed_a, const void *packed_b, void *C, int64_t c_stride_h,
                          int64_t c_stride_w, int m, int n, int k, float range, void *scratch, size_t scratch_bytes,
                          hipStream_t stream, bool tickets_zeroed = false, bool c_bf16 = false) {
    const float inv_r2 = 1.0f / (range * range);  // op_mm.cuh:99, one rounding per operation (host IEEE)
    return launch_gemm_dequant(packed_view(packed_a, m, k), packed_view(packed_b, n, k), C, c_stride_h, c_stride_w, m,
                               n, inv_r2, scratch, scratch_bytes, stream, nullptr, false, tickets_zeroed, c_bf16);
}

}  // namespace

extern "C" {

size_t qgemm_packed_size(int rows, int k) {
    if (rows < 0 || k < 1) return 0;
    return packed_bytes(rows, k);
}

size_t op_mm_quantize_workspace_size(int m, int n, int k) {
    if (!dims_ok(m, n, k)) return 0;
    return ChainWorkspace(m, n, k).end;
}

int qgemm_pack_a(const float *A, int64_t a_stride_h, int64_t a_stride_w, int m, int k, float range, void *packed_a,
                 void *stream) {
    return qgemm_pack_a_dt(A, QGEMM_F32, a_stride_h, a_stride_w, m, k, range, packed_a, stream);
}

int qgemm_pack_b(const float *B, int64_t b_stride_h, int64_t b_stride_w, int k, int n, float range, void *packed_b,
                 void *stream) {
    if (!B || !packed_b || n < 0 || k < 1) return err(hipErrorInvalidValue);
    if (n == 0) return 0;
    // reduction vectors = columns of B: (vector stride, element stride) = (stride_w, stride_h)
    return err(pack_vectors(B, b_stride_w, b_stride_h, n, k, range, packed_view(packed_b, n, k),
                            static_cast<hipStream_t>(stream)));
}

int qgemm_mm_packed(const void *packed_a, const void *packed_b, float *C, int64_t c_stride_h, int64_t c_stride_w,
                    int m, int n, int k, float range, void *stream) {
    return qgemm_mm_packed_dt(packed_a, packed_b, C, QGEMM_F32, c_stride_h, c_stride_w, m, n, k, range, stream);
}

int qgemm_mm_packed_i32(const void *packed_a, const void *packed_b, int32_t *Acc, int m, int n, int k, void *stream) {
    if (!packed_a || !packed_b || !Acc || !dims_ok(m, n, k)) return err(hipErrorInvalidValue);
    if (m == 0 || n == 0) return 0;
    return err(launch_gemm_i32(packed_view(packed_a, m, k), packed_view(packed_b, n, k), Acc, m, n,
                               static_cast<hipStream_t>(stream)));
}

int op_mm_quantize_ws(const float *A, int64_t a_stride_h, int64_t a_stride_w, const float *B, int64_t b_stride_h,
                      int64_t b_stride_w, float *C, int64_t c_stride_h, int64_t c_stride_w, int m, int n, int k,
                      float range, void *workspace, size_t ws_bytes, void *stream) {
    // op_mm.cuh:71-72: shape agreement and device residency are asserted by the reference
    if (!A || !B || !C || !dims_ok(m, n, k)) return err(hipErrorInvalidValue);
    if (m == 0 || n == 0) return 0;
    const ChainWorkspace ws(m, n, k);
    if (!workspace || ws_bytes < ws.end) return err(hipErrorInvalidValue);
    char *scratch = static_cast<char *>(workspace);
    char *pa = scratch + ws.a, *pb = scratch + ws.b;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto gemm = [&](bool tickets_zeroed) {
        return err(mm_packed_impl(pa, pb, C, c_stride_h, c_stride_w, m, n, k, range, scratch, ws.scratch_bytes, s,
                                  tickets_zeroed));
    };
    // the pack launch zeroes the split-K tickets at the start of the workspace (the GEMM then needs no
    // zeroing launch of its own)
    uint32_t *tickets = reinterpret_cast<uint32_t *>(scratch);
    const int ntickets = (int)(gemm_ticket_bytes(m, n, k) / 4);
    // Common case (row-major X and W): X's row pass and W's column-absmax pass share one launch,
    // then W's quantize/transpose pass, then the GEMM -- three launches in all.
    if (a_stride_w == 1 && b_stride_w == 1 && k > 1) {
        const PackedView va = packed_view(pa, m, k), vb = packed_view(pb, n, k);
        // K <= 4096: W read once (single-pass strips) -- two launches in all
        hipError_t e = launch_pack_single_pass(A, a_stride_h, m, k, va, B, b_stride_h, n, vb, range, s, tickets, ntickets);
        if (e == hipSuccess) return gemm(true);
        if (e != hipErrorNotSupported) return err(e);
        e = launch_pack_two_pass(A, a_stride_h, m, k, va, B, b_stride_h, n, vb, range, s, tickets, ntickets);
        if (e == hipSuccess) return gemm(true);
        if (e != hipErrorNotSupported) return err(e);
    }
    int rc = qgemm_pack_a(A, a_stride_h, a_stride_w, m, k, range, pa, stream);
    if (rc) return rc;
    rc = qgemm_pack_b(B, b_stride_h, b_stride_w, k, n, range, pb, stream);
    if (rc) return rc;
    return gemm(false);
}

int op_mm_quantize_ex(const float *A, int64_t a_stride_h, int64_t a_stride_w, const float *B, int64_t b_stride_h,
                      int64_t b_stride_w, float *C, int64_t c_stride_h, int64_t c_stride_w, int m, int n, int k,
                      float range, void *stream) {
    if (!A || !B || !C || !dims_ok(m, n, k)) return err(hipErrorInvalidValue);
    if (m == 0 || n == 0) return 0;
    const size_t need = op_mm_quantize_workspace_size(m, n, k);
    void *ws = nullptr;
    hipError_t e = cached_workspace(need, static_cast<hipStream_t>(stream), &ws);
    if (e != hipSuccess) return err(e);
    return op_mm_quantize_ws(A, a_stride_h, a_stride_w, B, b_stride_h, b_stride_w, C, c_stride_h, c_stride_w, m, n, k,
                             range, ws, need, stream);
}

int op_mm_quantize(const float *A, const float *B, float *C, int m, int n, int k) {
    return op_mm_quantize_ex(A, k, 1, B, n, 1, C, n, 1, m, n, k, kDefaultRange, nullptr);
}

int qgemm_mm_fp32(const float *A, int64_t a_stride_h, int64_t a_stride_w, const float *B, int64_t b_stride_h,
                  int64_t b_stride_w, float *C, int64_t c_stride_h, int64_t c_stride_w, int m, int n, int k,
                  void *stream) {
    if (!A || !B || !C || !dims_ok(m, n, k)) return err(hipErrorInvalidValue);
    if (m == 0 || n == 0) return 0;
    return err(launch_mm_f32(A, a_stride_h, a_stride_w, B, b_stride_h, b_stride_w, C, c_stride_h, c_stride_w, m, n, k,
                             static_cast<hipStream_t>(stream)));
}

int qgemm_error_stats(const float *C, const float *O, int64_t count, int reference_order, double *stats,
                      void *stream) {
    if (!C || !O || !stats || count < 1) return err(hipErrorInvalidValue);
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *scratch = nullptr;
    hipError_t e = cached_scratch(error_stats_scratch_bytes(), s, kUseErrorStats, &scratch);
    if (e != hipSuccess) return err(e);
    return err(launch_error_stats(C, O, count, reference_order != 0, stats, scratch, s));
}

int qgemm_linear(const float *X, int64_t x_stride_h, int m, int k, const void *packed_w, int n, const float *bias,
                 int relu, float *Y, int64_t y_stride_h, void *workspace, size_t ws_bytes, void *stream) {
    return qgemm_linear_dt(X, QGEMM_F32, x_stride_h, m, k, packed_w, n, bias, relu, Y, QGEMM_F32, y_stride_h, workspace,
                           ws_bytes, stream);
}

// ---- bf16 activations and outputs: the same chain, only its two ends change (include/qgemm.h) ----

int qgemm_pack_a_dt(const void *A, int a_dtype, int64_t a_stride_h, int64_t a_stride_w, int m, int k, float range,
                    void *packed_a, void *stream) {
    if (!dtype_ok(a_dtype)) return err(hipErrorInvalidValue);
    if (!A || !packed_a || m < 0 || k < 1) return err(hipErrorInvalidValue);
    if (m == 0) return 0;
    // reduction vectors = rows of A: (row stride, element stride) = (stride_h, stride_w)
    return err(pack_vectors(A, a_dtype, a_stride_h, a_stride_w, m, k, range, packed_view(packed_a, m, k),
                            static_cast<hipStream_t>(stream)));
}

int qgemm_mm_packed_dt(const void *packed_a, const void *packed_b, void *C, int c_dtype, int64_t c_stride_h,
                       int64_t c_stride_w, int m, int n, int k, float range, void *stream) {
    if (!dtype_ok(c_dtype)) return err(hipErrorInvalidValue);
    if (!packed_a || !packed_b || !C || !dims_ok(m, n, k)) return err(hipErrorInvalidValue);
    if (m == 0 || n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *scratch = nullptr;
    const size_t sb = gemm_scratch_bytes(m, n, k);
    if (sb) {
        hipError_t e = cached_scratch(sb, s, kUseSplitK, &scratch);
        if (e != hipSuccess) return err(e);
    }
    return err(mm_packed_impl(packed_a, packed_b, C, c_stride_h, c_stride_w, m, n, k, range, scratch, sb, s,
                              /*tickets_zeroed=*/true, /*c_bf16=*/c_dtype == QGEMM_BF16));
}

int qgemm_linear_dt(const void *X, int x_dtype, int64_t x_stride_h, int m, int k, const void *packed_w, int n,
                    const float *bias, int relu, void *Y, int y_dtype, int64_t y_stride_h, void *workspace,
                    size_t ws_bytes, void *stream) {
    if (!dtype_ok(x_dtype) || !dtype_ok(y_dtype)) return err(hipErrorInvalidValue);
    if (!X || !packed_w || !Y || m < 0 || n < 0 || k < 1 || (relu && !bias)) return err(hipErrorInvalidValue);
    if (m == 0 || n == 0) return 0;
    const ChainWorkspace ws(m, n, k);
    if (!workspace || ws_bytes < ws.b) return err(hipErrorInvalidValue);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char *scratch = static_cast<char *>(workspace);
    const PackedView va = packed_view(scratch + ws.a, m, k);
    const hipError_t e = pack_vectors(X, x_dtype, x_stride_h, 1, m, k, kDefaultRange, va, s);
    if (e != hipSuccess) return err(e);
    const float inv_r2 = 1.0f / (kDefaultRange * kDefaultRange);
    return err(launch_gemm_dequant(va, packed_view(packed_w, n, k), Y, y_stride_h, 1, m, n, inv_r2, scratch,
                                   ws.scratch_bytes, s, bias, relu != 0, false, y_dtype == QGEMM_BF16));
}

size_t qgemm_linear_workspace_size(int m, int n, int k) {
    if (m < 0 || n < 0 || k < 1) return 0;
    return ChainWorkspace(m, n, k).b;
}

size_t op_mm_quantize_prepacked_workspace_size(int m, int n, int k) { return qgemm_linear_workspace_size(m, n, k); }

int op_mm_quantize_prepacked_ws(const float *A, int64_t a_stride_h, const void *packed_b, float *C, int64_t c_stride_h,
                                int m, int n, int k, void *workspace, size_t ws_bytes, void *stream) {
    // op_mm.cuh:71-72: shape agreement and device residency are asserted by the reference
    if (!A || !packed_b || !C || !dims_ok(m, n, k)) return err(hipErrorInvalidValue);
    return qgemm_linear(A, a_stride_h, m, k, packed_b, n, nullptr, 0, C, c_stride_h, workspace, ws_bytes, stream);
}

int op_mm_quantize_prepacked(const float *A, const void *packed_b, float *C, int m, int n, int k) {
    if (!A || !packed_b || !C || !dims_ok(m, n, k)) return err(hipErrorInvalidValue);
    if (m == 0 || n == 0) return 0;
    const size_t need = qgemm_linear_workspace_size(m, n, k);
    void *ws = nullptr;
    hipError_t e = cached_workspace(need, nullptr, &ws);
    if (e != hipSuccess) return err(e);
    return op_mm_quantize_prepacked_ws(A, k, packed_b, C, n, m, n, k, ws, need, nullptr);
}

int qgemm_softmax_rows(const float *S, float *P, int64_t rows, int w, float scale, void *stream) {
    if (!S || !P) return err(hipErrorInvalidValue);
    return err(launch_softmax_rows(S, P, rows, w, scale, static_cast<hipStream_t>(stream)));
}

int qgemm_softmax_rows_causal(const float *S, float *P, int64_t rows, int w, float scale, int seq_q, int q_pos0,
                              void *stream) {
    if (!S || !P) return err(hipErrorInvalidValue);
    return err(launch_softmax_rows_causal(S, P, rows, w, scale, seq_q, q_pos0, static_cast<hipStream_t>(stream)));
}

int qgemm_add_layernorm_rows(const float *A, const float *B, float *Y, int64_t rows, int w, void *stream) {
    if (!A || !B || !Y) return err(hipErrorInvalidValue);
    return err(launch_add_layernorm_rows(A, B, Y, rows, w, static_cast<hipStream_t>(stream)));
}

int qgemm_encoder_create_rows(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_rows,
                              uint64_t seed, void **encoder) {
    if (!encoder) return err(hipErrorInvalidValue);
    Stack *E = nullptr;
    hipError_t e = stack_create(d_model, n_heads, d_ff, n_blocks, max_seq, 0, seed, /*cross=*/false, false, false, &E, 1,
                                max_rows);
    *encoder = E;
    return err(e);
}

int qgemm_encoder_create(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, uint64_t seed,
                         void **encoder) {
    return qgemm_encoder_create_rows(d_model, n_heads, d_ff, n_blocks, max_seq, 0, seed, encoder);
}

int qgemm_encoder_forward_batch(void *encoder, const float *X, float *Y, int n_seqs, const int *seq_lens,
                                void *stream) {
    return err(encoder_forward_batch(static_cast<Stack *>(encoder), X, Y, n_seqs, seq_lens,
                                     static_cast<hipStream_t>(stream)));
}

int qgemm_encoder_forward(void *encoder, const float *X, float *Y, int seq, void *stream) {
    return err(encoder_forward(static_cast<Stack *>(encoder), X, Y, seq, static_cast<hipStream_t>(stream)));
}

int qgemm_encoder_destroy(void *encoder) {
    stack_destroy(static_cast<Stack *>(encoder));
    return 0;
}

// the fallback's scores, n_heads x seq_q x seq_kv floats; nothing inside the fused launch's envelope
size_t qgemm_attention_workspace_size(int seq_q, int seq_kv, int n_heads, int d_k) {
    if (seq_q < 0 || seq_kv < 1 || seq_kv > 4096 || n_heads < 1 || d_k < 1) return 0;
    if (attention_fused_ok(seq_kv, d_k)) return 0;
    return sizeof(float) * (size_t)n_heads * (size_t)seq_q * (size_t)seq_kv;
}

// qgemm_attention (q_pos0 = kNoMask) and qgemm_attention_causal: the same checks and the same workspace
static int attention_entry(const float *Q, int64_t q_stride_h, const float *K, int64_t k_stride_h, const float *V,
                           int64_t v_stride_h, float *O, int64_t o_stride_h, int seq_q, int seq_kv, int n_heads,
                           int d_k, float scale, int q_pos0, void *workspace, size_t ws_bytes, void *stream) {
    if (!Q || !K || !V || !O || seq_q < 0 || seq_kv < 1 || seq_kv > 4096 || n_heads < 1 || d_k < 1 || q_pos0 < kNoMask)
        return err(hipErrorInvalidValue);
    const size_t need = qgemm_attention_workspace_size(seq_q, seq_kv, n_heads, d_k);
    if (need && (!workspace || ws_bytes < need)) return err(hipErrorInvalidValue);
    if (seq_q == 0) return 0;
    return err(launch_attention(Q, q_stride_h, K, k_stride_h, V, v_stride_h, O, o_stride_h, seq_q, seq_kv, n_heads, d_k,
                                scale, q_pos0, need ? static_cast<float *>(workspace) : nullptr,
                                static_cast<hipStream_t>(stream)));
}

int qgemm_attention(const float *Q, int64_t q_stride_h, const float *K, int64_t k_stride_h, const float *V,
                    int64_t v_stride_h, float *O, int64_t o_stride_h, int seq_q, int seq_kv, int n_heads, int d_k,
                    float scale, void *workspace, size_t ws_bytes, void *stream) {
    return attention_entry(Q, q_stride_h, K, k_stride_h, V, v_stride_h, O, o_stride_h, seq_q, seq_kv, n_heads, d_k,
                           scale, kNoMask, workspace, ws_bytes, stream);
}

int qgemm_attention_causal(const float *Q, int64_t q_stride_h, const float *K, int64_t k_stride_h, const float *V,
                           int64_t v_stride_h, float *O, int64_t o_stride_h, int seq_q, int seq_kv, int n_heads,
                           int d_k, float scale, int q_pos0, void *workspace, size_t ws_bytes, void *stream) {
    if (q_pos0 < 0) return err(hipErrorInvalidValue);
    return attention_entry(Q, q_stride_h, K, k_stride_h, V, v_stride_h, O, o_stride_h, seq_q, seq_kv, n_heads, d_k,
                           scale, q_pos0, workspace, ws_bytes, stream);
}

// the largest single-call workspace over the sequences: 0 exactly when one table launch serves the call
size_t qgemm_attention_varlen_workspace_size(int n_seqs, const int *seq_q, const int *seq_kv, int n_heads, int d_k) {
    if (n_seqs < 0 || n_seqs > QGEMM_VARLEN_MAX_SEQS || !seq_q || !seq_kv) return 0;
    size_t need = 0;
    for (int b = 0; b < n_seqs; ++b)
        need = std::max(need, qgemm_attention_workspace_size(seq_q[b], seq_kv[b], n_heads, d_k));
    return need;
}

int qgemm_attention_varlen(const float *Q, int64_t q_stride_h, const float *K, int64_t k_stride_h, const float *V,
                           int64_t v_stride_h, float *O, int64_t o_stride_h, int n_seqs, const int64_t *q_row0,
                           const int *seq_q, const int64_t *kv_row0, const int *seq_kv, const int *q_pos0, int n_heads,
                           int d_k, float scale, void *workspace, size_t ws_bytes, void *stream) {
    static_assert(QGEMM_VARLEN_MAX_SEQS == kVarlenMaxSeqs, "the header's cap is the table's size");
    if (!Q || !K || !V || !O || !q_row0 || !seq_q || !kv_row0 || !seq_kv || n_seqs < 0 ||
        n_seqs > QGEMM_VARLEN_MAX_SEQS || n_heads < 1 || d_k < 1)
        return err(hipErrorInvalidValue);
    for (int b = 0; b < n_seqs; ++b)  // the sizes the workspace query reads, before it reads them
        if (seq_q[b] < 0 || seq_kv[b] < 1 || seq_kv[b] > 4096) return err(hipErrorInvalidValue);
    const size_t need = qgemm_attention_varlen_workspace_size(n_seqs, seq_q, seq_kv, n_heads, d_k);
    if (need && (!workspace || ws_bytes < need)) return err(hipErrorInvalidValue);
    return err(launch_attention_varlen(Q, q_stride_h, K, k_stride_h, V, v_stride_h, O, o_stride_h, n_seqs, q_row0, seq_q,
                                       kv_row0, seq_kv, q_pos0, n_heads, d_k, scale,
                                       need ? static_cast<float *>(workspace) : nullptr,
                                       static_cast<hipStream_t>(stream)));
}

int qgemm_attention_varlen_plan(int n_seqs, const int *seq_q, const int *seq_kv, int n_heads, int d_k,
                                const char **kernel) {
    if (n_seqs < 0 || n_seqs > QGEMM_VARLEN_MAX_SEQS || !seq_q || !seq_kv || n_heads < 1 || d_k < 1)
        return err(hipErrorInvalidValue);
    for (int b = 0; b < n_seqs; ++b)
        if (seq_q[b] < 0 || seq_kv[b] < 1 || seq_kv[b] > 4096) return err(hipErrorInvalidValue);
    if (kernel) *kernel = attention_varlen_plan_name(n_seqs, seq_kv, d_k);
    return 0;
}

int qgemm_decoder_create_ex(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq,
                            uint64_t seed, int flags, void **decoder) {
    if (!decoder) return err(hipErrorInvalidValue);
    *decoder = nullptr;
    if (flags & ~(QGEMM_DECODER_CAUSAL | QGEMM_DECODER_KV_CACHE)) return err(hipErrorInvalidValue);
    if ((flags & QGEMM_DECODER_KV_CACHE) && !(flags & QGEMM_DECODER_CAUSAL)) return err(hipErrorInvalidValue);
    Stack *D = nullptr;
    hipError_t e = stack_create(d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq, seed, /*cross=*/true,
                                (flags & QGEMM_DECODER_CAUSAL) != 0, (flags & QGEMM_DECODER_KV_CACHE) != 0, &D);
    *decoder = D;
    return err(e);
}

int qgemm_decoder_create(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq, uint64_t seed,
                         void **decoder) {
    return qgemm_decoder_create_ex(d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq, seed, 0, decoder);
}

int qgemm_decoder_forward(void *decoder, const float *X, const float *enc_out, float *Y, int seq, int enc_seq,
                          void *stream) {
    return err(decoder_forward(static_cast<Stack *>(decoder), X, enc_out, Y, seq, enc_seq,
                               static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_begin(void *decoder, const float *enc_out, int enc_seq, void *stream) {
    return qgemm_decoder_begin_slot(decoder, 0, enc_out, enc_seq, stream);
}

int qgemm_decoder_step(void *decoder, const float *X, float *Y, int pos, int n, void *stream) {
    return qgemm_decoder_step_slot(decoder, 0, X, Y, pos, n, stream);
}

int qgemm_attention_decode_batched(const float *Q, int64_t q_stride_h, const float *K, int64_t k_stride_h,
                                   int64_t k_stride_seq, const float *V, int64_t v_stride_h, int64_t v_stride_seq,
                                   float *O, int64_t o_stride_h, int n_seqs, int rows_per_seq, const int *kv_slot,
                                   const int *seq_kv, const int *q_pos0, int n_heads, int d_k, float scale,
                                   void *stream) {
    static_assert(QGEMM_DECODE_MAX_BATCH == kDecodeMaxBatch, "the header's cap is the table's size");
    return err(launch_attention_batched(Q, q_stride_h, K, k_stride_h, k_stride_seq, V, v_stride_h, v_stride_seq, O,
                                        o_stride_h, n_seqs, rows_per_seq, kv_slot, seq_kv, q_pos0, n_heads, d_k, scale,
                                        static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_create_rows(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq,
                              uint64_t seed, int flags, int n_slots, int max_rows, void **decoder) {
    if (!decoder) return err(hipErrorInvalidValue);
    *decoder = nullptr;
    if (flags != (QGEMM_DECODER_CAUSAL | QGEMM_DECODER_KV_CACHE) || n_slots < 1 || n_slots > QGEMM_DECODE_MAX_BATCH)
        return err(hipErrorInvalidValue);
    Stack *D = nullptr;
    hipError_t e = stack_create(d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq, seed, /*cross=*/true, true, true,
                                &D, n_slots, max_rows);
    *decoder = D;
    return err(e);
}

int qgemm_decoder_create_slots(int d_model, int n_heads, int d_ff, int n_blocks, int max_seq, int max_enc_seq,
                               uint64_t seed, int flags, int n_slots, void **decoder) {
    return qgemm_decoder_create_rows(d_model, n_heads, d_ff, n_blocks, max_seq, max_enc_seq, seed, flags, n_slots, 0,
                                     decoder);
}

int qgemm_decoder_step_varlen(void *decoder, int n_seqs, const int *slots, const int *pos, const int *n_rows,
                              const float *X, float *Y, void *stream) {
    return err(decoder_step_varlen(static_cast<Stack *>(decoder), n_seqs, slots, pos, n_rows, X, Y,
                                   static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_begin_slot(void *decoder, int slot, const float *enc_out, int enc_seq, void *stream) {
    return err(decoder_begin_slot(static_cast<Stack *>(decoder), slot, enc_out, enc_seq,
                                  static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_step_slot(void *decoder, int slot, const float *X, float *Y, int pos, int n, void *stream) {
    return err(decoder_step_slot(static_cast<Stack *>(decoder), slot, X, Y, pos, n, static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_step_batch(void *decoder, int n_seqs, const int *slots, const int *pos, int rows_per_seq,
                             const float *X, float *Y, void *stream) {
    return err(decoder_step_batch(static_cast<Stack *>(decoder), n_seqs, slots, pos, rows_per_seq, X, Y,
                                  static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_copy_slot(void *decoder, int dst_slot, int src_slot, void *stream) {
    return err(decoder_copy_slot(static_cast<Stack *>(decoder), dst_slot, src_slot, static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_gather_slots(void *decoder, int n_groups, int beams, const int *dst_slots, const int *src_slots,
                               const int32_t *parents, const int *n_rows, void *stream) {
    return err(decoder_gather_slots(static_cast<Stack *>(decoder), n_groups, beams, dst_slots, src_slots, parents, n_rows,
                                    static_cast<hipStream_t>(stream)));
}

int qgemm_attention_decode_indirect(const float *Q, int64_t q_stride_h, const float *K, int64_t k_stride_h,
                                    int64_t k_stride_seq, const float *V, int64_t v_stride_h, int64_t v_stride_seq,
                                    float *O, int64_t o_stride_h, int n_seqs, int rows_per_seq, const uint8_t *row_slab,
                                    int64_t row_slab_stride, int n_slabs, const int *tab_row, const int *seq_kv,
                                    const int *q_pos0, int n_heads, int d_k, float scale, void *stream) {
    return err(launch_attention_indirect(Q, q_stride_h, K, k_stride_h, k_stride_seq, V, v_stride_h, v_stride_seq, O,
                                         o_stride_h, n_seqs, rows_per_seq, row_slab, row_slab_stride, n_slabs, tab_row,
                                         seq_kv, q_pos0, n_heads, d_k, scale, static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_beam_begin(void *decoder, int n_groups, int beams, const int *slots, const int *src_slots,
                             const int *pos, void *stream) {
    return err(decoder_beam_begin(static_cast<Stack *>(decoder), n_groups, beams, slots, src_slots, pos,
                                  static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_step_batch_indirect(void *decoder, int n_seqs, const int *slots, const int *cross_slots,
                                      const int *pos, int rows_per_seq, const float *X, float *Y, void *stream) {
    return err(decoder_step_batch_indirect(static_cast<Stack *>(decoder), n_seqs, slots, cross_slots, pos, rows_per_seq,
                                           X, Y, static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_beam_reindex(void *decoder, int n_groups, int beams, const int *slots, const int32_t *parents,
                               const int *n_rows, void *stream) {
    return err(decoder_beam_reindex(static_cast<Stack *>(decoder), n_groups, beams, slots, parents, n_rows,
                                    static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_read_beam_table(void *decoder, uint8_t *out, void *stream) {
    return err(decoder_read_beam_table(static_cast<Stack *>(decoder), out, static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_read_slot(void *decoder, int block, int slot, float *self_rows, float *cross_rows, void *stream) {
    return err(decoder_read_slot(static_cast<Stack *>(decoder), block, slot, self_rows, cross_rows,
                                 static_cast<hipStream_t>(stream)));
}

int qgemm_decoder_slot_state(void *decoder, int slot, int *enc_seq, int *filled) {
    return err(decoder_slot_state(static_cast<Stack *>(decoder), slot, enc_seq, filled));
}

int qgemm_decoder_slot_begun(void *decoder, int slot, int *begun) {
    int enc_seq;
    if (!begun) return err(hipErrorInvalidValue);
    const hipError_t e = decoder_slot_state(static_cast<Stack *>(decoder), slot, &enc_seq, nullptr);
    if (e) return err(e);
    *begun = decoder_slot_begun(static_cast<Stack *>(decoder), slot) ? 1 : 0;
    return 0;
}

int qgemm_decoder_destroy(void *decoder) {
    stack_destroy(static_cast<Stack *>(decoder));
    return 0;
}

// ---- caller-supplied weights: every check sits with the launch it guards (weights.hip, transformer.hip)

int qgemm_pack_b_window(const void *B, int b_dtype, int64_t b_stride_h, int64_t b_stride_w, int k, int n_total, int col0,
                        int ncols, float range, void *packed_b, void *stream) {
    return err(launch_pack_b_window(B, b_dtype, b_stride_h, b_stride_w, k, n_total, col0, ncols, range, packed_b,
                                    static_cast<hipStream_t>(stream)));
}

int qgemm_pack_b_window_plan(const void *B, int b_dtype, int64_t b_stride_h, int64_t b_stride_w, int k, int n_total,
                             int col0, int ncols, const char **kernel) {
    if (!pack_b_window_ok(B, b_dtype, b_stride_h, b_stride_w, k, n_total, col0, ncols)) return (int)hipErrorInvalidValue;
    if (kernel) *kernel = pack_b_window_path(B, b_dtype, b_stride_h, b_stride_w, ncols);
    return 0;
}

int qgemm_model_weight_shape(void *model, int kind, int *rows, int *cols, int *heads) {
    return err(stack_weight_shape(static_cast<Stack *>(model), kind, rows, cols, heads));
}

int qgemm_model_set_weight(void *model, int block, int kind, int head, const void *W, int dtype, int64_t stride_h,
                           int64_t stride_w, void *stream) {
    return err(stack_set_weight(static_cast<Stack *>(model), block, kind, head, W, dtype, stride_h, stride_w,
                                static_cast<hipStream_t>(stream)));
}

int qgemm_model_packed_weight(void *model, int block, int which, const void **packed, int *n, int *k) {
    return err(stack_packed_weight(static_cast<Stack *>(model), block, which, packed, n, k));
}

int qgemm_model_bias(void *model, int block, int kind, const float **bias, int *n) {
    return err(stack_bias(static_cast<Stack *>(model), block, kind, bias, n));
}

int qgemm_model_rope_tables(void *model, const float **cos, const float **sin, int *rows, int *half) {
    return err(stack_rope_tables(static_cast<Stack *>(model), cos, sin, rows, half));
}

// ---- rotary position embeddings: every check sits with the launch it guards (rope.hip)

int qgemm_rope_rows(float *X, int64_t stride_h, int64_t rows, int groups, int d_k, const float *cos, const float *sin,
                    int table_rows, int pos0, void *stream) {
    return err(launch_rope_rows(X, stride_h, rows, groups, d_k, cos, sin, table_rows, pos0,
                                static_cast<hipStream_t>(stream)));
}

int qgemm_rope_rows_varlen(float *X, int64_t stride_h, int groups, int d_k, const float *cos, const float *sin,
                           int table_rows, int n_seqs, const int64_t *row0, const int *n_rows, const int *pos0,
                           void *stream) {
    return err(launch_rope_rows_varlen(X, stride_h, groups, d_k, cos, sin, table_rows, n_seqs, row0, n_rows, pos0,
                                       static_cast<hipStream_t>(stream)));
}

// ---- the standard block ----

int qgemm_layernorm_rows(const float *A, const float *B_or_null, const float *gamma, const float *beta, float eps,
                         float *Y, int64_t rows, int w, void *stream) {
    return err(launch_layernorm_rows(A, B_or_null, gamma, beta, eps, Y, rows, w, static_cast<hipStream_t>(stream)));
}

int qgemm_layernorm_pack_a(const float *A, const float *B_or_null, const float *gamma, const float *beta, float eps,
                           float *Y, int64_t rows, int w, float range, void *packed_a, void *stream) {
    if (!packed_a || rows < 0 || rows > INT32_MAX || w < 1 || w > 4096) return err(hipErrorInvalidValue);
    return err(launch_layernorm_rows_pack(A, B_or_null, gamma, beta, eps, Y, rows, w, range,
                                          packed_view(packed_a, (int)rows, w), static_cast<hipStream_t>(stream)));
}

int qgemm_prenorm_pack_a(const float *A, const float *B_or_null, const float *gamma, const float *beta, float eps,
                         float *S_or_null, int64_t rows, int w, float range, void *packed_a, void *stream) {
    if (!packed_a || rows < 0 || rows > INT32_MAX || w < 1 || w > 4096) return err(hipErrorInvalidValue);
    return err(launch_prenorm_pack(A, B_or_null, gamma, beta, eps, S_or_null, rows, w, range,
                                   packed_view(packed_a, (int)rows, w), static_cast<hipStream_t>(stream)));
}

int qgemm_add_rows(const float *A, const float *B, float *S, int64_t rows, int w, void *stream) {
    return err(launch_add_rows(A, B, S, rows, w, static_cast<hipStream_t>(stream)));
}

int qgemm_gelu_rows(const float *X, int64_t x_stride_h, float *Y, int64_t y_stride_h, int64_t rows, int w,
                    void *stream) {
    return err(launch_gelu_rows(X, x_stride_h, Y, y_stride_h, rows, w, static_cast<hipStream_t>(stream)));
}

int qgemm_gelu_pack_a(const float *X, int64_t x_stride_h, int m, int k, float range, void *packed_a, void *stream) {
    if (!packed_a || m < 0 || k < 1 || k > 16384) return err(hipErrorInvalidValue);
    return err(launch_gelu_pack(X, x_stride_h, m, k, range, packed_view(packed_a, m, k),
                                static_cast<hipStream_t>(stream)));
}

// ---- Llama-style blocks: the RMS norm and the gated FFN's pack ----

int qgemm_rmsnorm_rows(const float *A, const float *B_or_null, const float *gamma, float eps, float *Y, int64_t rows,
                       int w, void *stream) {
    return err(launch_rmsnorm_rows(A, B_or_null, gamma, eps, Y, rows, w, static_cast<hipStream_t>(stream)));
}

int qgemm_rmsnorm_pack_a(const float *A, const float *B_or_null, const float *gamma, float eps, float *Y, int64_t rows,
                         int w, float range, void *packed_a, void *stream) {
    if (!packed_a || rows < 0 || rows > INT32_MAX || w < 1 || w > 4096) return err(hipErrorInvalidValue);
    return err(launch_rmsnorm_rows_pack(A, B_or_null, gamma, eps, Y, rows, w, range, packed_view(packed_a, (int)rows, w),
                                        static_cast<hipStream_t>(stream)));
}

int qgemm_prenorm_rms_pack_a(const float *A, const float *B_or_null, const float *gamma, float eps, float *S_or_null,
                             int64_t rows, int w, float range, void *packed_a, void *stream) {
    if (!packed_a || rows < 0 || rows > INT32_MAX || w < 1 || w > 4096) return err(hipErrorInvalidValue);
    return err(launch_prenorm_rms_pack(A, B_or_null, gamma, eps, S_or_null, rows, w, range,
                                       packed_view(packed_a, (int)rows, w), static_cast<hipStream_t>(stream)));
}

int qgemm_glu_rows(const float *X, int64_t x_stride_h, float *Y, int64_t y_stride_h, int64_t rows, int w, int activation,
                   void *stream) {
    return err(launch_glu_rows(X, x_stride_h, Y, y_stride_h, rows, w, activation, static_cast<hipStream_t>(stream)));
}

int qgemm_glu_pack_a(const float *X, int64_t x_stride_h, int m, int k, int activation, float range, void *packed_a,
                     void *stream) {
    if (!packed_a || m < 0 || k < 1 || k > 16384) return err(hipErrorInvalidValue);
    return err(launch_glu_pack(X, x_stride_h, m, k, activation, range, packed_view(packed_a, m, k),
                               static_cast<hipStream_t>(stream)));
}

int qgemm_model_create(const qgemm_model_desc *desc, void **model) {
    if (!model) return err(hipErrorInvalidValue);
    *model = nullptr;
    if (!desc || desc->size != sizeof(qgemm_model_desc)) return err(hipErrorInvalidValue);
    const qgemm_model_desc &d = *desc;
    if ((d.cross != 0 && d.cross != 1) || !stack_arch_ok(d.arch, d.cross != 0) ||
        !stack_activation_ok(d.arch, d.activation, d.d_ff) || !(d.ln_eps >= 0.0f) || d.n_slots < 0 || d.max_rows < 0)
        return err(hipErrorInvalidValue);
    const int n_slots = d.n_slots ? d.n_slots : 1;
    bool causal = false, kv_cache = false;
    if (!d.cross) {  // qgemm_encoder_create_rows
        if (d.flags || n_slots != 1) return err(hipErrorInvalidValue);
    } else if (n_slots > 1 || d.max_rows > 0) {  // qgemm_decoder_create_rows
        if (d.flags != (QGEMM_DECODER_CAUSAL | QGEMM_DECODER_KV_CACHE) || n_slots > QGEMM_DECODE_MAX_BATCH)
            return err(hipErrorInvalidValue);
        causal = kv_cache = true;
    } else {  // qgemm_decoder_create_ex
        if (d.flags & ~(QGEMM_DECODER_CAUSAL | QGEMM_DECODER_KV_CACHE)) return err(hipErrorInvalidValue);
        if ((d.flags & QGEMM_DECODER_KV_CACHE) && !(d.flags & QGEMM_DECODER_CAUSAL)) return err(hipErrorInvalidValue);
        causal = (d.flags & QGEMM_DECODER_CAUSAL) != 0;
        kv_cache = (d.flags & QGEMM_DECODER_KV_CACHE) != 0;
    }
    Stack *S = nullptr;
    const hipError_t e = stack_create(d.d_model, d.n_heads, d.d_ff, d.n_blocks, d.max_seq, d.cross ? d.max_enc_seq : 0,
                                      d.seed, d.cross != 0, causal, kv_cache, &S, n_slots, d.max_rows, d.arch,
                                      d.activation, d.ln_eps);
    *model = S;
    return err(e);
}

int qgemm_model_info(void *model, qgemm_model_desc *desc) {
    StackDesc sd;
    if (!desc) return err(hipErrorInvalidValue);
    const hipError_t e = stack_describe(static_cast<Stack *>(model), &sd);
    if (e) return err(e);
    *desc = qgemm_model_desc{(uint32_t)sizeof(qgemm_model_desc), sd.cross, sd.d_model, sd.n_heads, sd.d_ff, sd.n_blocks,
                             sd.max_seq, sd.max_enc_seq, sd.seed, sd.flags, sd.n_slots, sd.max_rows, sd.arch,
                             sd.activation, sd.ln_eps};
    return 0;
}

size_t qgemm_mm_outlier_workspace_size(int m, int n, int k) {
    if (!dims_ok(m, n, k)) return 0;
    return align256(outlier_scratch_bytes(m, n, k)) + op_mm_quantize_workspace_size(m, n, k);
}

int qgemm_mm_outlier(const float *A, const float *B, float *C, int m, int n, int k, float threshold, void *workspace,
                     size_t ws_bytes, void *stream) {
    if (!A || !B || !C || !dims_ok(m, n, k) || !(threshold >= 0.0f)) return err(hipErrorInvalidValue);
    if (m == 0 || n == 0) return 0;
    const size_t need = qgemm_mm_outlier_workspace_size(m, n, k);
    if (!workspace || ws_bytes < need) return err(hipErrorInvalidValue);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char *scratch = static_cast<char *>(workspace);
    char *ws2 = scratch + align256(outlier_scratch_bytes(m, n, k));
    const ChainWorkspace ws(m, n, k);
    {
        // fast path: the packed operands in the plain chain's slots of ws2 (no split-K: no tickets)
        const hipError_t e = outlier_fast(A, B, C, m, n, k, threshold, scratch, packed_view(ws2 + ws.a, m, k),
                                          packed_view(ws2 + ws.b, n, k), kDefaultRange, s);
        if (e != hipErrorNotSupported) return err(e);
    }
    float *Xm = nullptr, *Wm = nullptr;
    hipError_t e = outlier_prepare(A, k, B, n, m, n, k, threshold, scratch, &Xm, &Wm, s);
    if (e != hipSuccess) return err(e);
    // the int8 part on the outlier-free operands (their scales no longer see the outliers)
    const int rc = op_mm_quantize_ws(Xm, k, 1, Wm, n, 1, C, n, 1, m, n, k, kDefaultRange, ws2, ws.end, stream);
    if (rc) return rc;
    return err(outlier_finish(A, k, B, n, nullptr, nullptr, false, m, n, k, scratch, C, n, s));
}

// [outlier scratch without the W' slot (count and column list first)][the prepacked chain's workspace]
size_t qgemm_linear_outlier_workspace_size(int m, int n, int k) {
    if (!dims_ok(m, n, k)) return 0;
    return align256(outlier_linear_scratch_bytes(m, k)) + ChainWorkspace(m, n, k).b;
}

int qgemm_linear_outlier(const float *X, int64_t x_stride_h, int m, int k, const void *packed_w, int n,
                         const float *bias, int relu, float threshold, float *Y, int64_t y_stride_h, void *workspace,
                         size_t ws_bytes, void *stream) {
    if (!X || !packed_w || !Y || !dims_ok(m, n, k) || !(threshold >= 0.0f) || (relu && !bias))
        return err(hipErrorInvalidValue);
    if (m == 0 || n == 0) return 0;
    if (!workspace || ws_bytes < qgemm_linear_outlier_workspace_size(m, n, k)) return err(hipErrorInvalidValue);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char *scratch = static_cast<char *>(workspace);
    char *ws2 = scratch + align256(outlier_linear_scratch_bytes(m, k));
    const ChainWorkspace ws(m, n, k);
    const PackedView va = packed_view(ws2 + ws.a, m, k), vb = packed_view(packed_w, n, k);
    {
        // fast path (no split-K: no tickets)
        const hipError_t e = outlier_linear_fast(X, x_stride_h, m, n, k, threshold, scratch, va, vb, bias, relu != 0, Y,
                                                 y_stride_h, s);
        if (e != hipErrorNotSupported) return err(e);
    }
    float *Xm = nullptr;
    hipError_t e = outlier_prepare(X, x_stride_h, nullptr, 0, m, n, k, threshold, scratch, &Xm, nullptr, s);
    if (e != hipSuccess) return err(e);
    // the int8 part on X' and the cached weight, without bias: the chain is added first
    if ((e = launch_pack_rows(Xm, k, 1, m, k, kDefaultRange, va, s)) != hipSuccess) return err(e);
    const float inv_r2 = 1.0f / (kDefaultRange * kDefaultRange);
    e = launch_gemm_dequant(va, vb, Y, y_stride_h, 1, m, n, inv_r2, ws2, ws.scratch_bytes, s);
    if (e != hipSuccess) return err(e);
    return err(outlier_finish(X, x_stride_h, nullptr, 0, &vb, bias, relu != 0, m, n, k, scratch, Y, y_stride_h, s));
}

int qgemm_outlier_count(int k, const void *workspace, int *count) {
    if (!workspace || !count || k < 1) return err(hipErrorInvalidValue);
    return outlier_count_slot(workspace, count);
}

int qgemm_set_gemm_events(void *start_event, void *stop_event) {
    set_gemm_events(static_cast<hipEvent_t>(start_event), static_cast<hipEvent_t>(stop_event));
    return 0;
}

int qgemm_set_event_mode(int mode) {
    if (mode != 0 && mode != 1) return err(hipErrorInvalidValue);
    set_gemm_event_mode(mode);
    return 0;
}

int qgemm_fill_uniform(float *dst, int64_t count, uint64_t seed, float lo, float hi, void *stream) {
    if (!dst || count < 0) return err(hipErrorInvalidValue);
    return err(launch_fill_uniform(dst, count, seed, lo, hi, static_cast<hipStream_t>(stream)));
}

int qgemm_gemm_plan(int m, int n, int k, int *tile, const char **kernel) {
    if (m < 1 || n < 1 || k < 1) return -(int)hipErrorInvalidValue;
    return gemm_plan_info(m, n, round_up(k, kKPad), tile, kernel);
}

int qgemm_mm_fp32_plan(int m, int n, int k, int batch, const void *A, int64_t a_stride_h, int64_t a_stride_w,
                       int64_t a_batch_stride, const void *B, int64_t b_stride_h, int64_t b_stride_w,
                       int64_t b_batch_stride, const char **kernel) {
    if (m < 1 || n < 1 || k < 1 || batch < 1) return (int)hipErrorInvalidValue;
    const MmF32Plan p = mm_f32_plan(m, n, k, batch, a_stride_h, a_stride_w, a_batch_stride, mm_f32_al16(A), b_stride_h,
                                    b_stride_w, b_batch_stride, mm_f32_al16(B));
    if (kernel) *kernel = p.name;
    return 0;
}

int qgemm_attention_plan(int seq_q, int seq_kv, int n_heads, int d_k, const char **kernel) {
    if (seq_q < 0 || seq_kv < 1 || seq_kv > 4096 || n_heads < 1 || d_k < 1) return (int)hipErrorInvalidValue;
    if (kernel) *kernel = attention_plan_name(seq_q, seq_kv, d_k);
    return 0;
}

#ifndef QGEMM_SRC_HASH
#define QGEMM_SRC_HASH "unknown"
#endif

// the same hash as a tagged literal in the file itself, so a build step can compare a binary with the tree
// without loading it (qgemm_amd.file_hash)
__attribute__((used)) static const char kSrcHashTag[] = "QGEMM_SRC_HASH=" QGEMM_SRC_HASH;

const char *qgemm_version(void) {
    static char buf[192];
    snprintf(buf, sizeof buf, "qgemm 0.1.0 gfx950 %s src=%s", gemm_config_name(), QGEMM_SRC_HASH);
    return buf;
}

}  // extern "C"
