// ref_driver -- runs the reference's own operators, compiled for gfx950, on recorded inputs.
//
// TEST INFRASTRUCTURE ONLY.  The product never links, loads or calls this program.  It includes the reference's
// headers by path (-I<reference>/src, after -Ioracle/ref/compat) and calls their functions; it holds no line of them.
// Built by `make -C oracle ref` into oracle/_ref/ref_driver (never committed); tests/ref_cases.py writes the case file
// and reads the result file.
//
//   ref_driver <cases.bin> <results.bin>
//
// Both files are little-endian data:
//   file   := u32 magic 'RPIN', u32 version (1), u32 ncases, case*
//   case   := u32 op, i32 p[12], f32 f[2], u32 ntensors, tensor*          (case file)
//           | u32 ntensors, tensor*                                       (result file)
//   tensor := u32 dtype (0 f32, 1 i8, 2 i32), u32 h, u32 w, h*w elements, row-major
// A view spec is five ints: flags (bit 0 transpose(), bit 1 slice()), then h0, h1, w0, w1 of the slice, taken after
// the transpose.  Every case runs in this one process.  Every output buffer holds the sentinel before the reference's
// operator runs; after every case the device is synchronised and the last error read, and on any error the program
// exits non-zero without running another case.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ops/op_mm.cuh"
#include "ops/op_reduction.cuh"
#include "ops/op_elemwise.cuh"
#include "ops/op_softmax.cuh"
#include "ops/op_layernorm.cuh"
#include "modules/attention.cuh"
#include "modules/linear.cuh"

#undef N  // op_elemwise.cuh leaves a macro of this name behind

unsigned long long randgen_seed = 1;  // declared extern by op_elemwise.cuh; nothing here draws random numbers

namespace {

constexpr uint32_t kMagic = 0x4e495052u;  // "RPIN"
constexpr uint32_t kSentinelF32 = 0x7fc0deadu;  // a quiet NaN no operator here produces
constexpr int kSentinelByte = 0x5a;

enum Op : uint32_t {
    OP_MM_F32 = 1, OP_QCHAIN = 2, OP_QMM = 3, OP_QMM_BIAS_RELU = 4, OP_SCALE_SOFTMAX = 5, OP_ADD_LAYERNORM = 6,
    OP_ATTENTION = 7, OP_LINEAR = 8, OP_EXP = 9, OP_POW2 = 10,
};

enum DType : uint32_t { F32 = 0, I8 = 1, I32 = 2 };

struct HostTensor {
    uint32_t dtype = F32, h = 0, w = 0;
    std::vector<unsigned char> bytes;
};

[[noreturn]] void die(const char *what, int code = 2)
{
    std::fprintf(stderr, "ref_driver: %s\n", what);
    std::exit(code);
}

void need(bool ok, const char *what)
{
    if (!ok) die(what);
}

size_t elem_size(uint32_t dtype)
{
    need(dtype <= I32, "unknown dtype");
    return dtype == I8 ? 1 : 4;
}

void read_exact(std::FILE *f, void *p, size_t n)
{
    if (n && std::fread(p, 1, n, f) != n) die("case file is truncated");
}

HostTensor read_tensor(std::FILE *f)
{
    HostTensor t;
    uint32_t hdr[3];
    read_exact(f, hdr, sizeof hdr);
    t.dtype = hdr[0], t.h = hdr[1], t.w = hdr[2];
    need(t.h >= 1 && t.w >= 1 && t.h <= (1u << 20) && t.w <= (1u << 20), "tensor shape out of range");
    t.bytes.resize((size_t)t.h * t.w * elem_size(t.dtype));
    read_exact(f, t.bytes.data(), t.bytes.size());
    return t;
}

void write_tensor(std::FILE *f, const HostTensor &t)
{
    uint32_t hdr[3] = {t.dtype, t.h, t.w};
    if (std::fwrite(hdr, 1, sizeof hdr, f) != sizeof hdr ||
        (t.bytes.size() && std::fwrite(t.bytes.data(), 1, t.bytes.size(), f) != t.bytes.size()))
        die("cannot write the result file");
}

template <typename T> constexpr uint32_t dtype_of();
template <> constexpr uint32_t dtype_of<float>() { return F32; }
template <> constexpr uint32_t dtype_of<int8_t>() { return I8; }
template <> constexpr uint32_t dtype_of<int>() { return I32; }

void hip_ok(hipError_t e, const char *what)
{
    if (e != hipSuccess) {
        std::fprintf(stderr, "ref_driver: %s: %s\n", what, hipGetErrorString(e));
        std::exit(3);
    }
}

// a device tensor of the reference's own type holding a host tensor
template <typename T> Tensor<T> upload(const HostTensor &h)
{
    need(h.dtype == dtype_of<T>(), "input tensor has the wrong dtype");
    Tensor<T> t{(int32_t)h.h, (int32_t)h.w, true};
    hip_ok(hipMemcpy(t.rawp, h.bytes.data(), h.bytes.size(), hipMemcpyHostToDevice), "upload");
    return t;
}

template <typename T> void upload_into(Tensor<T> &t, const HostTensor &h)
{
    need(h.dtype == dtype_of<T>() && (int)h.h == t.h && (int)h.w == t.w, "parameter tensor has the wrong shape");
    need(t.offset == 0 && t.stride_w == 1 && t.stride_h == t.w, "parameter tensor is not contiguous");
    hip_ok(hipMemcpy(t.rawp, h.bytes.data(), h.bytes.size(), hipMemcpyHostToDevice), "upload");
}

// a fresh contiguous device tensor, every element the sentinel
template <typename T> Tensor<T> sentinel(int h, int w)
{
    need(h >= 1 && w >= 1, "empty output");
    Tensor<T> t{h, w, true};
    size_t n = (size_t)h * w;
    if (dtype_of<T>() == F32) {
        std::vector<uint32_t> fill(n, kSentinelF32);
        hip_ok(hipMemcpy(t.rawp, fill.data(), n * 4, hipMemcpyHostToDevice), "sentinel fill");
    } else {
        hip_ok(hipMemset(t.rawp, kSentinelByte, n * sizeof(T)), "sentinel fill");
    }
    return t;
}

template <typename T> HostTensor download(const Tensor<T> &t)
{
    need(t.offset == 0 && t.stride_w == 1 && t.stride_h == t.w, "output tensor is not contiguous");
    HostTensor h;
    h.dtype = dtype_of<T>(), h.h = (uint32_t)t.h, h.w = (uint32_t)t.w;
    h.bytes.resize((size_t)t.h * t.w * sizeof(T));
    hip_ok(hipMemcpy(h.bytes.data(), t.rawp, h.bytes.size(), hipMemcpyDeviceToHost), "download");
    return h;
}

template <typename T> Tensor<T> view(const Tensor<T> &base, const int32_t *spec)
{
    Tensor<T> t = base;
    if (spec[0] & 1) t = t.transpose();
    if (spec[0] & 2) {
        need(0 <= spec[1] && spec[1] < spec[2] && spec[2] <= t.h && 0 <= spec[3] && spec[3] < spec[4] &&
                 spec[4] <= t.w, "slice outside its tensor");
        t = t.slice(spec[1], spec[2], spec[3], spec[4]);
    }
    return t;
}

// the driver's own two operations: the overloads softmax_kernel<float> and layernorm_kernel<float> call
__global__ void exp_table_kernel(const float *in, float *out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = exp(in[i]);
}

__global__ void pow2_table_kernel(const float *in, float *out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pow(in[i], 2);
}

struct Case {
    uint32_t op = 0;
    int32_t p[12] = {};
    float f[2] = {};
    std::vector<HostTensor> in;
};

void need_inputs(const Case &c, size_t n)
{
    need(c.in.size() == n, "wrong number of input tensors for the op");
}

std::vector<HostTensor> run_case(const Case &c)
{
    std::vector<HostTensor> out;
    switch (c.op) {
    case OP_MM_F32: {
        need_inputs(c, 2);
        Tensor<float> A = view(upload<float>(c.in[0]), c.p), B = view(upload<float>(c.in[1]), c.p + 5);
        need(A.w == B.h, "A.w != B.h");
        Tensor<float> C = sentinel<float>(A.h, B.w);
        op_mm(A, B, C);
        out.push_back(download(C));
        break;
    }
    case OP_QCHAIN: {  // the calls of op_quantized_mm one by one, every intermediate kept
        need_inputs(c, 2);
        Tensor<float> X = view(upload<float>(c.in[0]), c.p), W = view(upload<float>(c.in[1]), c.p + 5);
        need(X.w == W.h && W.h >= 2, "X.w != W.h, or K < 2 (the reference leaves Cw[1..] unwritten at K = 1)");
        float range = c.f[0], inv_r2 = c.f[1];
        Tensor<float> Cx = sentinel<float>(X.h, 1), Cw = sentinel<float>(1, W.w);
        op_absmax(X, Cx);
        op_absmax(W, Cw);
        Tensor<float> sx = sentinel<float>(X.h, 1), sw = sentinel<float>(1, W.w);
        op_inv_divide(Cx, range, sx);
        op_inv_divide(Cw, range, sw);
        Tensor<int8_t> Xq = sentinel<int8_t>(X.h, X.w), Wq = sentinel<int8_t>(W.h, W.w);
        op_multiply<float, int8_t>(X, sx, Xq);
        op_multiply<float, int8_t>(W, sw, Wq);
        Tensor<int> Acc = sentinel<int>(X.h, W.w);
        op_mm<int8_t, int>(Xq, Wq, Acc);
        Tensor<float> Outer = sentinel<float>(X.h, W.w);
        op_mm<float, float>(Cx, Cw, Outer);
        Tensor<float> Odq = sentinel<float>(X.h, W.w), O = sentinel<float>(X.h, W.w);
        op_dequantize(Acc, Outer, Odq);
        op_multiply(Odq, inv_r2, O);
        out.push_back(download(Cx));
        out.push_back(download(Cw));
        out.push_back(download(sx));
        out.push_back(download(sw));
        out.push_back(download(Xq));
        out.push_back(download(Wq));
        out.push_back(download(Acc));
        out.push_back(download(Outer));
        out.push_back(download(Odq));
        out.push_back(download(O));
        break;
    }
    case OP_QMM: {
        need_inputs(c, 2);
        Tensor<float> X = view(upload<float>(c.in[0]), c.p), W = view(upload<float>(c.in[1]), c.p + 5);
        need(X.w == W.h && W.h >= 2, "X.w != W.h, or K < 2");
        Tensor<float> O = sentinel<float>(X.h, W.w);
        op_quantized_mm(X, W, O, c.f[0]);
        out.push_back(download(O));
        break;
    }
    case OP_QMM_BIAS_RELU: {
        need_inputs(c, 3);
        Tensor<float> X = upload<float>(c.in[0]), W = upload<float>(c.in[1]), b = upload<float>(c.in[2]);
        need(X.w == W.h && W.h >= 2 && b.h == 1 && b.w == W.w, "shapes of X, W, b");
        Tensor<float> O = sentinel<float>(X.h, W.w), Y = sentinel<float>(X.h, W.w), R = sentinel<float>(X.h, W.w);
        op_quantized_mm(X, W, O, c.f[0]);
        op_add(O, b, Y);
        op_relu(Y, R);
        out.push_back(download(O));
        out.push_back(download(Y));
        out.push_back(download(R));
        break;
    }
    case OP_SCALE_SOFTMAX: {
        need_inputs(c, 1);
        Tensor<float> S = upload<float>(c.in[0]);
        Tensor<float> scaled = sentinel<float>(S.h, S.w), P = sentinel<float>(S.h, S.w);
        op_multiply(S, c.f[0], scaled);
        op_softmax(scaled, P);
        out.push_back(download(scaled));
        out.push_back(download(P));
        break;
    }
    case OP_ADD_LAYERNORM: {
        need_inputs(c, 2);
        Tensor<float> A = upload<float>(c.in[0]), B = upload<float>(c.in[1]);
        need(A.h == B.h && A.w == B.w, "A and B differ in shape");
        Tensor<float> sum = sentinel<float>(A.h, A.w), Y = sentinel<float>(A.h, A.w);
        op_add(A, B, sum);
        op_layernorm(sum, Y);
        out.push_back(download(sum));
        out.push_back(download(Y));
        break;
    }
    case OP_ATTENTION: {
        need_inputs(c, 4);
        int d_model = c.p[0], d_k = c.p[1], d_v = c.p[2];
        need(d_model >= 1 && d_k >= 1 && d_v >= 1, "attention dimensions");
        Tensor<float> X = upload<float>(c.in[0]);
        need(X.w == d_model, "X.w != d_model");
        AttentionLayer<float> layer(d_model, d_k, d_v, true);
        upload_into(layer.W_q.t, c.in[1]);
        upload_into(layer.W_k.t, c.in[2]);
        upload_into(layer.W_v.t, c.in[3]);
        Tensor<float> O = sentinel<float>(X.h, d_v);
        layer.forward(X, O);
        out.push_back(download(O));
        break;
    }
    case OP_LINEAR: {
        need_inputs(c, 3);
        Tensor<float> X = upload<float>(c.in[0]);
        int in_dim = (int)c.in[1].h, out_dim = (int)c.in[1].w;
        need(X.w == in_dim, "X.w != in_dim");
        LinearLayer<float> layer(in_dim, out_dim, true);
        std::vector<Parameter<float> *> params = layer.parameters();
        need(params.size() == 2, "LinearLayer::parameters()");
        upload_into(params[0]->t, c.in[1]);
        upload_into(params[1]->t, c.in[2]);
        Tensor<float> Y = sentinel<float>(X.h, out_dim);
        layer.forward(X, Y);
        out.push_back(download(Y));
        break;
    }
    case OP_EXP:
    case OP_POW2: {
        need_inputs(c, 1);
        Tensor<float> a = upload<float>(c.in[0]);
        Tensor<float> r = sentinel<float>(a.h, a.w);
        int n = a.h * a.w, blocks = (n + 255) / 256;
        if (c.op == OP_EXP)
            exp_table_kernel<<<blocks, 256>>>(a.rawp, r.rawp, n);
        else
            pow2_table_kernel<<<blocks, 256>>>(a.rawp, r.rawp, n);
        out.push_back(download(r));
        break;
    }
    default:
        die("unknown op");
    }
    return out;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) die("usage: ref_driver <cases.bin> <results.bin>");
    std::FILE *fin = std::fopen(argv[1], "rb");
    if (!fin) die("cannot open the case file");
    uint32_t hdr[3];
    read_exact(fin, hdr, sizeof hdr);
    need(hdr[0] == kMagic && hdr[1] == 1, "not a version-1 case file");
    uint32_t ncases = hdr[2];
    std::FILE *fout = std::fopen(argv[2], "wb");
    if (!fout) die("cannot open the result file");
    if (std::fwrite(hdr, 1, sizeof hdr, fout) != sizeof hdr) die("cannot write the result file");
    for (uint32_t i = 0; i < ncases; ++i) {
        Case c;
        uint32_t nin;
        read_exact(fin, &c.op, 4);
        read_exact(fin, c.p, sizeof c.p);
        read_exact(fin, c.f, sizeof c.f);
        read_exact(fin, &nin, 4);
        need(nin <= 8, "too many input tensors");
        for (uint32_t t = 0; t < nin; ++t) c.in.push_back(read_tensor(fin));
        std::vector<HostTensor> out = run_case(c);
        hipError_t sync = hipDeviceSynchronize(), last = hipGetLastError();
        if (sync != hipSuccess || last != hipSuccess) {
            std::fprintf(stderr, "ref_driver: case %u (op %u): %s\n", i, c.op,
                         hipGetErrorString(sync != hipSuccess ? sync : last));
            return 3;
        }
        uint32_t nout = (uint32_t)out.size();
        if (std::fwrite(&nout, 1, 4, fout) != 4) die("cannot write the result file");
        for (const HostTensor &t : out) write_tensor(fout, t);
    }
    if (std::fclose(fout) != 0) die("cannot write the result file");
    std::fclose(fin);
    return 0;
}
