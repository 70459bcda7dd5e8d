// ConvNeXt kernels: the fused depthwise 7x7 convolution + bias + LayerNorm (+ affine) that opens every block, and a LayerNorm
// over rows of T for the stem and the downsampling layers.  Activations are NHWC in the compute type T (f16, bf16, f32); the
// pointwise layers (fc1 / fc2), the stem and the downsampling convolutions run in conv.hip's implicit GEMM (conv_gemm_ext).
//
// dwconv7_ln: one workgroup = one segment of XT pixels of one output row (XT = W rounded up to 4 on every layer of the four
// networks, so a workgroup owns a whole row) and ALL C channels of them.
//   phase 1: work item = (8-channel chunk, run of 4 adjacent output pixels).  For each of the 7 input rows the item reads the
//            10 input pixels its run touches (16-byte loads of 8 channels, taps outside the image skipped = zero padding)
//            and accumulates the 7 x 4 products in f32 (fmaf), tap order fixed.  + bias, rounded to T (what the conv's
//            output is in torch), into LDS [XT][C].
//   phase 2: a group of TPP lanes (a power of two inside one wave) per pixel: mean, then the sum of squared deviations, each
//            summed by every lane over its channel chunks in order and combined by an xor butterfly (the same bits on every
//            lane), in f32 from the T-rounded values; out = (y - mean) / sqrt(var + eps) * g + b, rounded to T, 16-byte stores.
// No reduction crosses workgroups and the segmenting depends on (W, C, T) only, so a pixel's bits do not depend on the batch.
// Weights are f32, tap-major [49][C] (dw_weight[(ky * 7 + kx) * C + c]); bias, LayerNorm gain and shift f32 [C].
//
// layernorm_rows: one wave per row of C (% 8) channels, the same two-pass f32 statistics, 16-byte loads and stores.
#include "kernel_util.h"

namespace ap {
namespace {

constexpr int DW_THREADS = 256;
constexpr int DW_RUN = 4;                      // output pixels per phase-1 work item
constexpr int DW_MAX_LDS = 64 * 1024;          // bytes of LDS a workgroup may stage (the four networks use <= 43 008)

struct DwArgs {
    const void* x;              // T [n, H, W, C]
    const float* w;             // f32 [49][C]
    const float* bias;          // f32 [C]
    const float* g;             // f32 [C]
    const float* b;             // f32 [C]
    void* out;                  // T [n, H, W, C]
    int H, W, C, XT, nseg, tpp;
    float eps;
};

template <typename T>
__global__ __launch_bounds__(DW_THREADS) void dwconv7_ln(DwArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dw_lds[];
    T* ys = (T*)dw_lds;                                    // [XT][C], the conv output rounded to T
    const int C = a.C, nch = C / 8;
    const int seg = blockIdx.x % a.nseg, row = blockIdx.x / a.nseg;
    const int oy = row % a.H, img = row / a.H;
    const int x0 = seg * a.XT, xe = min(a.W, x0 + a.XT), npx = xe - x0;
    const int nruns = (npx + DW_RUN - 1) / DW_RUN;
    const T* x = (const T*)a.x;

    // phase 1: depthwise 7x7 + bias -> LDS
    for (int item = threadIdx.x; item < nch * nruns; item += DW_THREADS) {
        const int c8 = item % nch, run = item / nch;
        const int px = x0 + run * DW_RUN;
        float acc[DW_RUN][8];
#pragma unroll
        for (int p = 0; p < DW_RUN; ++p)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[p][e] = 0.f;
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = oy + ky - 3;
            if (iy < 0 || iy >= a.H) continue;
            float wv[7][8];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) load8(a.w + (size_t)(ky * 7 + kx) * C + c8 * 8, wv[kx]);
            const T* xrow = x + ((size_t)img * a.H + iy) * a.W * C + c8 * 8;
#pragma unroll
            for (int j = 0; j < DW_RUN + 6; ++j) {
                const int ix = px - 3 + j;
                if (ix < 0 || ix >= a.W) continue;
                float v[8];
                load8(xrow + (size_t)ix * C, v);
#pragma unroll
                for (int p = 0; p < DW_RUN; ++p) {
                    const int kx = j - p;
                    if (kx < 0 || kx >= 7) continue;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[p][e] = fmaf(v[e], wv[kx][e], acc[p][e]);
                }
            }
        }
        float bv[8];
        load8(a.bias + c8 * 8, bv);
#pragma unroll
        for (int p = 0; p < DW_RUN; ++p) {
            if (px + p >= xe) break;
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = acc[p][e] + bv[e];
            store8(ys + (size_t)(px + p - x0) * C + c8 * 8, o);
        }
    }
    __syncthreads();

    // phase 2: LayerNorm of each pixel by a group of tpp lanes
    const int tpp = a.tpp, l = threadIdx.x & (tpp - 1);
    T* out = (T*)a.out;
    for (int q = threadIdx.x / tpp; q < npx; q += DW_THREADS / tpp) {
        const T* y = ys + (size_t)q * C;
        float s = 0.f;
        for (int k = l; k < nch; k += tpp) {
            float v[8];
            load8(y + k * 8, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[e];
        }
        for (int o = tpp >> 1; o >= 1; o >>= 1) s += __shfl_xor(s, o, tpp);
        const float mean = s / (float)C;
        float ss = 0.f;
        for (int k = l; k < nch; k += tpp) {
            float v[8];
            load8(y + k * 8, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[e] - mean; ss = fmaf(d, d, ss); }
        }
        for (int o = tpp >> 1; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, tpp);
        const float rstd = 1.0f / sqrtf(ss / (float)C + a.eps);
        T* dst = out + (((size_t)img * a.H + oy) * a.W + x0 + q) * C;
        for (int k = l; k < nch; k += tpp) {
            float v[8], gv[8], bv[8], o[8];
            load8(y + k * 8, v);
            load8(a.g + k * 8, gv);
            load8(a.b + k * 8, bv);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (v[e] - mean) * rstd * gv[e] + bv[e];
            store8(dst + k * 8, o);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void layernorm_rows(const T* x, int rows, int C, const float* g, const float* b, float eps,
                                                      T* out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                 // a whole wave
    const T* y = x + (size_t)r * C;
    wave_layernorm8([&](int k) { return y + k * 8; }, C / 8, C, g, b, eps, out + (size_t)r * C);
}

}  // namespace

int launch_dwconv7_ln_nhwc(int dtype, const void* x, int n, int h, int w, int c, const float* dw_weight, const float* dw_bias,
                           const float* ln_weight, const float* ln_bias, float eps, void* out, hipStream_t stream) {
    AP_REQUIRE(x && dw_weight && dw_bias && ln_weight && ln_bias && out, "dwconv7_ln_nhwc: null pointer");
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16 || dtype == AP_F32, "dwconv7_ln_nhwc: dtype %d", dtype);
    AP_REQUIRE(n >= 0 && h > 0 && w > 0 && c > 0 && c % 8 == 0, "dwconv7_ln_nhwc: n %d h %d w %d c %d (c %% 8 == 0)", n, h, w, c);
    AP_REQUIRE(eps > 0.f, "dwconv7_ln_nhwc: eps %g", (double)eps);
    AP_REQUIRE(aligned16(x, dw_weight, dw_bias, ln_weight, ln_bias, out), "dwconv7_ln_nhwc: pointers must be 16-byte aligned");
    AP_REQUIRE(x != out, "dwconv7_ln_nhwc: in place is not supported (a workgroup reads the rows of its neighbours)");
    const size_t row_bytes = (size_t)c * dtype_size(dtype);
    AP_REQUIRE(DW_RUN * row_bytes <= DW_MAX_LDS, "dwconv7_ln_nhwc: c %d too wide", c);
    if (n == 0) return AP_OK;
    int xt = (int)align_up((size_t)w, DW_RUN);
    while ((size_t)xt * row_bytes > DW_MAX_LDS) xt -= DW_RUN;
    const int nseg = (w + xt - 1) / xt;
    int tpp = 64;
    while (tpp > 1 && tpp * xt > DW_THREADS) tpp >>= 1;
    const size_t blocks = (size_t)n * h * nseg;
    AP_REQUIRE(blocks < (size_t)1 << 31, "dwconv7_ln_nhwc: grid too large");
    DwArgs a{x, dw_weight, dw_bias, ln_weight, ln_bias, out, h, w, c, xt, nseg, tpp, eps};
    const size_t lds = (size_t)xt * row_bytes;
    return dispatch_dtype("dwconv7_ln_nhwc", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        dwconv7_ln<T><<<(unsigned)blocks, DW_THREADS, lds, stream>>>(a);
    });
}

int launch_layernorm_rows(int dtype, const void* x, int rows, int c, const float* weight, const float* bias, float eps, void* out,
                          hipStream_t stream) {
    AP_REQUIRE(x && weight && bias && out, "layernorm_rows: null pointer");
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16 || dtype == AP_F32, "layernorm_rows: dtype %d", dtype);
    AP_REQUIRE(rows >= 0 && c > 0 && c % 8 == 0, "layernorm_rows: rows %d c %d (c %% 8 == 0)", rows, c);
    AP_REQUIRE(eps > 0.f, "layernorm_rows: eps %g", (double)eps);
    AP_REQUIRE(aligned16(x, weight, bias, out), "layernorm_rows: pointers must be 16-byte aligned");
    if (rows == 0) return AP_OK;
    // four rows per workgroup, the row index blockIdx.x * 4 + wave in int: rows + 3 must not overflow
    AP_REQUIRE(rows <= 0x7FFFFFFF - 3, "layernorm_rows: rows %d too many (at most 2^31 - 4)", rows);
    const unsigned blocks = (unsigned)((rows + 3) / 4);
    return dispatch_dtype("layernorm_rows", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        layernorm_rows<T><<<blocks, 256, 0, stream>>>((const T*)x, rows, c, weight, bias, eps, (T*)out);
    });
}

}  // namespace ap

extern "C" {

int ap_dwconv7_ln_nhwc(int dtype, const void* x, int n, int h, int w, int c, const float* dw_weight, const float* dw_bias,
                       const float* ln_weight, const float* ln_bias, float eps, void* out, ap_stream_t stream) {
    return ap::launch_dwconv7_ln_nhwc(dtype, x, n, h, w, c, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, (hipStream_t)stream);
}

int ap_layernorm_rows(int dtype, const void* x, int rows, int c, const float* weight, const float* bias, float eps, void* out,
                      ap_stream_t stream) {
    return ap::launch_layernorm_rows(dtype, x, rows, c, weight, bias, eps, out, (hipStream_t)stream);
}

}  // extern "C"
