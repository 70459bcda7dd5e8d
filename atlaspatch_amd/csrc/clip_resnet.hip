// Kernels of the OpenAI CLIP ResNet image towers (clip_resnet.cpp) that conv.hip and attn_pool.hip do not already have:
// the 2x2 average pool that carries every stride of the "modified" ResNet, and the token matrix of its attention-pool head.
// Activations are NHWC in the compute type T; both kernels are HBM-bound (every input element is read once, every output
// element written once, 16 bytes per access) and use no atomics: an image's result does not depend on the batch.
//
// avgpool2x2_nhwc: out[img][oy][ox][c] = T((x[2oy][2ox] + x[2oy][2ox+1]) + (x[2oy+1][2ox] + x[2oy+1][2ox+1])) / 4), f32 sums.
//   One thread per output pixel and 16-byte chunk of channels; no LDS.
// clip_attnpool_tokens: x T [n, hw, c] (the final map, already token-major), pos f32 [hw + 1, c] ->
//   tokens[img][0]     = T(mean_p x[img][p] + pos[0])          (the mean summed in f32; the same row packed into q_rows[img])
//   tokens[img][1 + p] = T(x[img][p] + pos[1 + p])
//   One workgroup per (image, 64 chunks of channels): 4 row groups x 64 chunk lanes.  Row group g streams rows g, g + 4, ..,
//   writes their token rows and keeps its column sums in registers; the four partial sums meet in LDS in a fixed order.
#include "kernel_util.h"

namespace ap {
namespace {

template <typename T>
__global__ __launch_bounds__(256) void avgpool2x2_kernel(const T* __restrict__ x, int n, int H, int W, int C, T* __restrict__ out) {
    constexpr int CH = 16 / sizeof(T);
    using V = typename Vec16<T>::type;
    const int chunks = C / CH, Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)n * Ho * Wo * chunks;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int cc = (int)(t % chunks);
        const size_t p = t / chunks;
        const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
        const size_t img = p / ((size_t)Wo * Ho);
        const T* s = x + ((img * H + 2 * oy) * W + 2 * ox) * C + (size_t)cc * CH;
        const V a = *(const V*)s, b = *(const V*)(s + C);
        const V c = *(const V*)(s + (size_t)W * C), d = *(const V*)(s + (size_t)W * C + C);
        V o;
#pragma unroll
        for (int e = 0; e < CH; ++e) o[e] = from_f32<T>((((float)a[e] + (float)b[e]) + ((float)c[e] + (float)d[e])) * 0.25f);
        *(V*)(out + p * C + (size_t)cc * CH) = o;
    }
}

constexpr int TOK_LANES = 64, TOK_GROUPS = 4;

template <typename T>
__global__ __launch_bounds__(TOK_LANES * TOK_GROUPS) void clip_attnpool_tokens_kernel(const T* __restrict__ x, const float* __restrict__ pos,
                                                                                        int hw, int C, T* __restrict__ tokens,
                                                                                        T* __restrict__ q_rows) {
    constexpr int CH = 16 / sizeof(T);
    using V = typename Vec16<T>::type;
    __shared__ float part[TOK_GROUPS][TOK_LANES][CH];
    const int lane = threadIdx.x & (TOK_LANES - 1), grp = threadIdx.x / TOK_LANES;
    const int chunk = blockIdx.x * TOK_LANES + lane;
    const bool live = chunk < C / CH;
    const size_t img = blockIdx.y;
    const int c0 = chunk * CH;
    float sum[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) sum[e] = 0.f;
    if (live) {
        const T* xi = x + img * hw * C + c0;
        T* ti = tokens + (img * (hw + 1) + 1) * C + c0;
        for (int p = grp; p < hw; p += TOK_GROUPS) {
            const V v = *(const V*)(xi + (size_t)p * C);
            const f32x4* pp = (const f32x4*)(pos + (size_t)(1 + p) * C + c0);
            V o;
#pragma unroll
            for (int q = 0; q < CH / 4; ++q) {
                const f32x4 pv = pp[q];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float f = (float)v[4 * q + e];
                    sum[4 * q + e] += f;
                    o[4 * q + e] = from_f32<T>(f + pv[e]);
                }
            }
            *(V*)(ti + (size_t)p * C) = o;
        }
    }
#pragma unroll
    for (int e = 0; e < CH; ++e) part[grp][lane][e] = sum[e];
    __syncthreads();
    if (grp == 0 && live) {
        V o;
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            const float s = (part[0][lane][e] + part[1][lane][e]) + (part[2][lane][e] + part[3][lane][e]);
            o[e] = from_f32<T>(s / (float)hw + pos[c0 + e]);
        }
        *(V*)(tokens + img * (hw + 1) * C + c0) = o;
        *(V*)(q_rows + img * C + c0) = o;
    }
}

}  // namespace

int launch_avgpool2x2_nhwc(int dtype, const void* x, int n, int h, int w, int c, void* out, hipStream_t stream) {
    AP_REQUIRE(x && out, "avgpool2x2_nhwc: null pointer");
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16 || dtype == AP_F32, "avgpool2x2_nhwc: dtype %d", dtype);
    AP_REQUIRE(n >= 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && c > 0 && c % 8 == 0,
               "avgpool2x2_nhwc: n %d h %d w %d c %d (h, w even, c %% 8 == 0)", n, h, w, c);
    AP_REQUIRE(aligned16(x, out), "avgpool2x2_nhwc: pointers must be 16-byte aligned");
    AP_REQUIRE(x != out, "avgpool2x2_nhwc: out must not alias x");
    if (n == 0) return AP_OK;
    const size_t work = (size_t)n * (h / 2) * (w / 2) * ((size_t)c * dtype_size(dtype) / 16);
    return dispatch_dtype("avgpool2x2_nhwc", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        avgpool2x2_kernel<T><<<grid_1d(work, 65536), 256, 0, stream>>>((const T*)x, n, h, w, c, (T*)out);
    });
}

int launch_clip_attnpool_tokens(int dtype, const void* x, const float* pos, int n, int hw, int c, void* tokens_out, void* q_rows_out,
                                hipStream_t stream) {
    AP_REQUIRE(x && pos && tokens_out && q_rows_out, "clip_attnpool_tokens: null pointer");
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16 || dtype == AP_F32, "clip_attnpool_tokens: dtype %d", dtype);
    AP_REQUIRE(n >= 0 && n <= 65535 && hw > 0 && hw <= 4096 && c > 0 && c % 8 == 0 && c <= 65536,
               "clip_attnpool_tokens: n %d hw %d c %d (n <= 65535, hw <= 4096, c %% 8 == 0, c <= 65536)", n, hw, c);
    AP_REQUIRE(aligned16(x, pos, tokens_out, q_rows_out), "clip_attnpool_tokens: pointers must be 16-byte aligned");
    if (n == 0) return AP_OK;
    const int chunks = (int)((size_t)c * dtype_size(dtype) / 16);
    dim3 grid((chunks + TOK_LANES - 1) / TOK_LANES, n), block(TOK_LANES * TOK_GROUPS);
    return dispatch_dtype("clip_attnpool_tokens", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        clip_attnpool_tokens_kernel<T><<<grid, block, 0, stream>>>((const T*)x, pos, hw, c, (T*)tokens_out, (T*)q_rows_out);
    });
}

}  // namespace ap

extern "C" {

int ap_avgpool2x2_nhwc(int dtype, const void* x, int n, int h, int w, int c, void* out, ap_stream_t stream) {
    return ap::launch_avgpool2x2_nhwc(dtype, x, n, h, w, c, out, (hipStream_t)stream);
}

int ap_clip_attnpool_tokens(int dtype, const void* x, const float* pos, int n, int hw, int c, void* tokens_out, void* q_rows_out,
                            ap_stream_t stream) {
    return ap::launch_clip_attnpool_tokens(dtype, x, pos, n, hw, c, tokens_out, q_rows_out, (hipStream_t)stream);
}

}  // extern "C"
