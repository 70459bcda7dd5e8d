// Convolutional encoder kernels (ResNet family): implicit-GEMM convolution with a fused BatchNorm / residual / ReLU epilogue,
// the NHWC preprocess of the stem, max pool 3x3 s2 p1 and the global average pool.  Activations are NHWC in the compute type T.
//
// Implicit GEMM: out[m][co] = sum_k A[m][k] W[co][k] with m = (image, oy, ox) -- one output pixel per row, M = n Ho Wo --
// and k = (ky, kx, c) -- K = kh kw Cin, so that a run of channels of ONE input pixel is contiguous in k.  A is never
// materialised: the tile loader gathers A[m][k0 .. k0 + 8) (16 bytes) straight from the input pixel (oy s - p + ky,
// ox s - p + kx), and a tap outside the image reads as zero (the zero padding of the conv's input).  Cin % 8 == 0 (16-bit
// types: one chunk = 8 channels; f32: two chunks of 4) keeps every chunk inside one pixel; the stem's 3 channels are padded
// to 8 by its preprocess, with zero weights behind the padding.  W is [Cout][K] (the host permutes torch's [Cout][Cin][ky][kx]).
//
// Tile: 128 pixel rows x 64 output channels x 128 bytes of K (64 f16 / bf16, 32 f32) per step, 256 threads = 4 waves in
// 2 x 2, each wave a 64 x 32 block = two 32 x 32 MFMA accumulators (v_mfma_f32_32x32x16_{f16,bf16}; float32:
// v_mfma_f32_32x32x2_f32, exact f32 products).  Global -> registers -> LDS, with the next K step's loads issued before the
// current step's MFMAs.  Cout % 64 == 0 covers every layer of the five networks (64 .. 2048) with one tile; the M tail
// (7 x 7 x n rows in the last stage) is masked row by row.  Epilogue: + bias (BatchNorm folded on the host, f32), + residual
// (T, the output's shape), ReLU, store T.
//
// conv_implicit_gemm<T, EXT = true> is the ConvNeXt instantiation (ap_conv2d_nhwc_ex): Cout % 32 == 0, the last N tile's
// upper 32 columns masked (no weight row read, no store), and a GELU (erf) epilogue beside ReLU.  EXT = false is the ResNet
// kernel behind ap_conv2d_nhwc; its instruction stream is the one it had before EXT existed.
#include "kernel_util.h"

namespace ap {
namespace {

constexpr int CBM = 128, CBN = 64, CTHREADS = 256;
constexpr int KBYTES = 128;                 // K bytes per step and row
constexpr int LDS_ROW = KBYTES + 16;        // 144-byte rows: the 32 rows of a fragment read hit 64 distinct banks per 16 lanes

struct ConvArgs {
    const void* x;          // T [n, H, W, Cin]
    const void* w;          // T [Cout, K], K = k * k * Cin ordered (ky, kx, c)
    const float* bias;      // f32 [Cout]
    const void* resid;      // T [M, Cout] or null
    void* out;              // T [M, Cout]
    int H, W, Cin, Ho, Wo, Cout, ks, stride, pad, K, M;
    int act;                // EXT = false: ReLU if nonzero; EXT = true: ACT_NONE / ACT_RELU / ACT_GELU
};

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2 };

// Mma32x32 on fragments read at LDS byte addresses
template <typename T> __device__ __forceinline__ f32x16 mma_at(const char* a, const char* b, f32x16 c) {
    return Mma32x32<T>::run(*(const typename Mma32x32<T>::Frag*)a, *(const typename Mma32x32<T>::Frag*)b, c);
}

template <typename T> __device__ __forceinline__ float to_f32(T v) { return (float)v; }

template <typename T, bool EXT>
__global__ __launch_bounds__(CTHREADS) void conv_implicit_gemm(ConvArgs a) {
    constexpr int CH = 16 / sizeof(T);                 // elements per 16-byte chunk
    constexpr int KT = KBYTES / sizeof(T);             // K elements per step
    constexpr int KSTEP = Mma32x32<T>::K;
    __shared__ __attribute__((aligned(16))) char As[CBM * LDS_ROW];
    __shared__ __attribute__((aligned(16))) char Bs[CBN * LDS_ROW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntiles = EXT ? (a.Cout + CBN - 1) / CBN : a.Cout / CBN;
    const int mt = blockIdx.x / ntiles, nt = blockIdx.x - mt * ntiles;
    const int m0 = mt * CBM, n0 = nt * CBN;

    // this thread's loads: chunk kc of rows r0 + 32 i (A, i < 4) and r0 + 32 i (B, i < 2)
    const int kc = tid & 7, r0 = tid >> 3;
    int pix_img[4], pix_iy[4], pix_ix[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + r0 + 32 * i;
        if (m < a.M) {
            const int hw = a.Ho * a.Wo;
            const int img = m / hw, rem = m - img * hw;
            const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
            pix_img[i] = img;
            pix_iy[i] = oy * a.stride - a.pad;
            pix_ix[i] = ox * a.stride - a.pad;
        } else {
            pix_img[i] = -1; pix_iy[i] = 0; pix_ix[i] = 0;
        }
    }
    const T* x = (const T*)a.x;
    const T* w = (const T*)a.w;

    u32x4 ra[4], rb[2];
    auto load = [&](int k0) {
        const int k = k0 + kc * CH;
        const bool kin = k < a.K;
        const int tap = kin ? k / a.Cin : 0;
        const int c = k - tap * a.Cin;
        const int ky = tap / a.ks, kx = tap - ky * a.ks;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int iy = pix_iy[i] + ky, ix = pix_ix[i] + kx;
            const bool ok = kin && pix_img[i] >= 0 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) v = *(const u32x4*)(x + (((size_t)pix_img[i] * a.H + iy) * a.W + ix) * a.Cin + c);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if constexpr (EXT) {                       // the 32-wide tail: rows past Cout read as zeros
                if (kin && n0 + r0 + 32 * i < a.Cout) v = *(const u32x4*)(w + (size_t)(n0 + r0 + 32 * i) * a.K + k);
            } else {
                if (kin) v = *(const u32x4*)(w + (size_t)(n0 + r0 + 32 * i) * a.K + k);
            }
            rb[i] = v;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) *(u32x4*)(As + (r0 + 32 * i) * LDS_ROW + kc * 16) = ra[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *(u32x4*)(Bs + (r0 + 32 * i) * LDS_ROW + kc * 16) = rb[i];
    };

    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

    // fragment addresses: 16-bit types, lane holds k = 8 fh .. 8 fh + 7 of its row; f32, k = fh
    const int koff = (sizeof(T) == 2 ? 8 * fh : fh) * (int)sizeof(T);
    const char* pa0 = As + (wm * 64 + fr) * LDS_ROW + koff;
    const char* pa1 = pa0 + 32 * LDS_ROW;
    const char* pb = Bs + (wn * 32 + fr) * LDS_ROW + koff;

    load(0);
    for (int k0 = 0; k0 < a.K; k0 += KT) {
        __syncthreads();                               // the previous step's fragment reads are done
        stash();
        __syncthreads();
        if (k0 + KT < a.K) load(k0 + KT);              // in flight during this step's MFMAs
#pragma unroll
        for (int s = 0; s < KT / KSTEP; ++s) {
            const int off = s * KSTEP * (int)sizeof(T);
            acc[0] = mma_at<T>(pa0 + off, pb + off, acc[0]);
            acc[1] = mma_at<T>(pa1 + off, pb + off, acc[1]);
        }
    }

    // epilogue: C/D map col = lane & 31, row = (j & 3) + 8 (j >> 2) + 4 (lane >> 5)
    const int n = n0 + wn * 32 + fr;
    if constexpr (EXT) {
        if (n >= a.Cout) return;                       // a whole wave: the upper half of the 32-wide tail tile
    }
    const float b = a.bias[n];
    const T* resid = (const T*)a.resid;
    T* out = (T*)a.out;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int m = m0 + wm * 64 + i * 32 + (j & 3) + 8 * (j >> 2) + 4 * fh;
            if (m >= a.M) continue;
            const size_t o = (size_t)m * a.Cout + n;
            float v = acc[i][j] + b;
            if (resid) v += to_f32(resid[o]);
            if constexpr (EXT) {
                if (a.act == ACT_RELU) v = v > 0.f ? v : 0.f;
                else if (a.act == ACT_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
            } else {
                if (a.act) v = v > 0.f ? v : 0.f;
            }
            out[o] = from_f32<T>(v);
        }
}

// u8 HWC tiles -> centre crop -> normalised NHWC with channels padded to 8 (zeros): the stem's input.  The values are the
// preprocess LUT's (the same ((x / 255) - mean) / std, two true divisions, as every other preprocess of this library).
template <typename T>
__global__ __launch_bounds__(256) void preproc_nhwc8(const uint8_t* src, int n, int h, int w, int top, int left, int S,
                                                     const T* lut, T* dst) {
    const size_t total = (size_t)n * S * S;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (size_t)gridDim.x * 256) {
        const int img = (int)(p / ((size_t)S * S));
        const int rem = (int)(p - (size_t)img * S * S);
        const int y = rem / S, xx = rem - y * S;
        const uint8_t* px = src + (((size_t)img * h + top + y) * w + left + xx) * 3;
        T v[8];
        v[0] = lut[px[0]];
        v[1] = lut[256 + px[1]];
        v[2] = lut[512 + px[2]];
#pragma unroll
        for (int c = 3; c < 8; ++c) v[c] = from_f32<T>(0.f);
        T* d = dst + p * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c) d[c] = v[c];
    }
}

// max pool 3x3, stride 2, padding 1: taps outside the image are skipped (not counted as 0).  One thread per output pixel and
// 16-byte chunk of channels.
template <typename T>
__global__ __launch_bounds__(256) void maxpool3x3s2(const T* x, int n, int H, int W, int C, int Ho, int Wo, T* out) {
    constexpr int CH = 16 / sizeof(T);
    const int chunks = C / CH;
    const size_t total = (size_t)n * Ho * Wo * chunks;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int cc = (int)(t % chunks);
        const size_t p = t / chunks;
        const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), img = (int)(p / ((size_t)Wo * Ho));
        float m[CH];
#pragma unroll
        for (int e = 0; e < CH; ++e) m[e] = -__builtin_inff();
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = oy * 2 - 1 + dy;
            if (iy < 0 || iy >= H) continue;
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = ox * 2 - 1 + dx;
                if (ix < 0 || ix >= W) continue;
                const T* s = x + (((size_t)img * H + iy) * W + ix) * C + cc * CH;
#pragma unroll
                for (int e = 0; e < CH; ++e) m[e] = fmaxf(m[e], to_f32(s[e]));
            }
        }
        T* d = out + p * C + cc * CH;
#pragma unroll
        for (int e = 0; e < CH; ++e) d[e] = from_f32<T>(m[e]);
    }
}

// global average pool: out f32 [n, C] = (sum over the HW pixels, f32, in pixel order) / HW
template <typename T>
__global__ __launch_bounds__(256) void avgpool_nhwc(const T* x, int n, int HW, int C, float* out) {
    const size_t total = (size_t)n * C;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int c = (int)(t % C);
        const size_t img = t / C;
        const T* s = x + img * HW * C + c;
        float sum = 0.f;
        for (int p = 0; p < HW; ++p) sum += to_f32(s[(size_t)p * C]);
        out[t] = sum / (float)HW;
    }
}

// The implicit GEMM's launcher.  EXT = false: ap_conv2d_nhwc (ResNet; Cout % 64, act = ReLU flag); EXT = true: ap_conv2d_nhwc_ex
// (ConvNeXt; Cout % 32 through the masked N tail, act 0 none / 1 ReLU / 2 GELU).
template <bool EXT>
int launch_conv2d(int dtype, const void* x, int n, int h, int w, int cin, const void* weight, const float* bias, int cout, int ksize,
                  int stride, int pad, const void* resid, int act, void* out, hipStream_t stream) {
    const char* who = EXT ? "conv2d_nhwc_ex" : "conv2d_nhwc";
    const int cout_step = EXT ? 32 : CBN;
    AP_REQUIRE(x && weight && bias && out, "%s: null pointer", who);
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16 || dtype == AP_F32, "%s: dtype %d", who, dtype);
    AP_REQUIRE(n >= 0 && h > 0 && w > 0, "%s: shape n %d h %d w %d", who, n, h, w);
    AP_REQUIRE(cin > 0 && cin % 8 == 0, "%s: Cin %d must be a multiple of 8 (pad the channels with zeros)", who, cin);
    AP_REQUIRE(cout > 0 && cout % cout_step == 0, "%s: Cout %d must be a multiple of %d", who, cout, cout_step);
    AP_REQUIRE(ksize >= 1 && ksize <= 7 && stride >= 1 && stride <= 4 && pad >= 0 && pad < ksize,
               "%s: kernel %d stride %d pad %d", who, ksize, stride, pad);
    AP_REQUIRE(h + 2 * pad >= ksize && w + 2 * pad >= ksize, "%s: %dx%d input smaller than the %d kernel", who, h, w, ksize);
    AP_REQUIRE(aligned16(x, weight, out, resid), "%s: pointers must be 16-byte aligned", who);
    if (EXT) {
        AP_REQUIRE(act == ACT_NONE || act == ACT_RELU || act == ACT_GELU, "%s: activation %d (0 none, 1 ReLU, 2 GELU)", who, act);
    } else {
        act = act ? ACT_RELU : ACT_NONE;
    }
    const int ho = (h + 2 * pad - ksize) / stride + 1, wo = (w + 2 * pad - ksize) / stride + 1;
    const size_t M = (size_t)n * ho * wo;
    // the kernel forms its row indices m0 + r (r < CBM) in int: the last tile's must stay below 2^31
    AP_REQUIRE(M <= ((size_t)1 << 31) - CBM && (size_t)ksize * ksize * cin < (size_t)1 << 24,
               "%s: problem too large (n * Ho * Wo = %zu rows, at most 2^31 - %d)", who, M, CBM);
    if (M == 0) return AP_OK;
    ConvArgs a{x, weight, bias, resid, out, h, w, cin, ho, wo, cout, ksize, stride, pad, ksize * ksize * cin, (int)M, act};
    const size_t blocks = (M + CBM - 1) / CBM * (size_t)((cout + CBN - 1) / CBN);
    AP_REQUIRE(blocks < (size_t)1 << 31, "%s: grid too large", who);
    return dispatch_dtype(who, dtype, [&](auto tag) {
        conv_implicit_gemm<typename decltype(tag)::type, EXT><<<(unsigned)blocks, CTHREADS, 0, stream>>>(a);
    });
}

}  // namespace

int launch_conv2d_nhwc(int dtype, const void* x, int n, int h, int w, int cin, const void* weight, const float* bias, int cout,
                       int ksize, int stride, int pad, const void* resid, int relu, void* out, hipStream_t stream) {
    return launch_conv2d<false>(dtype, x, n, h, w, cin, weight, bias, cout, ksize, stride, pad, resid, relu, out, stream);
}

int launch_conv2d_nhwc_ex(int dtype, const void* x, int n, int h, int w, int cin, const void* weight, const float* bias, int cout,
                          int ksize, int stride, int pad, const void* resid, int act, void* out, hipStream_t stream) {
    return launch_conv2d<true>(dtype, x, n, h, w, cin, weight, bias, cout, ksize, stride, pad, resid, act, out, stream);
}

int launch_preproc_nhwc8(const uint8_t* src, int n, int h, int w, int top, int left, int S, const float mean[3],
                         const float stdv[3], void* dst, int dtype, hipStream_t stream) {
    AP_REQUIRE(src && dst && mean && stdv && n >= 0 && S > 0 && top >= 0 && left >= 0 && top + S <= h && left + S <= w,
               "preproc_nhwc8: bad arguments (%dx%d tile, crop %d at %d, %d)", h, w, S, top, left);
    if (n == 0) return AP_OK;
    const void* lut = nullptr;
    int rc = get_norm_lut(mean, stdv, dtype, stream, &lut);
    if (rc != AP_OK) return rc;
    return dispatch_dtype("preproc_nhwc8", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        preproc_nhwc8<T><<<grid_1d((size_t)n * S * S, 65536), 256, 0, stream>>>(src, n, h, w, top, left, S, (const T*)lut, (T*)dst);
    });
}

int launch_maxpool3x3s2_nhwc(int dtype, const void* x, int n, int h, int w, int c, void* out, hipStream_t stream) {
    AP_REQUIRE(x && out && n >= 0 && h > 0 && w > 0 && c > 0 && c % 8 == 0, "maxpool3x3s2_nhwc: n %d h %d w %d c %d (c %% 8 == 0)",
               n, h, w, c);
    AP_REQUIRE(aligned16(x, out), "maxpool3x3s2_nhwc: pointers must be 16-byte aligned");
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    if (n == 0) return AP_OK;
    const size_t work = (size_t)n * ho * wo * c / (16 / dtype_size(dtype));
    return dispatch_dtype("maxpool3x3s2_nhwc", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        maxpool3x3s2<T><<<grid_1d(work, 65536), 256, 0, stream>>>((const T*)x, n, h, w, c, ho, wo, (T*)out);
    });
}

int launch_avgpool_nhwc(int dtype, const void* x, int n, int hw, int c, float* out, hipStream_t stream) {
    AP_REQUIRE(x && out && n >= 0 && hw > 0 && c > 0, "avgpool_nhwc: n %d hw %d c %d", n, hw, c);
    if (n == 0) return AP_OK;
    return dispatch_dtype("avgpool_nhwc", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        avgpool_nhwc<T><<<grid_1d((size_t)n * c, 65536), 256, 0, stream>>>((const T*)x, n, hw, c, out);
    });
}

}  // namespace ap

extern "C" {

int ap_conv2d_nhwc(int dtype, const void* x, int n, int h, int w, int cin, const void* weight, const float* bias, int cout,
                   int ksize, int stride, int pad, const void* resid, int relu, void* out, ap_stream_t stream) {
    return ap::launch_conv2d_nhwc(dtype, x, n, h, w, cin, weight, bias, cout, ksize, stride, pad, resid, relu, out,
                                  (hipStream_t)stream);
}

int ap_conv2d_nhwc_ex(int dtype, const void* x, int n, int h, int w, int cin, const void* weight, const float* bias, int cout,
                      int ksize, int stride, int pad, const void* resid, int act, void* out, ap_stream_t stream) {
    return ap::launch_conv2d_nhwc_ex(dtype, x, n, h, w, cin, weight, bias, cout, ksize, stride, pad, resid, act, out,
                                     (hipStream_t)stream);
}

int ap_maxpool3x3s2_nhwc(int dtype, const void* x, int n, int h, int w, int c, void* out, ap_stream_t stream) {
    return ap::launch_maxpool3x3s2_nhwc(dtype, x, n, h, w, c, out, (hipStream_t)stream);
}

int ap_avgpool_nhwc(int dtype, const void* x, int n, int hw, int c, float* out, ap_stream_t stream) {
    return ap::launch_avgpool_nhwc(dtype, x, n, hw, c, out, (hipStream_t)stream);
}

}  // extern "C"
