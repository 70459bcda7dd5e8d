// Swin kernels (CHIEF-CTransPath): shifted-window attention over 7x7 windows at head dimension 32, and patch merging (the
// 2x2 gather) fused with its LayerNorm over 4C channels.  Activations are token-major NHWC in the compute type T (f16, bf16,
// f32); the linear layers (qkv, proj, fc1, fc2, the merge's reduction) run in conv.hip's implicit GEMM with ksize 1.
//
// Window attention.  The cyclic shift, the window partition, the region mask and their reverses are index arithmetic: token
// (yi, xi) of window (wy, wx) of the map rolled by (-shift, -shift) is the source pixel ((7 wy + yi + shift) % H,
// (7 wx + xi + shift) % W), and its output goes back to that pixel.  The region label of a rolled position is the pair of its
// slices [0, H-7) | [H-7, H-shift) | [H-shift, H) per axis; inside one window only the last window row / column mixes two
// labels (yi >= 7 - shift or not), so "different label" is two comparisons.  Masked pairs get -100 (not -inf), added after
// the bias as transformers' SwinSelfAttention does; shift 0 has no mask.
//
// f16 / bf16: one wave per (head, run of windows), four waves per workgroup; 49 tokens padded to 64.
//   S^T = K Q^T   4 x 4 tiles of one v_mfma_f32_16x16x32 each (the head dimension is exactly one K step).  The Q and K
//                 fragments are 16-byte global loads (a token's head slice is 64 contiguous bytes): no LDS.  With K as the
//                 first operand a lane holds, per query tile, query (lane & 15) and keys 16 jt + 4 (lane >> 4) + e.
//   softmax       in registers, f32: * scale + bias (+ mask), padded keys excluded, row max and sum over the lane's 16 values
//                 and an xor-16 / xor-32 butterfly (the same bits on the four lanes of a row); exp2 of the pre-scaled logits.
//   O^T = V^T P^T 4 x 2 tiles x 2 K steps.  P stays in registers: the lane's 8 probabilities of a K step (keys 32 ks + 4 q + e
//                 and 32 ks + 16 + 4 q + e) ARE its operand fragment once the key order of the K step is taken to be that
//                 one, and V^T is read from LDS in the same order.  V goes global -> registers -> LDS transposed
//                 ([32][72] T per wave, padded keys zero).  O is scaled by 1 / sum in f32 and stored 8 bytes per lane;
//                 padded query rows are never stored.
//   The relative-position bias of the wave's head (f32 [49][49]) is held in registers across the wave's windows.
// f32: one wave per (window, head); K and V staged in LDS as f32, lane t < 49 owns query row t: 32-term fmaf dot products in
//   ascending order, two passes over the keys (row maximum; expf and fmaf P V), scaled by 1 / sum -- exact f32, no MFMA.
// No atomics and no reduction across waves: a token's bits do not depend on the batch or on the run length.
//
// patch_merge_ln: one wave per output pixel; channel chunk k of the 4C row comes from source pixel (2 oy + dy, 2 ox + dx) with
// quadrant k / (C / 8) = dy + 2 dx (x[0::2,0::2] | x[1::2,0::2] | x[0::2,1::2] | x[1::2,1::2]); two-pass f32 statistics.
#include <algorithm>
#include "kernel_util.h"
#include "gemm_epilogue.h"

namespace ap {
namespace {

constexpr int WIN = 7, WT = 49, HD = 32;
constexpr int WA_WAVES = 4;
constexpr int VT_LD = 72;                     // keys per V^T row in LDS (64 + 8: 144-byte rows)
constexpr float MASK_VALUE = -100.0f;
constexpr float LOG2E = 1.4426950408889634f;

struct WaArgs {
    const void* qkv;            // T [n, H, W, 3 C], q | k | v, C = heads * 32
    const float* bias;          // f32 [heads][49][49]
    void* out;                  // T [n, H, W, C]
    int H, W, heads, shift, nwy, nwx;
    long nwin;                  // n * nwy * nwx
    int wpw;                    // 16-bit kernel: windows per wave
    long ngroups;               // ... and runs of wpw windows
    float scale;
};

// element index of the source pixel of token (yi, xi) of window `win`
__device__ __forceinline__ size_t source_pixel(const WaArgs& a, long win, int yi, int xi) {
    const int per = a.nwy * a.nwx;
    const long img = win / per;
    const int r = (int)(win - img * per);
    const int wy = r / a.nwx, wx = r - wy * a.nwx;
    int sy = wy * WIN + yi + a.shift, sx = wx * WIN + xi + a.shift;
    if (sy >= a.H) sy -= a.H;
    if (sx >= a.W) sx -= a.W;
    return ((size_t)img * a.H + sy) * a.W + sx;
}

template <typename T>
__global__ __launch_bounds__(WA_WAVES * 64) void swin_window_attention_mma(WaArgs a) {
    using Frag = typename Mma16x16<T>::Frag;
    __shared__ __attribute__((aligned(16))) T vt_all[WA_WAVES][HD * VT_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    T* vt = vt_all[wave];
    const long g = (long)blockIdx.x * WA_WAVES + wave;
    const int head = (int)(g % a.heads);
    const long grp = g / a.heads;
    const bool wave_ok = grp < a.ngroups;
    const int C = a.heads * HD;
    const int edge = WIN - a.shift;              // yi >= edge: the second label of the last window row (shift > 0)

    // the lane's four rows (query tile it / key-or-value tile it, row l15) and its 16 key columns: fixed for every window
    int ty[4], tx[4];
    bool tv[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int i = it * 16 + l15;
        tv[it] = i < WT;
        ty[it] = tv[it] ? i / WIN : 0;
        tx[it] = tv[it] ? i - ty[it] * WIN : 0;
    }
    f32x4 bias[4][4];
    unsigned key_hy = 0, key_hx = 0, key_ok = 0;   // bit jt * 4 + e
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = jt * 16 + q * 4 + e;
            const bool ok = j < WT;
            const int jy = j / WIN, jx = j - jy * WIN;
            key_ok |= (ok ? 1u : 0u) << (jt * 4 + e);
            key_hy |= (ok && jy >= edge ? 1u : 0u) << (jt * 4 + e);
            key_hx |= (ok && jx >= edge ? 1u : 0u) << (jt * 4 + e);
#pragma unroll
            for (int it = 0; it < 4; ++it)
                bias[it][jt][e] = (wave_ok && tv[it] && ok) ? a.bias[((size_t)head * WT + it * 16 + l15) * WT + j] : 0.f;
        }

    const T* qkv = (const T*)a.qkv;
    T* out = (T*)a.out;
    const Frag zero = __builtin_bit_cast(Frag, u32x4{0u, 0u, 0u, 0u});
    for (int k = 0; k < a.wpw; ++k) {
        const long win = grp * a.wpw + k;
        const bool ok = wave_ok && win < a.nwin;
        bool last_y = false, last_x = false;
        if (ok && a.shift > 0) {
            const int r = (int)(win % ((long)a.nwy * a.nwx));
            last_y = r / a.nwx == a.nwy - 1;
            last_x = r % a.nwx == a.nwx - 1;
        }
        size_t pix[4];
        Frag qf[4], kf[4], vf[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            qf[it] = zero; kf[it] = zero; vf[it] = zero;
            pix[it] = 0;
            if (ok && tv[it]) {
                pix[it] = source_pixel(a, win, ty[it], tx[it]);
                const T* p = qkv + pix[it] * (size_t)(3 * C) + head * HD + q * 8;
                qf[it] = *(const Frag*)p;
                kf[it] = *(const Frag*)(p + C);
                vf[it] = *(const Frag*)(p + 2 * C);
            }
        }
        __syncthreads();                          // the previous window's V^T reads are done
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int e = 0; e < 8; ++e) vt[(q * 8 + e) * VT_LD + it * 16 + l15] = vf[it][e];

        f32x4 s[4][4];
        float inv[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) s[it][jt] = Mma16x16<T>::run(kf[jt], qf[it], f32x4{0.f, 0.f, 0.f, 0.f});
            const bool qhy = ty[it] >= edge, qhx = tx[it] >= edge;
            float m = -3.0e38f;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned bit = 1u << (jt * 4 + e);
                    float v = s[it][jt][e] * a.scale + bias[it][jt][e];
                    const bool masked = (last_y && qhy != ((key_hy & bit) != 0)) || (last_x && qhx != ((key_hx & bit) != 0));
                    if (masked) v += MASK_VALUE;
                    if (!(key_ok & bit)) v = -1.0e30f;
                    s[it][jt][e] = v;
                    m = fmaxf(m, v);
                }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float sum = 0.f;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = __builtin_amdgcn_exp2f((s[it][jt][e] - m) * LOG2E);
                    s[it][jt][e] = p;
                    sum += p;
                }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            inv[it] = 1.0f / sum;
        }
        __syncthreads();                          // V^T is in LDS
        Frag vtf[2][2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const T* row = vt + (dt * 16 + l15) * VT_LD + ks * 32 + q * 4;
                const u32x2 lo = *(const u32x2*)row, hi = *(const u32x2*)(row + 16);
                vtf[dt][ks] = __builtin_bit_cast(Frag, u32x4{lo[0], lo[1], hi[0], hi[1]});
            }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            Frag pf[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    pf[ks][e] = from_f32<T>(s[it][2 * ks][e]);
                    pf[ks][4 + e] = from_f32<T>(s[it][2 * ks + 1][e]);
                }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) o = Mma16x16<T>::run(vtf[dt][ks], pf[ks], o);
                o *= inv[it];
                if (ok && tv[it]) *(u32x2*)(out + pix[it] * (size_t)C + head * HD + dt * 16 + q * 4) = pack4<T>(o);
            }
        }
    }
}

__global__ __launch_bounds__(WA_WAVES * 64) void swin_window_attention_f32(WaArgs a) {
    __shared__ __attribute__((aligned(16))) float kv_all[WA_WAVES][2][WT * HD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* ks = kv_all[wave][0];
    float* vs = kv_all[wave][1];
    const long item = (long)blockIdx.x * WA_WAVES + wave;
    const bool ok = item < a.nwin * a.heads;
    const int head = (int)(item % a.heads);
    const long win = item / a.heads;
    const int C = a.heads * HD;
    const float* qkv = (const float*)a.qkv;
    if (ok) {
        for (int id = lane; id < WT * (HD / 4); id += 64) {
            const int t = id >> 3, c = id & 7;
            const float* p = qkv + source_pixel(a, win, t / WIN, t % WIN) * (size_t)(3 * C) + head * HD + c * 4;
            *(f32x4*)(ks + t * HD + c * 4) = *(const f32x4*)(p + C);
            *(f32x4*)(vs + t * HD + c * 4) = *(const f32x4*)(p + 2 * C);
        }
    }
    __syncthreads();
    if (!ok || lane >= WT) return;
    const int yi = lane / WIN, xi = lane - yi * WIN;
    const size_t pix = source_pixel(a, win, yi, xi);
    float qr[HD];
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) {
        const f32x4 v = *(const f32x4*)(qkv + pix * (size_t)(3 * C) + head * HD + c * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) qr[c * 4 + e] = v[e];
    }
    bool last_y = false, last_x = false;
    if (a.shift > 0) {
        const int r = (int)(win % ((long)a.nwy * a.nwx));
        last_y = r / a.nwx == a.nwy - 1;
        last_x = r % a.nwx == a.nwx - 1;
    }
    const int edge = WIN - a.shift;
    const bool qhy = yi >= edge, qhx = xi >= edge;
    const float* brow = a.bias + ((size_t)head * WT + lane) * WT;
    auto logit = [&](int j) {                     // the same instructions in both passes: the same bits
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < HD; ++c) d = fmaf(qr[c], ks[j * HD + c], d);
        float v = d * a.scale + brow[j];
        const int jy = j / WIN;
        const bool masked = (last_y && qhy != (jy >= edge)) || (last_x && qhx != (j - jy * WIN >= edge));
        if (masked) v += MASK_VALUE;
        return v;
    };
    // two passes over the keys (row maximum, then exponentials and P V) instead of 49 live logits per lane
    float m = -3.0e38f;
#pragma unroll 1
    for (int j = 0; j < WT; ++j) m = fmaxf(m, logit(j));
    float sum = 0.f;
    float o[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) o[c] = 0.f;
#pragma unroll 1
    for (int j = 0; j < WT; ++j) {
        const float p = expf(logit(j) - m);
        sum += p;
#pragma unroll
        for (int c = 0; c < HD; ++c) o[c] = fmaf(p, vs[j * HD + c], o[c]);
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int c = 0; c < HD; ++c) o[c] *= inv;
    float* dst = (float*)a.out + pix * (size_t)C + head * HD;
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) *(f32x4*)(dst + c * 4) = f32x4{o[c * 4], o[c * 4 + 1], o[c * 4 + 2], o[c * 4 + 3]};
}

// ---- patch merging + LayerNorm
template <typename T>
__global__ __launch_bounds__(256) void patch_merge_ln(const T* x, long rows, int H, int W, int C, const float* g, const float* b,
                                                      float eps, T* out) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                 // a whole wave
    const int Ho = H / 2, Wo = W / 2;
    const int ox = (int)(r % Wo), oy = (int)((r / Wo) % Ho);
    const long img = r / ((long)Wo * Ho);
    const int per = C / 8, nch = 4 * per;
    const T* base = x + (((size_t)img * H + 2 * oy) * W + 2 * ox) * C;
    auto chunk = [&](int k) {                              // 8 channels of the gathered 4C row
        const int quad = k / per;
        return base + ((size_t)(quad & 1) * W + (quad >> 1)) * C + (k - quad * per) * 8;
    };
    wave_layernorm8(chunk, nch, 4 * C, g, b, eps, out + (size_t)r * 4 * C);
}

}  // namespace

int launch_swin_window_attention(int dtype, const void* qkv, int n, int h, int w, int heads, int shift, const float* rel_bias,
                                 void* out, hipStream_t stream) {
    AP_REQUIRE(qkv && rel_bias && out, "swin_window_attention: null pointer");
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16 || dtype == AP_F32, "swin_window_attention: dtype %d", dtype);
    AP_REQUIRE(n >= 0 && h > 0 && w > 0 && h % WIN == 0 && w % WIN == 0 && h <= 4096 && w <= 4096,
               "swin_window_attention: n %d h %d w %d (h and w multiples of the 7-token window)", n, h, w);
    AP_REQUIRE(heads >= 1 && heads <= 1024, "swin_window_attention: heads %d", heads);
    AP_REQUIRE(shift >= 0 && shift < WIN, "swin_window_attention: shift %d outside [0, 7)", shift);
    AP_REQUIRE(aligned16(qkv, out), "swin_window_attention: pointers must be 16-byte aligned");
    AP_REQUIRE(qkv != out, "swin_window_attention: in place is not supported");
    if (n == 0) return AP_OK;
    WaArgs a{};
    a.qkv = qkv; a.bias = rel_bias; a.out = out;
    a.H = h; a.W = w; a.heads = heads; a.shift = shift; a.nwy = h / WIN; a.nwx = w / WIN;
    a.nwin = (long)n * a.nwy * a.nwx;
    a.scale = 0.17677669529663687f;              // 32^-0.5
    const long items = a.nwin * heads;
    if (dtype == AP_F32) {
        const long blocks = (items + WA_WAVES - 1) / WA_WAVES;
        AP_REQUIRE(blocks < (long)1 << 31, "swin_window_attention: grid too large");
        swin_window_attention_f32<<<(unsigned)blocks, WA_WAVES * 64, 0, stream>>>(a);
        AP_HIP_CHECK(hipGetLastError());
        return AP_OK;
    }
    // windows per wave: the head's bias table is loaded once per wave; short runs while the grid is small
    a.wpw = (int)std::max<long>(1, std::min<long>(8, items / 4096));
    a.ngroups = (a.nwin + a.wpw - 1) / a.wpw;
    const long blocks = (a.ngroups * heads + WA_WAVES - 1) / WA_WAVES;
    AP_REQUIRE(blocks < (long)1 << 31, "swin_window_attention: grid too large");
    return dispatch_half("swin_window_attention", dtype, [&](auto tag) {
        swin_window_attention_mma<typename decltype(tag)::type><<<(unsigned)blocks, WA_WAVES * 64, 0, stream>>>(a);
    });
}

int launch_patch_merge_ln(int dtype, const void* x, int n, int h, int w, int c, const float* ln_weight, const float* ln_bias,
                          float eps, void* out, hipStream_t stream) {
    AP_REQUIRE(x && ln_weight && ln_bias && out, "patch_merge_ln: null pointer");
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16 || dtype == AP_F32, "patch_merge_ln: dtype %d", dtype);
    AP_REQUIRE(n >= 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && c > 0 && c % 8 == 0,
               "patch_merge_ln: n %d h %d w %d c %d (h and w even, c %% 8 == 0)", n, h, w, c);
    AP_REQUIRE(eps > 0.f, "patch_merge_ln: eps %g", (double)eps);
    AP_REQUIRE(aligned16(x, ln_weight, ln_bias, out), "patch_merge_ln: pointers must be 16-byte aligned");
    AP_REQUIRE(x != out, "patch_merge_ln: in place is not supported");
    if (n == 0) return AP_OK;
    const long rows = (long)n * (h / 2) * (w / 2);
    const long blocks = (rows + 3) / 4;
    AP_REQUIRE(blocks < (long)1 << 31, "patch_merge_ln: grid too large");
    return dispatch_dtype("patch_merge_ln", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        patch_merge_ln<T><<<(unsigned)blocks, 256, 0, stream>>>((const T*)x, rows, h, w, c, ln_weight, ln_bias, eps, (T*)out);
    });
}

}  // namespace ap

extern "C" {

int ap_swin_window_attention(int dtype, const void* qkv, int n, int h, int w, int heads, int shift, const float* rel_bias,
                             void* out, ap_stream_t stream) {
    return ap::launch_swin_window_attention(dtype, qkv, n, h, w, heads, shift, rel_bias, out, (hipStream_t)stream);
}

int ap_patch_merge_ln(int dtype, const void* x, int n, int h, int w, int c, const float* ln_weight, const float* ln_bias, float eps,
                      void* out, ap_stream_t stream) {
    return ap::launch_patch_merge_ln(dtype, x, n, h, w, c, ln_weight, ln_bias, eps, out, (hipStream_t)stream);
}

}  // extern "C"
