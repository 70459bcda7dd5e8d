// The small toolkit every kernel file shares: 16-byte vector types, 4- and 8-element loads and stores, the MFMA wrappers,
// DPP / wave / block reductions, the one-wave-per-row LayerNorm, and on the host the pointer / dtype / grid predicates and the
// runtime-dtype -> template dispatch.  What only the two GEMM kernels use stays in gemm_mma.h.
#pragma once
#include <type_traits>
#include "ap_common.h"

namespace ap {

// ---- host predicates ----------------------------------------------------------------------
template <typename... P> inline bool aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }
inline bool known_dtype(int dt) { return dt == AP_F32 || dt == AP_F16 || dt == AP_BF16; }
inline bool half_dtype(int dt) { return dt == AP_F16 || dt == AP_BF16; }
// workgroups of 256 threads that cover `work` items, at most `cap` (grid-stride kernels)
inline unsigned grid_1d(size_t work, size_t cap = 0x7fffffff) {
    const size_t b = (work + 255) / 256;
    return (unsigned)(b < cap ? b : cap);
}

// ---- runtime dtype -> template argument ---------------------------------------------------
// f gets a TypeTag<T> (`using T = typename decltype(tag)::type;`) and launches the kernel; any other dtype sets the error
// and launches nothing.  f returns nothing (its one launch is then checked here) or a status of its own.
template <typename T> struct TypeTag { using type = T; };
template <typename F, typename T> inline int dispatch_call(const char* who, F& f, TypeTag<T> tag) {
    if constexpr (std::is_void_v<decltype(f(tag))>) {
        f(tag);
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return AP_OK;
        set_error("%s: kernel launch failed: %s", who, hipGetErrorString(e));
        return AP_ERR_HIP;
    } else {
        return f(tag);
    }
}
template <typename F> inline int dispatch_half(const char* who, int dtype, F&& f) {
    if (dtype == AP_F16) return dispatch_call(who, f, TypeTag<f16>{});
    if (dtype == AP_BF16) return dispatch_call(who, f, TypeTag<bf16>{});
    set_error("%s: dtype %d (f16 / bf16 only)", who, dtype);
    return AP_ERR_INVALID;
}
template <typename F> inline int dispatch_dtype(const char* who, int dtype, F&& f) {
    if (dtype == AP_F16) return dispatch_call(who, f, TypeTag<f16>{});
    if (dtype == AP_BF16) return dispatch_call(who, f, TypeTag<bf16>{});
    if (dtype == AP_F32) return dispatch_call(who, f, TypeTag<float>{});
    set_error("%s: unknown dtype %d", who, dtype);
    return AP_ERR_INVALID;
}

namespace {

// ---- vectors --------------------------------------------------------------------------------
template <typename T> struct Vec16;        // type: the 16-byte vector of T; half: the 8-byte one; oct: 8 elements of T
template <> struct Vec16<f16> { using type = f16x8; using half = f16x4; using oct = f16x8; };
template <> struct Vec16<bf16> { using type = bf16x8; using half = bf16x4; using oct = bf16x8; };
template <> struct Vec16<float> { using type = f32x4; typedef float half __attribute__((ext_vector_type(2))); typedef float oct __attribute__((ext_vector_type(8))); };

// 8 consecutive elements <-> float[8] (16-bit types: one 16-byte access; f32: two)
template <typename T> __device__ __forceinline__ void load8(const T* p, float v[8]) {
    if constexpr (sizeof(T) == 2) {
        const u32x4 r = *(const u32x4*)p;
        T e[8];
        __builtin_memcpy(e, &r, 16);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)e[i];
    } else {
        const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
    }
}

template <typename T> __device__ __forceinline__ void store8(T* p, const float v[8]) {
    if constexpr (sizeof(T) == 2) {
        T e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = from_f32<T>(v[i]);
        u32x4 r;
        __builtin_memcpy(&r, e, 16);
        *(u32x4*)p = r;
    } else {
        *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
        *(f32x4*)(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
}

// 4 / 8 consecutive elements <-> f32x4 (8: two adjacent f32x4, ONE 16-byte access of a 16-bit type)
template <typename T> __device__ __forceinline__ f32x4 load_vec4(const T* p) {
    if constexpr (sizeof(T) == 2) {
        const typename Vec16<T>::half h = *(const typename Vec16<T>::half*)p;
        return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    } else {
        return *(const f32x4*)p;
    }
}
template <typename T> __device__ __forceinline__ void store_vec4(T* p, f32x4 v) {
    if constexpr (sizeof(T) == 2) {
        typename Vec16<T>::half h = {(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
        *(typename Vec16<T>::half*)p = h;
    } else {
        *(f32x4*)p = v;
    }
}
template <typename T> __device__ __forceinline__ void load_vec8(const T* p, f32x4& a, f32x4& b) {
    if constexpr (sizeof(T) == 2) {
        const typename Vec16<T>::type h = *(const typename Vec16<T>::type*)p;
        a = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        b = f32x4{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
    } else {
        a = *(const f32x4*)p;
        b = *(const f32x4*)(p + 4);
    }
}
template <typename T> __device__ __forceinline__ void store_vec8(T* p, f32x4 a, f32x4 b) {
    if constexpr (sizeof(T) == 2) {
        typename Vec16<T>::type h = {(T)a[0], (T)a[1], (T)a[2], (T)a[3], (T)b[0], (T)b[1], (T)b[2], (T)b[3]};
        *(typename Vec16<T>::type*)p = h;
    } else {
        *(f32x4*)p = a;
        *(f32x4*)(p + 4) = b;
    }
}

// ---- MFMA -----------------------------------------------------------------------------------
template <typename T> struct Mma32x32;     // v_mfma_f32_32x32x16_{f16,bf16} / 32x32x2f32; K = k values per instruction
template <> struct Mma32x32<f16> {
    using Frag = f16x8;
    static constexpr int K = 16;
    static __device__ __forceinline__ f32x16 run(Frag a, Frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma32x32<bf16> {
    using Frag = bf16x8;
    static constexpr int K = 16;
    static __device__ __forceinline__ f32x16 run(Frag a, Frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma32x32<float> {
    using Frag = float;
    static constexpr int K = 2;
    static __device__ __forceinline__ f32x16 run(Frag a, Frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    }
};

template <typename T> struct Mma16x16;     // v_mfma_f32_16x16x32_{f16,bf16}; operand map: gemm_mma.h
template <> struct Mma16x16<f16> {
    using Frag = f16x8;
    static __device__ __forceinline__ f32x4 run(Frag a, Frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma16x16<bf16> {
    using Frag = bf16x8;
    static __device__ __forceinline__ f32x4 run(Frag a, Frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

// ---- reductions -----------------------------------------------------------------------------
#define AP_DPP_F32(V, CTRL) __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, (V)), (CTRL), 0xF, 0xF, true))
// sum over the 8 lanes that share (lane >> 3): xor-1, xor-2 (quad permutes), mirror within 8 -- every lane gets the total
__device__ __forceinline__ float sum8(float v) {
    v += AP_DPP_F32(v, 0xB1);
    v += AP_DPP_F32(v, 0x4E);
    v += AP_DPP_F32(v, 0x141);
    return v;
}
// ... and over the 16 lanes of a DPP row (mirror within 16 last): all VALU + DPP
__device__ __forceinline__ float sum16(float v) {
    v = sum8(v);
    v += AP_DPP_F32(v, 0x140);
    return v;
}

// xor butterfly over the 64 lanes: the same bits on every lane
template <typename V> __device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// sum / max over a 256-thread workgroup through red[4] (LDS); two barriers
__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = is_max ? fmaxf(v, o) : v + o;
    }
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    const float a = red[0], b = red[1], c = red[2], d = red[3];
    return is_max ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : (a + b) + (c + d);
}

// LayerNorm of one row of n = 8 nch elements by one wave: chunk(k) is the address of the row's k-th 8 elements of T, gamma / beta
// f32 [n], dst the dense output row.  Two-pass f32 statistics (mean, then the sum of squared deviations), each summed by every lane
// over its chunks in order and combined by wave_sum; 16-byte loads and stores.
template <typename T, typename Chunk>
__device__ __forceinline__ void wave_layernorm8(Chunk chunk, int nch, int n, const float* gamma, const float* beta, float eps, T* dst) {
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int k = lane; k < nch; k += 64) {
        float v[8];
        load8(chunk(k), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[e];
    }
    const float mean = wave_sum(s) / (float)n;
    float ss = 0.f;
    for (int k = lane; k < nch; k += 64) {
        float v[8];
        load8(chunk(k), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[e] - mean; ss = fmaf(d, d, ss); }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)n + eps);
    for (int k = lane; k < nch; k += 64) {
        float v[8], gv[8], bv[8], o[8];
        load8(chunk(k), v);
        load8(gamma + k * 8, gv);
        load8(beta + k * 8, bv);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[e] - mean) * rstd * gv[e] + bv[e];
        store8(dst + k * 8, o);
    }
}

}  // namespace
}  // namespace ap
