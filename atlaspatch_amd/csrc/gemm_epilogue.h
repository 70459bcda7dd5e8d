// The GEMM epilogue family, defined ONCE for the two MFMA kernels (gemm.hip: 128 x 128 tiles, gemm256.hip: persistent
// 256 x 256 tiles) and for the C ABI (capi.cpp).  launch_gemm_impl picks a kernel from M, N and the CU count, so the same
// layer runs on one or the other depending on the batch size: the two must agree bit for bit, and they do because every
// piece of epilogue arithmetic below -- and every list of "which epilogues ..." -- exists here and nowhere else.
//
// Adding an activation:
//   1. the enum value(s) in ap_common.h (GemmEpilogue: a BIAS_ and a NORM_ form) and an EpiAct value here;
//   2. one row per enum value in kEpiTraits;
//   3. the packed two-value routine in ap_common.h, called from act4 (and its libm form from act_f32 for float32 buffers);
//   4. the AP_EPI_* define(s) in include/atlaspatch_hip.h with the same code (capi.cpp static_asserts the equality);
//   5. fc1_epilogue in vit.cpp, where a model's configuration chooses it.
// No kernel, launcher or check is touched: they all go through the traits and dispatch_epilogue.
#pragma once
#include <type_traits>
#include "ap_common.h"

namespace ap {

enum EpiAct { ACT_NONE, ACT_GELU, ACT_GELU_S /* GELU on input pre-scaled by kGeluS */, ACT_QGELU, ACT_GTANH, ACT_SWIGLU /* gate */ };

struct EpiTraits {
    int epi;
    bool norm;       // fused LayerNorm: accumulators start from zero, y = rstd acc + (nmr colsum + bias); needs colsum / rowstats
    bool resid;      // residual-stream epilogue: 16-bit add in place + row partial sums; needs partial
    EpiAct act;
    bool split;      // has a split-f16 form (float32 buffers, gemm.hip)
    bool k256;       // implemented by the 256 x 256 kernel
};
constexpr EpiTraits kEpiTraits[] = {
    {EPI_BIAS_STORE,   false, false, ACT_NONE,   true,  true},
    {EPI_BIAS_GELU,    false, false, ACT_GELU,   true,  true},
    {EPI_BIAS_RESID,   false, false, ACT_NONE,   true,  true},
    {EPI_PATCH_EMBED,  false, false, ACT_NONE,   true,  false},
    {EPI_NORM_STORE,   true,  false, ACT_NONE,   false, true},
    {EPI_NORM_GELU,    true,  false, ACT_GELU_S, false, true},
    {EPI_RESID_STATS,  false, true,  ACT_NONE,   false, true},
    {EPI_PATCH_STREAM, false, true,  ACT_NONE,   false, true},
    {EPI_NORM_SWIGLU,  true,  false, ACT_SWIGLU, false, true},
    {EPI_NORM_QGELU,   true,  false, ACT_QGELU,  false, true},
    {EPI_BIAS_QGELU,   false, false, ACT_QGELU,  true,  true},
    {EPI_NORM_GTANH,   true,  false, ACT_GTANH,  false, true},
    {EPI_BIAS_GTANH,   false, false, ACT_GTANH,  true,  true},
};
constexpr int kNumEpilogues = sizeof(kEpiTraits) / sizeof(kEpiTraits[0]);
constexpr bool epi_table_in_order(int i = 0) { return i == kNumEpilogues || (kEpiTraits[i].epi == i && epi_table_in_order(i + 1)); }
static_assert(epi_table_in_order(), "kEpiTraits: row i describes epilogue code i");

constexpr int EPI_UNKNOWN = -1;                  // what dispatch_epilogue hands over for a code outside the enum: every trait is false
constexpr bool epi_known(int e) { return e >= 0 && e < kNumEpilogues; }
constexpr bool epi_is_norm(int e) { return epi_known(e) && kEpiTraits[e].norm; }
constexpr bool epi_is_resid(int e) { return epi_known(e) && kEpiTraits[e].resid; }
constexpr EpiAct epi_act(int e) { return epi_known(e) ? kEpiTraits[e].act : ACT_NONE; }
constexpr bool epi_has_split(int e) { return epi_known(e) && kEpiTraits[e].split; }
constexpr bool epi_in_gemm256(int e) { return epi_known(e) && kEpiTraits[e].k256; }

// "this epilogue has the operands it needs" (launch_gemm_impl, gemm256_supports, ap_gemm_fused)
inline bool epi_operands_ok(int e, const GemmArgs& a) {
    if (epi_is_norm(e)) return a.colsum && a.rowstats;
    if (e == EPI_PATCH_STREAM) return a.partial && a.pos16 && a.P > 0 && a.R >= 0;
    return !epi_is_resid(e) || a.partial != nullptr;
}

// runtime code -> compile-time constant: f(std::integral_constant<int, EPI>{}); the caller filters with the traits
// (`if constexpr (epi_in_gemm256(EPI)) ... else` its own error, which a code outside the enum reaches as EPI_UNKNOWN)
template <typename F> int dispatch_epilogue(int epilogue, F&& f) {
    switch (epilogue) {
#define AP_EPI_CASE(E) case E: return f(std::integral_constant<int, E>{})
        AP_EPI_CASE(EPI_BIAS_STORE); AP_EPI_CASE(EPI_BIAS_GELU); AP_EPI_CASE(EPI_BIAS_RESID); AP_EPI_CASE(EPI_PATCH_EMBED);
        AP_EPI_CASE(EPI_NORM_STORE); AP_EPI_CASE(EPI_NORM_GELU); AP_EPI_CASE(EPI_RESID_STATS); AP_EPI_CASE(EPI_PATCH_STREAM);
        AP_EPI_CASE(EPI_NORM_SWIGLU); AP_EPI_CASE(EPI_NORM_QGELU); AP_EPI_CASE(EPI_BIAS_QGELU); AP_EPI_CASE(EPI_NORM_GTANH);
        AP_EPI_CASE(EPI_BIAS_GTANH);
#undef AP_EPI_CASE
    }
    return f(std::integral_constant<int, EPI_UNKNOWN>{});
}

// CUs of the current device (first call's device; 256 when the query fails): grid size of the persistent kernel and the
// kernel choice of launch_gemm_impl
inline int device_cu_count() {
    static const int num_cu = [] {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
        return prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }();
    return num_cu;
}

namespace {

// the activation on a lane's four values, two at a time: the packed routines of ap_common.h (16-bit results)
template <EpiAct ACT> __device__ __forceinline__ f32x4 act4(f32x4 v) {
    static_assert(ACT != ACT_SWIGLU, "the gate takes two operands: swiglu2");
    if constexpr (ACT == ACT_NONE) return v;
    else {
        const f32x2_t lo = {v[0], v[1]}, hi = {v[2], v[3]};
        f32x2_t a, b;
        if constexpr (ACT == ACT_GELU) { a = gelu_sigmoid_poly2(lo); b = gelu_sigmoid_poly2(hi); }
        if constexpr (ACT == ACT_GELU_S) { a = gelu_sigmoid_poly2_s(lo); b = gelu_sigmoid_poly2_s(hi); }
        if constexpr (ACT == ACT_QGELU) { a = quick_gelu2(lo); b = quick_gelu2(hi); }
        if constexpr (ACT == ACT_GTANH) { a = gelu_tanh2(lo); b = gelu_tanh2(hi); }
        return f32x4{a[0], a[1], b[0], b[1]};
    }
}
// ... and its float32 form on libm (float32 buffers: gemm.hip only)
template <EpiAct ACT> __device__ __forceinline__ float act_f32(float x) {
    static_assert(ACT != ACT_SWIGLU && ACT != ACT_GELU_S, "16-bit epilogues only");
    if constexpr (ACT == ACT_GELU) return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
    if constexpr (ACT == ACT_QGELU) return x / (1.0f + expf(-1.702f * x));
    if constexpr (ACT == ACT_GTANH) {
        // x / (1 + exp(-2 u)) with libm expf keeps the RELATIVE accuracy in the negative tail, where
        // 1 + tanhf(u) cancels; u = sqrt(2 / pi) (x + 0.044715 x^3) by two fma
        const float u2 = -1.5957691216057308f * fmaf(0.044715f * x * x, x, x);
        return x / (1.0f + expf(u2));
    }
    return x;
}

// fused LayerNorm on a lane's four values, two per instruction (v_pk_fma_f32): y = rstd * acc + (nmr * colsum + bias),
// rs2 = {rstd, rstd}, nm2 = {nmr, nmr} of the row (ACT_GELU_S: the caller has multiplied rstd, nmr and bias by kGeluS)
__device__ __forceinline__ f32x4 norm_affine4(f32x2_t rs2, f32x2_t nm2, f32x4 v, f32x4 cs, f32x4 bb) {
    const f32x2_t lo = __builtin_elementwise_fma(rs2, f32x2_t{v[0], v[1]},
        __builtin_elementwise_fma(nm2, f32x2_t{cs[0], cs[1]}, f32x2_t{bb[0], bb[1]}));
    const f32x2_t hi = __builtin_elementwise_fma(rs2, f32x2_t{v[2], v[3]},
        __builtin_elementwise_fma(nm2, f32x2_t{cs[2], cs[3]}, f32x2_t{bb[2], bb[3]}));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
}

template <typename T> __device__ __forceinline__ u32x2 pack4(f32x4 v);
template <> __device__ __forceinline__ u32x2 pack4<f16>(f32x4 v) {
    f16x4 h = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
    return __builtin_bit_cast(u32x2, h);
}
template <> __device__ __forceinline__ u32x2 pack4<bf16>(f32x4 v) {
    bf16x4 h = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    return __builtin_bit_cast(u32x2, h);
}

// The residual-stream epilogues' element step on one dword = two packed T values.  resid_add2: y = T(d + r) (d = the branch
// output already rounded to T, r = the stream); stats2: s += sum(y), q += sum(y^2) in f32.  The two kernels chain these in
// different, documented orders (gemm_mma.h: resid_add_stats, 8 values per lane; gemm.hip: 4 + 4 across lane ^ 32).
template <typename T> __device__ __forceinline__ uint32_t resid_add2(uint32_t d, uint32_t r);
template <typename T> __device__ __forceinline__ void stats2(uint32_t y, float& s, float& q);
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
template <> __device__ __forceinline__ uint32_t resid_add2<f16>(uint32_t d, uint32_t r) {
    return __builtin_bit_cast(uint32_t, (f16x2_t)(__builtin_bit_cast(f16x2_t, d) + __builtin_bit_cast(f16x2_t, r)));   // v_pk_add_f16: correctly rounded
}
template <> __device__ __forceinline__ void stats2<f16>(uint32_t y, float& s, float& q) {
    const f16x2_t c = __builtin_bit_cast(f16x2_t, y);
    s = __builtin_amdgcn_fdot2(c, f16x2_t{(_Float16)1.0f, (_Float16)1.0f}, s, false);
    q = __builtin_amdgcn_fdot2(c, c, q, false);
}
template <> __device__ __forceinline__ uint32_t resid_add2<bf16>(uint32_t d, uint32_t r) {
    const float d0 = __builtin_bit_cast(float, d << 16), d1 = __builtin_bit_cast(float, d & 0xffff0000u);
    const float r0 = __builtin_bit_cast(float, r << 16), r1 = __builtin_bit_cast(float, r & 0xffff0000u);
    const bf16x4 c4 = {(bf16)(d0 + r0), (bf16)(d1 + r1), (bf16)0.0f, (bf16)0.0f};
    return __builtin_bit_cast(u32x2, c4)[0];
}
template <> __device__ __forceinline__ void stats2<bf16>(uint32_t y, float& s, float& q) {
    const float c0 = __builtin_bit_cast(float, y << 16), c1 = __builtin_bit_cast(float, y & 0xffff0000u);
    s += c0 + c1;
    q = __builtin_fmaf(c1, c1, __builtin_fmaf(c0, c0, q));
}

}  // namespace
}  // namespace ap
