// v_mfma_f32_32x32x16 against v_mfma_f32_16x16x32 (f16 and bf16) at the operating point of gemm256's main loop: does the chip hold a
// higher clock on the 16x16x32 shape when the loop is the one that kernel runs?
//
// Two loops that differ only in the MFMA shape.  Each: one 512-thread workgroup per CU (96 KiB of LDS keeps a second one out),
// 8 waves = 2 (m) x 4 (n), per-wave tile 128 m x 64 n = 128 accumulator registers, one 64-deep K-tile (256 activation rows +
// 256 weight rows of 128 bytes) resident in LDS in the product's image (16-byte chunk ^= (row >> 1) & 7), and EVERY fragment
// re-read from LDS by ds_read_b128 in every iteration (24 reads per wave and iteration, as in the product; 32 MFMAs of 32x32x16 or
// 64 of 16x16x32).  No global traffic inside the loop, no barriers: this is the MFMA + fragment-read core alone.  Operands are
// uniform random in [-1, 1).  Per arm: wall time per launch (HIP events around the last launches of a >= 2 s back-to-back
// burst), wave cycles (s_memtime around the loop, median over workgroups) and the in-kernel clock (d s_memtime / d s_memrealtime
// x 100 MHz).  The stamps go to a buffer of their own.  Arms alternate in one process, 7 rounds, median and range.
//
// Second part: one wave computes a 32 x 32 block of C = A B^T with f32 accumulation in ascending k (K = 768 and 3072, accumulator
// started from zero) with either shape, the operands being the same; the two results are compared bitwise.
//
//   hipcc --offload-arch=gfx950 -O3 tools/isa_probes/mfma_shape_probe.hip -o mfma_shape_probe && ./mfma_shape_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

template <bool BF> struct Op;
template <> struct Op<false> {
    using Frag = f16x8;
    static __device__ __forceinline__ f32x16 m32(Frag a, Frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 m16(Frag a, Frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct Op<true> {
    using Frag = bf16x8;
    static __device__ __forceinline__ f32x16 m32(Frag a, Frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 m16(Frag a, Frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

constexpr int kRowBytes = 128, kRows = 512;            // LDS rows 0..255: activations (m), 256..511: weights (n)
constexpr int kImage = kRows * kRowBytes;              // 64 KiB
constexpr int kLds = 96 * 1024;                        // more than half a CU's LDS: one workgroup per CU

// stamps[block] = {d s_memtime, d s_memrealtime}
template <bool BF, int SHAPE>
__global__ __launch_bounds__(512, 2) void loop_kernel(const uint16_t* __restrict__ src, float* __restrict__ sink, long long* __restrict__ stamps,
                                                      int iters) {
    __shared__ __attribute__((aligned(16))) char smem[kLds];
    using Frag = typename Op<BF>::Frag;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 2, wc = wave & 3;
    // the image: row r, 16-byte chunk c of the source lands on chunk c ^ ((r >> 1) & 7)
    for (int i = threadIdx.x; i < kRows * 8; i += 512) {
        const int r = i >> 3, c = i & 7;
        *(u32x4*)(smem + r * kRowBytes + ((c ^ ((r >> 1) & 7)) << 4)) = *(const u32x4*)((const char*)src + (size_t)i * 16);
    }
    __syncthreads();

    int off = 0;                                       // opaque per iteration: the reads cannot be hoisted out of the loop
    long long t0, t1, r0, r1;
    if constexpr (SHAPE == 32) {
        f32x16 acc[2][4];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[nb][mb][e] = 0.0f;
        const int l31 = lane & 31, hi = lane >> 5, xr = (l31 >> 1) & 7;          // block bases are multiples of 32 rows
        int pa[4], pb[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int co = ((kk * 2 + hi) ^ xr) << 4;
            pa[kk] = (wr * 128 + l31) * kRowBytes + co;
            pb[kk] = (256 + wc * 64 + l31) * kRowBytes + co;
        }
        t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
        for (int it = 0; it < iters; ++it) {
            asm volatile("" : "+v"(off));
            const char* base = smem + off;
            Frag fb[2][4];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) fb[nb][kk] = *(const Frag*)(base + nb * 32 * kRowBytes + pb[kk]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {              // 64 m rows at a time, as the product's phases do
                Frag fa[2][4];
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) fa[mb][kk] = *(const Frag*)(base + (h * 64 + mb * 32) * kRowBytes + pa[kk]);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                        for (int mb = 0; mb < 2; ++mb) acc[nb][h * 2 + mb] = Op<BF>::m32(fb[nb][kk], fa[mb][kk], acc[nb][h * 2 + mb]);
            }
        }
        t1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
        float s = 0.0f;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int e = 0; e < 16; ++e) s += acc[nb][mb][e];
        sink[(size_t)blockIdx.x * 512 + threadIdx.x] = s;
    } else {
        f32x4 acc[4][8];                               // [n block of 16][m block of 16]
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int mb = 0; mb < 8; ++mb)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[nb][mb][e] = 0.0f;
        const int l15 = lane & 15, q = lane >> 4, xr = (l15 >> 1) & 7;           // block bases are multiples of 16 rows
        int pa[2], pb[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int co = ((kk * 4 + q) ^ xr) << 4;
            pa[kk] = (wr * 128 + l15) * kRowBytes + co;
            pb[kk] = (256 + wc * 64 + l15) * kRowBytes + co;
        }
        t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
        for (int it = 0; it < iters; ++it) {
            asm volatile("" : "+v"(off));
            const char* base = smem + off;
            Frag fb[4][2];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) fb[nb][kk] = *(const Frag*)(base + nb * 16 * kRowBytes + pb[kk]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                Frag fa[4][2];
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) fa[mb][kk] = *(const Frag*)(base + (h * 64 + mb * 16) * kRowBytes + pa[kk]);
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) acc[nb][h * 4 + mb] = Op<BF>::m16(fb[nb][kk], fa[mb][kk], acc[nb][h * 4 + mb]);
            }
        }
        t1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
        float s = 0.0f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int mb = 0; mb < 8; ++mb)
#pragma unroll
                for (int e = 0; e < 4; ++e) s += acc[nb][mb][e];
        sink[(size_t)blockIdx.x * 512 + threadIdx.x] = s;
    }
    if (threadIdx.x == 0) {
        stamps[2 * blockIdx.x] = t1 - t0;
        stamps[2 * blockIdx.x + 1] = r1 - r0;
    }
}

// One wave: C[n][m] (32 x 32, f32) = sum_k W[n][k] A[m][k], K-contiguous operands of K elements per row, the weight fragment as
// the first MFMA operand (as in the product), ascending k, accumulator started from zero.
template <bool BF, int SHAPE>
__global__ __launch_bounds__(64) void order_kernel(const uint16_t* __restrict__ w, const uint16_t* __restrict__ a, float* __restrict__ c, int K) {
    using Frag = typename Op<BF>::Frag;
    const int lane = threadIdx.x;
    if constexpr (SHAPE == 32) {
        const int l31 = lane & 31, hi = lane >> 5;
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        for (int k = 0; k < K; k += 16) {
            const Frag fw = *(const Frag*)(w + (size_t)l31 * K + k + hi * 8);
            const Frag fx = *(const Frag*)(a + (size_t)l31 * K + k + hi * 8);
            acc = Op<BF>::m32(fw, fx, acc);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) c[(8 * (e >> 2) + 4 * hi + (e & 3)) * 32 + l31] = acc[e];
    } else {
        const int l15 = lane & 15, q = lane >> 4;
        f32x4 acc[2][2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[nb][mb][e] = 0.0f;
        for (int k = 0; k < K; k += 32) {
            Frag fw[2], fx[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                fw[b] = *(const Frag*)(w + (size_t)(b * 16 + l15) * K + k + q * 8);
                fx[b] = *(const Frag*)(a + (size_t)(b * 16 + l15) * K + k + q * 8);
            }
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) acc[nb][mb] = Op<BF>::m16(fw[nb], fx[mb], acc[nb][mb]);
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int e = 0; e < 4; ++e) c[(nb * 16 + 4 * q + e) * 32 + mb * 16 + l15] = acc[nb][mb][e];
    }
}

static uint32_t g_seed = 12345u;
static float urand() {                                  // uniform in [-1, 1)
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) * (1.0f / 8388608.0f) - 1.0f;
}
static uint16_t to16(float v, bool bf) {
    if (bf) {
        uint32_t u;
        memcpy(&u, &v, 4);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    }
    const _Float16 h = (_Float16)v;
    uint16_t r;
    memcpy(&r, &h, 2);
    return r;
}

struct Sample { double ms, cycles, ghz; };

template <bool BF, int SHAPE>
static int run_arm(const uint16_t* src, float* sink, long long* stamps, int blocks, int iters, Sample* out) {
    hipEvent_t e0, e1, w0, w1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); CK(hipEventCreate(&w0)); CK(hipEventCreate(&w1));
    // >= 2 s of back-to-back launches: batches of 16 until the elapsed device time passes it
    float warm = 0.0f;
    CK(hipEventRecord(w0));
    while (warm < 2000.0f) {
        for (int i = 0; i < 16; ++i) loop_kernel<BF, SHAPE><<<blocks, 512>>>(src, sink, stamps, iters);
        CK(hipEventRecord(w1));
        CK(hipEventSynchronize(w1));
        CK(hipEventElapsedTime(&warm, w0, w1));
    }
    const int timed = 16;
    CK(hipEventRecord(e0));
    for (int i = 0; i < timed; ++i) loop_kernel<BF, SHAPE><<<blocks, 512>>>(src, sink, stamps, iters);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<long long> h(2 * blocks);
    CK(hipMemcpy(h.data(), stamps, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    std::vector<double> cyc(blocks), clk(blocks);
    for (int b = 0; b < blocks; ++b) {
        cyc[b] = (double)h[2 * b];
        clk[b] = (double)h[2 * b] / (double)h[2 * b + 1] * 0.1;      // s_memrealtime ticks at 100 MHz -> GHz
    }
    std::sort(cyc.begin(), cyc.end());
    std::sort(clk.begin(), clk.end());
    out->ms = ms / timed;
    out->cycles = cyc[blocks / 2];
    out->ghz = clk[blocks / 2];
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1)); CK(hipEventDestroy(w0)); CK(hipEventDestroy(w1));
    return 0;
}

static void summarise(const char* name, std::vector<Sample> v, double flop) {
    auto col = [&](auto f, double* lo, double* med, double* hi) {
        std::vector<double> x;
        for (const Sample& s : v) x.push_back(f(s));
        std::sort(x.begin(), x.end());
        *lo = x.front(); *med = x[x.size() / 2]; *hi = x.back();
    };
    double a, b, c;
    col([](const Sample& s) { return s.ms; }, &a, &b, &c);
    printf("%-16s ms/launch %8.4f [%8.4f .. %8.4f]   fs/FLOP %7.4f  (%7.1f TFLOP/s)", name, b, a, c, b * 1e12 / flop, flop / b * 1e-9);
    col([](const Sample& s) { return s.cycles; }, &a, &b, &c);
    printf("   wave cycles %11.0f [%11.0f .. %11.0f]", b, a, c);
    col([](const Sample& s) { return s.ghz; }, &a, &b, &c);
    printf("   clock GHz %6.3f [%6.3f .. %6.3f]\n", b, a, c);
}

template <bool BF>
static int timing(const char* dt, int blocks, int iters, float* sink, long long* stamps, bool* gate) {
    std::vector<uint16_t> h((size_t)kImage / 2);
    for (auto& x : h) x = to16(urand(), BF);
    uint16_t* src;
    CK(hipMalloc(&src, kImage));
    CK(hipMemcpy(src, h.data(), kImage, hipMemcpyHostToDevice));
    const int rounds = 7;
    std::vector<Sample> s32(rounds), s16(rounds);
    for (int r = 0; r < rounds; ++r) {
        if (run_arm<BF, 32>(src, sink, stamps, blocks, iters, &s32[r])) return 1;
        if (run_arm<BF, 16>(src, sink, stamps, blocks, iters, &s16[r])) return 1;
        printf("  %s round %d: 32x32x16 %.4f ms %.3f GHz | 16x16x32 %.4f ms %.3f GHz\n", dt, r, s32[r].ms, s32[r].ghz, s16[r].ms, s16[r].ghz);
        fflush(stdout);
    }
    const double flop = 2.0 * 256 * 256 * 64 * (double)iters * blocks;
    char name[64];
    snprintf(name, sizeof name, "%s 32x32x16", dt);
    summarise(name, s32, flop);
    snprintf(name, sizeof name, "%s 16x16x32", dt);
    summarise(name, s16, flop);
    double slow16 = 0.0, fast32 = 1e30, m32[7], m16[7];
    for (int r = 0; r < rounds; ++r) {
        slow16 = std::max(slow16, s16[r].ms); fast32 = std::min(fast32, s32[r].ms);
        m32[r] = s32[r].ms; m16[r] = s16[r].ms;
    }
    std::sort(m32, m32 + rounds); std::sort(m16, m16 + rounds);
    *gate = slow16 < fast32;
    printf("%s: median wall ratio 32x32x16 / 16x16x32 = %.4f; slowest 16x16x32 round %.4f ms, fastest 32x32x16 round %.4f ms -> ranges %s\n", dt,
           m32[rounds / 2] / m16[rounds / 2], slow16, fast32, *gate ? "do not overlap, 16x16x32 faster" : "overlap or 16x16x32 slower");
    CK(hipFree(src));
    return 0;
}

template <bool BF>
static int order(const char* dt) {
    for (int K : {768, 3072}) {
        std::vector<uint16_t> hw((size_t)32 * K), ha((size_t)32 * K);
        for (auto& x : hw) x = to16(urand(), BF);
        for (auto& x : ha) x = to16(urand(), BF);
        uint16_t *w, *a;
        float* c;
        CK(hipMalloc(&w, hw.size() * 2)); CK(hipMalloc(&a, ha.size() * 2)); CK(hipMalloc(&c, 2 * 1024 * sizeof(float)));
        CK(hipMemcpy(w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
        CK(hipMemcpy(a, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
        order_kernel<BF, 32><<<1, 64>>>(w, a, c, K);
        order_kernel<BF, 16><<<1, 64>>>(w, a, c + 1024, K);
        CK(hipDeviceSynchronize());
        std::vector<float> h(2048);
        CK(hipMemcpy(h.data(), c, 2048 * sizeof(float), hipMemcpyDeviceToHost));
        int diff = 0;
        double maxrel = 0.0, maxerr32 = 0.0, maxerr16 = 0.0;
        for (int n = 0; n < 32; ++n)
            for (int m = 0; m < 32; ++m) {
                double ref = 0.0;                       // float64 reference: a wrong operand map shows as an error of order one
                for (int k = 0; k < K; ++k) {
                    auto val = [&](uint16_t b) {
                        if (BF) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return (double)f; }
                        _Float16 hh; memcpy(&hh, &b, 2); return (double)hh;
                    };
                    ref += val(hw[(size_t)n * K + k]) * val(ha[(size_t)m * K + k]);
                }
                const float x = h[n * 32 + m], y = h[1024 + n * 32 + m];
                if (memcmp(&x, &y, 4) != 0) {
                    ++diff;
                    maxrel = std::max(maxrel, std::fabs((double)x - (double)y) / std::max(1e-30, std::fabs(ref)));
                }
                maxerr32 = std::max(maxerr32, std::fabs(x - ref));
                maxerr16 = std::max(maxerr16, std::fabs(y - ref));
            }
        printf("%s K = %4d: %4d of 1024 accumulators differ bitwise between the shapes (largest |difference| / |exact| %.3g); "
               "max |error| against float64: 32x32x16 %.3g, 16x16x32 %.3g\n", dt, K, diff, maxrel, maxerr32, maxerr16);
        CK(hipFree(w)); CK(hipFree(a)); CK(hipFree(c));
    }
    return 0;
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 6000;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int blocks = prop.multiProcessorCount;
    printf("%s, %d CUs, %d iterations of one 256 x 256 x 64 K-tile per workgroup and launch, 7 alternating rounds, >= 2 s of launches before each sample\n",
           prop.name, blocks, iters);
    float* sink;
    long long* stamps;
    CK(hipMalloc(&sink, (size_t)blocks * 512 * sizeof(float)));
    CK(hipMalloc(&stamps, (size_t)blocks * 2 * sizeof(long long)));
    if (order<false>("f16") || order<true>("bf16")) return 1;
    fflush(stdout);
    bool g16 = false, gbf = false;
    if (timing<false>("f16", blocks, iters, sink, stamps, &g16)) return 1;
    if (timing<true>("bf16", blocks, iters, sink, stamps, &gbf)) return 1;
    printf("gate (f16: slowest 16x16x32 round faster than fastest 32x32x16 round): %s\n", g16 ? "MET" : "NOT MET");
    return 0;
}
