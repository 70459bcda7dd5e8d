// Library-level entry points of the C ABI: error text, device info, K1 wrappers.
#include <cstdarg>
#include <cstdio>
#include <cstdio>
#include <climits>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <vector>
#include <zlib.h>
#include <cmath>
#include "kernel_util.h"
#include "gemm_epilogue.h"

namespace ap {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap_;
    va_start(ap_, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap_);
    va_end(ap_);
}

// The zero row of ap_gemm_split_f16_windows mode 1: zero-initialised memory of the code object itself, which the loader
// fills when it places the object on a device.  No first call has anything to allocate, to zero on some stream or to publish,
// so no call on another stream or thread can find it half made.
constexpr int kZeroFloats = 16384;
__attribute__((used)) __device__ float g_zero_row[kZeroFloats];

}  // namespace ap

extern "C" {

int ap_abi_version(void) { return AP_ABI_VERSION; }

const char* ap_last_error(void) { return ap::g_error; }

int ap_device_info(int device, char* name, int name_cap, int* cu_count, size_t* hbm_bytes) {
    hipDeviceProp_t prop;
    AP_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (name && name_cap > 0) {
        snprintf(name, (size_t)name_cap, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return AP_OK;
}

int ap_preproc_u8hwc_to_chw(const uint8_t* src, int n, int h, int w, int crop_top, int crop_left,
                            int oh, int ow, const float mean[3], const float stdv[3], void* dst,
                            int dst_dtype, ap_stream_t stream) {
    return ap::preproc_chw(src, n, h, w, crop_top, crop_left, oh, ow, mean, stdv, dst, dst_dtype,
                           (hipStream_t)stream);
}

int ap_preproc_u8hwc_to_chw_any(const uint8_t* src, int n, int h, int w, int crop_top, int crop_left,
                                int oh, int ow, const float mean[3], const float stdv[3], void* dst,
                                int dst_dtype, ap_stream_t stream) {
    return ap::preproc_chw_any(src, n, h, w, crop_top, crop_left, oh, ow, mean, stdv, dst, dst_dtype,
                               (hipStream_t)stream);
}

int ap_preproc_u8hwc_to_patchrows(const uint8_t* src, int n, int h, int w, int crop_top,
                                  int crop_left, int oh, int ow, int ps, const float mean[3],
                                  const float stdv[3], void* dst, int ld, int dst_dtype,
                                  ap_stream_t stream) {
    return ap::preproc_patchrows(src, n, h, w, crop_top, crop_left, oh, ow, ps, mean, stdv, dst, ld,
                                 dst_dtype, (hipStream_t)stream);
}

int ap_host_gather_tiles(void* dst, const void* const* src, int n, size_t bytes_each) {
    AP_REQUIRE(dst && (src || n == 0) && n >= 0, "ap_host_gather_tiles: bad arguments");
    char* d = (char*)dst;
    for (int i = 0; i < n; ++i) {
        AP_REQUIRE(src[i], "ap_host_gather_tiles: null tile %d", i);
        memcpy(d + (size_t)i * bytes_each, src[i], bytes_each);
    }
    return AP_OK;
}

int ap_host_format_passports(const int32_t* coords, int n, const char* prefix, const char* suffix, char* out, int width) {
    AP_REQUIRE((coords || n == 0) && prefix && suffix && out && n >= 0 && width > 0, "ap_host_format_passports: bad arguments");
    const size_t plen = strlen(prefix), slen = strlen(suffix);
    std::vector<char> line(plen + slen + 128);
    memcpy(line.data(), prefix, plen);
    for (int i = 0; i < n; ++i) {
        const int32_t* c = coords + (size_t)i * 5;
        char* p = line.data() + plen;
        // "__x{X}_y{Y}_rw{RW}_rh{RH}_lv{LV}": decimal int32 fields, '-' for negatives (Python's str(int))
        static const char* const tags[5] = {"__x", "_y", "_rw", "_rh", "_lv"};
        for (int f = 0; f < 5; ++f) {
            for (const char* t = tags[f]; *t; ++t) *p++ = *t;
            uint32_t v = (uint32_t)c[f];
            if (c[f] < 0) { *p++ = '-'; v = 0u - v; }
            char digits[12];
            int nd = 0;
            do { const uint32_t q = v / 10u; digits[nd++] = (char)('0' + (v - q * 10u)); v = q; } while (v);
            while (nd) *p++ = digits[--nd];
        }
        memcpy(p, suffix, slen);
        const size_t len = (size_t)(p - line.data()) + slen;
        char* o = out + (size_t)i * width;
        const size_t take = len < (size_t)width ? len : (size_t)width;      // NumPy's S<width> truncates longer strings
        memcpy(o, line.data(), take);
        memset(o + take, 0, (size_t)width - take);                           // ... and pads shorter ones with NUL
    }
    return AP_OK;
}

int ap_host_inflate_tiles(void* dst, const char* const* paths, int n, size_t bytes_each) {
    AP_REQUIRE(dst && (paths || n == 0) && n >= 0 && bytes_each > 0, "ap_host_inflate_tiles: bad arguments");
    std::vector<unsigned char> buf;
    for (int i = 0; i < n; ++i) {
        AP_REQUIRE(paths[i], "ap_host_inflate_tiles: null path %d", i);
        FILE* f = fopen(paths[i], "rb");
        AP_REQUIRE(f, "ap_host_inflate_tiles: cannot open %s", paths[i]);
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        buf.resize(size > 0 ? (size_t)size : 1);
        const size_t got = size > 0 ? fread(buf.data(), 1, (size_t)size, f) : 0;
        fclose(f);
        AP_REQUIRE(size > 0 && got == (size_t)size, "ap_host_inflate_tiles: short read of %s", paths[i]);
        uLongf len = (uLongf)bytes_each;
        const int zr = uncompress((Bytef*)dst + (size_t)i * bytes_each, &len, buf.data(), (uLong)size);
        AP_REQUIRE(zr == Z_OK && len == bytes_each, "ap_host_inflate_tiles: %s does not inflate to %zu bytes (zlib %d)",
                   paths[i], bytes_each, zr);
    }
    return AP_OK;
}

int ap_host_synth_tiles(void* dst, const int32_t* xy, int n, int side, int level_ds, int level, int64_t width,
                        int64_t height, uint32_t seed, const int64_t* ellipses, int k) {
    AP_REQUIRE(dst && (xy || n == 0) && (ellipses || k == 0) && n >= 0 && side > 0 && level_ds > 0 && k >= 0,
               "ap_host_synth_tiles: bad arguments");
    auto mix = [](uint32_t a) { a ^= a >> 16; a *= 0x7FEB352Du; a ^= a >> 15; a *= 0x846CA68Bu; a ^= a >> 16; return a; };
    uint8_t* o = (uint8_t*)dst;
    for (int t = 0; t < n; ++t) {
        for (int py = 0; py < side; ++py) {
            const long long gy = (long long)xy[2 * t + 1] + (long long)py * level_ds, uy = gy >> 4;
            long long last_ux = INT64_MIN;
            bool tissue = false;
            for (int px = 0; px < side; ++px, o += 3) {
                const long long gx = (long long)xy[2 * t] + (long long)px * level_ds, ux = gx >> 4;
                if (gx < 0 || gy < 0 || gx >= width || gy >= height) { o[0] = o[1] = o[2] = 0; continue; }
                if (ux != last_ux) {           // the ellipse test lives on a 16-pixel lattice: once per lattice cell
                    last_ux = ux;
                    tissue = false;
                    for (int e = 0; e < k && !tissue; ++e) {
                        const long long a = ellipses[4 * e + 2], b = ellipses[4 * e + 3];
                        const long long dx = (ux - ellipses[4 * e]) * b, dy = (uy - ellipses[4 * e + 1]) * a, ab = a * b;
                        tissue = dx * dx + dy * dy <= ab * ab;
                    }
                }
                const uint32_t h = mix((uint32_t)gx * 0x9E3779B1u + (uint32_t)gy * 0x85EBCA77u + seed + (uint32_t)level * 0xC2B2AE3Du);
                const int n0 = h & 0xFF, n1 = (h >> 8) & 0xFF, n2 = (h >> 16) & 0xFF, bg = 236 + (n0 & 7);
                o[0] = (uint8_t)(tissue ? 168 + (n0 >> 2) : bg);
                o[1] = (uint8_t)(tissue ? 72 + (n1 >> 1) : bg);
                o[2] = (uint8_t)(tissue ? 136 + (n2 >> 2) : bg);
            }
        }
    }
    return AP_OK;
}

int ap_tile_content_counts(const uint8_t* tiles, int n, int h, int w, int black_thresh, int white_sat_thresh,
                           int white_value_thresh, uint32_t* counts, ap_stream_t stream) {
    return ap::tile_content_counts(tiles, n, h, w, black_thresh, white_sat_thresh, white_value_thresh,
                                   (unsigned*)counts, (hipStream_t)stream);
}

using ap::aligned16;
using ap::half_dtype;
using ap::known_dtype;
static inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// The layout rule of ap_gemm / ap_gemm_fused (include/atlaspatch_hip.h states it): what the two MFMA kernels assume of a call
// without checking it.  LDS-DMA stages 16 bytes per lane from A and W; a lane stores four consecutive columns (the 256 x 256
// kernel: 16 bytes), reads bias / gamma / colsum as float4 and the row statistics of a row pair as 16 bytes, and writes the partial
// sums as float2.
static int gemm_contract(const char* fn, int dtype, int epilogue, const ap::GemmArgs& g, int impl) {
    const size_t es = ap::dtype_size(dtype), oes = epilogue == ap::EPI_BIAS_RESID ? 4 : es;
    const int kt = 128 / (int)es, ocols = epilogue == ap::EPI_NORM_SWIGLU ? g.N / 2 : g.N;
    const int nt = g.split ? 32 : 128;       // the split-f16 form (impl 129) masks the 128-wide tile's tail
    AP_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0, "%s: empty problem %d x %d x %d", fn, g.M, g.N, g.K);
    AP_REQUIRE(g.N % nt == 0 && g.K % kt == 0, "%s: N = %d must be a multiple of %d and K = %d of %d", fn, g.N, nt, g.K, kt);
    AP_REQUIRE(g.lda >= g.K && g.ldw >= g.K && g.ldo >= ocols, "%s: row strides (lda %d, ldw %d, ldo %d) smaller than the rows (K = %d, %d output columns)",
               fn, g.lda, g.ldw, g.ldo, g.K, ocols);
    AP_REQUIRE(((size_t)g.lda * es) % 16 == 0 && ((size_t)g.ldw * es) % 16 == 0 && aligned16(g.A, g.W),
               "%s: A and W need 16-byte aligned pointers and row strides", fn);
    AP_REQUIRE(g.ldo % 4 == 0 && ((uintptr_t)g.out % (4 * oes)) == 0, "%s: out needs ldo %% 4 == 0 and a pointer aligned to four elements (%zu bytes)",
               fn, 4 * oes);
    AP_REQUIRE(aligned16(g.bias, g.gamma, g.colsum, g.rowstats) && aligned8(g.partial),
               "%s: bias / gamma / colsum / rowstats need 16-byte aligned pointers, partial an 8-byte aligned one", fn);
    AP_REQUIRE((impl != 256 && impl != 257) || ap::gemm256_supports(dtype, epilogue, g),
               "%s: impl %d (the 256 x 256 kernel) takes f16 / bf16, N %% 256 == 0, K %% 128 == 0, K >= 128, 16-byte aligned output rows, 255 rows of A / W below 4 GiB, "
               "M <= 2^29 under the NORM epilogues", fn, impl);
    return AP_OK;
}

int ap_gemm(int dtype, int epilogue, const void* A, int lda, const void* W, int ldw, int M, int N,
            int K, const float* bias, const float* gamma, void* out, int ldo, int impl, int variant,
            ap_stream_t stream) {
    AP_REQUIRE(A && W && bias && out, "ap_gemm: null pointer");
    static_assert(AP_EPI_BIAS == ap::EPI_BIAS_STORE && AP_EPI_BIAS_GELU == ap::EPI_BIAS_GELU && AP_EPI_BIAS_RESID == ap::EPI_BIAS_RESID &&
                  AP_EPI_BIAS_QUICK_GELU == ap::EPI_BIAS_QGELU && AP_EPI_BIAS_GELU_TANH == ap::EPI_BIAS_GTANH, "AP_EPI_* are the GemmEpilogue codes");
    AP_REQUIRE(ap::epi_known(epilogue) && !ap::epi_is_norm(epilogue) && !ap::epi_is_resid(epilogue) && epilogue != ap::EPI_PATCH_EMBED,
               "ap_gemm: unknown epilogue %d", epilogue);
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16 || dtype == AP_F32, "ap_gemm: unknown dtype %d", dtype);
    AP_REQUIRE(impl == 0 || impl == 128 || impl == 129 || impl == 256 || impl == 257,
               "ap_gemm: impl %d (0 = pick, 128, 129 = split-f16 products, 256; 257 = the A/B twin)", impl);
    ap::GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = M; g.N = N; g.K = K;
    g.bias = bias; g.gamma = gamma; g.out = out; g.ldo = ldo;
    if (impl == 129) {                       // float32 buffers, split-f16 products: W = the rows ap_split_f16_weights made
        AP_REQUIRE(dtype == AP_F32, "ap_gemm: impl 129 (split-f16 products) takes float32 buffers");
        g.split = 1;
        impl = 128;
    }
    if (const int rc = gemm_contract("ap_gemm", dtype, epilogue, g, impl); rc != AP_OK) return rc;
    return ap::launch_gemm_impl(dtype, epilogue, g, impl, variant, (hipStream_t)stream);
}

int ap_split_f16_weights(const float* w32, void* out, size_t count, ap_stream_t stream) {
    return ap::launch_split_f16_weights(w32, out, count, (hipStream_t)stream);
}

static int gemm_split_f16(const float* A, int lda, const void* w_split, int M, int N, int K, const float* bias, int act,
                          const float* resid, int ldr, float* out, int ldo, int win_mode, int b, int h, int w, int ws, ap_stream_t stream) {
    AP_REQUIRE(A && w_split && out, "ap_gemm_split_f16: null pointer");
    AP_REQUIRE(act == 0 || act == 1, "ap_gemm_split_f16: act %d (0 none, 1 GELU)", act);
    AP_REQUIRE(M > 0 && N > 0 && N % 32 == 0 && K > 0 && K % 32 == 0, "ap_gemm_split_f16: %d x %d x %d (N and K multiples of 32)", M, N, K);
    AP_REQUIRE(lda >= K && lda % 4 == 0 && ldo >= N && ldo % 4 == 0 && (!resid || (ldr >= N && ldr % 4 == 0)), "ap_gemm_split_f16: strides");
    AP_REQUIRE(aligned16(A, w_split, out, resid, bias), "ap_gemm_split_f16: 16-byte aligned pointers");
    ap::GemmArgs g{};
    g.A = A; g.lda = lda; g.W = w_split; g.ldw = K; g.M = M; g.N = N; g.K = K;
    g.bias = bias; g.out = out; g.ldo = ldo; g.resid = resid; g.ldr = ldr; g.split = 1;
    if (win_mode != 0) {
        AP_REQUIRE((win_mode == 1 || win_mode == 2) && b > 0 && h > 0 && w > 0 && ws > 0, "ap_gemm_split_f16_windows: mode %d, %d x %d x %d, window %d", win_mode, b, h, w, ws);
        g.win_mode = win_mode; g.win_ws = ws; g.win_H = h; g.win_W = w; g.win_nwy = (h + ws - 1) / ws; g.win_nwx = (w + ws - 1) / ws;
        AP_REQUIRE((long)b * g.win_nwy * g.win_nwx * ws * ws == (long)M, "ap_gemm_split_f16_windows: M = %d is not %d images x %d x %d windows of %d x %d", M, b,
                   g.win_nwy, g.win_nwx, ws, ws);
        if (win_mode == 1) {
            // padding rows of the gathered operand: ap::g_zero_row, one copy per device.  Every thread and every stream reads the
            // same row, and it is complete before anyone can ask for it; only its address is looked up once per device (the
            // predictor's warm-up forward comes before any stream capture).
            static std::mutex zero_mu;
            static float* zero_rows[64] = {};
            int dev = 0;
            AP_HIP_CHECK(hipGetDevice(&dev));
            AP_REQUIRE(dev >= 0 && dev < 64 && K <= ap::kZeroFloats, "ap_gemm_split_f16_windows: device %d / K %d", dev, K);
            {
                std::lock_guard<std::mutex> lock(zero_mu);
                if (!zero_rows[dev]) {
                    void* row = nullptr;
                    AP_HIP_CHECK(hipGetSymbolAddress(&row, HIP_SYMBOL(ap::g_zero_row)));
                    zero_rows[dev] = (float*)row;
                }
                g.zero_row = zero_rows[dev];
            }
        }
    }
    return ap::launch_gemm_impl(AP_F32, act == 1 ? ap::EPI_BIAS_GELU : ap::EPI_BIAS_STORE, g, 128, 0, (hipStream_t)stream);
}

int ap_gemm_split_f16(const float* A, int lda, const void* w_split, int M, int N, int K, const float* bias, int act,
                      const float* resid, int ldr, float* out, int ldo, ap_stream_t stream) {
    return gemm_split_f16(A, lda, w_split, M, N, K, bias, act, resid, ldr, out, ldo, 0, 0, 0, 0, 0, stream);
}

int ap_gemm_split_f16_windows(const float* A, int lda, const void* w_split, int M, int N, int K, const float* bias, int act,
                              const float* resid, int ldr, float* out, int ldo, int win_mode, int b, int h, int w, int ws,
                              ap_stream_t stream) {
    return gemm_split_f16(A, lda, w_split, M, N, K, bias, act, resid, ldr, out, ldo, win_mode, b, h, w, ws, stream);
}

int ap_gemm_fused(int dtype, int epilogue, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
                  const float* bias, const float* colsum, const float* rowstats, float* partial, void* out, int ldo,
                  int impl, ap_stream_t stream) {
    AP_REQUIRE(A && W && bias && out, "ap_gemm_fused: null pointer");
    AP_REQUIRE(dtype == AP_F16 || dtype == AP_BF16, "ap_gemm_fused: f16 / bf16 only");
    static_assert(AP_EPI_NORM == ap::EPI_NORM_STORE && AP_EPI_NORM_GELU == ap::EPI_NORM_GELU && AP_EPI_NORM_SWIGLU == ap::EPI_NORM_SWIGLU &&
                  AP_EPI_NORM_QUICK_GELU == ap::EPI_NORM_QGELU && AP_EPI_NORM_GELU_TANH == ap::EPI_NORM_GTANH &&
                  AP_EPI_RESID_STATS == ap::EPI_RESID_STATS, "AP_EPI_* are the GemmEpilogue codes");
    AP_REQUIRE(ap::epi_is_norm(epilogue) || epilogue == ap::EPI_RESID_STATS, "ap_gemm_fused: unknown epilogue %d", epilogue);
    ap::GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = M; g.N = N; g.K = K;
    g.bias = bias; g.colsum = colsum; g.rowstats = rowstats; g.partial = partial; g.out = out; g.ldo = ldo;
    AP_REQUIRE(ap::epi_operands_ok(epilogue, g), "ap_gemm_fused: missing operand for epilogue %d", epilogue);
    const int variant = (int)((unsigned)impl >> 12);      // bits 12..: kernel tuning variant (tools only), low 12 bits: implementation
    impl &= 0xfff;
    AP_REQUIRE(impl == 0 || impl == 128 || impl == 256 || impl == 257, "ap_gemm_fused: impl %d (0 = pick, 128, 256; 257 = the A/B twin)", impl);
    if (const int rc = gemm_contract("ap_gemm_fused", dtype, epilogue, g, impl); rc != AP_OK) return rc;
    return ap::launch_gemm_impl(dtype, epilogue, g, impl, variant, (hipStream_t)stream);
}

int ap_stream_init(int dtype, const float* tok, int rows, int dim, float eps, void* x, float* rowstats, ap_stream_t stream) {
    AP_REQUIRE(tok && x && rowstats, "ap_stream_init: null pointer");
    return ap::launch_stream_init(dtype, tok, rows, dim, eps, x, rowstats, (hipStream_t)stream);
}

int ap_rowstats_finalize(const float* partial, int rows, int groups, int dim, float eps, float* rowstats, ap_stream_t stream) {
    AP_REQUIRE(partial && rowstats && groups > 0 && dim > 0, "ap_rowstats_finalize: bad arguments");
    return ap::launch_rowstats_finalize(partial, rows, groups, dim, eps, rowstats, (hipStream_t)stream);
}

int ap_gemm_trace(long long* device_buf, int tiles_per_workgroup) {
    ap::set_gemm_trace(device_buf, device_buf ? tiles_per_workgroup : 0);
    return AP_OK;
}

int ap_layernorm(int out_dtype, const float* x, long stride, int rows, int dim, const float* gamma,
                 const float* beta, float eps, void* out, ap_stream_t stream) {
    AP_REQUIRE(x && gamma && beta && out, "ap_layernorm: null pointer");
    return ap::launch_layernorm(out_dtype, x, stride, rows, dim, gamma, beta, eps, out, (hipStream_t)stream);
}

// What ap_attention and ap_attention_scaled refuse before anything is launched: the launchers assume all of it.  Both kernels
// move 16 bytes per lane (LDS-DMA and fragment loads of q / k / v, row-wise stores of out; the float32 strip kernel's widest
// access is one f32x4), and every row and head offset is a multiple of 16 bytes, so 16-byte alignment of the two pointers
// is the whole rule, in float32 as well.
static int attention_args_ok(const char* who, int dtype, const void* qkv, const void* out, int n, int tokens, int heads, int head_dim) {
    AP_REQUIRE(qkv && out, "%s: null pointer", who);
    AP_REQUIRE(known_dtype(dtype), "%s: unknown dtype %d", who, dtype);
    AP_REQUIRE(n >= 0 && tokens > 0 && heads > 0, "%s: bad shape (n %d, %d tokens, %d heads)", who, n, tokens, heads);
    AP_REQUIRE(head_dim == 64 || ((head_dim == 96 || head_dim == 128) && dtype != AP_F32),
               "%s: head_dim %d unsupported (64; 96 / 128 in f16 / bf16)", who, head_dim);
    AP_REQUIRE(aligned16(qkv, out), "%s: qkv / out must be 16-byte aligned", who);
    // the tiled kernel addresses a key row by a 32-bit byte offset inside its image
    AP_REQUIRE(dtype == AP_F32 || (size_t)tokens * 3 * heads * head_dim * 2 < 0xffffffffull,
               "%s: %d tokens x %d heads x %d: an image's qkv rows exceed 4 GiB", who, tokens, heads, head_dim);
    return AP_OK;
}

int ap_attention(int dtype, const void* qkv, void* out, int n, int tokens, int heads, int head_dim,
                 ap_stream_t stream) {
    if (int rc = attention_args_ok("ap_attention", dtype, qkv, out, n, tokens, heads, head_dim)) return rc;
    return ap::launch_attention(dtype, qkv, out, n, tokens, heads, head_dim, 1.0f / sqrtf((float)head_dim), (hipStream_t)stream);
}

// ---- engine building blocks: the kernels vit.cpp chains, one export each.  Every wrapper checks what its launcher assumes
// without checking (a refusal launches nothing) and forwards; the launchers' own checks follow.
int ap_attention_scaled(int dtype, const void* qkv, void* out, int n, int tokens, int heads, int head_dim, float scale,
                        ap_stream_t stream) {
    if (int rc = attention_args_ok("ap_attention_scaled", dtype, qkv, out, n, tokens, heads, head_dim)) return rc;
    AP_REQUIRE(std::isfinite(scale) && scale > 0.f, "ap_attention_scaled: scale must be positive and finite");
    return ap::launch_attention(dtype, qkv, out, n, tokens, heads, head_dim, scale, (hipStream_t)stream);
}

int ap_attention_cls(int dtype, const void* q, const void* kv, int ld, int koff, int voff, void* out, int n, int tokens,
                     int heads, int head_dim, float scale, ap_stream_t stream) {
    AP_REQUIRE(q && kv && out, "ap_attention_cls: null pointer");
    AP_REQUIRE(known_dtype(dtype), "ap_attention_cls: unknown dtype %d", dtype);
    AP_REQUIRE(head_dim == 64 || head_dim == 96 || head_dim == 128, "ap_attention_cls: head_dim %d unsupported (64 / 96 / 128)", head_dim);
    AP_REQUIRE(n >= 0 && heads > 0 && heads <= (1 << 16), "ap_attention_cls: bad shape (n %d, %d heads)", n, heads);
    AP_REQUIRE(tokens > 0 && tokens <= 12000, "ap_attention_cls: %d tokens unsupported (1 .. 12000)", tokens);
    const long width = (long)heads * head_dim;
    AP_REQUIRE(ld > 0 && ld % 8 == 0 && koff >= 0 && voff >= 0 && koff % 8 == 0 && voff % 8 == 0 && koff + width <= ld && voff + width <= ld,
               "ap_attention_cls: k / v (offsets %d / %d, %ld wide) must lie inside rows of %d elements, all multiples of 8", koff, voff, width, ld);
    AP_REQUIRE(aligned16(q, kv) && (dtype != AP_F32 || (((uintptr_t)q | (uintptr_t)kv) & 31) == 0),
               "ap_attention_cls: q / kv must be aligned to 8 elements");
    AP_REQUIRE(std::isfinite(scale), "ap_attention_cls: scale must be finite");
    return ap::launch_attention_cls(dtype, q, kv, ld, koff, voff, out, n, tokens, heads, head_dim, scale, (hipStream_t)stream);
}

int ap_attention_probe(int dtype, const float* q, const void* kv, int ld, int koff, int voff, void* out, int n, int tokens,
                       int heads, int head_dim, float scale, ap_stream_t stream) {
    AP_REQUIRE(q && kv && out, "ap_attention_probe: null pointer");
    AP_REQUIRE(known_dtype(dtype), "ap_attention_probe: unknown dtype %d", dtype);
    AP_REQUIRE(head_dim == 64 || head_dim == 96 || head_dim == 128, "ap_attention_probe: head_dim %d unsupported (64 / 96 / 128)", head_dim);
    AP_REQUIRE(n >= 0 && heads > 0 && heads <= (1 << 16), "ap_attention_probe: bad shape (n %d, %d heads)", n, heads);
    AP_REQUIRE(tokens > 0 && tokens <= 12000, "ap_attention_probe: %d tokens unsupported (1 .. 12000)", tokens);
    const long width = (long)heads * head_dim;
    AP_REQUIRE(ld > 0 && ld % 8 == 0 && koff >= 0 && voff >= 0 && koff % 8 == 0 && voff % 8 == 0 && koff + width <= ld && voff + width <= ld,
               "ap_attention_probe: k / v (offsets %d / %d, %ld wide) must lie inside rows of %d elements, all multiples of 8", koff, voff, width, ld);
    AP_REQUIRE(aligned16(q, kv) && (dtype != AP_F32 || ((uintptr_t)kv & 31) == 0),
               "ap_attention_probe: q must be 16-byte aligned and kv aligned to 8 elements");
    AP_REQUIRE(std::isfinite(scale), "ap_attention_probe: scale must be finite");
    return ap::launch_attention_probe(dtype, q, kv, ld, koff, voff, out, n, tokens, heads, head_dim, scale, (hipStream_t)stream);
}

int ap_attn_pool(int dtype, const void* kv, const float* q, void* out, int n, int tokens, int heads, ap_stream_t stream) {
    AP_REQUIRE(kv && q && out, "ap_attn_pool: null pointer");
    AP_REQUIRE(half_dtype(dtype), "ap_attn_pool: dtype %d (f16 / bf16 only)", dtype);
    AP_REQUIRE(n >= 0 && heads > 0 && heads <= (1 << 16), "ap_attn_pool: bad shape (n %d, %d heads)", n, heads);
    AP_REQUIRE(tokens > 0 && tokens <= 12000, "ap_attn_pool: %d tokens unsupported (1 .. 12000)", tokens);
    AP_REQUIRE(aligned16(kv), "ap_attn_pool: kv must be 16-byte aligned");
    return ap::launch_attn_pool(dtype, kv, q, out, n, tokens, heads, (hipStream_t)stream);
}

int ap_rope(int dtype, void* qkv, int n, int tokens, int prefix, int heads, int head_dim, const float* cos, const float* sin,
            int which, ap_stream_t stream) {
    AP_REQUIRE(qkv && cos && sin, "ap_rope: null pointer");
    AP_REQUIRE(known_dtype(dtype), "ap_rope: unknown dtype %d", dtype);
    AP_REQUIRE(n >= 0 && heads > 0 && prefix >= 0 && tokens > prefix, "ap_rope: bad shape (n %d, %d tokens, prefix %d, %d heads)", n, tokens,
               prefix, heads);
    AP_REQUIRE(head_dim > 0 && head_dim % 16 == 0, "ap_rope: head_dim %d must be a positive multiple of 16", head_dim);
    AP_REQUIRE(which >= 1 && which <= 3, "ap_rope: which %d (1 = q, 2 = k, 3 = both)", which);
    AP_REQUIRE(aligned16(qkv), "ap_rope: qkv must be 16-byte aligned");
    return ap::launch_rope(dtype, qkv, n, tokens, prefix, heads, head_dim, cos, sin, which, (hipStream_t)stream);
}

int ap_swiglu(int dtype, const void* x, int rows, int h, void* out, ap_stream_t stream) {
    AP_REQUIRE(x && out, "ap_swiglu: null pointer");
    AP_REQUIRE(known_dtype(dtype), "ap_swiglu: unknown dtype %d", dtype);
    AP_REQUIRE(rows >= 0 && h > 0 && h % 8 == 0, "ap_swiglu: bad shape (%d rows, h %d: a positive multiple of 8)", rows, h);
    AP_REQUIRE(aligned16(x, out), "ap_swiglu: x / out must be 16-byte aligned");
    return ap::launch_swiglu(dtype, x, rows, h, out, (hipStream_t)stream);
}

int ap_add2_layernorm(int delta_dtype, int out_dtype, float* x, long stride, const void* delta0, long dstride0, const float* ls0,
                      const void* delta1, long dstride1, const float* ls1, int store, int rows, int dim, const float* gamma,
                      const float* beta, float eps, void* out, ap_stream_t stream) {
    AP_REQUIRE(x && gamma && beta && out, "ap_add2_layernorm: null pointer");
    AP_REQUIRE(known_dtype(out_dtype) && ((!delta0 && !delta1) || known_dtype(delta_dtype)), "ap_add2_layernorm: unknown dtype (delta %d, out %d)",
               delta_dtype, out_dtype);
    AP_REQUIRE((!delta0 && !delta1) || delta_dtype == out_dtype || (delta_dtype != AP_F32 && out_dtype == AP_F32),
               "ap_add2_layernorm: unsupported dtype pair (delta %d, out %d): (T, T), (T, f32) or (f32, f32)", delta_dtype, out_dtype);
    AP_REQUIRE(rows >= 0 && dim > 0 && dim % 4 == 0 && dim <= 4096, "ap_add2_layernorm: bad shape (%d rows, dim %d: a multiple of 4 up to 4096)",
               rows, dim);
    AP_REQUIRE(store == 0 || store == 1, "ap_add2_layernorm: store %d (0 / 1)", store);
    // the 16-lane kernel (dim 768 / 1024) reads a 16-bit branch output eight elements at a time
    const long dmul = (dim == 768 || dim == 1024) && delta_dtype != AP_F32 ? 8 : 4;
    AP_REQUIRE(stride >= dim && stride % 4 == 0 && (!delta0 || (dstride0 >= dim && dstride0 % dmul == 0)) &&
                   (!delta1 || (dstride1 >= dim && dstride1 % dmul == 0)),
               "ap_add2_layernorm: row strides must be at least dim and multiples of 4 (16-bit delta at dim 768 / 1024: of 8)");
    AP_REQUIRE(aligned16(x, gamma, beta, out, delta0, delta1, ls0, ls1),
               "ap_add2_layernorm: every buffer must be 16-byte aligned");
    AP_REQUIRE(std::isfinite(eps) && eps >= 0.f, "ap_add2_layernorm: eps must be finite and non-negative");
    return ap::launch_add2_layernorm(delta_dtype, out_dtype, x, stride, delta0, dstride0, ls0, delta1, dstride1, ls1, store, rows, dim, gamma,
                                     beta, eps, out, (hipStream_t)stream);
}

int ap_fold_ln(int dtype, const float* w32, int rows, int cols, int ld, const float* gamma, const float* beta, const float* bias_in,
               void* wout, float* colsum, float* bias_out, int swiglu_h, ap_stream_t stream) {
    AP_REQUIRE(w32 && gamma && beta && bias_in && wout && colsum && bias_out, "ap_fold_ln: null pointer");
    AP_REQUIRE(half_dtype(dtype), "ap_fold_ln: dtype %d (f16 / bf16 only)", dtype);
    AP_REQUIRE(rows > 0 && cols > 0 && cols <= ld, "ap_fold_ln: bad shape (%d rows, %d cols, ld %d)", rows, cols, ld);
    AP_REQUIRE(swiglu_h == 0 || (swiglu_h > 0 && swiglu_h % 32 == 0 && rows == 2 * swiglu_h),
               "ap_fold_ln: swiglu_h %d needs rows = 2 h and h %% 32 == 0", swiglu_h);
    return ap::launch_fold_ln(dtype, w32, rows, cols, ld, gamma, beta, bias_in, wout, colsum, bias_out, (hipStream_t)stream, swiglu_h);
}

int ap_fold_ls(int dtype, const float* w32, int rows, int cols, int ld, const float* ls, const float* bias_in, void* wout,
               float* bias_out, ap_stream_t stream) {
    AP_REQUIRE(w32 && bias_in && wout && bias_out, "ap_fold_ls: null pointer");
    AP_REQUIRE(half_dtype(dtype), "ap_fold_ls: dtype %d (f16 / bf16 only)", dtype);
    AP_REQUIRE(rows > 0 && cols > 0 && cols <= ld, "ap_fold_ls: bad shape (%d rows, %d cols, ld %d)", rows, cols, ld);
    return ap::launch_fold_ls(dtype, w32, rows, cols, ld, ls, bias_in, wout, bias_out, (hipStream_t)stream);
}

int ap_cls_mean_pool(const float* y, int n, int tokens, int prefix, int dim, float* out, ap_stream_t stream) {
    AP_REQUIRE(y && out, "ap_cls_mean_pool: null pointer");
    AP_REQUIRE(n >= 0 && n <= 65535 && prefix >= 1 && tokens > prefix && dim > 0,
               "ap_cls_mean_pool: bad shape (n %d up to 65535, %d tokens, prefix %d, dim %d)", n, tokens, prefix, dim);
    return ap::launch_cls_mean_pool(y, n, tokens, prefix, dim, out, (hipStream_t)stream);
}

int ap_l2_normalize_rows(const float* x, long stride, int rows, int dim, float eps, float* out, ap_stream_t stream) {
    AP_REQUIRE(x && out, "ap_l2_normalize_rows: null pointer");
    AP_REQUIRE(rows >= 0 && dim > 0 && dim % 4 == 0 && stride >= dim && stride % 4 == 0,
               "ap_l2_normalize_rows: bad shape (%d rows, dim %d, stride %ld: multiples of 4, stride >= dim)", rows, dim, stride);
    AP_REQUIRE(aligned16(x, out), "ap_l2_normalize_rows: x and out must be 16-byte aligned");
    AP_REQUIRE(x != out || stride == dim, "ap_l2_normalize_rows: in place (out == x) needs dense rows, stride %ld != dim %d", stride, dim);
    AP_REQUIRE(eps > 0.f && std::isfinite(eps), "ap_l2_normalize_rows: eps must be positive and finite (a zero row is divided by it)");
    return ap::launch_l2_normalize_rows(x, stride, rows, dim, eps, out, (hipStream_t)stream);
}

int ap_stream_to_f32(int dtype, const void* x, long stride, int rows, int dim, float* dst, ap_stream_t stream) {
    AP_REQUIRE(x && dst, "ap_stream_to_f32: null pointer");
    AP_REQUIRE(half_dtype(dtype), "ap_stream_to_f32: dtype %d (f16 / bf16 only)", dtype);
    AP_REQUIRE(rows >= 0 && dim > 0 && dim % 4 == 0 && stride >= dim && stride % 4 == 0,
               "ap_stream_to_f32: bad shape (%d rows, dim %d, stride %ld: multiples of 4, stride >= dim)", rows, dim, stride);
    AP_REQUIRE(aligned16(dst) && ((uintptr_t)x & 7) == 0, "ap_stream_to_f32: x must be 8-byte and dst 16-byte aligned");
    return ap::launch_stream_to_f32(dtype, x, stride, rows, dim, dst, (hipStream_t)stream);
}

int ap_chw_to_patchrows(int x_dtype, int dtype, const void* x, int n, int S, int ps, void* dst, int ld, ap_stream_t stream) {
    AP_REQUIRE(x && dst, "ap_chw_to_patchrows: null pointer");
    AP_REQUIRE(known_dtype(x_dtype) && known_dtype(dtype), "ap_chw_to_patchrows: unknown dtype (input %d, output %d)", x_dtype, dtype);
    AP_REQUIRE(n >= 0 && ps > 0 && ps <= 1024 && S >= ps && S <= 16384 && S % ps == 0, "ap_chw_to_patchrows: image %d / patch %d unsupported", S, ps);
    AP_REQUIRE(ld >= 3 * ps * ps, "ap_chw_to_patchrows: ld %d is narrower than a patch row (%d)", ld, 3 * ps * ps);
    // ps % 4 == 0 takes the kernel that stores four elements at a time
    AP_REQUIRE(ps % 4 != 0 || (ld % 4 == 0 && aligned16(dst)), "ap_chw_to_patchrows: ld %d must be a multiple of 4 and dst 16-byte aligned", ld);
    return ap::launch_chw_to_patchrows(x_dtype, dtype, x, n, S, ps, dst, ld, (hipStream_t)stream);
}

int ap_cls_stream(int dtype, const float* prefix, int prefix_rows, int img_rows, int n, int tokens, int dim, void* x, float* partial,
                  ap_stream_t stream) {
    AP_REQUIRE(prefix && x && partial, "ap_cls_stream: null pointer");
    AP_REQUIRE(half_dtype(dtype), "ap_cls_stream: dtype %d (f16 / bf16 only)", dtype);
    AP_REQUIRE(dim > 0 && dim % 64 == 0, "ap_cls_stream: dim %d must be a positive multiple of 64", dim);
    AP_REQUIRE(prefix_rows > 0 && (img_rows == 0 || img_rows == prefix_rows), "ap_cls_stream: img_rows %d must be 0 or prefix_rows (%d > 0)",
               img_rows, prefix_rows);
    AP_REQUIRE(n >= 0 && tokens >= prefix_rows && (long)n * prefix_rows <= INT_MAX, "ap_cls_stream: bad shape (n %d, %d tokens, %d prefix rows)", n,
               tokens, prefix_rows);
    return ap::launch_cls_stream(dtype, prefix, prefix_rows, img_rows, n, tokens, dim, x, partial, (hipStream_t)stream);
}

int ap_cls_exact_update(int dtype, float* cls32, const float* branch, int n, int tokens, int dim, void* x, float* partial,
                        ap_stream_t stream) {
    AP_REQUIRE(cls32 && branch && x && partial, "ap_cls_exact_update: null pointer");
    AP_REQUIRE(half_dtype(dtype), "ap_cls_exact_update: dtype %d (f16 / bf16 only)", dtype);
    AP_REQUIRE(dim > 0 && dim % 64 == 0, "ap_cls_exact_update: dim %d must be a positive multiple of 64", dim);
    AP_REQUIRE(n >= 0 && tokens > 0, "ap_cls_exact_update: bad shape (n %d, %d tokens)", n, tokens);
    return ap::launch_cls_exact_update(dtype, cls32, branch, n, tokens, dim, x, partial, (hipStream_t)stream);
}

int ap_rowstats_finalize_cls(const float* partial, int rows, int groups, int dim, float eps, float* rowstats, int dtype, float* cls32,
                             const float* branch, void* x, int n, int tokens, ap_stream_t stream) {
    AP_REQUIRE(partial && rowstats, "ap_rowstats_finalize_cls: null pointer");
    AP_REQUIRE(rows >= 0 && dim > 0 && dim % 128 == 0 && groups == dim / 64,
               "ap_rowstats_finalize_cls: bad shape (%d rows, dim %d: a multiple of 128, groups %d = dim / 64)", rows, dim, groups);
    AP_REQUIRE(aligned16(partial), "ap_rowstats_finalize_cls: partial must be 16-byte aligned");
    AP_REQUIRE(!cls32 || (half_dtype(dtype) && branch && x && n > 0 && tokens > 0 && (long)n * tokens == rows),
               "ap_rowstats_finalize_cls: exact class rows need f16 / bf16, the branch buffer, the stream and rows == n * tokens");
    return ap::launch_rowstats_finalize_cls(partial, rows, groups, dim, eps, rowstats, dtype, cls32, branch, x, n, tokens, (hipStream_t)stream);
}

}  // extern "C"
