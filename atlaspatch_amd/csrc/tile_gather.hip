// ap_gather_patches: assemble patches that do not sit on the tile grid from decoded tiles (include/atlaspatch_hip.h).
//
//   out[p][r][c] = (r < vh && c < vw && slot >= 0) ? tiles[slot][(oy + r) % ts][(ox + c) % ts] : 0
//                  with slot = plan[p][4 + ((oy + r) / ts) * G + (ox + c) / ts]
//
// A pure byte mover: its floor is HBM, read plus write.  One lane forms 16 consecutive output bytes of one patch and stores
// them with one 16-byte store.  A patch row starts at byte 3 * ox of a tile row, so the source of those 16 bytes sits at any
// byte phase: the lane reads the five aligned dwords that cover it -- one 16-byte load at dword alignment plus one dword -- and
// funnels each output dword out of two neighbours with v_alignbyte_b32.  Neighbouring lanes read neighbouring 16-byte pieces
// of the same tile row, so a wave's loads cover ~1 KiB of consecutive bytes.  16 output bytes that span a tile border, a row
// end, the clip edge (vw / vh) or a missing tile are built from SEGMENTS: each segment is read as if the whole 16 bytes came
// from its tile (the dword indices clamped into the tile buffer, so nothing outside it is touched) and only its bytes are
// merged.  With 256-pixel patches and tiles one piece in 48 has two segments; the others take one trip through the loop.
#include "ap_common.h"

namespace ap {
namespace {

struct GatherArgs {
    const uint32_t* tiles;       // m tiles of tile_bytes each, 16-byte aligned
    const int32_t* plan;         // [n, 4 + G * G]
    uint8_t* out;
    long long tile_dwords_total; // m * tile_bytes / 4
    unsigned tile_bytes, ts, ts3, G, planw;
    unsigned row_bytes;          // pw * 3
    unsigned patch_bytes;        // ph * pw * 3 (< 2^24)
    unsigned pieces;             // ceil(patch_bytes / 16)
    float rcp_row, rcp_ts3, rcp_ts;
    int n;
};

// n / d for n < 2^24 (exact in float) with rcp = 1.0f / d: the float quotient is off by at most one
__device__ __forceinline__ unsigned udiv24(unsigned n, unsigned d, float rcp) {
    unsigned q = (unsigned)((float)n * rcp);
    const int rem = (int)n - (int)(q * d);
    if (rem < 0) --q;
    else if (rem >= (int)d) ++q;
    return q;
}

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__global__ __launch_bounds__(256) void gather_patches_kernel(GatherArgs a) {
    const unsigned piece = blockIdx.x * 256u + threadIdx.x;
    if (piece >= a.pieces) return;
    const unsigned b0 = piece * 16u;
    for (int p = (int)blockIdx.y; p < a.n; p += (int)gridDim.y) {
        const int32_t* pl = a.plan + (size_t)p * a.planw;
        const unsigned ox = (unsigned)pl[0], oy = (unsigned)pl[1];
        const unsigned vw3 = (unsigned)pl[2] * 3u, vh = (unsigned)pl[3];
        const unsigned end = min(16u, a.patch_bytes - b0);
        uint32_t acc[4] = {0u, 0u, 0u, 0u};
        unsigned o = 0;
        while (o < end) {
            const unsigned b = b0 + o;
            const unsigned r = udiv24(b, a.row_bytes, a.rcp_row), cb = b - r * a.row_bytes;
            unsigned len;
            if (r >= vh) {
                len = end - o;                                            // every later row is clipped too
            } else if (cb >= vw3) {
                len = min(end - o, a.row_bytes - cb);                     // the clipped right part of this row
            } else {
                const unsigned xb = ox * 3u + cb;                         // byte column in the G tiles' row
                const unsigned tx = udiv24(xb, a.ts3, a.rcp_ts3), xin = xb - tx * a.ts3;
                const unsigned y = oy + r, ty = udiv24(y, a.ts, a.rcp_ts), yin = y - ty * a.ts;
                len = min(min(end - o, a.ts3 - xin), vw3 - cb);
                const int slot = pl[4 + ty * a.G + tx];
                if (slot >= 0) {
                    // byte address (in the tile buffer) that output byte 0 of this piece would have in this segment's tile row
                    const long long addr = (long long)slot * a.tile_bytes + (long long)(yin * a.ts3 + xin) - (long long)o;
                    const long long d0 = addr >> 2;
                    const unsigned sh = (unsigned)(addr & 3);
                    uint32_t w[5];
                    if (d0 >= 0 && d0 + 5 <= a.tile_dwords_total) {
                        const u32x4_a4 v = *(const u32x4_a4*)(a.tiles + d0);
                        w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
                        w[4] = a.tiles[d0 + 4];
                    } else {
#pragma unroll
                        for (int i = 0; i < 5; ++i) {
                            const long long d = min(max(d0 + i, 0ll), a.tile_dwords_total - 1);
                            w[i] = a.tiles[d];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint32_t v = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
                        const int lo = max((int)o - 4 * i, 0), hi = min((int)(o + len) - 4 * i, 4);
                        if (hi > lo) {
                            const uint32_t mask = (0xFFFFFFFFu >> (8 * (4 - hi))) & (0xFFFFFFFFu << (8 * lo));
                            acc[i] |= v & mask;
                        }
                    }
                }
            }
            o += len;
        }
        uint8_t* dst = a.out + (size_t)p * a.patch_bytes + b0;
        if (end == 16u) {
            *(u32x4*)dst = u32x4{acc[0], acc[1], acc[2], acc[3]};
        } else {                                                          // the last piece of a patch whose size is no multiple of 16 (n == 1)
            for (unsigned k = 0; k < end; ++k) dst[k] = (uint8_t)(acc[k >> 2] >> (8 * (k & 3)));
        }
    }
}

}  // namespace
}  // namespace ap

extern "C" int ap_gather_patches(const uint8_t* tiles, int m, int ts, const int32_t* plan_host, int32_t* plan_dev, int n, int G, int pw,
                                 int ph, uint8_t* out, ap_stream_t stream) {
    using namespace ap;
    AP_REQUIRE(n >= 0 && m >= 0, "ap_gather_patches: bad n %d or m %d", n, m);
    AP_REQUIRE(ts > 0 && pw > 0 && ph > 0 && G > 0, "ap_gather_patches: bad ts %d, pw %d, ph %d or G %d", ts, pw, ph, G);
    AP_REQUIRE(out && plan_host && plan_dev && (tiles || m == 0), "ap_gather_patches: null pointer");
    AP_REQUIRE(((uintptr_t)tiles & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)plan_dev & 3) == 0 && ((uintptr_t)plan_host & 3) == 0,
               "ap_gather_patches: tiles and out must be 16-byte aligned, the plans 4-byte aligned");
    AP_REQUIRE((long long)G * ts >= (long long)(pw > ph ? pw : ph) + ts - 1 && G <= 1024,
               "ap_gather_patches: G %d tiles of %d do not cover a %d x %d patch at every offset", G, ts, pw, ph);
    const long long patch_bytes = (long long)ph * pw * 3, tile_bytes = (long long)ts * ts * 3;
    AP_REQUIRE(patch_bytes < (1ll << 24) && (long long)G * ts * 3 < (1ll << 24), "ap_gather_patches: patch %d x %d or tile row %d x %d too large", pw, ph, G, ts);
    AP_REQUIRE(tile_bytes % 16 == 0 && tile_bytes < (1ll << 31), "ap_gather_patches: every tile must start 16-byte aligned (ts %d)", ts);
    AP_REQUIRE(n <= 1 || patch_bytes % 16 == 0, "ap_gather_patches: every patch must start 16-byte aligned (%d x %d x 3 bytes)", pw, ph);
    const int planw = 4 + G * G;
    for (int p = 0; p < n; ++p) {                                         // the plan is checked on the host, before anything is uploaded
        const int32_t* pl = plan_host + (size_t)p * planw;
        AP_REQUIRE(pl[0] >= 0 && pl[0] < ts && pl[1] >= 0 && pl[1] < ts, "ap_gather_patches: patch %d: ox %d / oy %d outside [0, %d)", p, pl[0], pl[1], ts);
        AP_REQUIRE(pl[2] >= 0 && pl[2] <= pw && pl[3] >= 0 && pl[3] <= ph, "ap_gather_patches: patch %d: vw %d / vh %d outside the patch", p, pl[2], pl[3]);
        for (int k = 4; k < planw; ++k)
            AP_REQUIRE(pl[k] >= -1 && pl[k] < m, "ap_gather_patches: patch %d: slot %d of %d tiles", p, pl[k], m);
    }
    if (n == 0) return AP_OK;
    hipStream_t s = (hipStream_t)stream;
    AP_HIP_CHECK(hipMemcpyAsync(plan_dev, plan_host, (size_t)n * planw * sizeof(int32_t), hipMemcpyHostToDevice, s));
    GatherArgs a;
    a.tiles = (const uint32_t*)tiles;
    a.plan = plan_dev;
    a.out = out;
    a.tile_dwords_total = (long long)m * tile_bytes / 4;
    a.tile_bytes = (unsigned)tile_bytes;
    a.ts = (unsigned)ts;
    a.ts3 = (unsigned)ts * 3u;
    a.G = (unsigned)G;
    a.planw = (unsigned)planw;
    a.row_bytes = (unsigned)pw * 3u;
    a.patch_bytes = (unsigned)patch_bytes;
    a.pieces = (unsigned)((patch_bytes + 15) / 16);
    a.rcp_row = 1.0f / (float)a.row_bytes;
    a.rcp_ts3 = 1.0f / (float)a.ts3;
    a.rcp_ts = 1.0f / (float)a.ts;
    a.n = n;
    const dim3 grid((a.pieces + 255u) / 256u, (unsigned)(n < 65535 ? n : 65535)), block(256);
    hipLaunchKernelGGL(gather_patches_kernel, grid, block, 0, s, a);
    AP_HIP_CHECK(hipGetLastError());
    return AP_OK;
}
