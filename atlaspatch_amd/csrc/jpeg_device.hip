// K0, device half: JPEG tiles from their entropy-decoded coefficients (include/atlaspatch_hip.h: ap_jpeg_decode_tiles).
//
// libjpeg's JDCT_ISLOW decode with fancy upsampling, restated in integers: dequantise -> 8 x 8 inverse DCT (columns, then
// rows, 13-bit constants) -> range limit -> h2v1 / h2v2 triangle upsampling of the chroma planes -> YCbCr -> RGB.  Bit-equal
// to libjpeg-turbo (and so to Pillow) on every baseline stream the host reader (jpeg_host.cpp) admits.  AP_JPEG_RGB is the 4:4:4
// form without the last stage: three 1 x 1 components that ARE R, G, B (a TIFF level tagged Photometric 2, a stream libjpeg infers as
// RGB) go through IDCT, + 128 and the range limit per component and are interleaved as they are, which is what libjpeg's copy does.
//
// One workgroup = one tile x one band of 16 luma rows.  The band's blocks go through LDS in chunks of 64:
//   A  16-byte loads of coefficient rows and quantiser rows, product -> d[block][64] (int32)
//   B  one thread per (block, column): column pass in place
//   C  one thread per (block, row): row pass, + 128, clamp, 8 samples -> the component's plane in LDS
// then  D  one thread per 16 output pixels (48 bytes = three 16-byte stores, whatever the row pitch 3 * side is: the band's
// rows are contiguous in the output, so the band is cut at multiples of 16 pixels of the WHOLE output and the ragged first and
// last groups are written byte by byte; a side that is a multiple of 16 takes a form whose groups lie in one row each and share
// their LDS reads).  At 4:2:0 a band also needs the chroma row above and the one below it: the
// workgroup recomputes those two block rows (3 chroma block rows per band instead of 1) and stays single-pass, no workspace.
// Integer VALU work through LDS; the traffic is the coefficients in and the pixels out, once each.
#include "ap_common.h"
#include "jpeg_slot.h"

namespace ap {
namespace {

constexpr int kChunk = 64;              // blocks per LDS pass
constexpr int kBlkStride = 72;          // dwords per block in d: 8 blocks of a wave's column pass land in 64 different banks
constexpr int kDBytes = kChunk * kBlkStride * 4;
constexpr int kLdsLimit = 64 * 1024;
// jpeg_slot.h's kJpegDeviceMaxSide is the widest side the LDS sum of ap_jpeg_decode_tiles_ex admits at its worst sampling (4:4:4 / RGB)
static_assert(kDBytes + 48 * kJpegDeviceMaxSide <= kLdsLimit && kDBytes + 48 * (kJpegDeviceMaxSide + 8) > kLdsLimit, "kJpegDeviceMaxSide");

struct DecodeArgs {
    const uint8_t* slots;
    uint8_t* rgb;
    size_t slot_bytes;
    int n, side, bands;
    int ncomp;
    int wb[3], hb[3];
    unsigned off[3];
    int ccw, cch;          // chroma plane, cropped
    int crows;             // chroma rows a band keeps in LDS: 16, or 24 at 4:2:0 (block rows band - 1 .. band + 1)
    int py, pc;            // LDS pitches of the luma and chroma planes (= 8 * wb)
};

// one 1-D pass of jidctint.c (CONST_BITS 13), in place; descale by s with rounding
__device__ __forceinline__ void idct8(int (&v)[8], int s) {
    constexpr int f0298 = 2446, f0390 = 3196, f0541 = 4433, f0765 = 6270, f0899 = 7373, f1175 = 9633, f1501 = 12299,
                  f1847 = 15137, f1961 = 16069, f2053 = 16819, f2562 = 20995, f3072 = 25172;
    int z1 = (v[2] + v[6]) * f0541;
    const int t2 = z1 - v[6] * f1847, t3 = z1 + v[2] * f0765;
    const int t0 = (v[0] + v[4]) * 8192, t1 = (v[0] - v[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a = v[7], b = v[5], c = v[3], d = v[1];
    z1 = a + d;
    int z2 = b + c, z3 = a + c, z4 = b + d;
    const int z5 = (z3 + z4) * f1175;
    a *= f0298; b *= f2053; c *= f3072; d *= f1501;
    z1 *= -f0899; z2 *= -f2562;
    z3 = z3 * -f1961 + z5;
    z4 = z4 * -f0390 + z5;
    a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4;
    const int rnd = 1 << (s - 1);
    v[0] = (t10 + d + rnd) >> s; v[7] = (t10 - d + rnd) >> s;
    v[1] = (t11 + c + rnd) >> s; v[6] = (t11 - c + rnd) >> s;
    v[2] = (t12 + b + rnd) >> s; v[5] = (t12 - b + rnd) >> s;
    v[3] = (t13 + a + rnd) >> s; v[4] = (t13 - a + rnd) >> s;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// jdcolor.c, 16-bit fixed point: cb, cr with 128 already subtracted
__device__ __forceinline__ void ycc_to_rgb(int y, int cb, int cr, int& R, int& G, int& B) {
    R = clamp255(y + ((91881 * cr + 32768) >> 16));
    B = clamp255(y + ((116130 * cb + 32768) >> 16));
    G = clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
}

// pixel i of 16 into the 48 bytes w (i is a compile-time constant after unrolling)
__device__ __forceinline__ void pack_rgb(uint32_t (&w)[12], int i, int R, int G, int B) {
    w[(3 * i) >> 2] |= (uint32_t)R << (8 * ((3 * i) & 3));
    w[(3 * i + 1) >> 2] |= (uint32_t)G << (8 * ((3 * i + 1) & 3));
    w[(3 * i + 2) >> 2] |= (uint32_t)B << (8 * ((3 * i + 2) & 3));
}

__device__ __forceinline__ int byte_of(const u32x4& v, int m) { return (v[m >> 2] >> (8 * (m & 3))) & 255; }
__device__ __forceinline__ int byte_of(const u32x2& v, int m) { return (v[m >> 2] >> (8 * (m & 3))) & 255; }

// SAMPLING: AP_JPEG_*.  blockDim = 256, grid = n * bands, dynamic LDS = kDBytes + 16 * py + 2 * crows * pc.
template <int SAMPLING>
__global__ __launch_bounds__(256) void jpeg_decode_kernel(const DecodeArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int* const d = (int*)lds;
    uint8_t* const planeY = lds + kDBytes;
    uint8_t* const planeC = planeY + 16 * p.py;
    const int tid = threadIdx.x;
    const int tile = blockIdx.x / p.bands, band = blockIdx.x - tile * p.bands;
    const uint8_t* const slot = p.slots + (size_t)tile * p.slot_bytes;
    constexpr bool k420 = SAMPLING == AP_JPEG_420;
    constexpr bool kRgb = SAMPLING == AP_JPEG_RGB;          // planes 0, 1, 2 hold R, G, B: the 4:4:4 reads, no colour transform
    constexpr bool kFull = SAMPLING == AP_JPEG_444 || kRgb; // "chroma" planes at full resolution
    constexpr int kComps = SAMPLING == AP_JPEG_GRAY ? 1 : 3;

    // the band's block rows per component: [br0, br0 + nrows); rowbase = the block row that sits at LDS plane row 0
    int br0[3], cnt[3], rowbase[3];
    br0[0] = rowbase[0] = 2 * band;
    cnt[0] = min(2, p.hb[0] - 2 * band) * p.wb[0];
    for (int c = 1; c < 3; ++c) {
        if (kComps == 1) { br0[c] = rowbase[c] = cnt[c] = 0; continue; }
        if (k420) {
            rowbase[c] = band - 1;
            br0[c] = max(band - 1, 0);
            cnt[c] = (min(band + 2, p.hb[c]) - br0[c]) * p.wb[c];
        } else {
            br0[c] = rowbase[c] = 2 * band;
            cnt[c] = min(2, p.hb[c] - 2 * band) * p.wb[c];
        }
    }
    const int start1 = cnt[0], start2 = cnt[0] + cnt[1], total = start2 + cnt[2];

    for (int t0 = 0; t0 < total; t0 += kChunk) {
        // A: coefficient row x quantiser row -> d
        for (int u = tid; u < kChunk * 8; u += 256) {
            const int blk = u >> 3, r = u & 7, t = t0 + blk;
            if (t >= total) continue;
            const int c = t < start1 ? 0 : t < start2 ? 1 : 2;
            const int tl = t - (c == 0 ? 0 : c == 1 ? start1 : start2);
            const u32x4 cf = *(const u32x4*)(slot + p.off[c] + ((size_t)br0[c] * p.wb[c] + tl) * 128 + r * 16);
            const u32x4 q = *(const u32x4*)(slot + c * 128 + r * 16);
            int o[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[2 * k] = (int)(short)(cf[k] & 0xFFFF) * (int)(q[k] & 0xFFFF);
                o[2 * k + 1] = ((int)cf[k] >> 16) * (int)(q[k] >> 16);
            }
            int* dst = d + blk * kBlkStride + r * 8;
            *(u32x4*)dst = u32x4{(uint32_t)o[0], (uint32_t)o[1], (uint32_t)o[2], (uint32_t)o[3]};
            *(u32x4*)(dst + 4) = u32x4{(uint32_t)o[4], (uint32_t)o[5], (uint32_t)o[6], (uint32_t)o[7]};
        }
        __syncthreads();
        // B: columns, in place (thread = block, column)
        for (int u = tid; u < kChunk * 8; u += 256) {
            const int blk = u >> 3, j = u & 7;
            if (t0 + blk >= total) continue;
            int* col = d + blk * kBlkStride + j;
            int v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = col[r * 8];
            idct8(v, 11);
#pragma unroll
            for (int r = 0; r < 8; ++r) col[r * 8] = v[r];
        }
        __syncthreads();
        // C: rows -> samples in the component's plane (thread = block, row)
        for (int u = tid; u < kChunk * 8; u += 256) {
            const int blk = u >> 3, r = u & 7, t = t0 + blk;
            if (t >= total) continue;
            const int c = t < start1 ? 0 : t < start2 ? 1 : 2;
            const int tl = t - (c == 0 ? 0 : c == 1 ? start1 : start2);
            const int brl = tl / p.wb[c], bcol = tl - brl * p.wb[c];
            const int* row = d + blk * kBlkStride + r * 8;
            const u32x4 lo = *(const u32x4*)row, hi = *(const u32x4*)(row + 4);
            int v[8] = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            idct8(v, 18);
            uint32_t w0 = 0, w1 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w0 |= (uint32_t)clamp255(v[k] + 128) << (8 * k);
                w1 |= (uint32_t)clamp255(v[4 + k] + 128) << (8 * k);
            }
            uint8_t* plane = c == 0 ? planeY : planeC + (c - 1) * p.crows * p.pc;
            const int pitch = c == 0 ? p.py : p.pc;
            const int lrow = (br0[c] + brl - rowbase[c]) * 8 + r;
            *(u32x2*)(plane + lrow * pitch + bcol * 8) = u32x2{w0, w1};
        }
        __syncthreads();
    }

    // D: upsample + colour, 16 pixels of the whole output per thread
    const long long tile_px = (long long)p.side * p.side;
    const long long g0 = tile * tile_px + (long long)band * 16 * p.side;
    const int rows = min(16, p.side - band * 16);
    const long long g1 = g0 + (long long)rows * p.side;
    const uint8_t* const cbp = planeC;
    const uint8_t* const crp = planeC + p.crows * p.pc;
    const bool box = p.ccw <= 2;            // libjpeg upsamples a plane at most 2 samples wide by replication
    if ((p.side & 15) == 0) {
        // rows are whole groups: a thread takes 16 pixels of ONE row and shares their LDS reads -- 16 luma samples in one read,
        // the 8 chroma samples under them (and the neighbour on either side, replicated at the plane's ends, which is what the
        // first / last column formulas amount to) in one read per plane and row
        const int gpr = p.side >> 4;
        for (int u = tid; u < rows * gpr; u += 256) {
            const int ly = u / gpr, x0 = (u - ly * gpr) << 4;
            const u32x4 yv = *(const u32x4*)(planeY + ly * p.py + x0);
            int cb[16], cr[16];
            if (kFull) {
                const u32x4 bv = *(const u32x4*)(cbp + ly * p.pc + x0), rv = *(const u32x4*)(crp + ly * p.pc + x0);
#pragma unroll
                for (int i = 0; i < 16; ++i) { cb[i] = byte_of(bv, i); cr[i] = byte_of(rv, i); }
            } else if (SAMPLING == AP_JPEG_422 || SAMPLING == AP_JPEG_420) {
                const int j0 = x0 >> 1;
                int on, of = 0;
                if (SAMPLING == AP_JPEG_420) {
                    const int yy = band * 16 + ly, ci = yy >> 1;
                    const int far = (yy & 1) ? min(ci + 1, p.cch - 1) : max(ci - 1, 0);
                    on = (ci - 8 * (band - 1)) * p.pc;
                    of = (far - 8 * (band - 1)) * p.pc;
                } else {
                    on = ly * p.pc;
                }
                const int jl = max(j0 - 1, 0), jr = min(j0 + 8, p.ccw - 1);
                int sb[10], sr[10];         // samples j0 - 1 .. j0 + 8; at 4:2:0 after the vertical pass: 3 x near + far
                {
                    const u32x2 bv = *(const u32x2*)(cbp + on + j0), rv = *(const u32x2*)(crp + on + j0);
#pragma unroll
                    for (int k = 0; k < 8; ++k) { sb[k + 1] = byte_of(bv, k); sr[k + 1] = byte_of(rv, k); }
                    sb[0] = cbp[on + jl]; sr[0] = crp[on + jl];
                    sb[9] = cbp[on + jr]; sr[9] = crp[on + jr];
                }
                if (SAMPLING == AP_JPEG_420) {
                    const u32x2 bv = *(const u32x2*)(cbp + of + j0), rv = *(const u32x2*)(crp + of + j0);
#pragma unroll
                    for (int k = 0; k < 8; ++k) { sb[k + 1] = 3 * sb[k + 1] + byte_of(bv, k); sr[k + 1] = 3 * sr[k + 1] + byte_of(rv, k); }
                    sb[0] = 3 * sb[0] + cbp[of + jl]; sr[0] = 3 * sr[0] + crp[of + jl];
                    sb[9] = 3 * sb[9] + cbp[of + jr]; sr[9] = 3 * sr[9] + crp[of + jr];
                }
                constexpr int sh = SAMPLING == AP_JPEG_420 ? 4 : 2, re = SAMPLING == AP_JPEG_420 ? 8 : 1, ro = SAMPLING == AP_JPEG_420 ? 7 : 2;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int k = (i >> 1) + 1;
                    cb[i] = (i & 1) ? (3 * sb[k] + sb[k + 1] + ro) >> sh : (3 * sb[k] + sb[k - 1] + re) >> sh;
                    cr[i] = (i & 1) ? (3 * sr[k] + sr[k + 1] + ro) >> sh : (3 * sr[k] + sr[k - 1] + re) >> sh;
                }
            }
            uint32_t w[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) w[k] = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int y = byte_of(yv, i);
                int R = y, Gc = y, B = y;
                if (kRgb) { Gc = cb[i]; B = cr[i]; }
                else if (SAMPLING != AP_JPEG_GRAY) ycc_to_rgb(y, cb[i] - 128, cr[i] - 128, R, Gc, B);
                pack_rgb(w, i, R, Gc, B);
            }
            u32x4* o = (u32x4*)(p.rgb + (size_t)(g0 + (long long)ly * p.side + x0) * 3);
            o[0] = u32x4{w[0], w[1], w[2], w[3]};
            o[1] = u32x4{w[4], w[5], w[6], w[7]};
            o[2] = u32x4{w[8], w[9], w[10], w[11]};
        }
        return;
    }
    // any other side: groups of 16 pixels of the whole output, which may straddle rows and the band's ends
    for (long long G = g0 / 16 + tid; G * 16 < g1; G += 256) {
        const long long g = G * 16;
        const int lp = (int)(g - g0);       // negative in the band's first group when the band does not start on a multiple of 16
        const bool full = lp >= 0 && g + 16 <= g1;
        int ly = 0, x = lp;
        if (lp >= 0) { ly = lp / p.side; x = lp - ly * p.side; }
        uint32_t w[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool in = lp + i >= 0 && g + i < g1;
            int R = 0, Gc = 0, B = 0;
            if (in) {
                const int y = planeY[ly * p.py + x];
                if (SAMPLING == AP_JPEG_GRAY) {
                    R = Gc = B = y;
                } else {
                    int cb, cr;
                    if (kFull) {
                        cb = cbp[ly * p.pc + x];
                        cr = crp[ly * p.pc + x];
                    } else if (SAMPLING == AP_JPEG_422) {
                        const int j = x >> 1, o = ly * p.pc + j;
                        const int pb = cbp[o], pr = crp[o];
                        if (box || x == 0 || x == 2 * p.ccw - 1) {
                            cb = pb; cr = pr;
                        } else if (x & 1) {
                            cb = (3 * pb + cbp[o + 1] + 2) >> 2;
                            cr = (3 * pr + crp[o + 1] + 2) >> 2;
                        } else {
                            cb = (3 * pb + cbp[o - 1] + 1) >> 2;
                            cr = (3 * pr + crp[o - 1] + 1) >> 2;
                        }
                    } else {
                        const int yy = band * 16 + ly, ci = yy >> 1;
                        const int far = (yy & 1) ? min(ci + 1, p.cch - 1) : max(ci - 1, 0);
                        const int base = 8 * (band - 1);
                        const int j = x >> 1, on = (ci - base) * p.pc + j, of = (far - base) * p.pc + j;
                        if (box) {
                            cb = cbp[on]; cr = crp[on];
                        } else {
                            const int sb = 3 * cbp[on] + cbp[of], sr = 3 * crp[on] + crp[of];
                            if (x == 0) {
                                cb = (4 * sb + 8) >> 4; cr = (4 * sr + 8) >> 4;
                            } else if (x == 2 * p.ccw - 1) {
                                cb = (4 * sb + 7) >> 4; cr = (4 * sr + 7) >> 4;
                            } else if (x & 1) {
                                cb = (3 * sb + 3 * cbp[on + 1] + cbp[of + 1] + 7) >> 4;
                                cr = (3 * sr + 3 * crp[on + 1] + crp[of + 1] + 7) >> 4;
                            } else {
                                cb = (3 * sb + 3 * cbp[on - 1] + cbp[of - 1] + 8) >> 4;
                                cr = (3 * sr + 3 * crp[on - 1] + crp[of - 1] + 8) >> 4;
                            }
                        }
                    }
                    if (kRgb) { R = y; Gc = cb; B = cr; }
                    else ycc_to_rgb(y, cb - 128, cr - 128, R, Gc, B);
                }
                if (!full) {
                    uint8_t* o = p.rgb + (size_t)(g + i) * 3;
                    o[0] = (uint8_t)R; o[1] = (uint8_t)Gc; o[2] = (uint8_t)B;
                }
            }
            pack_rgb(w, i, R, Gc, B);
            if (++x == p.side) { x = 0; ++ly; }
        }
        if (full) {
            u32x4* o = (u32x4*)(p.rgb + (size_t)g * 3);
            o[0] = u32x4{w[0], w[1], w[2], w[3]};
            o[1] = u32x4{w[4], w[5], w[6], w[7]};
            o[2] = u32x4{w[8], w[9], w[10], w[11]};
        }
    }
}

}  // namespace
}  // namespace ap

extern "C" int ap_jpeg_decode_tiles_ex(const void* slots, int n, int side, int sampling, uint8_t* rgb, ap_stream_t stream) {
    using namespace ap;
    AP_REQUIRE(slots && rgb, "ap_jpeg_decode_tiles: null pointer");
    AP_REQUIRE(n >= 0 && side > 0, "ap_jpeg_decode_tiles: bad n %d or side %d", n, side);
    AP_REQUIRE(((uintptr_t)slots & 15) == 0 && ((uintptr_t)rgb & 15) == 0, "ap_jpeg_decode_tiles: slots and rgb must be 16-byte aligned");
    JpegGeom g;
    AP_REQUIRE(jpeg_geom(side, sampling, &g), "ap_jpeg_decode_tiles: bad side %d or sampling %d", side, sampling);
    DecodeArgs a;
    a.slots = (const uint8_t*)slots;
    a.rgb = rgb;
    a.slot_bytes = g.bytes;
    a.n = n;
    a.side = side;
    a.bands = (side + 15) / 16;
    a.ncomp = g.ncomp;
    for (int c = 0; c < 3; ++c) { a.wb[c] = g.wb[c]; a.hb[c] = g.hb[c]; a.off[c] = (unsigned)g.off[c]; }
    a.ccw = g.cw[1];
    a.cch = g.ch[1];
    a.crows = g.ncomp == 1 ? 0 : sampling == AP_JPEG_420 ? 24 : 16;
    a.py = 8 * g.wb[0];
    a.pc = 8 * g.wb[1];
    const size_t lds = (size_t)kDBytes + 16 * (size_t)a.py + 2 * (size_t)a.crows * a.pc;
    AP_REQUIRE(lds <= (size_t)kLdsLimit, "ap_jpeg_decode_tiles: side %d needs %zu bytes of LDS per workgroup (limit %d)", side, lds, kLdsLimit);
    AP_REQUIRE((long long)n * a.bands <= 0x7FFFFFFFLL, "ap_jpeg_decode_tiles: n %d x %d bands exceeds the grid", n, a.bands);
    if (n == 0) return AP_OK;
    const dim3 grid((unsigned)(n * a.bands)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (sampling) {
        case AP_JPEG_GRAY: hipLaunchKernelGGL(jpeg_decode_kernel<AP_JPEG_GRAY>, grid, block, lds, s, a); break;
        case AP_JPEG_444: hipLaunchKernelGGL(jpeg_decode_kernel<AP_JPEG_444>, grid, block, lds, s, a); break;
        case AP_JPEG_422: hipLaunchKernelGGL(jpeg_decode_kernel<AP_JPEG_422>, grid, block, lds, s, a); break;
        case AP_JPEG_RGB: hipLaunchKernelGGL(jpeg_decode_kernel<AP_JPEG_RGB>, grid, block, lds, s, a); break;
        default: hipLaunchKernelGGL(jpeg_decode_kernel<AP_JPEG_420>, grid, block, lds, s, a); break;
    }
    AP_HIP_CHECK(hipGetLastError());
    return AP_OK;
}

// the four codes this entry was published with; AP_JPEG_RGB stays an unknown sampling here
extern "C" int ap_jpeg_decode_tiles(const void* slots, int n, int side, int sampling, uint8_t* rgb, ap_stream_t stream) {
    AP_REQUIRE(sampling != AP_JPEG_RGB, "ap_jpeg_decode_tiles: bad side %d or sampling %d (AP_JPEG_RGB: ap_jpeg_decode_tiles_ex)", side, sampling);
    return ap_jpeg_decode_tiles_ex(slots, n, side, sampling, rgb, stream);
}
