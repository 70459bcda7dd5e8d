// Geometry of a JPEG coefficient slot (include/atlaspatch_hip.h: ap_jpeg_slot_bytes), shared by the host reader that
// fills slots (jpeg_host.cpp) and the device decoder that consumes them (jpeg_device.hip).
//
//   bytes 0 .. 383     uint16 quant[3][64], natural order, in the components' own order (unused tables zero)
//   bytes 384 .. 511   padding
//   then per component int16 [hb][wb][64], natural order, block rows major; wb x hb = the component's
//   width_in_blocks x height_in_blocks = ceil(downsampled size / 8), NOT the MCU-padded width of libjpeg's virtual arrays
#pragma once
#include <cstddef>

namespace ap {

constexpr int kJpegSlotHeader = 512;
constexpr int kJpegMaxSide = 65535;        // what a JPEG frame header can say
// The widest tile the device decoders take.  ap_jpeg_decode_tiles keeps a 16-row band of a tile in one workgroup's LDS
// (jpeg_device.hip: lds = kDBytes + 16 * py + 2 * crows * pc, checked against kLdsLimit = 64 KB).  The worst sampling is 4:4:4 / RGB,
// where py = pc = side rounded up to 8 and crows = 16: 18432 + 48 * 976 = 65280 fits, 18432 + 48 * 984 = 65664 does not
// (jpeg_device.hip asserts just that).  The stream stager, the entropy launch and the TIFF reader's level probe hold tiles to it,
// because the slots they make are for that decoder.
constexpr int kJpegDeviceMaxSide = 976;

struct JpegGeom {
    int ncomp;
    int hmax, vmax;        // luma sampling factors; chroma is 1 x 1
    int cw[3], ch[3];      // the components' planes, cropped: ceil(side * h_c / h_max) x ceil(side * v_c / v_max)
    int wb[3], hb[3];      // blocks
    size_t off[3];         // byte offset of the component's blocks in the slot
    size_t bytes;          // slot stride
};

// sampling: AP_JPEG_GRAY 0 / AP_JPEG_444 1 / AP_JPEG_422 2 / AP_JPEG_420 3 / AP_JPEG_RGB 4 (three 1 x 1 components coded as R, G, B:
// the geometry of 4:4:4, "luma" and "chroma" then read "R" and "G, B")
__host__ __device__ inline bool jpeg_geom(int side, int sampling, JpegGeom* g) {
    if (side <= 0 || side > kJpegMaxSide || sampling < 0 || sampling > 4) return false;
    g->ncomp = sampling == 0 ? 1 : 3;
    g->hmax = sampling == 2 || sampling == 3 ? 2 : 1;
    g->vmax = sampling == 3 ? 2 : 1;
    size_t off = kJpegSlotHeader;
    for (int c = 0; c < 3; ++c) {
        const int h = c == 0 ? g->hmax : 1, v = c == 0 ? g->vmax : 1;
        const bool have = c < g->ncomp;
        g->cw[c] = have ? (side * h + g->hmax - 1) / g->hmax : 0;
        g->ch[c] = have ? (side * v + g->vmax - 1) / g->vmax : 0;
        g->wb[c] = (g->cw[c] + 7) / 8;
        g->hb[c] = (g->ch[c] + 7) / 8;
        g->off[c] = off;
        off += (size_t)g->wb[c] * g->hb[c] * 128;
    }
    g->bytes = off;
    return true;
}

}  // namespace ap
