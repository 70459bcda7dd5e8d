// The in-memory "tables + stream" path of jpeg_host.cpp, shared by its own file readers and the TIFF reader (tiff_host.cpp).
// `tables` (may be null) is a tables-only stream -- TIFF's JPEGTables tag -- that goes through jpeg_read_header(..., FALSE) in
// front of the abbreviated tile stream `data`, as libtiff and OpenSlide do.  Every call returns AP_OK, AP_ERR_INVALID with the
// reason in `why`, or AP_ERR_UNSUPPORTED without a usable libjpeg.so.8.  Host only, callable from any thread.
#pragma once
#include <cstddef>
#include <cstdio>
#include "ap_common.h"
#include "jpeg_slot.h"

namespace ap {

// How a three-component stream's colour model is decided.  kJpegColourInfer: as libjpeg infers it from the stream's markers and
// component ids (a JPEG file).  kJpegColourRgb: the container says the components are R, G, B (a TIFF level with
// PhotometricInterpretation 2) -- libtiff then suppresses libjpeg's colour handling whatever the markers say, and so does this reader.
constexpr int kJpegColourInfer = 0, kJpegColourRgb = 1;
// what jpeg_classify leaves in *found when it refuses an RGB-coded stream because a component is subsampled
constexpr int kJpegRgbSubsampled = -2;

// The colour model a reader found for a stream, however it found it: the libjpeg reader from jpeg_color_space, the stream stager from
// JFIF, Adobe and the component ids, either from the container's override.
enum JpegModel { kJpegGrey, kJpegYCbCr, kJpegRgbCoded, kJpegOtherModel };

// The one statement of the device decoder's subset that both readers share (jpeg_host.cpp: read_one; jpeg_stream_host.cpp:
// jpeg_stream_stage): greyscale, YCbCr at 4:4:4 / 4:2:2 (2x1) / 4:2:0 (2x2) with 1x1 chroma, or RGB coded with three 1x1 components.
// `hv`: the sampling factors of the first min(ncomp, 3) components.  *found: the stream's AP_JPEG_* code, kJpegRgbSubsampled, or -1.
// `g` == nullptr asks nothing of the stream (the probe); else it must also be want_side square at want_sampling -- a colour model
// asked for as the other is said so -- and *g is that slot's geometry.  false: refused, the reason in `why`.
inline bool jpeg_classify(int ncomp, const int (*hv)[2], JpegModel model, int width, int height, int want_side, int want_sampling,
                          JpegGeom* g, int* found, char* why, size_t why_cap) {
#define refuse(...) (snprintf(why, why_cap, __VA_ARGS__), false)
    *found = -1;
    if (model == kJpegOtherModel || ncomp != (model == kJpegGrey ? 1 : 3)) return refuse("%d components: none of greyscale, YCbCr, RGB", ncomp);
    const auto one = [&](int c) { return hv[c][0] == 1 && hv[c][1] == 1; };
    int code = -1;
    if (model == kJpegRgbCoded) {
        for (int c = 0; c < 3; ++c)
            if (!one(c)) {
                *found = kJpegRgbSubsampled;
                return refuse("RGB-coded stream whose component %d has sampling factors %dx%d: only 1x1 components are read", c, hv[c][0], hv[c][1]);
            }
        code = AP_JPEG_RGB;
    } else if (model == kJpegGrey) {
        // libjpeg decodes a one-component frame with its sampling factors taken as 1 x 1 whatever they say; the readers want them said
        if (one(0)) code = AP_JPEG_GRAY;
    } else if (one(1) && one(2)) {
        const int h = hv[0][0], v = hv[0][1];
        code = h == 1 && v == 1 ? AP_JPEG_444 : h == 2 && v == 1 ? AP_JPEG_422 : h == 2 && v == 2 ? AP_JPEG_420 : -1;
    }
    if (code < 0)
        return refuse("sampling factors %dx%d%s are none of 4:4:4, 4:2:2 (2x1), 4:2:0 (2x2), greyscale", hv[0][0], hv[0][1],
                      model == kJpegGrey ? "" : " (or subsampled luma / oversampled chroma)");
    *found = code;
    if (!g) return true;
    if (code != want_sampling && (code == AP_JPEG_RGB || want_sampling == AP_JPEG_RGB))
        return refuse("%s stream (sampling %d) asked for as %s (sampling %d)", model == kJpegRgbCoded ? "RGB-coded" : model == kJpegGrey ? "greyscale" : "YCbCr",
                      code, want_sampling == AP_JPEG_RGB ? "RGB coded" : "greyscale / YCbCr", want_sampling);
    if (code != want_sampling) return refuse("sampling %d, expected %d", code, want_sampling);
    if (width != want_side || height != want_side) return refuse("tile is %d x %d, expected %d x %d", width, height, want_side, want_side);
    if (!jpeg_geom(want_side, want_sampling, g)) return refuse("bad side %d", want_side);
    return true;
#undef refuse
}

int jpeg_mem_ready(char* why, size_t why_cap);
// want_w x want_h RGB pixels into dst (rows of `stride` bytes); a stream libjpeg warns about is refused
int jpeg_mem_pixels(const unsigned char* tables, size_t tables_size, const unsigned char* data, size_t size, int want_w, int want_h,
                    unsigned char* dst, size_t stride, char* why, size_t why_cap, int colour = kJpegColourInfer);
// slot == nullptr: the probe (wh and sampling from the header); else the coefficient slot of jpeg_slot.h at want_side / want_sampling
int jpeg_mem_coefficients(const unsigned char* tables, size_t tables_size, const unsigned char* data, size_t size, int wh[2],
                          int* sampling, int want_side, int want_sampling, unsigned char* slot, char* why, size_t why_cap,
                          int colour = kJpegColourInfer);

}  // namespace ap
