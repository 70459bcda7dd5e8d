// The in-memory "tables + stream" path of jpeg_host.cpp, shared by its own file readers and the TIFF reader (tiff_host.cpp).
// `tables` (may be null) is a tables-only stream -- TIFF's JPEGTables tag -- that goes through jpeg_read_header(..., FALSE) in
// front of the abbreviated tile stream `data`, as libtiff and OpenSlide do.  Every call returns AP_OK, AP_ERR_INVALID with the
// reason in `why`, or AP_ERR_UNSUPPORTED without a usable libjpeg.so.8.  Host only, callable from any thread.
#pragma once
#include <cstddef>

namespace ap {

// How a three-component stream's colour model is decided.  kJpegColourInfer: as libjpeg infers it from the stream's markers and
// component ids (a JPEG file).  kJpegColourRgb: the container says the components are R, G, B (a TIFF level with
// PhotometricInterpretation 2) -- libtiff then suppresses libjpeg's colour handling whatever the markers say, and so does this reader.
constexpr int kJpegColourInfer = 0, kJpegColourRgb = 1;
// what jpeg_mem_coefficients leaves in *sampling when it refuses an RGB-coded stream because a component is subsampled
constexpr int kJpegRgbSubsampled = -2;

int jpeg_mem_ready(char* why, size_t why_cap);
// want_w x want_h RGB pixels into dst (rows of `stride` bytes); a stream libjpeg warns about is refused
int jpeg_mem_pixels(const unsigned char* tables, size_t tables_size, const unsigned char* data, size_t size, int want_w, int want_h,
                    unsigned char* dst, size_t stride, char* why, size_t why_cap, int colour = kJpegColourInfer);
// slot == nullptr: the probe (wh and sampling from the header); else the coefficient slot of jpeg_slot.h at want_side / want_sampling
int jpeg_mem_coefficients(const unsigned char* tables, size_t tables_size, const unsigned char* data, size_t size, int wh[2],
                          int* sampling, int want_side, int want_sampling, unsigned char* slot, char* why, size_t why_cap,
                          int colour = kJpegColourInfer);

}  // namespace ap
