// Native batched JPEG tile decode for the tile ring's host threads (no device work).
//
// The reference reads one tile per H5 row in the interpreter (services/feature_embedding.py:86-95 ->
// core/wsi/openslide_wsi.py:184-205: read_region(...).convert("RGB")); a real slide's tiles are JPEG streams.  The
// ring's decode threads call ap_host_decode_jpeg_tiles once per chunk: read + decode n tile files straight into
// consecutive slots of the pinned staging buffer, outside the interpreter lock.
//
// Decoder: the system's libjpeg-turbo (libjpeg.so.8, the jpeg8 ABI build Ubuntu ships; Pillow's own decoder is the
// same code base, so the pixels are the ones PIL.Image.open(...).convert("RGB") yields -- tested bit for bit).  The
// image has the shared object but no development headers, so the handful of declarations needed from <jpeglib.h>
// (JPEG_LIB_VERSION 80 layout) are restated below; the library itself validates them: jpeg_CreateDecompress
// rejects a caller whose sizeof(jpeg_decompress_struct) differs from its own, and the first use runs a self-check.
// If the library is missing or disagrees the entry point returns AP_ERR_UNSUPPORTED and the backend keeps reading
// tile by tile through Pillow.
#include <dlfcn.h>
#include <csetjmp>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>
#include "ap_common.h"
#include "jpeg_slot.h"
#include "jpeg_host.h"

namespace {

// ---- <jpeglib.h> subset, JPEG_LIB_VERSION 80 (libjpeg-turbo 2.x built --with-jpeg8), LP64 ----------------------------
typedef int boolean_t;
typedef unsigned int JDIMENSION;
typedef unsigned char JSAMPLE;
typedef JSAMPLE* JSAMPROW;
typedef JSAMPROW* JSAMPARRAY;

struct jpeg_error_mgr {
    void (*error_exit)(void* cinfo);
    void (*emit_message)(void* cinfo, int msg_level);
    void (*output_message)(void* cinfo);
    void (*format_message)(void* cinfo, char* buffer);
    void (*reset_error_mgr)(void* cinfo);
    int msg_code;
    union { int i[8]; char s[80]; } msg_parm;
    int trace_level;
    long num_warnings;
    const char* const* jpeg_message_table;
    int last_jpeg_message;
    const char* const* addon_message_table;
    int first_addon_message;
    int last_addon_message;
};

struct jpeg_decompress_struct {
    jpeg_error_mgr* err;                 // jpeg_common_fields
    void* mem;
    void* progress;
    void* client_data;
    boolean_t is_decompressor;
    int global_state;
    void* src;
    JDIMENSION image_width, image_height;
    int num_components;
    int jpeg_color_space;
    int out_color_space;
    unsigned int scale_num, scale_denom;
    double output_gamma;
    boolean_t buffered_image, raw_data_out;
    int dct_method;
    boolean_t do_fancy_upsampling, do_block_smoothing, quantize_colors;
    int dither_mode;
    boolean_t two_pass_quantize;
    int desired_number_of_colors;
    boolean_t enable_1pass_quant, enable_external_quant, enable_2pass_quant;
    JDIMENSION output_width, output_height;
    int out_color_components, output_components, rec_outbuf_height, actual_number_of_colors;
    JSAMPARRAY colormap;
    JDIMENSION output_scanline;
    int input_scan_number;
    JDIMENSION input_iMCU_row;
    int output_scan_number;
    JDIMENSION output_iMCU_row;
    int (*coef_bits)[64];
    void* quant_tbl_ptrs[4];
    void* dc_huff_tbl_ptrs[4];
    void* ac_huff_tbl_ptrs[4];
    int data_precision;
    void* comp_info;
    boolean_t is_baseline;               // >= v8
    boolean_t progressive_mode, arith_code;
    unsigned char arith_dc_L[16], arith_dc_U[16], arith_ac_K[16];
    unsigned int restart_interval;
    boolean_t saw_JFIF_marker;
    unsigned char JFIF_major_version, JFIF_minor_version, density_unit;
    unsigned short X_density, Y_density;
    boolean_t saw_Adobe_marker;
    unsigned char Adobe_transform;
    boolean_t CCIR601_sampling;
    void* marker_list;
    int max_h_samp_factor, max_v_samp_factor;
    int min_DCT_h_scaled_size, min_DCT_v_scaled_size;      // >= v7
    JDIMENSION total_iMCU_rows;
    JSAMPLE* sample_range_limit;
    int comps_in_scan;
    void* cur_comp_info[4];
    JDIMENSION MCUs_per_row, MCU_rows_in_scan;
    int blocks_in_MCU;
    int MCU_membership[10];
    int Ss, Se, Ah, Al;
    int block_size;                      // >= v8
    const int* natural_order;
    int lim_Se;
    int unread_marker;
    void *master, *main_, *coef, *post, *inputctl, *marker, *entropy, *idct, *upsample, *cconvert, *cquantize;
};

// what the coefficient reader (ap_host_jpeg_coefficients) needs beyond the pixel decoder's subset
typedef short JCOEF;
typedef JCOEF JBLOCK[64];
typedef JBLOCK* JBLOCKROW;
typedef JBLOCKROW* JBLOCKARRAY;
typedef void* jvirt_barray_ptr;

struct JQUANT_TBL {
    unsigned short quantval[64];         // natural order (not the zigzag order of the DQT marker)
    boolean_t sent_table;
};

struct jpeg_component_info {             // >= v7 layout (DCT_h_scaled_size / DCT_v_scaled_size)
    int component_id, component_index, h_samp_factor, v_samp_factor, quant_tbl_no, dc_tbl_no, ac_tbl_no;
    JDIMENSION width_in_blocks, height_in_blocks;
    int DCT_h_scaled_size, DCT_v_scaled_size;
    JDIMENSION downsampled_width, downsampled_height;
    boolean_t component_needed;
    int MCU_width, MCU_height, MCU_blocks, MCU_sample_width, last_col_width, last_row_height;
    JQUANT_TBL* quant_table;
    void* dct_table;
};

struct jpeg_memory_mgr {                 // only access_virt_barray (the 9th method) is called
    void* alloc_small; void* alloc_large; void* alloc_sarray; void* alloc_barray;
    void* request_virt_sarray; void* request_virt_barray; void* realize_virt_arrays; void* access_virt_sarray;
    JBLOCKARRAY (*access_virt_barray)(void* cinfo, jvirt_barray_ptr ptr, JDIMENSION start_row, JDIMENSION num_rows,
                                      boolean_t writable);
    void* free_pool; void* self_destruct;
    long max_memory_to_use, max_alloc_chunk;
};

constexpr int kJpegLibVersion = 80;
constexpr int JCS_GRAYSCALE = 1;
constexpr int JCS_RGB = 2;
constexpr int JCS_YCbCr = 3;
constexpr int JPEG_HEADER_OK = 1;
constexpr int JPEG_HEADER_TABLES_ONLY = 2;

struct Api {
    jpeg_error_mgr* (*std_error)(jpeg_error_mgr*);
    void (*create)(jpeg_decompress_struct*, int, size_t);
    void (*mem_src)(jpeg_decompress_struct*, const unsigned char*, unsigned long);
    int (*read_header)(jpeg_decompress_struct*, boolean_t);
    boolean_t (*start)(jpeg_decompress_struct*);
    JDIMENSION (*read_scanlines)(jpeg_decompress_struct*, JSAMPARRAY, JDIMENSION);
    boolean_t (*finish)(jpeg_decompress_struct*);
    void (*destroy)(jpeg_decompress_struct*);
    jvirt_barray_ptr* (*read_coefficients)(jpeg_decompress_struct*);
    bool ok = false;
    char why[200] = "";
};

struct ErrJmp {
    jpeg_error_mgr pub;
    jmp_buf jb;
    char text[200];
};

void on_error(void* cinfo) {
    jpeg_decompress_struct* c = (jpeg_decompress_struct*)cinfo;
    ErrJmp* e = (ErrJmp*)c->err;
    char buf[200] = "";
    if (e->pub.format_message) e->pub.format_message(cinfo, buf);
    snprintf(e->text, sizeof(e->text), "%s", buf);
    longjmp(e->jb, 1);
}
// libjpeg reports recoverable stream damage (premature end of data, bad Huffman code, ...) as WARNINGS (msg_level < 0):
// it injects a fake EOI / grey blocks and carries on.  Pillow raises on such a tile ("image file is truncated"), so a
// damaged tile must fail here too instead of being embedded as grey pixels: count the warnings, check after decoding.
void on_message(void* cinfo, int msg_level) {
    if (msg_level < 0) ((jpeg_decompress_struct*)cinfo)->err->num_warnings++;
}

Api g_api;
std::once_flag g_once;

// One libjpeg session over an in-memory stream: the error manager, the setjmp target, create, the tables-only header (`tables`, may be
// null: TIFF's JPEGTables tag, read with jpeg_read_header(..., FALSE) in front of an abbreviated `data`, as libtiff does), the main
// header, `body(c, warned)`, destroy on every exit.  A libjpeg error inside the body longjmps back into this frame, which is still
// live; so the body holds nothing with a destructor.  The body returns 0, or -1 with its reason in `why`; `warned()` refuses (true,
// reason in `why`) once libjpeg has warned.  WHEN it is asked is the body's: a decode asks behind its last byte, the probe never does
// (a header libjpeg warns about -- junk in front of a marker, an unknown JFIF version -- still says what the stream is).
template <class Body>
int session(const Api& api, const unsigned char* tables, size_t tables_size, const unsigned char* data, size_t size, char* why,
            size_t why_cap, Body body) {
    jpeg_decompress_struct c;
    ErrJmp err;
    memset(&c, 0, sizeof(c));
    c.err = api.std_error(&err.pub);
    err.pub.error_exit = on_error;
    err.pub.emit_message = on_message;
    err.text[0] = 0;
    volatile bool created = false;          // written between setjmp and a possible longjmp
    if (setjmp(err.jb)) {
        snprintf(why, why_cap, "libjpeg: %s", err.text);
        if (created) api.destroy(&c);
        return -1;
    }
    api.create(&c, kJpegLibVersion, sizeof(jpeg_decompress_struct));
    created = true;
    const auto warned = [&] {
        if (err.pub.num_warnings <= 0) return false;
        snprintf(why, why_cap, "libjpeg reported %ld warning(s): truncated or corrupt JPEG stream", err.pub.num_warnings);
        return true;
    };
    int rc = -1;
    if (tables && tables_size && (api.mem_src(&c, tables, (unsigned long)tables_size), api.read_header(&c, 0) != JPEG_HEADER_TABLES_ONLY))
        snprintf(why, why_cap, "JPEGTables is not a tables-only stream");
    else if (api.mem_src(&c, data, (unsigned long)size), api.read_header(&c, 1) != JPEG_HEADER_OK)
        snprintf(why, why_cap, "not a JPEG stream");
    else
        rc = body(c, warned);
    api.destroy(&c);
    return rc;
}

#define refuse(...) (snprintf(why, why_cap, __VA_ARGS__), -1)

// decode one in-memory JPEG into dst (rows of `stride` bytes); returns 0 or fills `why`.
// `colour`: ap::kJpegColourInfer leaves libjpeg's inference alone; ap::kJpegColourRgb (a TIFF level tagged Photometric 2) overrides it
// for a three-component stream: the components are R, G, B whatever the markers say, and libjpeg copies them.
int decode_one(const Api& api, const unsigned char* data, size_t size, int want_w, int want_h, unsigned char* dst,
               size_t stride, char* why, size_t why_cap, const unsigned char* tables = nullptr, size_t tables_size = 0,
               int colour = ap::kJpegColourInfer) {
    return session(api, tables, tables_size, data, size, why, why_cap, [&](jpeg_decompress_struct& c, const auto& warned) {
        if (colour == ap::kJpegColourRgb && c.num_components == 3) c.jpeg_color_space = JCS_RGB;
        c.out_color_space = JCS_RGB;          // what PIL's convert("RGB") yields for YCbCr and greyscale streams alike
        api.start(&c);
        if ((int)c.output_width != want_w || (int)c.output_height != want_h || c.output_components != 3)
            return refuse("tile is %u x %u x %d, expected %d x %d x 3", c.output_width, c.output_height, c.output_components, want_w, want_h);
        while (c.output_scanline < c.output_height) {
            JSAMPROW rows[4];
            const JDIMENSION left = c.output_height - c.output_scanline, nrows = left < 4 ? left : 4;
            for (JDIMENSION r = 0; r < nrows; ++r) rows[r] = dst + (size_t)(c.output_scanline + r) * stride;
            api.read_scanlines(&c, rows, nrows);
        }
        api.finish(&c);
        return warned() ? -1 : 0;
    });
}

// The entropy-decoded half of a decode: header checks, then (slot != nullptr) libjpeg's Huffman decoder behind
// jpeg_read_coefficients and a copy of every component's quantisation table and blocks into `slot` (jpeg_slot.h).  Fills
// wh / sampling from the header; slot == nullptr stops there (ap_host_jpeg_probe).  A stream outside the device decoder's
// subset -- jpeg_host.h: jpeg_classify, and of libjpeg's own fields baseline Huffman at 8 bit -- or one libjpeg warned about is
// refused with its reason in `why` and nothing written to the slot.  A three-component stream is RGB coded when libjpeg infers so
// (Adobe transform 0, or ids 'R' 'G' 'B' without a JFIF / Adobe marker) or, under ap::kJpegColourRgb, because the container says so.
// An RGB-coded stream with a subsampled component is refused before anything else, with *sampling = ap::kJpegRgbSubsampled.
int read_one(const Api& api, const unsigned char* data, size_t size, int wh[2], int* sampling, int want_side, int want_sampling,
             unsigned char* slot, char* why, size_t why_cap, const unsigned char* tables = nullptr, size_t tables_size = 0,
             int colour = ap::kJpegColourInfer) {
    return session(api, tables, tables_size, data, size, why, why_cap, [&](jpeg_decompress_struct& c, const auto& warned) {
        const jpeg_component_info* comp = (const jpeg_component_info*)c.comp_info;
        const int nc = c.num_components, space = c.jpeg_color_space;
        int hv[3][2] = {{0, 0}, {0, 0}, {0, 0}};
        for (int ci = 0; comp && ci < nc && ci < 3; ++ci) hv[ci][0] = comp[ci].h_samp_factor, hv[ci][1] = comp[ci].v_samp_factor;
        const ap::JpegModel model = !comp ? ap::kJpegOtherModel : nc == 1 && space == JCS_GRAYSCALE ? ap::kJpegGrey :
                                    nc == 3 && (colour == ap::kJpegColourRgb || space == JCS_RGB) ? ap::kJpegRgbCoded :
                                    nc == 3 && space == JCS_YCbCr ? ap::kJpegYCbCr : ap::kJpegOtherModel;
        ap::JpegGeom g;
        const bool taken = ap::jpeg_classify(nc, hv, model, (int)c.image_width, (int)c.image_height, want_side, want_sampling,
                                             slot ? &g : nullptr, sampling, why, why_cap);
        if (*sampling == ap::kJpegRgbSubsampled) return -1;
        // what only libjpeg's fields say stands in front of the shared refusals
        if (c.progressive_mode) return refuse("progressive stream");
        if (c.arith_code) return refuse("arithmetic-coded stream");
        if (c.data_precision != 8) return refuse("%d-bit samples", c.data_precision);
        if (!taken) return -1;                // `why` still holds jpeg_classify's reason: none of the three above wrote over it
        wh[0] = (int)c.image_width;
        wh[1] = (int)c.image_height;
        if (!slot) return 0;
        jvirt_barray_ptr* arrays = api.read_coefficients(&c);
        if (!arrays) return refuse("jpeg_read_coefficients suspended");
        // jpeg_read_coefficients has consumed the stream up to its EOI marker, so every warning is in by now.  No
        // jpeg_finish_decompress before the copy: it releases the image pool, which holds comp_info and the coefficient arrays.
        if (warned()) return -1;
        const jpeg_memory_mgr* mem = (const jpeg_memory_mgr*)c.mem;
        for (int ci = 0; ci < g.ncomp; ++ci)
            if ((int)comp[ci].width_in_blocks != g.wb[ci] || (int)comp[ci].height_in_blocks != g.hb[ci] || !comp[ci].quant_table)
                return refuse("component %d: %u x %u blocks (expected %d x %d) or no quantisation table", ci, comp[ci].width_in_blocks,
                              comp[ci].height_in_blocks, g.wb[ci], g.hb[ci]);
        memset(slot, 0, ap::kJpegSlotHeader);
        for (int ci = 0; ci < g.ncomp; ++ci) {
            memcpy(slot + (size_t)ci * 128, comp[ci].quant_table->quantval, 128);
            const size_t row_bytes = (size_t)g.wb[ci] * sizeof(JBLOCK);
            for (int r = 0; r < g.hb[ci]; ++r) {
                JBLOCKARRAY rows = mem->access_virt_barray(&c, arrays[ci], (JDIMENSION)r, 1, 0);
                memcpy(slot + g.off[ci] + (size_t)r * row_bytes, rows[0], row_bytes);
            }
        }
        return 0;
    });
}
#undef refuse

// 8 x 8 grey JFIF (all pixels 128): the load-time self-check of the restated declarations
const unsigned char kProbe[] = {
    0xFF,0xD8,0xFF,0xE0,0x00,0x10,0x4A,0x46,0x49,0x46,0x00,0x01,0x01,0x00,0x00,0x01,0x00,0x01,0x00,0x00,
    0xFF,0xDB,0x00,0x43,0x00,
    1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,
    0xFF,0xC0,0x00,0x0B,0x08,0x00,0x08,0x00,0x08,0x01,0x01,0x11,0x00,
    0xFF,0xC4,0x00,0x14,0x00, 1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0, 0x00,                 // DC table: one code (length 1) -> category 0
    0xFF,0xC4,0x00,0x14,0x10, 1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0, 0x00,                 // AC table: one code (length 1) -> EOB
    0xFF,0xDA,0x00,0x08,0x01,0x01,0x00,0x00,0x3F,0x00,
    0x3F,                                                                             // bits 0 (DC diff 0), 0 (EOB), padding 1s
    0xFF,0xD9};

void load_api() {
    Api& a = g_api;
    void* h = dlopen("libjpeg.so.8", RTLD_NOW | RTLD_LOCAL);
    if (!h) { snprintf(a.why, sizeof(a.why), "libjpeg.so.8 not found (%s)", dlerror()); return; }
    auto sym = [&](const char* name) { return dlsym(h, name); };
    a.std_error = (decltype(a.std_error))sym("jpeg_std_error");
    a.create = (decltype(a.create))sym("jpeg_CreateDecompress");
    a.mem_src = (decltype(a.mem_src))sym("jpeg_mem_src");
    a.read_header = (decltype(a.read_header))sym("jpeg_read_header");
    a.start = (decltype(a.start))sym("jpeg_start_decompress");
    a.read_scanlines = (decltype(a.read_scanlines))sym("jpeg_read_scanlines");
    a.finish = (decltype(a.finish))sym("jpeg_finish_decompress");
    a.destroy = (decltype(a.destroy))sym("jpeg_destroy_decompress");
    a.read_coefficients = (decltype(a.read_coefficients))sym("jpeg_read_coefficients");
    if (!a.std_error || !a.create || !a.mem_src || !a.read_header || !a.start || !a.read_scanlines || !a.finish || !a.destroy ||
        !a.read_coefficients) {
        snprintf(a.why, sizeof(a.why), "libjpeg.so.8 lacks a required symbol");
        return;
    }
    unsigned char px[8 * 8 * 3];
    memset(px, 0, sizeof(px));
    char why[160] = "";
    if (decode_one(a, kProbe, sizeof(kProbe), 8, 8, px, 24, why, sizeof(why)) != 0) {
        snprintf(a.why, sizeof(a.why), "libjpeg.so.8 self-check failed: %s", why);
        return;
    }
    for (unsigned char v : px)
        if (v != 128) { snprintf(a.why, sizeof(a.why), "libjpeg.so.8 self-check decoded %d, expected 128", (int)v); return; }
    // the coefficient reader's declarations (component info, memory manager, quantisation table): the same probe is one
    // block with DC 0 under an all-ones table; poison first so that a reader that delivers nothing is caught too
    ap::JpegGeom g;
    ap::jpeg_geom(8, AP_JPEG_GRAY, &g);
    unsigned char slot[ap::kJpegSlotHeader + 128];
    memset(slot, 0x5A, sizeof(slot));
    int wh[2], sampling = -1;
    if (g.bytes != sizeof(slot) || read_one(a, kProbe, sizeof(kProbe), wh, &sampling, 8, AP_JPEG_GRAY, slot, why, sizeof(why)) != 0) {
        snprintf(a.why, sizeof(a.why), "libjpeg.so.8 coefficient self-check failed: %s", why);
        return;
    }
    const unsigned short* q = (const unsigned short*)slot;
    const short* blk = (const short*)(slot + ap::kJpegSlotHeader);
    bool good = wh[0] == 8 && wh[1] == 8 && sampling == AP_JPEG_GRAY;
    for (int k = 0; k < 64; ++k) good = good && q[k] == 1 && blk[k] == 0;
    if (!good) { snprintf(a.why, sizeof(a.why), "libjpeg.so.8 coefficient self-check read other values than the probe holds"); return; }
    a.ok = true;
}

// whole file -> buf; the message names the file
int read_file(const char* what, const char* path, std::vector<unsigned char>& buf) {
    FILE* f = fopen(path, "rb");
    AP_REQUIRE(f, "%s: cannot open %s", what, path);
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.resize(size > 0 ? (size_t)size : 1);
    const size_t got = size > 0 ? fread(buf.data(), 1, (size_t)size, f) : 0;
    fclose(f);
    AP_REQUIRE(size > 0 && got == (size_t)size, "%s: short read of %s", what, path);
    buf.resize((size_t)size);
    return AP_OK;
}

// the library, loaded and self-checked once; the message names the entry that asked
int ready(const char* what) {
    std::call_once(g_once, load_api);
    if (!g_api.ok) { ap::set_error("%s: %s", what, g_api.why); return AP_ERR_UNSUPPORTED; }
    return AP_OK;
}

}  // namespace

// ---- the in-memory "tables + stream" path (jpeg_host.h): what the file readers below and the TIFF reader share ----------
namespace ap {

int jpeg_mem_ready(char* why, size_t why_cap) {
    std::call_once(g_once, load_api);
    if (!g_api.ok) { snprintf(why, why_cap, "%s", g_api.why); return AP_ERR_UNSUPPORTED; }
    return AP_OK;
}

int jpeg_mem_pixels(const unsigned char* tables, size_t tables_size, const unsigned char* data, size_t size, int want_w, int want_h,
                    unsigned char* dst, size_t stride, char* why, size_t why_cap, int colour) {
    if (int rc = jpeg_mem_ready(why, why_cap)) return rc;
    return decode_one(g_api, data, size, want_w, want_h, dst, stride, why, why_cap, tables, tables_size, colour) == 0 ? AP_OK : AP_ERR_INVALID;
}

int jpeg_mem_coefficients(const unsigned char* tables, size_t tables_size, const unsigned char* data, size_t size, int wh[2],
                          int* sampling, int want_side, int want_sampling, unsigned char* slot, char* why, size_t why_cap, int colour) {
    if (int rc = jpeg_mem_ready(why, why_cap)) return rc;
    return read_one(g_api, data, size, wh, sampling, want_side, want_sampling, slot, why, why_cap, tables, tables_size, colour) == 0
               ? AP_OK : AP_ERR_INVALID;
}

}  // namespace ap

extern "C" int ap_host_decode_jpeg_tiles(void* dst, const char* const* paths, int n, int side) {
    AP_REQUIRE(dst && (paths || n == 0) && n >= 0 && side > 0, "ap_host_decode_jpeg_tiles: bad arguments");
    if (int rc = ready("ap_host_decode_jpeg_tiles")) return rc;
    std::vector<unsigned char> buf;
    const size_t tile_bytes = (size_t)side * side * 3;
    for (int i = 0; i < n; ++i) {
        AP_REQUIRE(paths[i], "ap_host_decode_jpeg_tiles: null path %d", i);
        if (int rc = read_file("ap_host_decode_jpeg_tiles", paths[i], buf)) return rc;
        char why[200] = "";
        if (decode_one(g_api, buf.data(), buf.size(), side, side, (unsigned char*)dst + (size_t)i * tile_bytes,
                       (size_t)side * 3, why, sizeof(why)) != 0) {
            ap::set_error("ap_host_decode_jpeg_tiles: %s: %s", paths[i], why);
            return AP_ERR_INVALID;
        }
    }
    return AP_OK;
}

extern "C" size_t ap_jpeg_slot_bytes_ex(int side, int sampling) {
    ap::JpegGeom g;
    return ap::jpeg_geom(side, sampling, &g) ? g.bytes : 0;
}

// the four codes this entry was published with; AP_JPEG_RGB stays an unknown sampling here
extern "C" size_t ap_jpeg_slot_bytes(int side, int sampling) { return sampling == AP_JPEG_RGB ? 0 : ap_jpeg_slot_bytes_ex(side, sampling); }

extern "C" int ap_host_jpeg_probe(const char* path, int* width, int* height, int* sampling) {
    AP_REQUIRE(path && width && height && sampling, "ap_host_jpeg_probe: null pointer");
    if (int rc = ready("ap_host_jpeg_probe")) return rc;
    std::vector<unsigned char> buf;
    if (int rc = read_file("ap_host_jpeg_probe", path, buf)) return rc;
    char why[200] = "";
    int wh[2] = {0, 0}, found = -1;
    if (read_one(g_api, buf.data(), buf.size(), wh, &found, 0, 0, nullptr, why, sizeof(why)) != 0) {
        ap::set_error("ap_host_jpeg_probe: %s: %s", path, why);
        return AP_ERR_INVALID;
    }
    *width = wh[0];
    *height = wh[1];
    *sampling = found;
    return AP_OK;
}

extern "C" int ap_host_jpeg_coefficients(void* slots, const char* const* paths, int n, int side, int sampling) {
    AP_REQUIRE(slots && (paths || n == 0) && n >= 0, "ap_host_jpeg_coefficients: bad arguments");
    const size_t stride = ap_jpeg_slot_bytes_ex(side, sampling);
    AP_REQUIRE(stride, "ap_host_jpeg_coefficients: bad side %d or sampling %d", side, sampling);
    if (int rc = ready("ap_host_jpeg_coefficients")) return rc;
    std::vector<unsigned char> buf;
    for (int i = 0; i < n; ++i) {
        AP_REQUIRE(paths[i], "ap_host_jpeg_coefficients: null path %d", i);
        if (int rc = read_file("ap_host_jpeg_coefficients", paths[i], buf)) return rc;
        char why[200] = "";
        int wh[2], found;
        if (read_one(g_api, buf.data(), buf.size(), wh, &found, side, sampling, (unsigned char*)slots + (size_t)i * stride, why,
                     sizeof(why)) != 0) {
            ap::set_error("ap_host_jpeg_coefficients: %s: %s", paths[i], why);
            return AP_ERR_INVALID;
        }
    }
    return AP_OK;
}
