/*
 * atlaspatch_hip.h -- C ABI of the MI355X (gfx950) hot path of the AtlasPatch drop-in.
 *
 * One shared library (libatlaspatch_hip.so), plain pointers and sizes, no torch or
 * C++ types in any signature.  Every entry point returns 0 on success or a
 * negative AP_ERR_* code; nothing throws, nothing synchronises the device unless
 * its comment says so, and the caller owns every buffer.  Device pointers are
 * HIP device pointers (what torch.Tensor.data_ptr() returns on ROCm); a stream is
 * a hipStream_t passed as void* (NULL = the default stream).
 *
 * Each block cites the reference interface it replaces (paths under
 * /root/reference/atlas_patch).  INTEGRATION.md shows the ctypes stubs a
 * maintainer of the reference would add.
 *
 * Streams and threads (tests/test_gpu_streams.py; the test that backs each sentence in brackets):
 *  - Operators may be called at the same time from several host threads and on several streams, as long as no call writes
 *    a buffer that another call reads or writes.  Nothing the library owns is shared between two streams' kernels: the split-K
 *    scratch of ap_sgemm / ap_sgemm_stacked is kept per (device, stream), grow-only, for the life of the process
 *    [test_splitk_against_splitk, test_stacked_splitk_against_batched_splitk, test_splitk_against_non_split_controls,
 *    test_first_use_in_a_fresh_process[growth], test_host_threads].
 *  - ap_last_error() is per thread [test_host_threads].
 *  - One engine handle may run forwards on several streams at once, given a workspace and an output of its own per
 *    forward [test_one_vit_handle_on_two_streams]; different handles are independent [test_two_engines_on_two_streams].
 *    Two restrictions, read from the engines' code [not covered by a test]: not while profiling is enabled (the handle
 *    owns the events), and with AP_VIT_OPT_TWO_HALF_OVERLAP at most one forward of n >= 512 at a time (the handle owns the
 *    side stream and its two events; the test runs one such forward beside a smaller one).
 *  - *_set_param / *_set_params / *_finalize / *_set_option / *_profile_* are not concurrent with a forward on the same
 *    handle [not covered by a test: it is a restriction].
 *  - The first use of an operator, or of a larger shape, may allocate, upload and wait for its own upload (the scratch
 *    above, the normalisation and cv2 tables): it must happen outside a stream capture, and, for the per-stream scratch, on
 *    the stream that is then captured.  A captured graph keeps pointing at the scratch of the stream it was captured on:
 *    replay it on one stream at a time.  State that is shared is complete before it is published; the zero row of
 *    ap_gemm_split_f16_windows mode 1 is zero-initialised memory of the library's code object, complete when it is loaded
 *    [test_first_use_in_a_fresh_process[zero_row], [lut_first], [attr_first]].
 *  - Caches are per device.  The hipFuncSetAttribute guards (attention, device contours) are per process: a process that
 *    drives several devices is not covered by these tests.
 */
#ifndef ATLASPATCH_HIP_H
#define ATLASPATCH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AP_OK 0
#define AP_ERR_INVALID (-1)      /* bad argument (null pointer, size, unsupported shape) */
#define AP_ERR_HIP (-2)          /* a HIP runtime call failed; see ap_last_error() */
#define AP_ERR_WORKSPACE (-3)    /* workspace too small */
#define AP_ERR_UNSUPPORTED (-4)  /* valid request this build has no kernel for */
#define AP_ERR_STATE (-5)        /* object not finalised / already finalised */
#define AP_ERR_CAPACITY (-6)     /* output buffer too small; needed count is reported */

/* element types of device tensors */
#define AP_F32 0
#define AP_F16 1
#define AP_BF16 2

typedef void* ap_stream_t;

/* ---- library ---------------------------------------------------------------------- */
#define AP_ABI_VERSION 20                 /* what THIS header declares; compare with ap_abi_version() before any other call */
int ap_abi_version(void);                 /* bumps when a signature or a struct layout changes */
const char* ap_last_error(void);          /* thread-local text of the last failure */
int ap_device_info(int device, char* name, int name_cap, int* cu_count, size_t* hbm_bytes);

/* ---- K1: patch preprocess ----------------------------------------------------------
 * Replaces the per-item CPU transform + collate + H2D + cast of
 * models/patch/base.py:42-45,84-99 (PatchDataset.__getitem__ + DataLoader + .to()).
 * y = ((float(x) / 255) - mean[c]) / std[c] with two true divisions and no FMA
 * contraction, i.e. bit-identical in f32 to torchvision's ToTensor + Normalize;
 * the cast to f16/bf16 happens after normalisation (base.py:95-99).
 *
 * src: device uint8 [n, h, w, 3] (HWC RGB).  Output window: rows crop_top..crop_top+oh,
 * cols crop_left..crop_left+ow (centre crop of torchvision ImageClassification; no resample).
 * Offsets into src and dst are 64-bit (buffers beyond 4 GiB are fine); one workgroup per image and band of 8 rows (patch
 * rows: ps rows), so n * bands <= 2^31 - 1 (AP_ERR_INVALID beyond, nothing launched). */
int ap_preproc_u8hwc_to_chw(const uint8_t* src, int n, int h, int w,
                            int crop_top, int crop_left, int oh, int ow,
                            const float mean[3], const float stdv[3],
                            void* dst /* [n,3,oh,ow] */, int dst_dtype, ap_stream_t stream);

/* The same call for any output width (additive to ABI v20): a width that is a multiple of 8 runs the kernel above under its
 * own checks; any other width (the transform of a plugin's torch module on a tile of any size, encoders/device_transform.py)
 * runs an element-per-lane kernel with the same table, so the same bits.  ow <= 2^24; n * ceil(oh / 8) <= 2^31 - 1. */
int ap_preproc_u8hwc_to_chw_any(const uint8_t* src, int n, int h, int w,
                                int crop_top, int crop_left, int oh, int ow,
                                const float mean[3], const float stdv[3],
                                void* dst /* [n,3,oh,ow] */, int dst_dtype, ap_stream_t stream);

/* Same arithmetic, output laid out for the patch-embed GEMM: dst[(i*gh+py)*gw+px][c*ps*ps+ky*ps+kx]
 * with gh = oh/ps, gw = ow/ps, row length ld (>= 3*ps*ps, zero padded). */
int ap_preproc_u8hwc_to_patchrows(const uint8_t* src, int n, int h, int w,
                                  int crop_top, int crop_left, int oh, int ow, int ps,
                                  const float mean[3], const float stdv[3],
                                  void* dst, int ld, int dst_dtype, ap_stream_t stream);

/* ---- host side of the tile ring ----------------------------------------------------------
 * Copies n decoded tiles (host pointers, bytes_each bytes each) into consecutive slots of a pinned staging buffer.
 * Plain memcpy outside the interpreter lock: the decode threads of the ring that replaces the serial tile loop of
 * services/feature_embedding.py:81-96 call it once per chunk, so an in-memory tile source is not serialised by
 * per-tile NumPy slice assignments.  Host only, no device work. */
int ap_host_gather_tiles(void* dst, const void* const* src, int n, size_t bytes_each);
/* The same for tiles stored as zlib-deflated raw RGB files (the synthetic slide's compressed tile store): reads and
 * inflates n files straight into consecutive slots, one call per chunk -- the shape a native reader for a real slide
 * format takes (the reference's per-tile Python read, services/feature_embedding.py:86-95, cannot leave the interpreter). */
int ap_host_inflate_tiles(void* dst, const char* const* paths, int n, size_t bytes_each);

/* Passport strings of services/storage.py:387-392 for n coords rows, without the per-row Python f-string (58 938 rows of a
 * 100 000 x 100 000 slide: 75 ms in the interpreter): out[i] = prefix + "__x{X}_y{Y}_rw{RW}_rh{RH}_lv{LV}" + suffix, where the
 * caller passes prefix = slide stem and suffix = "_mag{MAG}_tmag{TMAG}_total{TOTAL}"; each entry is `width` bytes (NumPy
 * S<width>: NUL padded, truncated when longer).  coords: HOST int32 [n, 5].  Host only. */
int ap_host_format_passports(const int32_t* coords, int n, const char* prefix, const char* suffix, char* out, int width);

/* The same for tiles stored as baseline JPEG files (what a real slide's tiles are; core/wsi/openslide_wsi.py:184-205 decodes
 * them one by one in the interpreter): reads and decodes n files into consecutive side x side x 3 RGB slots with the
 * system's libjpeg-turbo (libjpeg.so.8, loaded on first use; the pixels are the ones PIL's Image.open(...).convert("RGB")
 * gives).  AP_ERR_UNSUPPORTED when that library is not usable on this host (the caller then decodes tile by tile),
 * AP_ERR_INVALID for a tile that is not side x side or not decodable. */
int ap_host_decode_jpeg_tiles(void* dst, const char* const* paths, int n, int side);

/* ---- K0: JPEG tile decode split at the entropy decoder ------------------------------------------
 * Only a JPEG stream's Huffman decode is serial; dequantisation, the 8 x 8 inverse DCT, chroma upsampling and YCbCr -> RGB
 * are independent per block and exactly defined in integers.  The host half (libjpeg-turbo's jpeg_read_coefficients, same
 * dlopen'd libjpeg.so.8 as above) delivers a tile's quantised coefficients in a SLOT; the device half turns n slots into the
 * RGB tiles ap_host_decode_jpeg_tiles / PIL's Image.open(...).convert("RGB") give, bit for bit (libjpeg's JDCT_ISLOW with
 * fancy upsampling, restated).  Subset: baseline Huffman, 8 bit, greyscale, YCbCr at one of the samplings below, or three 1 x 1
 * components coded as R, G, B (AP_JPEG_RGB: the slot and the geometry of 4:4:4, decoded without the colour transform).  A FILE is RGB
 * coded when libjpeg infers so (Adobe marker with transform 0, or ids 'R' 'G' 'B' without a JFIF / Adobe marker); a TIFF TILE when its
 * level is tagged PhotometricInterpretation 2, whatever its markers say (libtiff's rule, below).
 *
 * A slot is self-contained and ap_jpeg_slot_bytes(side, sampling) long (a multiple of 128; 0 on bad arguments):
 *   uint16 quant[3][64]   natural order, the components' own order, padded to 512 bytes
 *   per component         int16 [hb][wb][64], natural order, block rows major; wb x hb = ceil(downsampled size / 8), the
 *                         component's width_in_blocks x height_in_blocks (not libjpeg's MCU-padded array width)
 * (4:2:0 at side 256: 512 + 196 608 bytes, the RGB tile it replaces on the way to the device). */
#define AP_JPEG_GRAY 0
#define AP_JPEG_444 1
#define AP_JPEG_422 2                     /* luma 2x1 */
#define AP_JPEG_420 3                     /* luma 2x2 */
#define AP_JPEG_RGB 4                     /* three 1x1 components coded as R, G, B: the slot of 4:4:4, no colour transform */
size_t ap_jpeg_slot_bytes(int side, int sampling);
/* AP_JPEG_RGB came after the three entries that are handed a sampling and no stream to read it from -- ap_jpeg_slot_bytes,
 * ap_jpeg_decode_tiles, ap_jpeg_entropy_decode_tiles -- were published with "an unknown sampling is refused" for every code but the
 * first four.  They keep that contract to the letter (AP_JPEG_RGB: 0 / AP_ERR_INVALID).  Their *_ex twins have the same signatures
 * and the same behaviour and take all five codes; the host entries (probe, coefficients, streams, the TIFF reader), which report or
 * check the code against a stream, take AP_JPEG_RGB as they are.  A caller that handles RGB-coded tiles calls the *_ex entries. */
size_t ap_jpeg_slot_bytes_ex(int side, int sampling);
/* Header of one file: its size and sampling.  AP_ERR_INVALID for a stream outside the subset (the message names the file
 * and the reason), AP_ERR_UNSUPPORTED without a usable libjpeg.  Host only. */
int ap_host_jpeg_probe(const char* path, int* width, int* height, int* sampling);
/* Reads n files and entropy-decodes them into consecutive slots at `slots` (host memory, e.g. the ring's pinned staging
 * buffer), one call per chunk outside the interpreter lock.  AP_ERR_INVALID, naming the file and the reason, for a stream
 * that is progressive, arithmetic coded, not 8 bit, not grey / YCbCr / RGB, of another sampling than `sampling` (a YCbCr stream asked
 * for as AP_JPEG_RGB and an RGB-coded one asked for as anything else included), RGB coded with a subsampled component, not side x side,
 * or that libjpeg warned about (truncated / corrupt): that tile's slot and the slots after it are left untouched, the ones
 * before it are complete.  AP_ERR_UNSUPPORTED without a usable libjpeg.  Host only, no device work. */
int ap_host_jpeg_coefficients(void* slots, const char* const* paths, int n, int side, int sampling);
/* Device half: slots (device, 16-byte aligned, n slots at ap_jpeg_slot_bytes pitch) -> rgb uint8 [n, side, side, 3] (device,
 * 16-byte aligned).  Dequantise, inverse DCT, range limit, fancy upsampling, colour conversion in one kernel; no workspace.
 * AP_JPEG_RGB (ap_jpeg_decode_tiles_ex only): the components are written as R, G, B as they come out of the range limit, which is
 * what libjpeg's copy gives.
 * Reads nothing beyond n * slot_bytes and writes nothing beyond n * side * side * 3.  AP_ERR_INVALID for null or misaligned
 * pointers, side <= 0, a side whose band does not fit one workgroup's 64 KB of LDS (every sampling takes side <= 976), n < 0,
 * an unknown sampling; n == 0 is AP_OK. */
int ap_jpeg_decode_tiles(const void* slots, int n, int side, int sampling, uint8_t* rgb, ap_stream_t stream);
int ap_jpeg_decode_tiles_ex(const void* slots, int n, int side, int sampling, uint8_t* rgb, ap_stream_t stream);   /* + AP_JPEG_RGB */

/* ---- K0: the Huffman decode on the device as well (additive: AP_ABI_VERSION stays 20) ------------------------------------
 * The host only reads a tile's bytes and walks them once; the ring carries the compressed stream.  Per tile a DESCRIPTOR of
 * ap_jpeg_stream_header_bytes() = 2048 bytes (little endian, 16-byte aligned; csrc/jpeg_stream.h is the same layout as a struct):
 *   bytes    0 ..  383   uint16 quant[3][64], natural order, the components' own order (a slot's first 384 bytes)
 *   bytes  384 ..  447   uint8 huff_counts[4][16]: codes of length 1 .. 16 of the tables DC0, DC1, AC0, AC1 (raw DHT form)
 *   bytes  448 .. 1471   uint8 huff_symbols[4][256]
 *   bytes 1472 .. 1479   uint8 dc_sel[3], 0, ac_sel[3], 0: each component's table selectors
 *   bytes 1480 .. 1487   uint32 ncomp, uint32 payload_bytes
 *   bytes 1488 .. 1495   uint64 payload_offset into the arena, a multiple of 16
 *   bytes 1496 .. 1503   uint32 restart_interval (MCUs per interval; 0 = a restart-free tile), uint32 restart_count (intervals)
 *   bytes 1504 .. 1511   uint64 restart_table_offset into the arena, a multiple of 16
 *   bytes 1512 .. 2047   zero
 * and its PAYLOAD in a packed ARENA: the entropy-coded segment from the end of the SOS header to the marker that ends it (or
 * the end of the stream), byte stuffing removed, 16-byte aligned, zero filled to the next multiple of 16; whatever follows the
 * terminating marker is ignored, as libjpeg ignores it.  The three restart fields are zero in everything the entries without
 * AP_JPEG_STREAM_RESTART stage (see ap_host_jpeg_streams_ex below for the restart table).
 * The staging functions parse SOI, DQT, DHT, SOF0, DRI, SOS and the APPn / COM segments they skip with code of their own (no
 * libjpeg), every segment length checked against the buffer; the colour model of a three-component stream is inferred from JFIF /
 * Adobe markers and component ids exactly as libjpeg infers it.  Admitted: the subset of ap_host_jpeg_coefficients (AP_JPEG_RGB
 * included: an RGB-coded stream when, and only when, that code is asked for) restricted to baseline SOF0, one scan with every
 * component in frame order, a side that is a multiple of the MCU size (8, or 16 along a subsampled axis) and <= 976, no restart
 * interval and no RSTn marker (ap_host_jpeg_streams, ap_host_tiff_tile_streams and their _ex twins at flags 0; the _ex entries admit
 * both with AP_JPEG_STREAM_RESTART), Huffman tables 0 / 1 that exist and form a canonical code without over-subscription.  Everything
 * else is refused with AP_ERR_INVALID and the reason; the refusal contract is the one of ap_host_jpeg_coefficients: the tiles before
 * the first refused one are complete (*arena_used covers them), the descriptors from it on are untouched.  A tile that would overflow
 * the arena is refused too.  Host only, no device work. */
size_t ap_jpeg_stream_header_bytes(void);
/* bytes: the largest file size among paths, rounded up to 16: n times that is an arena no n of these tiles overflow. */
int ap_host_jpeg_stream_bound(const char* const* paths, int n, size_t* bytes);
/* The JPEG tile store.  descs: n descriptors; arena (16-byte aligned, arena_cap bytes): each file is read straight to where its
 * payload will start and unstuffed in place; *arena_used: the bytes of the arena that hold payloads afterwards. */
int ap_host_jpeg_streams(void* descs, void* arena, size_t arena_cap, size_t* arena_used, const char* const* paths, int n, int side,
                         int sampling);
/* RESTART INTERVALS (additive: AP_ABI_VERSION stays 20).  flags 0: ap_host_jpeg_streams to the letter, refusals and reasons included;
 * any bit but AP_JPEG_STREAM_RESTART is AP_ERR_INVALID.  With AP_JPEG_STREAM_RESTART a DRI segment is admitted, in the stream and in a
 * TIFF level's JPEGTables; the interval in force is the one of the tile's own stream, because libjpeg resets it at every SOI
 * (jdmarker.c: get_soi): a level whose DRI stands in its JPEGTables alone is one libjpeg cannot read either.  An interval of 0, or of
 * at least the frame's MCU count, means no marker: the tile is staged restart free, the three restart fields zero.  Otherwise
 * restart_interval = the DRI value, restart_count = ceil(MCUs / restart_interval), the RSTn markers are removed from the payload as
 * well (the padding bits in front of a marker stay: the tail of their interval), and the RESTART TABLE follows in the arena at the
 * first 16-byte boundary behind the payload's zero fill: restart_count little-endian uint32, entry k = the byte offset, relative to
 * the payload's first byte, at which interval k starts; entry 0 is 0, the entries are strictly increasing and below payload_bytes;
 * zero filled to a multiple of 16; *arena_used covers it.  A table of interval 1 takes 4 bytes per MCU: an arena share of the largest
 * file plus that, each rounded up to 16, is never overflowed.  Refused, because libjpeg would warn and the host reader refuses on
 * warnings: another number of markers than restart_count - 1, a marker whose number is not the next of RST0, RST1, ... modulo 8, a
 * marker at the scan's start, directly behind another or directly in front of the scan's end, a DRI segment whose length is not 4.  A
 * restart marker outside a scan stays refused. */
#define AP_JPEG_STREAM_RESTART 1
int ap_host_jpeg_streams_ex(void* descs, void* arena, size_t arena_cap, size_t* arena_used, const char* const* paths, int n, int side,
                            int sampling, int flags);
/* Device: descs (n descriptors) and arena (arena_bytes bytes), both device, 16-byte aligned -> slots: exactly the coefficient
 * slots of ap_jpeg_slot_bytes(side, sampling) pitch that ap_host_jpeg_coefficients fills (quantisers copied in, every coefficient
 * the stream does not code zero, DC values accumulated; bytes 384 .. 511 are padding and unspecified), so ap_jpeg_decode_tiles and
 * ap_gather_patches run unchanged behind it.  status (device int32 [n]): 0, or the reason the tile's slot is NOT to be used:
 * AP_JPEG_ENTROPY_BAD_CODE (bits no code matches), _BAD_INDEX (a run past coefficient 63: libjpeg folds it, this decoder flags it),
 * _EXHAUSTED (bits ran out before the last block), _LEFTOVER (whole bytes left after it), _BAD_DESCRIPTOR (a field outside its
 * bounds: component count, selectors, tables, or a payload that does not lie inside arena_bytes).  One workgroup per tile;
 * self-synchronising parallel Huffman decode over subsequences of subsequence_bits (0 = the default 1024; else a multiple of 32
 * in [32, 2^20]; a payload of more than 4096 subsequences gets longer ones).  On any input it reads nothing beyond n descriptors
 * and arena_bytes and writes nothing beyond n slots and n status words.  AP_ERR_INVALID for null or misaligned pointers, n < 0, a
 * side above 976 or no multiple of the MCU size, an unknown sampling, a bad subsequence_bits; n == 0 is AP_OK. */
#define AP_JPEG_ENTROPY_BAD_CODE 1
#define AP_JPEG_ENTROPY_BAD_INDEX 2
#define AP_JPEG_ENTROPY_EXHAUSTED 3
#define AP_JPEG_ENTROPY_LEFTOVER 4
#define AP_JPEG_ENTROPY_BAD_DESCRIPTOR 5
int ap_jpeg_entropy_decode_tiles(const void* descs, const void* arena, size_t arena_bytes, int n, int side, int sampling, void* slots,
                                 int32_t* status, int subsequence_bits, ap_stream_t stream);
int ap_jpeg_entropy_decode_tiles_ex(const void* descs, const void* arena, size_t arena_bytes, int n, int side, int sampling, void* slots,
                                    int32_t* status, int subsequence_bits, ap_stream_t stream);                     /* + AP_JPEG_RGB */
/* The same signature, argument checks and sampling codes as ap_jpeg_entropy_decode_tiles_ex, for launches that may hold tiles with
 * restart intervals (ATLASPATCH_JPEG_RESTART_DEVICE=1 on top of the two other switches makes the ring stage and decode them). Each
 * tile is decoded by the path its restart_interval selects; two kernels are launched over the n tiles and a workgroup whose tile is
 * not of its kind returns after reading the restart fields.  All three zero: slot and status byte for byte those of
 * ap_jpeg_entropy_decode_tiles_ex (an interval of 0 beside a count or a table offset is _BAD_DESCRIPTOR).  Otherwise one workgroup of
 * 256 lanes, lane l decoding the intervals l, l + 256, ... one after the other: every interval starts byte aligned, at block 0 of MCU
 * k * restart_interval, with the DC predictors at zero, so there is no guessed state, no rounds and no DC prefix sum, and
 * subsequence_bits (still checked) is not used.  The status codes PER INTERVAL: _BAD_CODE and _BAD_INDEX as above; _EXHAUSTED: an
 * interval's bits ran out before its last block; _LEFTOVER: one or more whole bytes are left in an interval behind its last block
 * (libjpeg counts them as discarded and warns); _BAD_DESCRIPTOR also: a restart_interval at or above the frame's MCU count (the
 * stager stages such a tile restart free), a restart_count that is not ceil(MCUs / restart_interval), a table that does not lie
 * inside arena_bytes, entry 0 not 0, an entry not strictly above its predecessor or not below payload_bytes.  The tile's status is
 * the first error in interval order.  The same memory-safety contract on any input: a table entry is read only below the checked
 * count, a payload word only below the interval's checked end. */
int ap_jpeg_entropy_decode_tiles_rst(const void* descs, const void* arena, size_t arena_bytes, int n, int side, int sampling, void* slots,
                                     int32_t* status, int subsequence_bits, ap_stream_t stream);

/* The same for a slide OpenSlide can open (the reference's production tile source): core/wsi/openslide_wsi.py:184-205 reads
 * one region per call in the interpreter -- openslide-python's read_region (premultiplied ARGB -> RGBA in its C helper, a
 * PIL image) + .convert("RGB") + np.array.  ap_host_openslide_read_tiles reads n regions of w x h pixels at `level` with
 * libopenslide's own openslide_read_region (thread-safe on one handle) and writes packed RGB into consecutive w*h*3-byte
 * slots: un-premultiplied exactly as openslide-python does (alpha 255: as stored; 0 < alpha < 255: (uint8)(255 * c / alpha);
 * alpha 0: the word's bytes as they lie, i.e. black for a premultiplied buffer), alpha dropped as PIL's RGBA -> RGB does.
 * xy: HOST int64 [n, 2] level-0 coordinates of the regions' top-left corners (openslide's convention).
 * libopenslide is resolved at first use by dlopen ($ATLASPATCH_LIBOPENSLIDE = explicit path, else libopenslide.so.1 /
 * .so.0 / .so): ap_host_openslide_available() = 1 / 0; without it open returns AP_ERR_UNSUPPORTED and the caller keeps the
 * per-tile openslide-python path.  The handle is independent of any openslide-python object on the same file. */
typedef struct ap_openslide ap_openslide;
int ap_host_openslide_available(void);
int ap_host_openslide_open(const char* path, ap_openslide** out);
int ap_host_openslide_read_tiles(ap_openslide* slide, const int64_t* xy, int n, int level, int w, int h, void* dst_rgb);
void ap_host_openslide_close(ap_openslide* slide);

/* ---- K0: tiled-JPEG TIFF / Aperio SVS slides, read natively (additive: AP_ABI_VERSION stays 20) -------
 * A dependency-free, read-only reader (no libtiff, no OpenSlide; pread only, so one handle serves every decode thread at once
 * and holds no file position).  Accepted: classic TIFF and BigTIFF in both byte orders, an IFD chain without cycles of at most
 * 4096 IFDs, tiled IFDs with Compression 7 (JPEG), BitsPerSample 8, SamplesPerPixel 1 or 3, PlanarConfiguration 1, an optional
 * JPEGTables stream per IFD.  Those IFDs are the LEVELS, widest first; stripped IFDs (Aperio's thumbnail, label, macro) are
 * skipped.  A tile whose offset or byte count is 0 is a MISSING tile.  ap_host_tiff_open refuses, naming the reason
 * (AP_ERR_UNSUPPORTED: no tiled JPEG level, another compression -- Aperio JPEG 2000 33003 / 33005, LZW, deflate, old-style
 * JPEG --, other sample layouts; AP_ERR_INVALID: an offset, count or tile extent outside the file, a tile size that is no
 * multiple of 16, tile counts that do not match the grid, arithmetic that would overflow, not a TIFF): the caller falls back
 * to another backend.  The file is untrusted: every offset read from it is checked against the file size before use.
 * Host only, no device work. */
typedef struct ap_tiff ap_tiff;
int ap_host_tiff_open(const char* path, ap_tiff** out);
void ap_host_tiff_close(ap_tiff* slide);
/* levels: the level count; resolution: double [2] = XResolution, YResolution of level 0 (0 = absent); resolution_unit: its
 * ResolutionUnit (1 none, 2 inch -- TIFF's default --, 3 centimetre); level 0's ImageDescription, NUL terminated and truncated to
 * description_cap, its full length in *description_bytes (description may be null with description_cap 0). */
int ap_host_tiff_info(const ap_tiff* slide, int* levels, double* resolution, int* resolution_unit, char* description,
                      size_t description_cap, size_t* description_bytes);
/* geometry: int64 [8] = width, height, tile_w, tile_h, tiles_x, tiles_y, sampling, bytes of the JPEGTables stream.
 * sampling: the AP_JPEG_* value probed from the level's first present tile, or -1 when the level's streams are outside
 * ap_jpeg_decode_tiles' subset (progressive, not square, wider than 976, no usable libjpeg, RGB-inferred streams in a level that is
 * not tagged RGB).  COLOUR MODEL, per level, by libtiff's rule: SamplesPerPixel 3 with PhotometricInterpretation (tag 262) = 2 makes
 * the level RGB CODED -- its tiles' three components are R, G, B whatever the streams' markers and component ids say, on every
 * route -- and it reports AP_JPEG_RGB (or -1).  Such a level whose first present tile has a subsampled component is refused at open
 * (AP_ERR_UNSUPPORTED, naming the sampling factors; libtiff rejects it with "Improper JPEG sampling factors").  Any other value of
 * the tag, or none, leaves the colour model to libjpeg's inference from the stream, as for a file. */
int ap_host_tiff_level(const ap_tiff* slide, int level, int64_t* geometry);
/* present: uint8 [tiles_y * tiles_x], row major: 1 = the file holds the tile, 0 = a missing tile. */
int ap_host_tiff_tile_present(const ap_tiff* slide, int level, uint8_t* present);
/* The host pixel route: n RGB patches [h, w, 3] into consecutive slots at dst, patch i with its top-left corner at LEVEL
 * coordinates xy[i] (HOST int64 [n, 2]).  The covered tiles are decoded by the dlopen'd libjpeg of ap_host_decode_jpeg_tiles
 * (JPEGTables through jpeg_read_header(..., FALSE) first, then the tile stream, as libtiff and OpenSlide do; in an RGB-coded level
 * jpeg_color_space is set to JCS_RGB before the decode starts, so libjpeg copies the components; elsewhere the colour space is the
 * one libjpeg infers from the stream), each tile once per call however many
 * patches cover it.  Pixels outside the level and pixels of missing tiles are 0; the padding of edge tiles never shows.
 * AP_ERR_INVALID, naming level and tile, for a tile that is not tile_w x tile_h, not decodable or that libjpeg warned about;
 * AP_ERR_UNSUPPORTED without a usable libjpeg. */
int ap_host_tiff_read_patches(const ap_tiff* slide, int level, const int64_t* xy, int n, int w, int h, void* dst);
/* The coefficient route (levels with sampling >= 0): entropy-decodes the m tiles tile_ids[i] = ty * tiles_x + tx (HOST int32)
 * into consecutive ap_jpeg_slot_bytes(tile_w, sampling) slots, the slot format and the refusals of ap_host_jpeg_coefficients.
 * A missing tile is refused too: the caller marks it absent in its gather plan instead of asking for it. */
int ap_host_tiff_tile_coefficients(const ap_tiff* slide, int level, const int32_t* tile_ids, int m, void* slots);
/* The stream route, the twin of ap_host_tiff_tile_coefficients for ap_jpeg_entropy_decode_tiles: every tile is read by pread
 * straight into the arena and staged as ap_host_jpeg_streams stages a file, the level's JPEGTables parsed once per call.
 * ap_host_tiff_max_tile_bytes: the level's largest TileByteCounts entry rounded up to 16 (0 on bad arguments): m times that is an
 * arena no m tiles of the level overflow. */
size_t ap_host_tiff_max_tile_bytes(const ap_tiff* slide, int level);
int ap_host_tiff_tile_streams(const ap_tiff* slide, int level, const int32_t* tile_ids, int m, void* descs, void* arena,
                              size_t arena_cap, size_t* arena_used);
/* flags as for ap_host_jpeg_streams_ex: 0 is ap_host_tiff_tile_streams to the letter; AP_JPEG_STREAM_RESTART admits a DRI segment in
 * the level's JPEGTables and in a tile's own stream; the tile's own is the one in force (its SOI resets the level's, as in libjpeg). */
int ap_host_tiff_tile_streams_ex(const ap_tiff* slide, int level, const int32_t* tile_ids, int m, void* descs, void* arena,
                                 size_t arena_cap, size_t* arena_used, int flags);

/* Device: patches that do not sit on the tile grid, assembled from decoded tiles (the output of ap_jpeg_decode_tiles).
 *   tiles  uint8 [m, ts, ts, 3]      device, 16-byte aligned
 *   plan   int32 [n, 4 + G*G]        per patch: ox, oy, vw, vh, then G*G tile slots row-major (-1 = a missing tile)
 *   out    uint8 [n, ph, pw, 3]      device, 16-byte aligned
 *   out[p][r][c] = (r < vh && c < vw && slot >= 0) ? tiles[slot][(oy+r) % ts][(ox+c) % ts] : 0
 *                  with slot = plan[p][4 + ((oy+r)/ts)*G + (ox+c)/ts]
 * 0 <= ox, oy < ts; G >= ceil((max(pw, ph) + ts - 1) / ts); vw <= pw and vh <= ph clip the patch at the level's right and
 * bottom edge (TIFF edge tiles are stored full size; their padding must not leak).  plan_host is the HOST copy: it is checked
 * here, before anything is uploaded or launched, and then copied to plan_dev (device, n * (4 + G*G) int32) on `stream`; it
 * must stay unchanged until that copy has run (pinned memory keeps the call asynchronous).  One lane forms 16 output bytes
 * from aligned loads and a byte-align step; writes nothing beyond n * ph * pw * 3.  AP_ERR_INVALID, with nothing launched, for
 * null or misaligned pointers, n < 0, m < 0, ts / pw / ph / G <= 0, a G too small, ox / oy / vw / vh out of range, a slot >= m,
 * tiles or (n > 1) patches whose starts are not 16-byte aligned (ts * ts * 3 or ph * pw * 3 no multiple of 16), a patch of
 * 2^24 bytes or more.  n == 0 is AP_OK. */
int ap_gather_patches(const uint8_t* tiles, int m, int ts, const int32_t* plan_host, int32_t* plan_dev, int n, int G, int pw, int ph,
                      uint8_t* out, ap_stream_t stream);

/* Host twin of ap_synth_tiles (below): renders n square tiles of a synthetic slide into consecutive slots of a pinned
 * staging buffer, outside the interpreter lock -- the synthetic slide's "native decoder" behind the ring's batched read
 * hook, so the host -> ring -> HBM path can be driven at full rate on the 100 000 x 100 000 slide.  xy: HOST int32 [n, 2]
 * level-0 corners; ellipses: HOST int64 [k, 4].  Bit-identical to core/wsi/synth_pixels.py::render_region. */
int ap_host_synth_tiles(void* dst, const int32_t* xy, int n, int side, int level_ds, int level,
                        int64_t width, int64_t height, uint32_t seed, const int64_t* ellipses, int k);

/* ---- Pillow-exact tile resampling ------------------------------------------------------
 * Replaces the PIL resize inside the per-item transform of encoders whose transform starts with Resize:
 * timm's Resize(224, bicubic) for uni_v1 (models/patch/uni.py:48-49) and open_clip's Resize(448, bicubic)
 * for conch_v1 (models/patch/conch.py:35-38), applied by PatchDataset.__getitem__ (models/patch/base.py:42-45).
 * Bit-identical to PIL.Image.resize for uint8 RGB: horizontal then vertical pass, 22-bit fixed-point weights.
 * bounds_* : device int32 [out, 2] (first input index, tap count); coeffs_* : device int32 [out, ksize_*]
 * (the tables of Pillow's precompute_coeffs + normalize_coeffs_8bpc, built by the host);
 * src uint8 [n, h, w, 3] -> dst uint8 [n, oh, ow, 3]; tmp: device scratch of n*h*ow*3 bytes.
 * Offsets into src, tmp and dst are 64-bit.  More than 65535 images take the two-pass kernels whatever the shape (the same
 * bytes); n*h*ow and n*oh*ow are at most 2^39 - 256 (fewer than 2^31 workgroups of 256; AP_ERR_INVALID beyond, nothing launched). */
int ap_resample_u8(const uint8_t* src, int n, int h, int w, uint8_t* dst, int oh, int ow,
                   const int32_t* bounds_x, const int32_t* coeffs_x, int ksize_x,
                   const int32_t* bounds_y, const int32_t* coeffs_y, int ksize_y,
                   uint8_t* tmp, ap_stream_t stream);

/* Pillow's Image.reduce((fx, fy), box) for one uint8 RGB image: the integer box reduction that Image.thumbnail(...,
 * reducing_gap=2.0) -- the reference's thumbnail call, services/segmentation.py:202-206, Pillow defaults -- runs before its
 * bicubic resize.  out[oy][ox] = ((sum of the block + n / 2) * (uint32)(2^32 / (256 n))) >> 24 (uint32 arithmetic, the
 * multiplier evaluated in float32), partial blocks at the right / bottom edge averaged over the pixels they have.
 * src: device uint8 [h, w, 3]; box = (box_x, box_y, box_w, box_h) inside it; dst: device uint8
 * [ceil(box_h / fy), ceil(box_w / fx), 3].  Bit-identical to Pillow (tested against it).  The resize that follows is
 * ap_resample_u8 with tables built for Pillow's `box` argument (utils/resample.py::pillow_resample_tables). */
int ap_pillow_reduce_u8(const uint8_t* src, int h, int w, int box_x, int box_y, int box_w, int box_h, int fx, int fy,
                        uint8_t* dst, ap_stream_t stream);

/* ---- cv2.resize for uint8 RGB ----------------------------------------------------------
 * Replaces the host cv2.resize calls of the path: services/feature_embedding.py:94-95 and
 * services/extraction.py:112-113 (cv2.resize(patch, (ps, ps)), INTER_LINEAR, on every tile whose level read is
 * not patch_size) and core/wsi/iwsi.py:305-321 (the 1.25x thumbnail: INTER_AREA when shrinking, INTER_CUBIC when
 * enlarging, INTER_LINEAR on request).  OpenCV's 8-bit arithmetic restated: integer-ratio area averages
 * (2 x 2 -> (sum + 2) >> 2, which INTER_LINEAR at exactly 2 x 2 is re-routed to), float32 area cells for other
 * shrink ratios, 11-bit fixed-point bilinear / bicubic (A = -0.75) with OpenCV's two-stage rounding; dsize equal
 * to the source size is a copy.  Per-axis tables are built by the library on first use of a shape (one
 * synchronous upload), then cached.
 * src: device uint8 [n, h, w, 3] -> dst: device uint8 [n, oh, ow, 3].  interpolation: cv2's constants.
 * flags: AP_CV_CUBIC_SCALAR = bicubic vertical pass in int32 for every element (OpenCV's scalar code); default =
 * what an x86-64 build executes (float32 vector loop for all but the last (ow * 3) % 8 elements of a row).
 * Offsets into src and dst are 64-bit; n * oh * ow is at most 2^39 - 256 (AP_ERR_INVALID beyond, nothing launched). */
#define AP_CV_INTER_LINEAR 1
#define AP_CV_INTER_CUBIC 2
#define AP_CV_INTER_AREA 3
#define AP_CV_CUBIC_SCALAR 1
int ap_cv2_resize_u8(const uint8_t* src, int n, int h, int w, uint8_t* dst, int oh, int ow,
                     int interpolation, int flags, ap_stream_t stream);

/* ---- tile content statistics (--no-fast-mode filters) -------------------------------
 * Replaces utils/image.py:7-41 (is_black_patch / is_white_patch), which services/extraction.py:112-116
 * applies to every candidate tile: counts[i] = { #pixels with cv2 RGB2GRAY < black_thresh,
 * #pixels with cv2 RGB2HSV S < white_sat_thresh and V >= white_value_thresh } (OpenCV's 8-bit fixed-point
 * conversions, bit-exact).  The caller compares count / (h*w) with 0.7 like the reference.
 * tiles: device uint8 [n, h, w, 3] (16-byte aligned, h*w % 16 == 0, a tile below 2^31 bytes); counts: device uint32 [n, 2].
 * Any n: more than 65535 tiles run as several launches on `stream`; offsets into tiles are 64-bit. */
int ap_tile_content_counts(const uint8_t* tiles, int n, int h, int w, int black_thresh,
                           int white_sat_thresh, int white_value_thresh, uint32_t* counts,
                           ap_stream_t stream);

/* ---- ViT encoder -------------------------------------------------------------------
 * Replaces `forward_fn(batch) or model(batch)` of models/patch/base.py:100 for the
 * ViT family the reference registers as vit_b_16 / vit_l_16 (models/patch/vit.py:9-38)
 * and uni_v1 (models/patch/uni.py:13-60): conv patch-embed, CLS + pos-embed, pre-LN
 * blocks (packed-QKV MHA, erf-GELU MLP, optional LayerScale), final LN, CLS token. */
typedef struct ap_vit ap_vit;

/* ABI v20: the structure is growth-safe.  Its first member is its own size as the CALLER compiled it; new fields are only
 * ever appended and all-zero always means "the behaviour before the field existed".  ap_vit_create reads exactly
 * struct_size bytes and accepts only sizes this structure has had in some ABI version:
 *   struct_size == ap_sizeof_vit_config()            the caller and the library agree;
 *   an earlier ABI's size (>= AP_VIT_CONFIG_SIZE_V20)  an older caller: the fields it does not know are taken as zero;
 *   struct_size > ap_sizeof_vit_config()               a newer caller on an older library: AP_ERR_UNSUPPORTED, unread;
 *   anything else                                      AP_ERR_INVALID, unread -- in particular a binding written for ABI <= 19,
 *                                                      whose structure had no size member and started with image_size
 *                                                      (224, 448, 518: never a size of this structure).
 * Fill the structure through ap_vit_config_init (C: `ap_vit_config_init(&cfg, sizeof cfg)`; ctypes:
 * `lib.ap_vit_config_init(byref(cfg), sizeof(cfg))`) and a binding can never hand over an uninitialised tail. */
typedef struct ap_vit_config {
    uint32_t struct_size; /* sizeof(ap_vit_config) as the caller sees it; written by ap_vit_config_init */
    int image_size;      /* 224 */
    int patch_size;      /* 16 */
    int dim;             /* 768 / 1024 */
    int depth;           /* 12 / 24 */
    int heads;           /* 12 / 16 */
    int mlp_dim;         /* 3072 / 4096 */
    float ln_eps;        /* 1e-6 (torchvision, timm) or 1e-12 (HF default) */
    int layer_scale;     /* 1: per-branch gamma (timm init_values, uni.py:35) */
    int compute_dtype;   /* AP_F16 / AP_BF16 / AP_F32: MFMA operand type; accumulation,
                            residual stream, LayerNorm and softmax are always f32 */
    int pool;            /* AP_POOL_CLS: final LN, class token (vit.py, uni.py).
                            AP_POOL_ATTN: final LN on all tokens, then the attentional pooler of
                            CONCH's visual tower with ONE query (models/patch/conch.py:52,
                            encode_image(proj_contrast=False, normalize=False)): LN_k, k/v
                            projection to pool_dim, softmax pooling per head, out_proj, LN.
                            AP_POOL_CLS_MEAN: final LN on all tokens, out = [class token | mean of the PATCH tokens]
                            (2 * dim floats; register tokens excluded): torch.cat([cls, patch_tokens.mean(1)], -1) of
                            models/patch/midnight.py:58-61, virchow.py:58-61,111-114, hoptimus.py:158-161 */
    int pool_dim;        /* 512 (conch_v1); heads of 64 (other widths: pool_head_dim of ap_vit_config_ex2) */
    int pool_heads;      /* 8 */
    float pool_ln_eps;   /* 1e-5 (open_clip LayerNorm) */
    /* ---- ABI v17: the rest of the reference's ViT zoo (models/patch/vit.py:9-15 vit_b_32 / vit_l_32 / vit_h_14,
     *      models/patch/uni.py:62-125 uni_v2).  All zero = the v16 behaviour. */
    int reg_tokens;      /* register tokens between the class token and the patches (timm reg_tokens; uni_v2: 8) */
    int no_embed_class;  /* 1: pos_embed has image_size^2 / patch_size^2 rows and is added to the PATCH tokens only (timm
                            no_embed_class, uni_v2); 0: pos_embed covers class (+ register) tokens too */
    int mlp_type;        /* AP_MLP_GELU: fc1 [mlp_dim, dim] -> GELU(erf) -> fc2 [dim, mlp_dim];
                            AP_MLP_SWIGLU: timm SwiGLUPacked -- fc1 [2 * mlp_dim, dim], silu(x[:, :mlp_dim]) * x[:, mlp_dim:],
                            fc2 [dim, mlp_dim] (uni_v2: mlp_dim 4096) */
    int head_dim;        /* 0 = dim / heads (must be 64); else the width of one head of q / k / v as STORED: qkv.weight has
                            3 * heads * head_dim rows, proj.weight heads * head_dim columns (64, 128, or -- float16 / bfloat16 --
                            96).  A model whose true head width is none of these (vit_h_14, Virchow: 80) is uploaded zero-padded
                            to the next one (96) with attn_scale set.  heads * head_dim may be smaller than dim (attention narrower
                            than the stream: dim 512, 2 heads of 64): accepted for every pooling as long as heads * head_dim is a
                            multiple of 128 (else AP_ERR_INVALID), and the workspace is sized for what the pooling heads put into
                            the blocks' q | k | v, attention-output and branch buffers (tested against a float64 reference) */
    float attn_scale;    /* 0 = 1 / sqrt(head_dim); else the softmax scale (vit_h_14: 1 / sqrt(80)) */
    /* ---- ABI v18: CLIP vision towers (models/patch/clip.py, plip.py, quilt.py: open_clip VisionTransformer / transformers
     *      CLIPVisionModel).  All zero = the v17 behaviour. */
    int pre_norm;        /* 1: LayerNorm on the embedded tokens (class + position added) before the first block (CLIP ln_pre /
                            pre_layrnorm); parameters pre_norm.weight | bias [dim] */
    int act;             /* AP_ACT_GELU (erf) or AP_ACT_QUICK_GELU (x * sigmoid(1.702 x), the OpenAI CLIP weights); AP_MLP_GELU only */
    int proj_dim;        /* 0, or P: the pooled vector (AP_POOL_CLS: final LN of the class token) is multiplied by
                            head_proj.weight [P, dim] without bias (CLIP visual projection: encode_image / get_image_features);
                            multiple of 128; ap_vit_embed_dim = P */
    int rope;            /* 1: no absolute position embedding use beyond pos_embed (upload zeros) and a rotary embedding on q / k of the
                            PATCH tokens in every block (transformers DINOv3ViTModel, models/patch/dinov3.py): parameters
                            rope.cos | rope.sin f32 [patches, head_dim] (the host builds them as the HF module does);
                            head_dim must be the true head width */
} ap_vit_config;
#define AP_VIT_CONFIG_SIZE_V20 92u   /* struct_size + the 22 fields of ABI v19: the smallest size ap_vit_create accepts */
/* Fields appended since ABI v20 (additive: AP_ABI_VERSION stays 20).  ap_vit_config itself keeps its v20 fields and size; a caller
 * that needs a newer field hands ap_vit_create an ap_vit_config_ex -- the SAME bytes followed by the appended fields -- cast to
 * ap_vit_config*, with base.struct_size = sizeof(ap_vit_config_ex) (ap_vit_config_init(&cfg.base, sizeof cfg) zero-fills all of it
 * and records that size).  All zero = the behaviour before the field existed, so the two sizes ap_vit_create accepts,
 * AP_VIT_CONFIG_SIZE_V20 and AP_VIT_CONFIG_SIZE_EX, mean the same for an old caller. */
typedef struct ap_vit_config_ex {
    ap_vit_config base;
    /* ---- SigLIP vision towers (models/patch/medsiglip.py:37,63: transformers SiglipVisionModel, get_image_features) */
    int no_class_token;  /* 1: the sequence is the patch tokens only (SiglipVisionEmbeddings: patch embedding + position embedding,
                            no class embedding): tokens = (image_size / patch_size)^2, pos_embed [tokens, dim] is added to every
                            row, there is no cls_token parameter, reg_tokens must be 0, and the pooling must be AP_POOL_MAP.
                            AP_VIT_OPT_EXACT_CLS is inert (there is no class row) and the last block always runs in full.  Not
                            combined with pre_norm or rope in this build */
} ap_vit_config_ex;
#define AP_VIT_CONFIG_SIZE_EX 96u    /* sizeof(ap_vit_config_ex) */
/* The second extension (additive as the first: AP_ABI_VERSION stays 20): ap_vit_config_ex followed by the attentional pooler's
 * fields for the ViT-L towers of CoCa (open_clip coca_ViT-L-14, models/patch/omiclip.py) and CONCH v1.5 (models/patch/conch.py:82-100).
 * Handed over like ap_vit_config_ex, with base.base.struct_size = sizeof(ap_vit_config_ex2); ap_vit_create takes exactly the
 * three sizes 92, 96 and 112.  All four fields zero = ap_vit_config_ex, bit for bit.  They go with AP_POOL_ATTN only. */
typedef struct ap_vit_config_ex2 {
    ap_vit_config_ex base;
    int pool_head_dim;        /* 0: the pooler's heads are 64 wide, on the kernel conch_v1 has always run (f16 / bf16 only).  64, 96
                                 or 128: pool_dim = pool_heads * pool_head_dim, softmax scale 1 / sqrt(pool_head_dim), on the
                                 one-query kernel of ap_attention_probe -- in float32 too, inside the float32 limits of the trunk
                                 (288 tokens, 64-wide trunk heads) */
    int pool_skip_final_norm; /* 1: no LayerNorm on the tokens after the last block (open_clip's VisionTransformer with an
                                 attentional pooler): the pooler's ln_k reads the residual stream, and there are no norm.weight |
                                 norm.bias parameters */
    int pool_proj_dim;        /* 0, or P2: the pooled vector (after ln_out) is multiplied by attn_pool.proj.weight [P2, pool_dim]
                                 without bias (open_clip `proj`); P2 % 128 == 0, P2 <= pool_dim; ap_vit_embed_dim = P2 */
    int out_normalize;        /* 1: every output row is divided by max(its L2 norm, 1e-12) (encode_image(normalize=True)) */
} ap_vit_config_ex2;
#define AP_VIT_CONFIG_SIZE_EX2 112u  /* sizeof(ap_vit_config_ex2) */
size_t ap_sizeof_vit_config(void);   /* sizeof(ap_vit_config) inside the library */
/* Zero-fills sizeof_caller bytes at cfg and records sizeof_caller in cfg->struct_size.  AP_ERR_INVALID when cfg is NULL,
 * sizeof_caller < AP_VIT_CONFIG_SIZE_V20 or not a multiple of 4. */
int ap_vit_config_init(ap_vit_config* cfg, size_t sizeof_caller);
#define AP_ACT_GELU 0
#define AP_ACT_QUICK_GELU 1
#define AP_ACT_GELU_TANH 2    /* 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))): transformers "gelu_pytorch_tanh", SigLIP's
                                hidden_act (models/patch/medsiglip.py); AP_MLP_GELU only */
#define AP_MLP_GELU 0
#define AP_MLP_SWIGLU 1
#define AP_POOL_CLS 0
#define AP_POOL_ATTN 1
#define AP_POOL_CLS_MEAN 2
/* AP_POOL_MAP: SigLIP's multi-head attention pooling head (transformers SiglipMultiheadAttentionPoolingHead; the features
 * models/patch/medsiglip.py returns are its output, `pooler_output`).  After the final LayerNorm on all tokens (y):
 *   kv = y W_kv^T + b_kv            [n * tokens, 2 * heads * head_dim]  (rows k; v of nn.MultiheadAttention's in_proj)
 *   a  = softmax_t(attn_scale * q_h . k_t) v_t   per (image, head); q = W_q probe + b_q is input independent (map.q)
 *   r  = a W_out^T + b_out          [n, dim]
 *   out = r + fc2(gelu_tanh(fc1(LayerNorm(r))))   f32 [n, dim]
 * heads, head_dim (as stored), attn_scale, ln_eps and mlp_dim are the trunk's; the MLP uses the tanh GELU whatever `act` is.
 * Requires no_class_token in this build.  f16 / bf16, and float32 inside its limits (288 tokens, 64-wide heads). */
#define AP_POOL_MAP 3

/* Validates cfg->struct_size as described above, then every field; *out is written only on success. */
int ap_vit_create(const ap_vit_config* cfg, ap_vit** out);
void ap_vit_destroy(ap_vit* m);

/* Upload one parameter (host float32, `count` elements).  Names:
 *   patch_embed.weight [dim,3,ps,ps]  patch_embed.bias [dim]  cls_token [dim]
 *   pos_embed [1+gh*gw, dim]          norm.weight / norm.bias [dim]
 *   blocks.<i>.ln1.weight|bias  blocks.<i>.qkv.weight [3dim,dim] (rows q;k;v)  blocks.<i>.qkv.bias
 *   blocks.<i>.proj.weight [dim,dim] | .bias   blocks.<i>.ls1 [dim]
 *   blocks.<i>.ln2.weight|bias  blocks.<i>.fc1.weight [mlp,dim] | .bias
 *   blocks.<i>.fc2.weight [dim,mlp] | .bias    blocks.<i>.ls2 [dim]
 * AP_POOL_ATTN adds (P = pool_dim):
 *   attn_pool.ln_k.weight|bias [dim]   attn_pool.kv.weight [2P, dim] (rows k_proj; v_proj)   attn_pool.kv.bias [2P]
 *   attn_pool.q [P]  (the projected query q_proj(ln_q(query)) + bias: input independent, computed by the host)
 *   attn_pool.out.weight [P, P] | .bias [P]   attn_pool.ln_out.weight|bias [P]
 *   ap_vit_config_ex2: attn_pool.proj.weight [pool_proj_dim, P] when pool_proj_dim > 0 (open_clip's `proj`, transposed; no bias);
 *   pool_skip_final_norm: there are no norm.weight / norm.bias parameters
 * AP_POOL_MAP adds (DA = heads * head_dim as stored, H = mlp_dim; SiglipMultiheadAttentionPoolingHead):
 *   map.q [DA]  (W_q probe + b_q, the query third of attention.in_proj applied to the probe: computed by the host)
 *   map.kv.weight [2 DA, dim] (rows k; v of attention.in_proj_weight, heads zero-padded to head_dim)   map.kv.bias [2 DA]
 *   map.out.weight [dim, DA] | map.out.bias [dim]   (attention.out_proj)
 *   map.ln.weight|bias [dim]   (layernorm)   map.fc1.weight [H, dim] | .bias [H]   map.fc2.weight [dim, H] | .bias [dim]
 * no_class_token: there is no cls_token parameter and pos_embed is [gh*gw, dim].
 * Synchronous (copies before returning).
 * Every upload that a derived buffer depends on UN-FINALISES the object -- forwards return AP_ERR_STATE until
 * ap_vit_finalize succeeds again:
 *   cls_token, reg_tokens, pos_embed   (since ABI v17; before it a class-token upload took effect at once) the prefix rows
 *                                      "class / register token + its position row" are built by ap_vit_finalize;
 *   pos_embed, blocks.*                f16 / bf16: the folded weights / the T copy of pos_embed are stale (see ap_vit_finalize).
 * patch_embed.*, norm.*, pre_norm.*, rope.*, head_proj.weight, attn_pool.* and map.* take effect immediately. */
int ap_vit_set_param(ap_vit* m, const char* name, const float* host, size_t count);
/* n parameters in one call (same semantics as n ap_vit_set_param calls, in order; stops at the first error) */
int ap_vit_set_params(ap_vit* m, const char* const* names, const float* const* host, const size_t* counts, int n);
/* Checks every parameter was set and, for f16 / bf16, builds the derived weights of the fused-LayerNorm dataflow from the
 * float32 uploads (LayerNorm gain / LayerScale folded into the block matrices, column sums, folded biases, a T copy of
 * pos_embed); the float32 copies are released afterwards.  Setting a blocks.* parameter or pos_embed later un-finalises the
 * object: forwards return AP_ERR_STATE until ap_vit_finalize succeeds again, which needs the qkv / proj / fc1 / fc2
 * matrices of every block uploaded again (AP_ERR_STATE otherwise) -- stale folded weights can never run. */
int ap_vit_finalize(ap_vit* m);

/* Options (defaults: off; the environment variables AP_VIT_FULL_LAST_BLOCK / AP_VIT_OVERLAP set the defaults once, when
 * the object is created -- nothing on the launch path reads the environment):
 *   AP_VIT_OPT_FULL_LAST_BLOCK    compute the last block for every token instead of the CLS row only (same features)
 *   AP_VIT_OPT_TWO_HALF_OVERLAP   run a batch >= 512 as two halves on two streams (same features)
 *   AP_VIT_OPT_F32_STREAM         f16 / bf16 only: keep the residual stream in float32 and normalise it with standalone
 *                                 add+LayerNorm launches (round 1's dataflow; environment default AP_VIT_F32_STREAM).
 *                                 The default for f16 / bf16 keeps the stream in the compute type -- what the reference's
 *                                 own model.half() does -- with LayerNorm fused into the neighbouring GEMMs
 *   AP_VIT_OPT_EXACT_CLS          (ABI v19; default ON, environment AP_VIT_NO_EXACT_CLS turns the default off) f16 / bf16 with
 *                                 the stream in the compute type and a class-token pooling (AP_POOL_CLS, AP_POOL_CLS_MEAN):
 *                                 the class rows' residual stream is additionally carried in float32 -- after every proj /
 *                                 fc2 launch an n-row GEMM adds the unrounded branch of the class rows to it, and the
 *                                 stream's class row becomes its rounding.  The features are the class row of the stream and
 *                                 nearly all of the 16-bit stream's error in them is that row's own 2 x depth roundings:
 *                                 ViT-B/16 float16 1.26e-3 -> 7.7e-4 against the CPU fp32 path, for < 1 % of the step
 *   AP_VIT_OPT_SPLIT_F16          (additive to ABI v20; float32 compute type only; default ON, environment AP_VIT_EXACT_F32 turns the default
 *                                 off) the float32-ACCURATE
 *                                 fast mode behind `--feature-precision float32` (cli.py:175-181, models/patch/base.py:95-106):
 *                                 every buffer, LayerNorm, softmax and the residual stream stay float32; only the GEMMs' inner
 *                                 products change from the exact f32 MFMA to three f16 MFMA passes on hi / lo halves
 *                                 (x = hi + 2^-11 lo, 22 of 24 mantissa bits; w a ~= w_hi a_hi + 2^-11 (w_hi a_lo + w_lo a_hi), f32
 *                                 accumulation).  The weights are split once, when the option is switched on (a second copy of the
 *                                 matrices, kept up to date by ap_vit_set_param).  Measured on ViT-B/16, depth 12, against the CPU fp32
 *                                 path: 1.1e-6 norm-wise / 1.4e-5 element-wise maximum (the exact chain: 2.0e-6 / 3.4e-5 -- its 768- to
 *                                 3072-long sequential f32 sums round more often than the MFMA's 16-wide ones) at 1.8x the rate.
 *                                 GEMM operands must stay inside f16's range (|x| < 65504; LayerNorm / attention / GELU outputs and
 *                                 weights do).  Off = the exact f32 MFMA chain (v_mfma_f32_32x32x2_f32) */
#define AP_VIT_OPT_FULL_LAST_BLOCK 0
#define AP_VIT_OPT_TWO_HALF_OVERLAP 1
#define AP_VIT_OPT_F32_STREAM 2
#define AP_VIT_OPT_EXACT_CLS 3
#define AP_VIT_OPT_SPLIT_F16 4
int ap_vit_set_option(ap_vit* m, int option, int value);

size_t ap_vit_workspace_bytes(const ap_vit* m, int n);
int ap_vit_embed_dim(const ap_vit* m);   /* dim (AP_POOL_CLS, AP_POOL_MAP), pool_dim (AP_POOL_ATTN) or 2 * dim (AP_POOL_CLS_MEAN);
                                            proj_dim / pool_proj_dim when the configuration has a projection */

/* Optional per-launch timing with HIP events recorded on the forward's own stream (what
 * bench.py's roofline block reads).  Off by default; when on, every kernel launch of a forward
 * is bracketed by two events.  ap_vit_profile_read synchronises on them, returns summed
 * milliseconds and launch counts per kind since the last read, and resets. */
#define AP_PROF_PREPROC 0
#define AP_PROF_GEMM_PATCH_EMBED 1
#define AP_PROF_GEMM_QKV 2
#define AP_PROF_GEMM_PROJ 3
#define AP_PROF_GEMM_FC1 4
#define AP_PROF_GEMM_FC2 5
#define AP_PROF_ATTENTION 6
#define AP_PROF_LAYERNORM 7
#define AP_PROF_CLS_TAIL 8      /* last block after its K/V projection, CLS rows only (see ap_vit_forward_u8); AP_POOL_MAP: the head */
#define AP_PROF_KINDS 9
int ap_vit_profile_enable(ap_vit* m, int on);
int ap_vit_profile_read(ap_vit* m, double* ms_by_kind, long long* launches_by_kind, int kinds);

/* patches: device uint8 [n, h, w, 3]; centre-cropped to image_size, normalised with
 * mean/std, embedded.  out: device float32 [n, ap_vit_embed_dim], 16-byte aligned: both forwards refuse another address with
 * AP_ERR_INVALID before any launch (the heads store four floats per lane).  workspace: 256-byte aligned, ap_vit_workspace_bytes(m, n)
 * bytes are all a forward touches; fewer: AP_ERR_WORKSPACE, nothing launched.  No forward reads a workspace byte it has not
 * written in the same call.  Asynchronous on `stream`.
 * For the CLS readout the last block computes K / V for every token and everything after that for the CLS row
 * only (nothing reads the other rows; identical features; AP_VIT_OPT_FULL_LAST_BLOCK disables it). */
int ap_vit_forward_u8(ap_vit* m, const uint8_t* patches, int n, int h, int w,
                      const float mean[3], const float stdv[3],
                      float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream);

/* x: device [n, 3, image_size, image_size] already normalised, dtype x_dtype (AP_F32 or the
 * compute dtype): the boundary a plugin `preprocess` feeds (models/patch/custom.py:31-43). */
int ap_vit_forward_chw(ap_vit* m, const void* x, int x_dtype, int n,
                       float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream);

/* ---- single operators of the encoder (the same kernels ap_vit_forward_* chains) ------
 * The operator-level seam a plugin `forward_fn` (models/patch/custom.py:31-43) can bind when it
 * builds its own block structure, and what the per-kernel parity tests call.  All pointers are
 * device pointers; dtype is the MFMA operand type (AP_F16 / AP_BF16 / AP_F32).
 *
 * ap_gemm:  C[m][n] = sum_k A[m][k] * W[n][k] + bias[n], then the epilogue:
 *   AP_EPI_BIAS        out T   [M, ldo] = C                       (nn.Linear)
 *   AP_EPI_BIAS_GELU   out T   [M, ldo] = gelu_erf(C)             (Linear + nn.GELU())
 *   AP_EPI_BIAS_RESID  out f32 [M, ldo] += C * (gamma ? gamma[n] : 1)   (residual add, LayerScale)
 *   AP_EPI_BIAS_QUICK_GELU  out T [M, ldo] = C * sigmoid(1.702 C)   (CLIP's QuickGELU: models/patch/clip.py, plip.py)
 *   AP_EPI_BIAS_GELU_TANH   out T [M, ldo] = 0.5 C (1 + tanh(sqrt(2 / pi) (C + 0.044715 C^3)))   (SigLIP's gelu_pytorch_tanh:
 *                           models/patch/medsiglip.py), evaluated as C * sigmoid(2 sqrt(2 / pi) (C + 0.044715 C^3)): one
 *                           exponential and one reciprocal, no NaN for any finite C, -> C and -> -0 for large |C|
 * A: T [M, lda], W: T [N, ldw] (both K-contiguous, the checkpoint's [out, in] layout), bias /
 * gamma: f32 [N].  N % 128 == 0 and K % (128 / sizeof(T)) == 0.  impl: 0 = pick, 128 = the
 * 128x128-tile kernel, 256 = the persistent 256x256-tile kernel (f16 / bf16, N % 256 == 0,
 * K % 128 == 0, K >= 128); variant selects a schedule variant of the 256 kernel (0 = default).
 *
 * Layout rule of ap_gemm and ap_gemm_fused (To = the output's element type: float for AP_EPI_BIAS_RESID, else T; the output has
 * N columns, N / 2 under AP_EPI_NORM_SWIGLU).  The three strides are independent, in elements, and what lies between a row's
 * end and the next row is neither read (A, W) nor written (out):
 *   M, N, K > 0;  lda >= K, ldw >= K, ldo >= the output's columns;
 *   A, W: 16-byte aligned pointers, lda * sizeof(T) and ldw * sizeof(T) multiples of 16 (LDS-DMA moves 16 bytes per lane);
 *   out: ldo % 4 == 0 and the pointer aligned to 4 * sizeof(To) (a lane stores four consecutive columns); the 256 x 256
 *        kernel stores 16 bytes per lane: impl 256 needs ldo * sizeof(To) % 16 == 0 and a 16-byte aligned pointer, and
 *        impl 0 picks it only then;
 *   sizes: the buffers may be of any size -- every row is addressed with 64 bits (row index x stride), so rows beyond element
 *        2^31 and byte 2^32 of A and out are as good as the first.  The 256 x 256 kernel keeps 32-bit BYTE offsets inside one
 *        tile and into rowstats: impl 256 needs 255 * lda * sizeof(T) + 128 and 255 * ldw * sizeof(T) + 128 below 2^32, and under
 *        the AP_EPI_NORM* epilogues M <= 2^29 (rowstats below 4 GiB) and N <= 2^30; impl 0 picks it only then;
 *   bias, gamma, colsum, rowstats: 16-byte aligned;  partial: 8-byte aligned (rowstats [M, 2] and partial [M, N / 64, 2] are dense).
 * Both entry points refuse anything else, and an impl that does not take the problem, with AP_ERR_INVALID and their name
 * in ap_last_error(); nothing is launched.  Whichever kernel runs, the same call gives the same bits.  impl 129 (below) is held
 * to the same rule with N % 32 == 0 in place of N % 128 == 0, and gamma, where given, is applied as by impl 128. */
#define AP_EPI_BIAS 0
#define AP_EPI_BIAS_GELU 1
#define AP_EPI_BIAS_RESID 2
#define AP_EPI_BIAS_QUICK_GELU 10
#define AP_EPI_BIAS_GELU_TANH 12
int ap_gemm(int dtype, int epilogue, const void* A, int lda, const void* W, int ldw,
            int M, int N, int K, const float* bias, const float* gamma, void* out, int ldo,
            int impl, int variant, ap_stream_t stream);
/* The float32-accurate fast product (what AP_VIT_OPT_SPLIT_F16 runs; added to ABI v20 without a layout change).
 * ap_split_f16_weights: w32 f32 [count] (count % 32 == 0: whole rows of a K that is a multiple of 32) -> out, the same
 * number of BYTES: per 32 consecutive values 32 f16 `hi` followed by 32 f16 `lo`, hi = f16(w), lo = f16((w - hi) * 2^11).
 * ap_gemm(AP_F32, ..., impl = 129) then takes such rows as W (ldw still in f32 elements), float32 A / bias / out, and
 * computes  sum_k  w_hi a_hi + 2^-11 (w_hi a_lo + w_lo a_hi)  with a split in registers, f32 accumulation: ~2^-22 per
 * product against the exact f32 chain of impl 128, at 2-3x its rate.  K % 32 == 0, N % 32 == 0 (the 128-wide tile's tail is
 * masked); otherwise the layout rule above, refused the same way.  |x| < 65504 for every operand value (hi = f16(x)). */
int ap_split_f16_weights(const float* w32, void* out, size_t count, ap_stream_t stream);
/* The same product as a row-wise float32 layer with an optional SEPARATE residual (the SAM2 trunk's Linear / MLP layers,
 * services/segmentation.py:120-180 runs them in float32):
 *   out[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) + resid[m][n]        act: 0 none, 1 GELU (erf)
 * A f32 [M, lda], w_split = ap_split_f16_weights of the f32 [N, K] matrix, bias f32 [N] or NULL, resid f32 [M, ldr] or NULL,
 * out f32 [M, ldo].  N % 32 == 0 (any such N: the 128-wide tile's tail is masked), K % 32 == 0, strides multiples of 4,
 * pointers 16-byte aligned.  A row's result does not depend on M (no split-K): batches stay bit-identical to single calls. */
int ap_gemm_split_f16(const float* A, int lda, const void* w_split, int M, int N, int K, const float* bias, int act,
                      const float* resid, int ldr, float* out, int ldo, ap_stream_t stream);
/* ... with the window (un)partition of the SAM2 trunk's windowed blocks folded in (sam2 hieradet.py window_partition /
 * window_unpartition as the reference's SAM2ImagePredictor runs them; replaces ap_window_partition / ap_window_unpartition_add
 * around the qkv / proj layers).  The token grid is b images of h x w tokens, cut into ws x ws windows, zero-padded at the
 * right / bottom edge; M = b * ceil(h / ws) * ceil(w / ws) * ws * ws window-order rows.
 *   win_mode 1: A is [b * h * w, lda] in IMAGE order; product row m takes the image row of window-order row m (zeros for a
 *               padding row); out [M, ldo] in window order (the qkv layer after norm1).
 *   win_mode 2: A is [M, lda] in window order; out / resid are [b * h * w, ld] in IMAGE order, padding rows are dropped
 *               (the proj layer + residual add). */
int ap_gemm_split_f16_windows(const float* A, int lda, const void* w_split, int M, int N, int K, const float* bias, int act,
                              const float* resid, int ldr, float* out, int ldo, int win_mode, int b, int h, int w, int ws,
                              ap_stream_t stream);

/* ---- fused-LayerNorm operators (what ap_vit_forward_* chains for f16 / bf16 unless AP_VIT_OPT_F32_STREAM is set) ----
 * The pre-LN block of the reference's encoders (nn.LayerNorm -> nn.Linear, models/patch/vit.py / uni.py / conch.py via
 * timm / torchvision Block.forward: x = x + ls1 * attn(norm1(x)); x = x + ls2 * mlp(norm2(x))) with the residual
 * stream x kept in T and NO standalone LayerNorm pass:
 *   LN(x) W^T + b  =  rstd[m] * (sum_k x[m][k] W'[n][k]  -  mean[m] * colsum[n]) + bias'[n]
 * with W' = T(W * gamma) (the caller folds the LayerNorm gain into the weights), colsum[n] = sum_k W'[n][k],
 * bias' = b + W beta and rowstats[m] = (rstd, -mean * rstd) of row m of x.
 *   AP_EPI_NORM         out T [M, ldo] = rstd * acc + (-mean rstd) * colsum[n] + bias[n]
 *   AP_EPI_NORM_GELU    out = gelu(that)
 *   AP_EPI_NORM_QUICK_GELU  out = that * sigmoid(1.702 * that)
 *   AP_EPI_NORM_GELU_TANH   out = gelu_tanh(that), as AP_EPI_BIAS_GELU_TANH (SigLIP: models/patch/medsiglip.py)
 *   AP_EPI_NORM_SWIGLU  timm SwiGLUPacked (models/patch/uni.py:91-93, uni_v2) with the gate in the epilogue: W / colsum / bias rows
 *                       INTERLEAVED in groups of 64 -- rows 64q .. 64q+31 = fc1 rows 32q .. (x1), rows 64q+32 .. 64q+63 = fc1 rows
 *                       N/2 + 32q .. (x2) -- and out T [M, N / 2]: out[m][32q + j] = silu(norm x1) * norm x2, one rounding
 *   AP_EPI_RESID_STATS  out T [M, ldo] (in place) = T(out + T(acc + bias[n]))  -- the residual add -- and
 *                       partial f32 [M, N / 64, 2] = per row and 64-column group (sum, sum of squares) of the NEW row;
 *                       ap_rowstats_finalize turns them into the next rowstats (deterministic, fixed order, double).
 * impl: 0 = pick, 256 = the persistent 256 x 256 kernel (N % 256 == 0, K % 128 == 0; any M >= 1), 128 = the 128 x 128
 * kernel (N % 128 == 0, K % 64 == 0); the two give the same bits (the statistics are summed in one fixed order).  f16 / bf16.
 * Strides and alignment: the layout rule stated at ap_gemm.
 * ap_stream_init: tok f32 [rows, dim] -> x T [rows, dim] + rowstats of the rounded rows (two-pass). */
#define AP_EPI_NORM 4
#define AP_EPI_NORM_GELU 5
#define AP_EPI_RESID_STATS 6
#define AP_EPI_NORM_SWIGLU 8
#define AP_EPI_NORM_QUICK_GELU 9
#define AP_EPI_NORM_GELU_TANH 11
int ap_gemm_fused(int dtype, int epilogue, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
                  const float* bias, const float* colsum, const float* rowstats, float* partial,
                  void* out, int ldo, int impl, ap_stream_t stream);
int ap_stream_init(int dtype, const float* tok, int rows, int dim, float eps, void* x, float* rowstats,
                   ap_stream_t stream);
int ap_rowstats_finalize(const float* partial, int rows, int groups, int dim, float eps, float* rowstats,
                         ap_stream_t stream);

/* Diagnostics for the persistent kernel's instrumented twin (impl 257; the product kernel, impl 256, carries no
 * diagnostic code): when device_buf is non-null every later impl-257 launch records, per (workgroup, tile) with tile < tiles_per_workgroup, eight int64 stamps of the
 * 100-MHz wall clock: [0] tile start, [1] K loop done, [2] staged stream drained, [3] bias loaded,
 * [4] epilogue done.  device_buf: int64 [grid, tiles_per_workgroup, 8].  Pass NULL to switch off. */
int ap_gemm_trace(long long* device_buf, int tiles_per_workgroup);

/* LayerNorm over the last dimension of f32 rows (row stride `stride` elements) -> dense
 * out [rows, dim] of out_dtype (nn.LayerNorm, eps inside the sqrt, biased variance). */
int ap_layernorm(int out_dtype, const float* x, long stride, int rows, int dim,
                 const float* gamma, const float* beta, float eps, void* out, ap_stream_t stream);

/* Multi-head self-attention on packed projections: qkv T [n * tokens, 3 * heads * head_dim]
 * (q | k | v), out T [n * tokens, heads * head_dim]; softmax(q k^T / sqrt(head_dim)) v in f32
 * (F.scaled_dot_product_attention without mask / dropout).  head_dim: 64 (any dtype), 96 or 128 (float16 / bfloat16).
 * qkv and out are 16-byte aligned (the kernels move 16 bytes per lane; float32 needs no more).  Refused with
 * AP_ERR_INVALID and text in ap_last_error() before anything is launched, as by ap_attention_scaled: a null or
 * misaligned pointer, an unknown dtype, n < 0, tokens <= 0, heads <= 0, a head_dim the type does not serve, and in
 * float16 / bfloat16 an image whose qkv rows reach 4 GiB (tokens * 3 * heads * head_dim * 2 bytes: rows are addressed by a
 * 32-bit offset).  float32: at most 288 tokens (AP_ERR_UNSUPPORTED beyond, nothing launched).  n = 0 is an empty launch. */
int ap_attention(int dtype, const void* qkv, void* out, int n, int tokens, int heads, int head_dim,
                 ap_stream_t stream);

/* ---- engine building blocks (additive to ABI v20) -----------------------------------------
 * The remaining kernels ap_vit_forward_* chains, one entry point each, so that each can be held against a reference of
 * its own.  T = the type `dtype` names.  Every function refuses (AP_ERR_INVALID, text in ap_last_error(), nothing
 * launched) a null pointer, a size that is not positive, a type it does not serve and a layout its kernel cannot
 * address; n = 0 or rows = 0 is an empty launch.  Pointers are 16-byte aligned unless stated.
 *
 * ap_attention_scaled: ap_attention with the softmax scale given (head widths stored zero-padded to 96: scale =
 *   1 / sqrt(true width)); scale > 0 and finite; alignment and refusals as ap_attention.  float32: 64-wide heads, at most
 *   288 tokens (AP_ERR_UNSUPPORTED beyond).
 * ap_attention_cls: one query row per (image, head) -- the class row of the last block.  q T [n, heads * head_dim]
 *   packed; k and v inside rows of kv T [n * tokens, ld] at columns koff + head * head_dim and voff + head * head_dim;
 *   out T [n, heads * head_dim] = softmax_t(scale * q . k_t) v_t, f32 arithmetic, the maximum subtracted before the
 *   exponential, one rounding.  head_dim 64 / 96 / 128; ld, koff, voff multiples of 8; 1 <= tokens <= 12000.  q and kv
 *   are aligned to eight elements: 16 bytes in f16 / bf16, 32 bytes in float32.
 * ap_attn_pool: attentional pooling with one learned query: kv T [n * tokens, 2 * heads * 64] (k | v), q f32
 *   [heads * 64] shared by every image, out T [n, heads * 64]; scale 1 / 8.  f16 / bf16; 1 <= tokens <= 12000.
 * ap_attention_probe: ap_attention_cls with ONE float32 query shared by every image -- the pooling step of SigLIP's
 *   attention-pooling head (models/patch/medsiglip.py; AP_POOL_MAP): q f32 [heads * head_dim], everything else as
 *   ap_attention_cls (kv / out of type T, head_dim 64 / 96 / 128, ld / koff / voff multiples of 8, 1 <= tokens <= 12000, kv
 *   aligned to eight elements, q to 16 bytes).
 * ap_rope: DINOv3's rotary embedding in place on the q (which & 1) and k (which & 2) parts of the packed qkv
 *   T [n * tokens, 3 * heads * head_dim], patch tokens only (rows >= prefix of every image), p = the patch's index:
 *     x'[j] = x[j] cos[p][j] - x[j + h] sin[p][j],   x'[j + h] = x[j + h] cos[p][j + h] + x[j] sin[p][j + h],   h = head_dim / 2
 *   cos / sin f32 [tokens - prefix, head_dim]; f32 arithmetic, one rounding; head_dim % 16 == 0; which 1 .. 3.
 * ap_swiglu: out[m][j] = T(silu(x[m][j]) * x[m][h + j]), x T [rows, 2h] dense, out T [rows, h] dense; f32 arithmetic;
 *   h % 8 == 0.
 * ap_add2_layernorm: x[row] += delta0[row] * ls0, then += delta1[row] * ls1 (f32, in that order; either delta and
 *   either LayerScale vector ls f32 [dim] may be NULL), then out[row] = LayerNorm(x[row]) (two-pass, biased variance,
 *   eps inside the sqrt) in out_dtype, dense [rows, dim].  x f32 rows of `stride` elements; the deltas are rows of
 *   delta_dtype with strides dstride0 / dstride1.  store = 1 writes the updated x back (only when a delta is given),
 *   store = 0 leaves x untouched.  (delta, out) types: (T, T), (T, f32), (f32, f32).  dim % 4 == 0, dim <= 4096; strides
 *   multiples of 4 (a 16-bit delta at dim 768 / 1024: of 8) and >= dim.
 * ap_fold_ln: the LayerNorm fold of a weight matrix w32 f32 [rows, ld] (cols <= ld used): wout T [rows, ld] =
 *   T(w32[n][k] * gamma[k]), zero for k >= cols; colsum[n] = sum_k float(wout[n][k]); bias_out[n] = bias_in[n] +
 *   sum_k w32[n][k] * beta[k].  swiglu_h > 0 (rows = 2 swiglu_h, swiglu_h % 32 == 0): output row r is built from source row
 *   (r % 64 < 32 ? 0 : swiglu_h) + 32 * (r / 64) + r % 32 -- AP_EPI_NORM_SWIGLU's order.  f16 / bf16.
 * ap_fold_ls: wout T [rows, ld] = T(w32[n][k] * ls[n]), zero for k >= cols; bias_out[n] = bias_in[n] * ls[n]; ls NULL:
 *   a plain conversion.  f16 / bf16.
 * ap_cls_mean_pool: y f32 [n * tokens, dim] -> out f32 [n, 2 * dim] = [row 0 of the image | mean of its rows prefix ..
 *   tokens - 1] (summed in double, one division); prefix >= 1, tokens > prefix.
 * ap_l2_normalize_rows: out f32 [rows, dim] dense = x[row] / max(||x[row]||, eps), x f32 rows of `stride` elements (torch
 *   F.normalize; the last step of CoCa's encode_image, out_normalize of ap_vit_config_ex2).  The squares are summed in double, so
 *   an element carries two float roundings (the norm's, the division's); a row whose norm is below eps is divided by eps: a zero
 *   row stays zero.  dim % 4 == 0, stride % 4 == 0, stride >= dim, eps > 0; out == x (in place) with stride == dim.
 * ap_stream_to_f32: x T rows of `stride` elements -> dst f32 [rows, dim] dense, exact.  f16 / bf16; dim, stride % 4 == 0.
 * ap_chw_to_patchrows: x [n, 3, S, S] of x_dtype -> dst T [n * g * g, ld], g = S / ps: row (img * g + py) * g + px, column
 *   (c * ps + ky) * ps + kx = x[img][c][py * ps + ky][px * ps + kx], one rounding; columns >= 3 ps^2 are not written.
 *   ld >= 3 ps^2; ps % 4 == 0 needs ld % 4 == 0.
 * ap_cls_stream: the prefix rows (class token, register tokens) of the T stream x [n * tokens, dim]:
 *   x[img * tokens + j] = T(prefix[img * img_rows + j]), j < prefix_rows, and partial f32 [n * tokens, dim / 64, 2] =
 *   (sum, sum of squares) per 64-column group of the rounded row.  img_rows = 0: one prefix f32 [prefix_rows, dim] for
 *   every image; img_rows = prefix_rows: one per image.  f16 / bf16; dim % 64 == 0.
 * ap_cls_exact_update: cls32[img] += branch[img] (f32 [n, dim] both), x[img * tokens] = T(cls32[img]) and that row's
 *   partial sums as above.  f16 / bf16; dim % 64 == 0.
 * ap_rowstats_finalize_cls: ap_rowstats_finalize (groups = dim / 64, dim % 128 == 0) and, when cls32 is not NULL (rows =
 *   n * tokens), the update of ap_cls_exact_update in the same launch: the rows img * tokens get the statistics of
 *   T(cls32[img] + branch[img]) computed from the rounded row itself, every other row those of its partial sums. */
int ap_attention_scaled(int dtype, const void* qkv, void* out, int n, int tokens, int heads, int head_dim, float scale,
                        ap_stream_t stream);
int ap_attention_cls(int dtype, const void* q, const void* kv, int ld, int koff, int voff, void* out, int n, int tokens,
                     int heads, int head_dim, float scale, ap_stream_t stream);
int ap_attn_pool(int dtype, const void* kv, const float* q, void* out, int n, int tokens, int heads, ap_stream_t stream);
int ap_attention_probe(int dtype, const float* q, const void* kv, int ld, int koff, int voff, void* out, int n, int tokens,
                       int heads, int head_dim, float scale, ap_stream_t stream);
int ap_rope(int dtype, void* qkv, int n, int tokens, int prefix, int heads, int head_dim, const float* cos, const float* sin,
            int which, ap_stream_t stream);
int ap_swiglu(int dtype, const void* x, int rows, int h, void* out, ap_stream_t stream);
int ap_add2_layernorm(int delta_dtype, int out_dtype, float* x, long stride, const void* delta0, long dstride0, const float* ls0,
                      const void* delta1, long dstride1, const float* ls1, int store, int rows, int dim, const float* gamma,
                      const float* beta, float eps, void* out, ap_stream_t stream);
int ap_fold_ln(int dtype, const float* w32, int rows, int cols, int ld, const float* gamma, const float* beta,
               const float* bias_in, void* wout, float* colsum, float* bias_out, int swiglu_h, ap_stream_t stream);
int ap_fold_ls(int dtype, const float* w32, int rows, int cols, int ld, const float* ls, const float* bias_in, void* wout,
               float* bias_out, ap_stream_t stream);
int ap_cls_mean_pool(const float* y, int n, int tokens, int prefix, int dim, float* out, ap_stream_t stream);
int ap_l2_normalize_rows(const float* x, long stride, int rows, int dim, float eps, float* out, ap_stream_t stream);
int ap_stream_to_f32(int dtype, const void* x, long stride, int rows, int dim, float* dst, ap_stream_t stream);
int ap_chw_to_patchrows(int x_dtype, int dtype, const void* x, int n, int S, int ps, void* dst, int ld, ap_stream_t stream);
int ap_cls_stream(int dtype, const float* prefix, int prefix_rows, int img_rows, int n, int tokens, int dim, void* x,
                  float* partial, ap_stream_t stream);
int ap_cls_exact_update(int dtype, float* cls32, const float* branch, int n, int tokens, int dim, void* x, float* partial,
                        ap_stream_t stream);
int ap_rowstats_finalize_cls(const float* partial, int rows, int groups, int dim, float eps, float* rowstats, int dtype,
                             float* cls32, const float* branch, void* x, int n, int tokens, ap_stream_t stream);

/* ---- ResNet encoder (additive to ABI v20) ------------------------------------------------
 * Replaces the torchvision resnet18 / 34 / 50 / 101 / 152 forward of models/patch/resnet.py (fc = Identity: the flattened
 * global average pool) with the implicit-GEMM convolution kernels of conv.hip.  Activations are NHWC in the compute type;
 * BatchNorm is folded into the convolutions by the caller (f32 weight and bias per convolution); accumulation is f32.
 * The structure follows the ap_vit_config rules: struct_size first, fields only ever appended, all-zero = the behaviour
 * before a field existed; fill it through ap_resnet_config_init. */
typedef struct ap_resnet ap_resnet;
typedef struct ap_resnet_config {
    uint32_t struct_size; /* sizeof(ap_resnet_config) as the caller sees it; written by ap_resnet_config_init */
    int block;            /* AP_RESNET_BASIC (resnet18 / 34) or AP_RESNET_BOTTLENECK (resnet50 / 101 / 152, expansion 4,
                             stride on the 3x3 conv as torchvision) */
    int depths[4];        /* blocks per stage: 2 2 2 2 / 3 4 6 3 / 3 4 6 3 / 3 4 23 3 / 3 8 36 3 */
    int stem_width;       /* 64: the stem's output channels and the first stage's width (multiple of 64) */
    int compute_dtype;    /* AP_F16 / AP_BF16 / AP_F32 (exact f32 MFMA products) */
    int image_size;       /* 224: the centre crop the network sees */
} ap_resnet_config;
#define AP_RESNET_CONFIG_SIZE_V20 36u   /* the smallest size ap_resnet_create accepts */
#define AP_RESNET_BASIC 0
#define AP_RESNET_BOTTLENECK 1
size_t ap_sizeof_resnet_config(void);
/* Zero-fills sizeof_caller bytes at cfg and records sizeof_caller in cfg->struct_size (AP_ERR_INVALID for NULL or a size
 * below AP_RESNET_CONFIG_SIZE_V20 / not a multiple of 4). */
int ap_resnet_config_init(ap_resnet_config* cfg, size_t sizeof_caller);
int ap_resnet_create(const ap_resnet_config* cfg, ap_resnet** out);
void ap_resnet_destroy(ap_resnet* m);
/* Upload one parameter (host float32, torch layout, `count` elements); synchronous.  Names (torchvision's, BatchNorm folded):
 *   conv1.weight [W, 3, 7, 7] | conv1.bias [W]
 *   layer<s>.<b>.conv<k>.weight [Cout, Cin, kh, kw] | .bias [Cout]     (k = 1, 2 basic; 1, 2, 3 bottleneck)
 *   layer<s>.<b>.downsample.weight [Cout, Cin, 1, 1] | .bias [Cout]     (the first block of a stage whose shape changes)
 * The host permutes the weights to [Cout][ky][kx][Cin] (the stem's Cin padded to 8 with zeros).  Setting a parameter
 * un-finalises the object. */
int ap_resnet_set_param(ap_resnet* m, const char* name, const float* host, size_t count);
int ap_resnet_finalize(ap_resnet* m);          /* AP_ERR_STATE if a parameter was never set */
size_t ap_resnet_workspace_bytes(const ap_resnet* m, int n);
int ap_resnet_embed_dim(const ap_resnet* m);   /* 8 x stem_width (basic) or 32 x stem_width (bottleneck) */
#define AP_RESNET_PROF_STEM 0      /* NHWC preprocess + 7x7 stem convolution */
#define AP_RESNET_PROF_CONV1X1 1
#define AP_RESNET_PROF_CONV3X3 2
#define AP_RESNET_PROF_POOL 3      /* max pool + global average pool */
#define AP_RESNET_PROF_KINDS 4
int ap_resnet_profile_enable(ap_resnet* m, int on);
int ap_resnet_profile_read(ap_resnet* m, double* ms_by_kind, long long* launches_by_kind, int kinds);
/* patches: device uint8 [n, h, w, 3] (h, w >= image_size): centre crop, normalise, network, global average pool.
 * out: device float32 [n, embed_dim] at any float-aligned address (the pool stores single floats: the same bits wherever out
 * lies).  Same arguments and workspace rules as ap_vit_forward_u8; asynchronous on `stream`. */
int ap_resnet_forward_u8(ap_resnet* m, const uint8_t* patches, int n, int h, int w,
                         const float mean[3], const float stdv[3],
                         float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream);

/* Single operators of the ResNet forward (NHWC, T = dtype, device pointers 16-byte aligned):
 * ap_conv2d_nhwc: out[n, Ho, Wo, cout] = act(conv(x, weight) + bias[co] (+ resid)), x T [n, h, w, cin] (cin % 8 == 0),
 *   weight T [cout][ksize][ksize][cin] (cout % 64 == 0), bias f32 [cout], resid T [n, Ho, Wo, cout] or NULL, relu 0 / 1;
 *   Ho = (h + 2 pad - ksize) / stride + 1; taps outside the image are zeros.  Offsets into x, resid and out are 64-bit; the
 *   output pixel index is an int, so n * Ho * Wo <= 2^31 - 128 (AP_ERR_INVALID beyond, nothing launched).
 * ap_maxpool3x3s2_nhwc: out T [n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, c] (padding 1; padded taps ignored), c % 8 == 0.
 * ap_avgpool_nhwc: out f32 [n, c] = mean over the hw pixels of x T [n, hw, c], summed in f32. */
int ap_conv2d_nhwc(int dtype, const void* x, int n, int h, int w, int cin, const void* weight, const float* bias, int cout,
                   int ksize, int stride, int pad, const void* resid, int relu, void* out, ap_stream_t stream);
int ap_maxpool3x3s2_nhwc(int dtype, const void* x, int n, int h, int w, int c, void* out, ap_stream_t stream);
int ap_avgpool_nhwc(int dtype, const void* x, int n, int hw, int c, float* out, ap_stream_t stream);

/* ---- ConvNeXt encoder (additive to ABI v20) ----------------------------------------------
 * Replaces the torchvision convnext_tiny / small / base / large forward of models/patch/convnext.py (classifier = Identity:
 * the flattened global average pool of the last stage, WITHOUT the head's LayerNorm) with the kernels of convnext.hip and
 * conv.hip.  Activations are NHWC in the compute type; accumulation and LayerNorm statistics are f32; every LayerNorm has
 * eps 1e-6 and every GELU is the erf form.  Same structure rules as ap_resnet_config. */
typedef struct ap_convnext ap_convnext;
typedef struct ap_convnext_config {
    uint32_t struct_size; /* sizeof(ap_convnext_config) as the caller sees it; written by ap_convnext_config_init */
    int depths[4];        /* blocks per stage: 3 3 9 3 (tiny) / 3 3 27 3 (small, base, large) */
    int widths[4];        /* channels per stage (multiples of 32): 96 192 384 768 / 128 256 512 1024 / 192 384 768 1536 */
    int compute_dtype;    /* AP_F16 / AP_BF16 / AP_F32 (exact f32 MFMA products) */
    int image_size;       /* 224: the centre crop the network sees (a multiple of 32) */
} ap_convnext_config;
#define AP_CONVNEXT_CONFIG_SIZE_V20 44u   /* the smallest size ap_convnext_create accepts */
size_t ap_sizeof_convnext_config(void);
int ap_convnext_config_init(ap_convnext_config* cfg, size_t sizeof_caller);
int ap_convnext_create(const ap_convnext_config* cfg, ap_convnext** out);
void ap_convnext_destroy(ap_convnext* m);
/* Upload one parameter (host float32, torch layout, `count` elements); synchronous.  Names (torchvision's; s = 1, 3, 5, 7
 * for the four stages, d = 2, 4, 6 for the downsampling layers in front of stages 2 - 4):
 *   features.0.0.weight [C0, 3, 4, 4] | .bias [C0]            stem convolution (stride 4)
 *   features.0.1.weight [C0] | .bias [C0]                      stem LayerNorm
 *   features.<s>.<j>.block.0.weight [C, 1, 7, 7] | .bias [C]   depthwise 7x7 convolution (padding 3)
 *   features.<s>.<j>.block.2.weight [C] | .bias [C]            LayerNorm
 *   features.<s>.<j>.block.3.weight [4C, C] | .bias [4C]       fc1 (GELU follows)
 *   features.<s>.<j>.block.5.weight [C, 4C] | .bias [C]        fc2 WITH layer_scale folded in by the caller (gamma_o * W[o],
 *                                                              gamma_o * b[o], in f32)
 *   features.<d>.0.weight [C] | .bias [C]                      downsampling LayerNorm
 *   features.<d>.1.weight [2C, C, 2, 2] | .bias [2C]           downsampling convolution (stride 2)
 * Setting a parameter un-finalises the object. */
int ap_convnext_set_param(ap_convnext* m, const char* name, const float* host, size_t count);
int ap_convnext_finalize(ap_convnext* m);          /* AP_ERR_STATE if a parameter was never set */
size_t ap_convnext_workspace_bytes(const ap_convnext* m, int n);
int ap_convnext_embed_dim(const ap_convnext* m);   /* widths[3] */
#define AP_CONVNEXT_PROF_STEM 0        /* preprocess + stem convolution + stem LayerNorm */
#define AP_CONVNEXT_PROF_DWCONV_LN 1
#define AP_CONVNEXT_PROF_FC1 2
#define AP_CONVNEXT_PROF_FC2 3
#define AP_CONVNEXT_PROF_DOWNSAMPLE 4  /* LayerNorm + 2x2 stride-2 convolution */
#define AP_CONVNEXT_PROF_POOL 5
#define AP_CONVNEXT_PROF_KINDS 6
int ap_convnext_profile_enable(ap_convnext* m, int on);
int ap_convnext_profile_read(ap_convnext* m, double* ms_by_kind, long long* launches_by_kind, int kinds);
/* Same arguments and semantics as ap_resnet_forward_u8 (out at any float-aligned address); out: device float32 [n, widths[3]]. */
int ap_convnext_forward_u8(ap_convnext* m, const uint8_t* patches, int n, int h, int w,
                           const float mean[3], const float stdv[3],
                           float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream);

/* Single operators of the ConvNeXt forward (NHWC, T = dtype, device pointers 16-byte aligned):
 * ap_conv2d_nhwc_ex: ap_conv2d_nhwc with cout % 32 == 0 and act 0 none / 1 ReLU / 2 GELU (erf), applied after the residual.
 * ap_dwconv7_ln_nhwc: y = T(depthwise 7x7 conv (padding 3) of x T [n, h, w, c] + dw_bias), then out T [n, h, w, c] =
 *   LayerNorm over the c channels of each pixel of y (f32 statistics, eps) * ln_weight + ln_bias; dw_weight f32 [49][c]
 *   (tap-major: [(ky * 7 + kx) * c + ch]), the rest f32 [c]; c % 8 == 0; out must not alias x.
 * ap_layernorm_rows: out T [rows, c] = LayerNorm of each row of x T [rows, c] (f32 statistics, eps) * weight + bias;
 *   rows <= 2^31 - 4 (AP_ERR_INVALID beyond). */
int ap_conv2d_nhwc_ex(int dtype, const void* x, int n, int h, int w, int cin, const void* weight, const float* bias, int cout,
                      int ksize, int stride, int pad, const void* resid, int act, void* out, ap_stream_t stream);
int ap_dwconv7_ln_nhwc(int dtype, const void* x, int n, int h, int w, int c, const float* dw_weight, const float* dw_bias,
                       const float* ln_weight, const float* ln_bias, float eps, void* out, ap_stream_t stream);
int ap_layernorm_rows(int dtype, const void* x, int rows, int c, const float* weight, const float* bias, float eps, void* out,
                      ap_stream_t stream);

/* ---- Swin encoder: CHIEF-CTransPath (additive to ABI v20) --------------------------------
 * Replaces the timm swin_tiny_patch4_window7_224 forward with the convolutional stem of models/patch/chief_ctranspath.py
 * (head = Identity: the mean over the 49 tokens of the final LayerNorm's output) with the kernels of swin.hip, convnext.hip
 * and conv.hip.  Activations are token-major NHWC in the compute type; accumulation, softmax and LayerNorm statistics are
 * f32; every LayerNorm has eps 1e-5 and the GELU is the erf form.  Block j of a stage shifts its windows by 0 (j even, or
 * the stage's map is a single window) or window / 2.  Same structure rules as ap_resnet_config. */
typedef struct ap_swin ap_swin;
typedef struct ap_swin_config {
    uint32_t struct_size; /* sizeof(ap_swin_config) as the caller sees it; written by ap_swin_config_init */
    int depths[4];        /* blocks per stage: 2 2 6 2 */
    int heads[4];         /* attention heads per stage: 3 6 12 24 (embed_dim * 2^s / heads[s] must be 32) */
    int embed_dim;        /* 96: the first stage's width (a multiple of 32); stage s has embed_dim * 2^s channels */
    int window;           /* 7 */
    int compute_dtype;    /* AP_F16 / AP_BF16 / AP_F32 (exact f32 products) */
    int image_size;       /* 224: the centre crop the network sees (a multiple of 224) */
} ap_swin_config;
#define AP_SWIN_CONFIG_SIZE_V20 52u   /* the smallest size ap_swin_create accepts */
size_t ap_sizeof_swin_config(void);
int ap_swin_config_init(ap_swin_config* cfg, size_t sizeof_caller);
/* AP_ERR_INVALID for a window other than 7, a head dimension other than 32 in any stage, or an image size that is not a
 * multiple of 224. */
int ap_swin_create(const ap_swin_config* cfg, ap_swin** out);
void ap_swin_destroy(ap_swin* m);
/* Upload one parameter (host float32, torch layout, `count` elements); synchronous.  Names (timm's, BatchNorm folded into
 * the stem's convolutions by the caller; E = embed_dim, C = E * 2^s, s = 0..3, d = 1..3):
 *   patch_embed.proj.0.weight [E/8, 3, 3, 3] | .bias [E/8]          stem convolution 1 (stride 2, padding 1; ReLU follows)
 *   patch_embed.proj.3.weight [E/4, E/8, 3, 3] | .bias [E/4]        stem convolution 2 (stride 2, padding 1; ReLU follows)
 *   patch_embed.proj.6.weight [E, E/4, 1, 1] | .bias [E]            stem projection
 *   patch_embed.norm.weight [E] | .bias [E]
 *   layers.<d>.downsample.norm.weight [2C] | .bias [2C]              patch merging in front of stage d: LayerNorm(4 C_{d-1})
 *   layers.<d>.downsample.reduction.weight [C, 2C]                   ... and its bias-free linear layer
 *   layers.<s>.blocks.<j>.norm1.weight [C] | .bias [C]
 *   layers.<s>.blocks.<j>.attn.qkv.weight [3C, C] | .bias [3C]       rows q | k | v, head-major inside each
 *   layers.<s>.blocks.<j>.attn.relative_position_bias_table [169, heads[s]]
 *   layers.<s>.blocks.<j>.attn.proj.weight [C, C] | .bias [C]
 *   layers.<s>.blocks.<j>.norm2.weight [C] | .bias [C]
 *   layers.<s>.blocks.<j>.mlp.fc1.weight [4C, C] | .bias [4C]        (GELU follows)
 *   layers.<s>.blocks.<j>.mlp.fc2.weight [C, 4C] | .bias [C]
 *   norm.weight [8E] | .bias [8E]                                    final LayerNorm
 * The library pads the stem's channels to the implicit GEMM's granularity with zeros and expands each bias table to
 * f32 [heads][49][49].  Setting a parameter un-finalises the object. */
int ap_swin_set_param(ap_swin* m, const char* name, const float* host, size_t count);
int ap_swin_finalize(ap_swin* m);          /* AP_ERR_STATE if a parameter was never set */
size_t ap_swin_workspace_bytes(const ap_swin* m, int n);
int ap_swin_embed_dim(const ap_swin* m);   /* 8 x embed_dim */
#define AP_SWIN_PROF_STEM 0            /* preprocess + the three stem convolutions + patch_embed.norm */
#define AP_SWIN_PROF_LN 1              /* norm1, norm2 and the final LayerNorm */
#define AP_SWIN_PROF_QKV 2
#define AP_SWIN_PROF_WINDOW_ATTN 3
#define AP_SWIN_PROF_PROJ 4            /* + residual */
#define AP_SWIN_PROF_FC1 5             /* + GELU */
#define AP_SWIN_PROF_FC2 6             /* + residual */
#define AP_SWIN_PROF_MERGE 7           /* 2x2 gather + LayerNorm, and the reduction */
#define AP_SWIN_PROF_POOL 8
#define AP_SWIN_PROF_KINDS 9
int ap_swin_profile_enable(ap_swin* m, int on);
int ap_swin_profile_read(ap_swin* m, double* ms_by_kind, long long* launches_by_kind, int kinds);
/* Same arguments and semantics as ap_convnext_forward_u8 (out at any float-aligned address); out: device float32 [n, 8 x embed_dim]. */
int ap_swin_forward_u8(ap_swin* m, const uint8_t* patches, int n, int h, int w,
                       const float mean[3], const float stdv[3],
                       float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream);

/* Single operators of the Swin forward (token-major NHWC, T = dtype, device pointers 16-byte aligned):
 * ap_swin_window_attention: qkv T [n, h, w, 3 * heads * 32] (q | k | v, head-major) -> out T [n, h, w, heads * 32]: roll the
 *   map by (-shift, -shift), cut it into 7x7 windows, per window and head softmax(q k^T 32^-0.5 + rel_bias[head] + M) v, reverse
 *   the windows and roll back -- all as index arithmetic inside one kernel.  rel_bias f32 [heads][49][49] (token i = 7 yi + xi).
 *   M (shift > 0 only) is -100 where the two tokens lie in different regions of the rolled map, the regions being the slices
 *   [0, h-7) | [h-7, h-shift) | [h-shift, h) per axis.  h % 7 == 0, w % 7 == 0, h, w <= 4096, 0 <= shift < 7, 1 <= heads <= 1024; out must not alias
 *   qkv.  f32 accumulation and softmax; no atomics: a token's result does not depend on n.
 * ap_patch_merge_ln: x T [n, h, w, c] (h, w even, c % 8 == 0) -> out T [n, h/2, w/2, 4c] = LayerNorm over the 4c channels
 *   (f32 statistics, eps; ln_weight / ln_bias f32 [4c]) of x[0::2,0::2] | x[1::2,0::2] | x[0::2,1::2] | x[1::2,1::2]
 *   (rows, columns) concatenated along the channels; out must not alias x. */
int ap_swin_window_attention(int dtype, const void* qkv, int n, int h, int w, int heads, int shift, const float* rel_bias,
                             void* out, ap_stream_t stream);
int ap_patch_merge_ln(int dtype, const void* x, int n, int h, int w, int c, const float* ln_weight, const float* ln_bias, float eps,
                      void* out, ap_stream_t stream);

/* ---- OpenAI CLIP ResNet image towers (additive to ABI v20) --------------------------------
 * Replaces open_clip's encode_image for RN50 / RN101 / RN50x4 / RN50x16 / RN50x64 with the `openai` weights
 * (models/patch/clip.py: clip_rn50, clip_rn101, clip_rn50x4, clip_rn50x16, clip_rn50x64) with the kernels of conv.hip,
 * clip_resnet.hip and attn_pool.hip.  The network is CLIP's modified ResNet: a stem of three 3x3 convolutions (the first of
 * stride 2) and a 2x2 average pool; bottleneck blocks (expansion 4) in which every convolution has stride 1 and a stride of 2
 * is a 2x2 average pool behind the 3x3 convolution and in front of the shortcut's 1x1 projection; and an attention-pool
 * head: the mean of the final map's g x g tokens (g = image_size / 32) is put in front of them, a positional embedding is added
 * to all g g + 1, and the mean token alone queries them (C = 32 x width channels in heads of 64, scale 1 / 8) before the output
 * projection.  Activations are NHWC in the compute type; BatchNorm is folded into the convolutions by the caller;
 * accumulation, the pools' sums and the softmax are f32.  Maps whose channel count is not a multiple of 32 are stored padded
 * with channels that are exactly zero.  Same structure rules as ap_resnet_config. */
typedef struct ap_clip_resnet ap_clip_resnet;
typedef struct ap_clip_resnet_config {
    uint32_t struct_size; /* sizeof(ap_clip_resnet_config) as the caller sees it; written by ap_clip_resnet_config_init */
    int depths[4];        /* blocks per stage: 3 4 6 3 / 3 4 23 3 / 4 6 10 6 / 6 8 18 8 / 3 15 36 10, each 1 .. 64 */
    int width;            /* 64 / 64 / 80 / 96 / 128: the stem's output channels and the first stage's planes (a multiple of 16) */
    int image_size;       /* 224 / 224 / 288 / 384 / 448: the centre crop the network sees (a multiple of 32 in 64 .. 1024) */
    int output_dim;       /* 1024 / 512 / 640 / 768 / 1024: the embedding (a multiple of 32) */
    int compute_dtype;    /* AP_F16 / AP_BF16 / AP_F32 (exact f32 MFMA products) */
} ap_clip_resnet_config;
#define AP_CLIP_RESNET_CONFIG_SIZE_V20 36u   /* the smallest size ap_clip_resnet_create accepts */
size_t ap_sizeof_clip_resnet_config(void);
int ap_clip_resnet_config_init(ap_clip_resnet_config* cfg, size_t sizeof_caller);
/* AP_ERR_INVALID (before any device call) for an image size that is not a multiple of 32 or lies outside 64 .. 1024, a width
 * that is not a multiple of 16, a depth outside 1 .. 64 or an output dimension that is not a multiple of 32. */
int ap_clip_resnet_create(const ap_clip_resnet_config* cfg, ap_clip_resnet** out);
void ap_clip_resnet_destroy(ap_clip_resnet* m);
/* Upload one parameter (host float32, torch layout, `count` elements); synchronous.  Names (BatchNorm folded; W = width,
 * P = W 2^(s-1) the planes of layer<s>, C = 32 W, g = image_size / 32):
 *   conv1.weight [W/2, 3, 3, 3] | conv2.weight [W/2, W/2, 3, 3] | conv3.weight [W, W/2, 3, 3] | conv<k>.bias
 *   layer<s>.<b>.conv1.weight [P, Cin, 1, 1] | .conv2.weight [P, P, 3, 3] | .conv3.weight [4P, P, 1, 1] | .conv<k>.bias
 *   layer<s>.<b>.downsample.weight [4P, Cin, 1, 1] | .bias [4P]        (the first block of every stage)
 *   attnpool.pos [g g + 1, C]                                           (any other row count is refused: no interpolation)
 *   attnpool.q.weight [C, C] | .bias [C]
 *   attnpool.kv.weight [2C, C] | .bias [2C]                             (k_proj's rows, then v_proj's)
 *   attnpool.c.weight [output_dim, C] | .bias [output_dim]
 * The library permutes the weights to [Cout][ky][kx][Cin] and pads both channel counts with zeros.  Setting a parameter
 * un-finalises the object. */
int ap_clip_resnet_set_param(ap_clip_resnet* m, const char* name, const float* host, size_t count);
int ap_clip_resnet_finalize(ap_clip_resnet* m);          /* AP_ERR_STATE if a parameter was never set */
size_t ap_clip_resnet_workspace_bytes(const ap_clip_resnet* m, int n);
int ap_clip_resnet_embed_dim(const ap_clip_resnet* m);   /* output_dim */
#define AP_CLIP_RESNET_PROF_STEM 0      /* NHWC preprocess + the three stem convolutions */
#define AP_CLIP_RESNET_PROF_CONV1X1 1
#define AP_CLIP_RESNET_PROF_CONV3X3 2
#define AP_CLIP_RESNET_PROF_AVGPOOL 3   /* every 2x2 average pool: the stem's and the strided blocks' two each */
#define AP_CLIP_RESNET_PROF_HEAD 4      /* tokens, k | v and q projections, attention, output projection, T -> f32 */
#define AP_CLIP_RESNET_PROF_KINDS 5
int ap_clip_resnet_profile_enable(ap_clip_resnet* m, int on);
int ap_clip_resnet_profile_read(ap_clip_resnet* m, double* ms_by_kind, long long* launches_by_kind, int kinds);
/* Same arguments and semantics as ap_resnet_forward_u8; out: device float32 [n, output_dim] at any float-aligned address, the
 * same bits wherever it lies (float32: the last convolution writes a 16-byte aligned out itself and goes through a workspace
 * buffer and a copy otherwise). */
int ap_clip_resnet_forward_u8(ap_clip_resnet* m, const uint8_t* patches, int n, int h, int w,
                              const float mean[3], const float stdv[3],
                              float* out, void* workspace, size_t workspace_bytes, ap_stream_t stream);

/* Single operators of the CLIP ResNet forward (NHWC, T = dtype: f16 / bf16 / f32, device pointers 16-byte aligned):
 * ap_avgpool2x2_nhwc: x T [n, h, w, c] (h, w even, c % 8 == 0) -> out T [n, h/2, w/2, c]: the mean of each 2x2 block, the four
 *   taps summed in f32 as (x00 + x01) + (x10 + x11), one rounding; out must not alias x.
 * ap_clip_attnpool_tokens: x T [n, hw, c] and pos f32 [hw + 1, c] -> tokens_out T [n, hw + 1, c]: row 0 = T(mean over the hw
 *   rows of x (summed in f32) + pos[0]), row 1 + p = T(x[p] + pos[1 + p]); q_rows_out T [n, c] receives row 0 again, packed.
 *   One pass over x; c % 8 == 0, c <= 65536, hw <= 4096, n <= 65535; no atomics: an image's rows do not depend on n. */
int ap_avgpool2x2_nhwc(int dtype, const void* x, int n, int h, int w, int c, void* out, ap_stream_t stream);
int ap_clip_attnpool_tokens(int dtype, const void* x, const float* pos, int n, int hw, int c, void* tokens_out, void* q_rows_out,
                            ap_stream_t stream);

/* ---- float32 operator set of the SAM2 (Hiera-T) tissue segmenter ------------------------
 * Replaces the torch modules behind SAM2ImagePredictor.set_image / predict as the reference drives them
 * (services/segmentation.py:120-140: one 1024 x 1024 thumbnail per slide, box prompt = whole image,
 * multimask_output=False, mask_threshold 0.0).  The host chains these (atlaspatch_amd/services/sam2_hip.py);
 * all tensors are float32, channels-last ([tokens, C]), device pointers.
 *
 * ap_sgemm: out[b][m][n] = act(alpha * sum_k A[b][m][k] * W[b][n][k] + bias[n]) + resid[b][m][n]
 *   (W[b][k][n] when w_is_kn).  act: 0 none, 1 GELU (erf), 2 ReLU.  ld* = row strides, stride* = batch strides
 *   in elements; bias / resid may be NULL.  Any M, N, K. */
int ap_sgemm(const float* A, long lda, long strideA, const float* W, long ldw, long strideW, int w_is_kn,
             int batch, int M, int N, int K, float alpha, const float* bias, int act,
             const float* resid, long ldr, long strideR, float* out, long ldo, long strideO, ap_stream_t stream);
/* The same for `stack` equally shaped problems stacked along M (a batch of images through a row-wise layer), NT weights,
 * no batch strides: every output row goes through exactly the arithmetic it would go through alone (the split-K plan is
 * the single problem's), so the result does not depend on how many images are stacked; M % stack == 0. */
int ap_sgemm_stacked(const float* A, long lda, const float* W, long ldw, int stack, int M, int N, int K, const float* bias,
                     int act, const float* resid, long ldr, float* out, long ldo, ap_stream_t stream);
int ap_softmax_rows(float* x, long ld, int rows, int cols, ap_stream_t stream);     /* in place */
/* Fused attention of the trunk (hieradet.py MultiScaleAttention -> F.scaled_dot_product_attention), image-wide blocks
 * (batch = 1) and windowed blocks (batch = number of windows, window b owns rows b * tq .. of q / out and b * tk .. of k / v):
 * out[b*tq + t][h*d + c] = sum_j softmax_j(scale * q[b*tq + t][h*d + :] . k[b*tk + j][h*d + :]) v[b*tk + j][h*d + c];
 * float32, head h at column h * d; exact-f32 MFMA, online softmax, the scores never reach memory.  d in {32, 64, 96};
 * any tq, tk >= 1; row strides multiples of 4 floats, q / k / out 16-byte aligned. */
int ap_sattention_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, int batch, int heads,
                      int tq, int tk, int d, float scale, float* out, long ldo, ap_stream_t stream);
/* The same operator (same arguments, float32 in and out) with both products as split-f16 MFMA passes:
 * a b ~= a_hi b_hi + 2^-11 (a_hi b_lo + a_lo b_hi) on v_mfma_f32_32x32x16_f16 with f32 accumulation, hi = f16(x),
 * lo = f16((x - hi) * 2^11): the split of ap_split_f16_weights, x = hi + lo 2^-11 to 2^-21 |x| + 2^-36, so float32-accurate
 * (~2^-22 per product) for values of every size inside f16's range, |x| < 65504; the softmax stays float32.  Held per element
 * to the bound of the exact chain (tests/test_gpu_split_f16.py).  2x the rate of the exact chain on the image-wide blocks. */
int ap_sattention_split_f16(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, int batch, int heads,
                            int tq, int tk, int d, float scale, float* out, long ldo, ap_stream_t stream);
/* uint8 [h, w, 3] -> rows [(h/4)*(w/4), 147] of ((x/255) - mean) / std in (c, ky, kx) order: the im2col of
 * Hiera's PatchEmbed conv (7x7, stride 4, pad 3). */
int ap_sam2_patchify(const uint8_t* image, int h, int w, const float mean[3], const float stdv[3], float* out,
                     ap_stream_t stream);
/* hieradet.py window_partition / window_unpartition on [b, h, w, c]: windows [b * ceil(h/ws) * ceil(w/ws), ws*ws, c],
 * zero padded / cropped. */
int ap_window_partition(const float* x, int b, int h, int w, int c, int ws, float* win, ap_stream_t stream);
int ap_window_unpartition(const float* win, int b, int h, int w, int c, int ws, float* x, ap_stream_t stream);
/* x = resid + window_unpartition(win): the block's `x = shortcut + drop_path(attn(...))` in the same pass (hieradet.py MultiScaleBlock) */
int ap_window_unpartition_add(const float* win, const float* resid, int b, int h, int w, int c, int ws, float* x,
                              ap_stream_t stream);
/* 2x2 stride-2 max pool on [b, h, w, c] whose pixels are ld_in elements apart -> dense [b, h/2, w/2, c] */
int ap_maxpool2x2(const float* in, long ld_in, int b, int h, int w, int c, float* out, ap_stream_t stream);
int ap_add(float* out, const float* a, const float* b, size_t n, ap_stream_t stream);
int ap_add_rowvec(float* out, const float* a, const float* vec, size_t rows, int cols, ap_stream_t stream);
int ap_gelu(float* x, size_t n, ap_stream_t stream);
/* FpnNeck top-down: out [2h, 2w, c] = lateral + nearest-x2(prev [h, w, c]) */
int ap_upsample2x_add(float* out, const float* lateral, const float* prev, int h, int w, int c, ap_stream_t stream);
/* ConvTranspose2d(kernel 2, stride 2) epilogue: g [h*w, cout*4] (column co*4 + dy*2 + dx) -> out [2h, 2w, cout]
 * = g + bias[co] (+ skip) (GELU when act = 1) */
int ap_convt2x2_shuffle(const float* g, const float* bias, const float* skip, float* out, int h, int w, int cout,
                        int act, ap_stream_t stream);
/* postprocess_masks: bilinear x4 (align_corners False) of logits [size, size], then > threshold -> float {0,1} */
int ap_bilinear_up4_threshold(const float* logits, int size, float threshold, float* mask, ap_stream_t stream);
/* _resize_mask (services/segmentation.py:112-118: PIL NEAREST back to the thumbnail's shape) as a gather:
 * dst[y][x] = src[yidx[y]][xidx[x]]; yidx int32 [oh], xidx int32 [ow] (device; built on the host with Pillow's
 * accumulated-double index arithmetic, utils/resample.py::pillow_nearest_index; entries must lie inside src). */
int ap_gather2d_f32(const float* src, int src_h, int src_w, const int32_t* yidx, const int32_t* xidx, int oh, int ow,
                    float* dst, ap_stream_t stream);

/* ---- tissue mask -> patch coordinates ----------------------------------------------
 * Replaces utils/contours.py:41-131 (mask_to_contours, scale_contours) and the grid scan of
 * services/extraction.py:67-128 (_in_tissue, _iter_patch_entries, FourPointContainment). */
typedef struct ap_contours ap_contours;

/* mask: HOST float32 [h, w].  Thresholds (> 0.5) on the device, follows borders
 * (Suzuki-Abe, RETR_CCOMP / CHAIN_APPROX_NONE semantics), applies the area / hole filters
 * of mask_to_contours and scales to level 0 with scale_contours' float32 truncation.
 * Synchronous. */
int ap_contours_from_mask(const float* mask, int h, int w, double tissue_area_thresh,
                          int min_hole_area, int max_n_holes, double sx, double sy,
                          ap_contours** out, ap_stream_t stream);
void ap_contours_destroy(ap_contours* c);
int ap_contours_count(const ap_contours* c);                 /* tissue contours */
int ap_contours_num_holes(const ap_contours* c, int i);
/* points of tissue contour i (hole < 0) or of its hole `hole`; scaled=0 -> mask space.
 * Returns the point count; copies min(count, cap) int32 (x, y) pairs into xy. */
int ap_contours_points(const ap_contours* c, int i, int hole, int scaled, int32_t* xy, int cap);

/* Grid scan on the device.  coords: HOST int32 [cap, 5] rows (x, y, read_w, read_h, level) in
 * the reference's order.  *n_rows receives the total (also when it exceeds cap ->
 * AP_ERR_CAPACITY).  Synchronous. */
int ap_grid_coords(const ap_contours* c, int patch_size_src, int step_src,
                   int read_w, int read_h, int level,
                   int32_t* coords, size_t cap, size_t* n_rows, ap_stream_t stream);

/* ---- synthetic slide tiles ------------------------------------------
 * Renders tiles of a synthetic slide straight into HBM: dst uint8 [n, ps, ps, 3] for the n
 * level-0 top-left corners xy (device int32 [n, 2]).  Bit-identical to
 * atlaspatch_amd/core/wsi/synth_pixels.py.  ellipses: device int64 [k, 4]. */
int ap_synth_tiles(const int32_t* xy, int n, int ps, int level_ds, int level,
                   int64_t width, int64_t height, uint32_t seed,
                   const int64_t* ellipses, int k, uint8_t* dst, ap_stream_t stream);
/* One w x h region of pyramid level `level` whose level-0 corner is (x, y): dst uint8 [h, w, 3].  The whole-level read of
 * the thumbnail path (core/wsi/iwsi.py:246-323 reads the level nearest 1.25x in full) for synthetic slides, in HBM. */
int ap_synth_region(int64_t x, int64_t y, int w, int h, int level_ds, int level,
                    int64_t width, int64_t height, uint32_t seed,
                    const int64_t* ellipses, int k, uint8_t* dst, ap_stream_t stream);

/* Measurement aid (bench.py): one launch of 1024 single-wave workgroups; each writes, into the slot of the compute unit it ran on
 * -- slot = XCC_ID (3 bits) << 8 | SE_ID (3) << 5 | SH_ID (1) << 4 | CU_ID (4), from HW_REG_XCC_ID / HW_REG_HW_ID -- the pair
 * out[2 slot + 0] = s_memtime (shader-clock ticks), out[2 slot + 1] = s_memrealtime (100 MHz ticks) as one 16-byte store.
 * s_memtime counters of different compute units are NOT aligned with each other (offsets of 1e7 ticks and more inside one XCD),
 * so only stamps of the SAME compute unit may be differenced.  out: AP_CLOCK_PROBE_SLOTS * 2 int64 in device memory, zeroed by
 * the caller.  Two probes on one stream around a region give the average shader clock there per compute unit that both reached:
 * GHz = 0.1 * d(memtime) / d(memrealtime).  No reference counterpart.  (ABI v18: v17 keyed the slots by XCD only.) */
#define AP_CLOCK_PROBE_SLOTS 2048
int ap_clock_probe(long long* out, ap_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ATLASPATCH_HIP_H */
