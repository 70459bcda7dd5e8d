// A JPEG tile as it crosses the ring when the device also takes the Huffman decode (include/atlaspatch_hip.h:
// ap_host_jpeg_streams / ap_jpeg_entropy_decode_tiles), shared by the host parser that stages it (jpeg_stream_host.cpp), the
// decode core (jpeg_entropy_core.h) and the kernel (jpeg_entropy.hip), the way jpeg_slot.h is shared.
//
// Per tile a fixed-size DESCRIPTOR (ap_jpeg_stream_header_bytes() = 2048 bytes, little endian, 16-byte aligned):
//   bytes    0 ..  383   uint16 quant[3][64], natural order, in the components' own order (unused tables zero): a slot's first 384 bytes
//   bytes  384 ..  447   uint8 huff_counts[4][16]: codes of length 1 .. 16 of the tables DC0, DC1, AC0, AC1 (raw DHT form; all zero = absent)
//   bytes  448 .. 1471   uint8 huff_symbols[4][256]: their symbols, in code order
//   bytes 1472 .. 1474   uint8 dc_sel[3]: each component's DC table (0 / 1);  byte 1475 zero
//   bytes 1476 .. 1478   uint8 ac_sel[3]: each component's AC table (0 / 1);  byte 1479 zero
//   bytes 1480 .. 1483   uint32 ncomp (1 or 3)
//   bytes 1484 .. 1487   uint32 payload_bytes
//   bytes 1488 .. 1495   uint64 payload_offset: into the arena, a multiple of 16
//   bytes 1496 .. 1499   uint32 restart_interval: MCUs per restart interval; 0 = a restart-free tile (everything the entries without
//                        AP_JPEG_STREAM_RESTART stage)
//   bytes 1500 .. 1503   uint32 restart_count: the number of intervals, ceil(MCUs / restart_interval); 0 on a restart-free tile
//   bytes 1504 .. 1511   uint64 restart_table_offset: into the arena, a multiple of 16; 0 on a restart-free tile
//   bytes 1512 .. 2047   zero
// and its PAYLOAD in a packed arena: the entropy-coded segment from the end of the SOS header to the marker that ends it (or the end
// of the stream), byte stuffing and RSTn markers removed, 16-byte aligned, followed by zeros up to the next multiple of 16.
//
// A tile with restart intervals (ap_host_jpeg_streams_ex / ap_host_tiff_tile_streams_ex with AP_JPEG_STREAM_RESTART; decoded by
// ap_jpeg_entropy_decode_tiles_rst, jpeg_restart_core.h) also has a RESTART TABLE in the arena, at the first 16-byte boundary behind
// the payload's zero fill: restart_count little-endian uint32, entry k the byte offset, relative to the payload's first byte, at which
// interval k starts.  Entry 0 is 0, the entries are strictly increasing and every one is below payload_bytes; the table is zero
// filled to a multiple of 16.  The padding bits in front of a marker stay in the payload: they are the tail of their interval.
// Every interval starts byte aligned, at block 0 of MCU k * restart_interval, with the DC predictors at zero.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ap {

constexpr int kJpegStreamHeader = 2048;
constexpr uint32_t kJpegStreamMaxPayload = (1u << 20) - 16;     // a bit position fits 23 bits (jpeg_entropy_core.h packs it so)

struct JpegStreamDesc {
    uint16_t quant[3][64];
    uint8_t huff_counts[4][16];
    uint8_t huff_symbols[4][256];
    uint8_t dc_sel[4];
    uint8_t ac_sel[4];
    uint32_t ncomp;
    uint32_t payload_bytes;
    uint64_t payload_offset;
    uint32_t restart_interval;
    uint32_t restart_count;
    uint64_t restart_table_offset;
    uint8_t reserved[kJpegStreamHeader - 1512];
};
static_assert(sizeof(JpegStreamDesc) == kJpegStreamHeader, "descriptor layout");
static_assert(offsetof(JpegStreamDesc, huff_counts) == 384 && offsetof(JpegStreamDesc, huff_symbols) == 448 &&
              offsetof(JpegStreamDesc, dc_sel) == 1472 && offsetof(JpegStreamDesc, ncomp) == 1480 &&
              offsetof(JpegStreamDesc, payload_offset) == 1488, "descriptor layout");
static_assert(offsetof(JpegStreamDesc, restart_interval) == 1496 && offsetof(JpegStreamDesc, restart_count) == 1500 &&
              offsetof(JpegStreamDesc, restart_table_offset) == 1504 && offsetof(JpegStreamDesc, reserved) == 1512, "descriptor layout");

constexpr int kJpegStreamRestart = 1;                            // include/atlaspatch_hip.h: AP_JPEG_STREAM_RESTART

// What a stream's table segments have defined so far; a tables-only stream (TIFF's JPEGTables) is parsed into one, once, and
// handed to every tile of the level.
struct JpegStreamTables {
    uint16_t quant[4][64];
    bool have_quant[4] = {false, false, false, false};
    uint8_t counts[4][16];           // DC0, DC1, AC0, AC1
    uint8_t symbols[4][256];
    bool have_huff[4] = {false, false, false, false};
    bool jfif = false, adobe = false;
    int adobe_transform = 0;
    unsigned restart = 0;
};
int jpeg_stream_tables(const unsigned char* tables, size_t tables_size, JpegStreamTables* out, char* why, size_t why_cap);

// Stage one tile (jpeg_stream_host.cpp).  `preset` (may be null): the tables that stand in front of the abbreviated or complete
// stream `data`.  The payload goes to arena + *used, which must be 16-byte aligned; `data` may BE arena + *used (bytes read
// straight into the arena: the unstuffing pass then runs in place).  AP_OK: *desc filled, *used advanced to the next multiple of 16
// behind the payload.  AP_ERR_INVALID: refused, the reason in `why`, *desc and *used untouched.  No libjpeg, callable from any thread.
// `colour`: jpeg_host.h's kJpegColourInfer (0) or kJpegColourRgb (1: the container says the three components are R, G, B).
// `flags`: 0, or kJpegStreamRestart: a restart interval below the frame's MCU count is admitted, its markers are checked (their count,
// their numbers RST0, RST1, ... modulo 8, none directly in front of the scan's end, no empty interval) and dropped, and the restart
// table follows the payload; *used then advances behind the table.
int jpeg_stream_stage(const JpegStreamTables* preset, const unsigned char* data, size_t size, int want_side, int want_sampling,
                      JpegStreamDesc* desc, unsigned char* arena, size_t arena_cap, size_t* used, char* why, size_t why_cap,
                      int colour = 0, int flags = 0);

}  // namespace ap
