// K0, host half when the device takes the Huffman decode as well (include/atlaspatch_hip.h: ap_host_jpeg_streams): a marker parser
// of its own -- no libjpeg -- that turns a tile's JPEG stream into the descriptor and the unstuffed payload of jpeg_stream.h.
//
// The input is untrusted: every segment length is checked against the buffer before a byte of the segment is read.  What is admitted
// is the subset both readers share (jpeg_host.h: jpeg_classify, the one statement of it) restricted to what ap_jpeg_entropy_decode_tiles takes; everything else
// is refused with its reason, and the caller's next route (coefficients, then pixels) takes the tile:
//   baseline sequential Huffman (SOF0), 8 bit; one scan with every component, in frame order; greyscale, YCbCr at 4:4:4 / 4:2:2
//   (2x1) / 4:2:0 (2x2) with 1x1 chroma, or RGB coded with three 1x1 components; the requested side and sampling; a side that is a
//   multiple of the MCU size and <= 976 (jpeg_slot.h: kJpegDeviceMaxSide); Huffman tables 0 / 1 that exist and form a canonical
//   code the way libjpeg checks it (jdhuff.c: jpeg_make_d_derived_tbl), DC categories <= 15; no restart interval and no RSTn marker
//   through ap_host_jpeg_streams / ap_host_tiff_tile_streams and through their _ex twins at flags 0.  With AP_JPEG_STREAM_RESTART the
//   _ex entries admit a DRI segment.  The one in force is the stream's own: a JPEGTables preset may hold one, but the tile's SOI resets
//   it, as libjpeg's does.  An interval of 0, or of at least the frame's MCU count, is a restart-free tile; otherwise the scan must
//   hold exactly ceil(MCUs / interval) - 1 markers, numbered RST0, RST1, ... modulo 8 in order, none at the scan's start, behind
//   another marker or directly in front of the scan's end -- what libjpeg would warn about, and the host reader refuses on warnings.
//   A restart marker outside a scan stays refused.
// The colour space is inferred as libjpeg does (jdapimin.c: default_decompress_parms): JFIF -> YCbCr; Adobe transform 0 -> RGB;
// neither: component ids 'R' 'G' 'B' -> RGB -- unless the container decides it (jpeg_host.h: kJpegColourRgb, a TIFF level tagged
// Photometric 2: RGB whatever the markers say).  RGB is admitted when AP_JPEG_RGB was asked for and refused under any other code;
// a YCbCr stream asked for as AP_JPEG_RGB is refused.
//
// The entropy-coded segment is walked once, memchr from FF to FF: FF 00 -> FF, FF FF -> fill, FF D0..D7 -> refused, or on a restart
// tile dropped with the payload offset behind it noted as the next interval's start, any other marker (or the end of the buffer: a
// truncated tile, which the device flags) ends it.  Destination <= source, so the pass runs in place when the tile was read straight
// into the arena; the restart table is written behind the payload only when the pass is through.
#include <sys/stat.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ap_common.h"
#include "jpeg_host.h"
#include "jpeg_slot.h"
#include "jpeg_stream.h"

namespace ap {
namespace {

constexpr unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

using Tables = JpegStreamTables;

struct Frame {
    bool seen = false;
    int width = 0, height = 0, ncomp = 0;
    int id[3], tq[3], hv[3][2] = {{0, 0}, {0, 0}, {0, 0}};
};

struct Walk {
    const unsigned char* d;
    size_t n, at = 0;
    char* why;
    size_t why_cap;
    bool fail(const char* fmt, long a = 0, long b = 0) {
        snprintf(why, why_cap, fmt, a, b);
        return false;
    }
    // the next marker code, past fill bytes; false at the end of the buffer or on a byte that is no marker
    bool marker(int* m) {
        if (at >= n) return fail("stream cut inside a header: no marker at byte %ld", (long)at);
        if (d[at] != 0xFF) return fail("byte %ld is no marker", (long)at);
        while (at < n && d[at] == 0xFF) ++at;
        if (at >= n) return fail("stream cut inside a header: no marker at byte %ld", (long)at);
        *m = d[at++];
        return true;
    }
    // a segment's body: [*body, *body + *len) lies inside the buffer
    bool segment(int m, const unsigned char** body, size_t* len) {
        if (n - at < 2) return fail("stream cut inside a header: marker %02lX has no length", m);
        const size_t L = ((size_t)d[at] << 8) | d[at + 1];
        if (L < 2) return fail("marker %02lX: segment length %ld", m, (long)L);
        if (L > n - at) return fail("marker %02lX: segment length %ld runs past the buffer", m, (long)L);
        *body = d + at + 2;
        *len = L - 2;
        at += L;
        return true;
    }
};

bool read_dqt(Walk& w, const unsigned char* p, size_t len, Tables& t) {
    while (len) {
        const int pq = p[0] >> 4, tq = p[0] & 15;
        if (pq > 1 || tq > 3) return w.fail("DQT: precision %ld or table %ld", pq, tq);
        const size_t need = 1 + (pq ? 128 : 64);
        if (len < need) return w.fail("DQT: segment too short");
        for (int k = 0; k < 64; ++k)
            t.quant[tq][kZigzag[k]] = pq ? (uint16_t)((p[1 + 2 * k] << 8) | p[2 + 2 * k]) : p[1 + k];
        t.have_quant[tq] = true;
        p += need;
        len -= need;
    }
    return true;
}

bool read_dht(Walk& w, const unsigned char* p, size_t len, Tables& t) {
    while (len) {
        if (len < 17) return w.fail("DHT: segment too short");
        const int tc = p[0] >> 4, th = p[0] & 15;
        if (tc > 1 || th > 3) return w.fail("DHT: class %ld or table %ld", tc, th);
        if (th > 1) return w.fail("DHT: table %ld (a baseline stream has tables 0 and 1)", th);
        size_t total = 0;
        int last = 0;
        for (int l = 1; l <= 16; ++l) {
            total += p[l];
            if (p[l]) last = l;
        }
        if (total > 256) return w.fail("DHT: %ld symbols", (long)total);
        if (len < 17 + total) return w.fail("DHT: segment too short");
        // libjpeg's check while it assigns the codes: after the codes of length l the next code must still fit l bits
        long code = 0;
        for (int l = 1; l <= last; ++l) {
            code += p[l];
            if (code >= (1L << l)) return w.fail("DHT: over-subscribed code at length %ld", l);
            code <<= 1;
        }
        const int slot = 2 * tc + th;
        if (tc == 0)
            for (size_t k = 0; k < total; ++k)
                if (p[17 + k] > 15) return w.fail("DHT: DC category %ld", p[17 + k]);
        memcpy(t.counts[slot], p + 1, 16);
        memset(t.symbols[slot], 0, 256);
        memcpy(t.symbols[slot], p + 17, total);
        t.have_huff[slot] = true;
        p += 17 + total;
        len -= 17 + total;
    }
    return true;
}

bool read_app(int m, const unsigned char* p, size_t len, Tables& t) {
    if (m == 0xE0 && len >= 14 && !memcmp(p, "JFIF\0", 5)) t.jfif = true;
    if (m == 0xEE && len >= 12 && !memcmp(p, "Adobe", 5)) {
        t.adobe = true;
        t.adobe_transform = p[11];
    }
    return true;
}

// a table segment (DQT, DHT, APPn, DRI, COM) into t: 1 = taken, 0 = another marker, -1 = refused, the reason in w.why
int table_segment(Walk& w, int m, const unsigned char* p, size_t len, Tables& t) {
    if (m == 0xDB) return read_dqt(w, p, len, t) ? 1 : -1;
    if (m == 0xC4) return read_dht(w, p, len, t) ? 1 : -1;
    if (m >= 0xE0 && m <= 0xEF) return read_app(m, p, len, t), 1;
    if (m == 0xFE) return 1;
    if (m != 0xDD) return 0;
    if (len != 2) return w.fail("DRI: segment length"), -1;
    t.restart = (p[0] << 8) | p[1];
    return 1;
}

// the tables-only stream of TIFF's JPEGTables: SOI, table segments, EOI
bool read_tables(Walk& w, Tables& t) {
    int m;
    if (w.n < 2 || w.d[0] != 0xFF || w.d[1] != 0xD8) return w.fail("JPEGTables is not a JPEG stream");
    w.at = 2;
    for (;;) {
        if (!w.marker(&m)) return false;
        if (m == 0xD9) return true;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        const unsigned char* p;
        size_t len;
        if (!w.segment(m, &p, &len)) return false;
        const int took = table_segment(w, m, p, len, t);
        if (took < 0) return false;
        if (!took) return w.fail("JPEGTables is not a tables-only stream: marker %02lX", m);
    }
}

}  // namespace

int jpeg_stream_tables(const unsigned char* tables, size_t tables_size, JpegStreamTables* out, char* why, size_t why_cap) {
    *out = JpegStreamTables();
    if (!tables || !tables_size) return AP_OK;
    Walk tw{tables, tables_size, 0, why, why_cap};
    return read_tables(tw, *out) ? AP_OK : AP_ERR_INVALID;
}

int jpeg_stream_stage(const JpegStreamTables* preset, const unsigned char* data, size_t size, int want_side, int want_sampling,
                      JpegStreamDesc* desc, unsigned char* arena, size_t arena_cap, size_t* used, char* why, size_t why_cap, int colour,
                      int flags) {
    constexpr int kInvalid = AP_ERR_INVALID;
    Tables t;
    if (preset) t = *preset;
    // libjpeg resets the restart interval at every SOI (jdmarker.c: get_soi), so under a JPEGTables stream with a DRI segment the interval
    // in force is still the tile's own; the entries without the flag keep refusing such a level, as they always did
    if (flags & kJpegStreamRestart) t.restart = 0;
    Walk w{data, size, 0, why, why_cap};
#define refuse(...) (w.fail(__VA_ARGS__), kInvalid)
    if (size < 2 || data[0] != 0xFF || data[1] != 0xD8) return refuse("not a JPEG stream");
    w.at = 2;
    Frame f;
    int dc_sel[3] = {0, 0, 0}, ac_sel[3] = {0, 0, 0};
    for (;;) {
        int m;
        if (!w.marker(&m)) return kInvalid;
        if (m == 0xD8 || m == 0x01) continue;
        if (m == 0xD9) return refuse("no scan before the end of the image");
        if (m >= 0xD0 && m <= 0xD7) return refuse("restart marker outside a scan");
        const unsigned char* p;
        size_t len;
        if (!w.segment(m, &p, &len)) return kInvalid;
        if (const int took = table_segment(w, m, p, len, t)) {
            if (took < 0) return kInvalid;
            continue;
        }
        if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) return refuse("progressive stream");
        if (m == 0xC9 || m == 0xCB || m == 0xCD || m == 0xCF || m == 0xCC) return refuse("arithmetic-coded stream");
        if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC7) return refuse("frame type %02lX is not baseline sequential", m);
        if (m == 0xC0) {
            if (f.seen) return refuse("two frame headers");
            if (len < 6) return refuse("SOF0: segment too short");
            if (p[0] != 8) return refuse("%ld-bit samples", p[0]);
            f.height = (p[1] << 8) | p[2];
            f.width = (p[3] << 8) | p[4];
            f.ncomp = p[5];
            if (f.ncomp != 1 && f.ncomp != 3) return refuse("%ld components: neither greyscale nor YCbCr", f.ncomp);
            if (len != 6 + 3 * (size_t)f.ncomp) return refuse("SOF0: segment length");
            for (int c = 0; c < f.ncomp; ++c) {
                f.id[c] = p[6 + 3 * c];
                f.hv[c][0] = p[7 + 3 * c] >> 4;
                f.hv[c][1] = p[7 + 3 * c] & 15;
                f.tq[c] = p[8 + 3 * c];
                if (f.tq[c] > 3) return refuse("SOF0: quantisation table %ld", f.tq[c]);
            }
            f.seen = true;
            continue;
        }
        if (m != 0xDA) return refuse("unexpected marker %02lX", m);
        // ---- SOS
        if (!f.seen) return refuse("scan before the frame header");
        if (len < 1 || len != 4 + 2 * (size_t)p[0]) return refuse("SOS: segment length");
        if (p[0] != f.ncomp) return refuse("the scan holds %ld of %ld components", p[0], f.ncomp);
        for (int c = 0; c < f.ncomp; ++c) {
            if (p[1 + 2 * c] != f.id[c]) return refuse("the scan's component %ld is out of frame order", c);
            dc_sel[c] = p[2 + 2 * c] >> 4;
            ac_sel[c] = p[2 + 2 * c] & 15;
            if (dc_sel[c] > 1 || ac_sel[c] > 1 || !t.have_huff[dc_sel[c]] || !t.have_huff[2 + ac_sel[c]])
                return refuse("component %ld selects a Huffman table that does not exist", c);
        }
        const unsigned char* tail = p + 1 + 2 * f.ncomp;
        if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) return refuse("SOS: not a full sequential scan");
        break;
    }
    // ---- what the frame says against what was asked for: the readers' shared rule (jpeg_host.h).  The colour model of a three-component
    // frame is this reader's own inference, or the container's word
    const bool rgb = colour == kJpegColourRgb || (t.jfif ? false : t.adobe ? t.adobe_transform == 0 : f.id[0] == 'R' && f.id[1] == 'G' && f.id[2] == 'B');
    JpegGeom g;
    int found;
    if (!jpeg_classify(f.ncomp, f.hv, f.ncomp == 1 ? kJpegGrey : rgb ? kJpegRgbCoded : kJpegYCbCr, f.width, f.height, want_side, want_sampling,
                       &g, &found, why, why_cap))
        return kInvalid;
    if (want_side > kJpegDeviceMaxSide) return refuse("side %ld is above the device decoder's %ld", want_side, kJpegDeviceMaxSide);
    if (want_side % (8 * g.hmax) || want_side % (8 * g.vmax)) return refuse("side %ld is no multiple of the MCU size", want_side);
    // MCUs per restart interval; 0: a restart-free tile, which an interval that covers the whole frame is as well
    const size_t mcus = (size_t)(want_side / (8 * g.hmax)) * (size_t)(want_side / (8 * g.vmax));
    size_t interval = 0, intervals = 0;
    if (t.restart) {
        if (!(flags & kJpegStreamRestart)) return refuse("restart interval %ld", (long)t.restart);
        if (t.restart < mcus) {
            interval = t.restart;
            intervals = (mcus + interval - 1) / interval;
        }
    }
    // entry k: where interval k starts in the payload.  One buffer per thread, kept from tile to tile: no allocation per tile
    thread_local std::vector<uint32_t> starts;
    starts.clear();
    if (interval) {
        starts.reserve(intervals);
        starts.push_back(0);
    }
    size_t markers = 0;
    for (int c = 0; c < f.ncomp; ++c)
        if (!t.have_quant[f.tq[c]]) return refuse("component %ld selects a quantisation table that does not exist", c);
    // ---- the entropy-coded segment, unstuffed, to arena + *used
    const size_t start = *used;
    if ((start & 15) || start > arena_cap) return refuse("arena offset %ld", (long)start);
    unsigned char* out = arena + start;
    const size_t room = arena_cap - start;
    size_t o = 0, i = w.at;
    while (i < size) {
        const unsigned char* ff = (const unsigned char*)memchr(data + i, 0xFF, size - i);
        const size_t run = ff ? (size_t)(ff - (data + i)) : size - i;
        if (run > room - o) return refuse("the arena would overflow");
        memmove(out + o, data + i, run);
        o += run;
        i += run;
        if (!ff) break;
        if (i + 1 >= size) { i = size; break; }                 // a lone FF ends the buffer: cut inside a marker
        const int nx = data[i + 1];
        if (nx == 0x00) {
            if (o >= room) return refuse("the arena would overflow");
            out[o++] = 0xFF;
            i += 2;
        } else if (nx == 0xFF) {
            i += 1;
        } else if (nx >= 0xD0 && nx <= 0xD7) {
            if (!interval) return refuse("restart marker in the scan");
            if (nx - 0xD0 != (int)(markers & 7)) return refuse("restart marker RST%ld where RST%ld is due", nx - 0xD0, (long)(markers & 7));
            ++markers;
            if (markers < intervals) {
                if (o == starts.back()) return refuse("restart interval %ld is empty", (long)(markers - 1));
                starts.push_back((uint32_t)o);
            }
            i += 2;
        } else {
            break;
        }
    }
    if (o > kJpegStreamMaxPayload) return refuse("entropy-coded segment of %ld bytes", (long)o);
    if (interval) {
        if (markers != intervals - 1) return refuse("restart markers: %ld found, %ld expected", (long)markers, (long)(intervals - 1));
        if (o == starts.back()) return refuse("restart marker directly in front of the end of the scan");
    }
    size_t padded = (o + 15) & ~(size_t)15;
    if (padded > room) return refuse("the arena would overflow");
    const size_t table_at = padded, table_bytes = (4 * intervals + 15) & ~(size_t)15;
    if (table_bytes > room - padded) return refuse("the arena would overflow");
    memset(out + o, 0, padded - o);
    if (interval) {                                                // the payload is final: the source bytes are not read again
        memset(out + table_at, 0, table_bytes);
        for (size_t k = 0; k < intervals; ++k)
            for (int b = 0; b < 4; ++b) out[table_at + 4 * k + b] = (unsigned char)(starts[k] >> (8 * b));
        padded += table_bytes;
    }
    // ---- the descriptor
    memset(desc, 0, sizeof(*desc));
    for (int c = 0; c < f.ncomp; ++c) {
        memcpy(desc->quant[c], t.quant[f.tq[c]], 128);
        desc->dc_sel[c] = (uint8_t)dc_sel[c];
        desc->ac_sel[c] = (uint8_t)ac_sel[c];
    }
    for (int s = 0; s < 4; ++s)
        if (t.have_huff[s]) {
            memcpy(desc->huff_counts[s], t.counts[s], 16);
            memcpy(desc->huff_symbols[s], t.symbols[s], 256);
        }
    desc->ncomp = (uint32_t)f.ncomp;
    desc->payload_bytes = (uint32_t)o;
    desc->payload_offset = start;
    if (interval) {
        desc->restart_interval = (uint32_t)interval;
        desc->restart_count = (uint32_t)intervals;
        desc->restart_table_offset = start + table_at;
    }
    *used = start + padded;
    return 0;
#undef refuse
}

}  // namespace ap


extern "C" size_t ap_jpeg_stream_header_bytes(void) { return ap::kJpegStreamHeader; }

extern "C" int ap_host_jpeg_stream_bound(const char* const* paths, int n, size_t* bytes) {
    AP_REQUIRE(bytes && (paths || n == 0) && n >= 0, "ap_host_jpeg_stream_bound: bad arguments");
    size_t most = 0;
    for (int i = 0; i < n; ++i) {
        struct stat st;
        AP_REQUIRE(paths[i] && stat(paths[i], &st) == 0 && st.st_size > 0, "ap_host_jpeg_stream_bound: cannot stat %s", paths[i] ? paths[i] : "(null)");
        if ((size_t)st.st_size > most) most = (size_t)st.st_size;
    }
    *bytes = (most + 15) & ~(size_t)15;
    return AP_OK;
}

// ap_host_jpeg_streams and its _ex twin: one body, one set of messages
static int stage_files(void* descs, void* arena, size_t arena_cap, size_t* arena_used, const char* const* paths, int n, int side,
                       int sampling, int flags) {
    AP_REQUIRE(descs && arena && arena_used && (paths || n == 0) && n >= 0, "ap_host_jpeg_streams: bad arguments");
    AP_REQUIRE(((uintptr_t)arena & 15) == 0 && ((uintptr_t)descs & 15) == 0, "ap_host_jpeg_streams: descs and arena must be 16-byte aligned");
    AP_REQUIRE(ap_jpeg_slot_bytes_ex(side, sampling), "ap_host_jpeg_streams: bad side %d or sampling %d", side, sampling);
    size_t used = 0;
    *arena_used = 0;
    for (int i = 0; i < n; ++i) {
        AP_REQUIRE(paths[i], "ap_host_jpeg_streams: null path %d", i);
        FILE* f = fopen(paths[i], "rb");
        AP_REQUIRE(f, "ap_host_jpeg_streams: cannot open %s", paths[i]);
        // the file goes straight into the arena, where its payload will start; one byte more is asked for to see the file's end
        unsigned char* at = (unsigned char*)arena + used;
        const size_t room = arena_cap - used;
        const size_t got = fread(at, 1, room, f);
        const bool more = got == room && fgetc(f) != EOF;
        fclose(f);
        if (more) {
            ap::set_error("ap_host_jpeg_streams: %s: the arena would overflow (%zu bytes left)", paths[i], room);
            return AP_ERR_INVALID;
        }
        AP_REQUIRE(got > 0, "ap_host_jpeg_streams: short read of %s", paths[i]);
        char why[200] = "";
        if (ap::jpeg_stream_stage(nullptr, at, got, side, sampling, (ap::JpegStreamDesc*)descs + i, (unsigned char*)arena, arena_cap,
                                  &used, why, sizeof(why), 0, flags) != 0) {
            ap::set_error("ap_host_jpeg_streams: %s: %s", paths[i], why);
            return AP_ERR_INVALID;
        }
        *arena_used = used;
    }
    return AP_OK;
}

extern "C" int ap_host_jpeg_streams(void* descs, void* arena, size_t arena_cap, size_t* arena_used, const char* const* paths, int n,
                                    int side, int sampling) {
    return stage_files(descs, arena, arena_cap, arena_used, paths, n, side, sampling, 0);
}

extern "C" int ap_host_jpeg_streams_ex(void* descs, void* arena, size_t arena_cap, size_t* arena_used, const char* const* paths, int n,
                                       int side, int sampling, int flags) {
    AP_REQUIRE((flags & ~AP_JPEG_STREAM_RESTART) == 0, "ap_host_jpeg_streams_ex: unknown flags %d", flags);
    return stage_files(descs, arena, arena_cap, arena_used, paths, n, side, sampling, flags);
}
