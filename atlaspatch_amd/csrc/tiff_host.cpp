// Native reader of tiled-JPEG TIFF slides (Aperio SVS and generic tiled TIFF; classic and BigTIFF, both byte orders): no libtiff,
// read-only, pread only -- one handle serves every decode thread at once and holds no file position.
//
// The reference reaches such files through OpenSlide (core/wsi/openslide_wsi.py:184-205: read_region(...).convert("RGB")), which
// hands out decoded pixels.  This reader hands out what the file holds: per pyramid level the grid of abbreviated baseline JPEG
// tile streams and the level's JPEGTables stream, either decoded to RGB patches on the host (ap_host_tiff_read_patches, the
// dlopen'd libjpeg of jpeg_host.cpp) or entropy-decoded into coefficient slots for ap_jpeg_decode_tiles
// (ap_host_tiff_tile_coefficients).  Levels are the tiled IFDs with Compression 7, widest first; stripped IFDs (Aperio's
// thumbnail, label and macro) are skipped, as OpenSlide's aperio / generic-tiff drivers treat them as associated images.
//
// Colour model, per level, by libtiff's rule: SamplesPerPixel 3 with PhotometricInterpretation 2 makes the tiles' components R, G, B
// whatever their markers say (AP_JPEG_RGB on every route); any other value, or no tag, leaves the inference to libjpeg as for a file.
//
// The file is untrusted input: every offset, count and extent read from it is checked against the file size before use, and
// every product is checked for overflow.  A file outside the accepted subset is refused at open with the reason.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "ap_common.h"
#include "jpeg_host.h"
#include "jpeg_slot.h"
#include "jpeg_stream.h"

namespace {

constexpr uint64_t kMaxIfds = 4096;
constexpr uint64_t kMaxTiles = 1ull << 26;         // per level
constexpr uint64_t kMaxTables = 1ull << 20;
constexpr uint64_t kMaxDescription = 1ull << 20;

struct Level {
    uint64_t w = 0, h = 0, tw = 0, th = 0, tx = 0, ty = 0;
    std::vector<uint64_t> off, cnt;
    std::vector<unsigned char> tables;
    std::string description;
    double xres = 0, yres = 0;
    int resunit = 0;
    int sampling = -1;
    bool rgb = false;                              // SamplesPerPixel 3 with PhotometricInterpretation 2: the tiles' components are R, G, B
    int colour() const { return rgb ? ap::kJpegColourRgb : ap::kJpegColourInfer; }
};

struct Entry {
    unsigned tag = 0, type = 0;
    uint64_t count = 0;
    unsigned char value[8] = {0};                  // the value / offset field as stored
};

// pread exactly n bytes at offset off into dst
bool pread_all(int fd, uint64_t off, void* dst, uint64_t n) {
    unsigned char* p = (unsigned char*)dst;
    while (n) {
        const ssize_t got = pread(fd, p, (size_t)n, (off_t)off);
        if (got <= 0) return false;
        p += got; off += (uint64_t)got; n -= (uint64_t)got;
    }
    return true;
}

size_t type_size(unsigned type) {
    switch (type) {
        case 1: case 2: case 6: case 7: return 1;
        case 3: case 8: return 2;
        case 4: case 9: case 11: case 13: return 4;
        case 5: case 10: case 12: case 16: case 17: case 18: return 8;
        default: return 0;
    }
}

}  // namespace

struct ap_tiff {
    int fd = -1;
    uint64_t size = 0;
    bool be = false, big = false;
    std::vector<Level> levels;
};

namespace {

struct Parser {
    ap_tiff& t;
    char why[256] = "";
    int code = AP_ERR_INVALID;

    bool fail(int c, const char* fmt, ...) {
        va_list va;
        va_start(va, fmt);
        vsnprintf(why, sizeof(why), fmt, va);
        va_end(va);
        code = c;
        return false;
    }
    bool read(uint64_t off, void* dst, uint64_t n) const {
        return off <= t.size && n <= t.size - off && pread_all(t.fd, off, dst, n);
    }
    uint64_t uint_at(const unsigned char* p, size_t bytes) const {
        uint64_t v = 0;
        for (size_t i = 0; i < bytes; ++i) v |= (uint64_t)p[i] << (8 * (t.be ? bytes - 1 - i : i));
        return v;
    }
    // the entry's payload: inline in the value field or at the offset it holds (checked against the file)
    bool payload(const Entry& e, uint64_t max_bytes, std::vector<unsigned char>& buf, const char* what) {
        const size_t ts = type_size(e.type);
        if (!ts) return fail(AP_ERR_INVALID, "%s: unknown field type %u", what, e.type);
        if (e.count > max_bytes / ts) return fail(AP_ERR_INVALID, "%s: %llu values exceed the limit", what, (unsigned long long)e.count);
        const uint64_t bytes = e.count * ts, inl = t.big ? 8 : 4;
        buf.resize((size_t)bytes);
        if (bytes <= inl) {
            memcpy(buf.data(), e.value, (size_t)bytes);
            return true;
        }
        const uint64_t off = uint_at(e.value, (size_t)inl);
        if (!read(off, buf.data(), bytes))
            return fail(AP_ERR_INVALID, "%s: %llu bytes at offset %llu lie outside the file (%llu bytes)", what, (unsigned long long)bytes,
                        (unsigned long long)off, (unsigned long long)t.size);
        return true;
    }
    bool uints(const Entry& e, uint64_t max_count, std::vector<uint64_t>& out, const char* what) {
        if (!(e.type == 1 || e.type == 3 || e.type == 4 || e.type == 13 || e.type == 16 || e.type == 18))
            return fail(AP_ERR_INVALID, "%s: field type %u is not an unsigned integer", what, e.type);
        const size_t ts = type_size(e.type);
        if (e.count > max_count) return fail(AP_ERR_INVALID, "%s: %llu values, at most %llu expected", what, (unsigned long long)e.count, (unsigned long long)max_count);
        std::vector<unsigned char> buf;
        if (!payload(e, max_count * ts, buf, what)) return false;
        out.resize((size_t)e.count);
        for (uint64_t i = 0; i < e.count; ++i) out[(size_t)i] = uint_at(buf.data() + i * ts, ts);
        return true;
    }
    bool one(const Entry& e, uint64_t& v, const char* what) {
        std::vector<uint64_t> a;
        if (!uints(e, 1, a, what)) return false;
        if (a.size() != 1) return fail(AP_ERR_INVALID, "%s: no value", what);
        v = a[0];
        return true;
    }
    bool rational(const Entry& e, double& v, const char* what) {
        v = 0;
        if (e.type != 5 || e.count < 1 || e.count > 16) return true;    // another type: the tag counts as absent
        std::vector<unsigned char> buf;
        if (!payload(e, 128, buf, what)) return false;
        const uint64_t num = uint_at(buf.data(), 4), den = uint_at(buf.data() + 4, 4);
        if (den) v = (double)num / (double)den;
        return true;
    }

    bool ifd(uint64_t off, std::vector<Entry>& entries, uint64_t& next) {
        unsigned char head[8];
        const size_t cb = t.big ? 8 : 2, eb = t.big ? 20 : 12, nb = t.big ? 8 : 4;
        if (!read(off, head, cb)) return fail(AP_ERR_INVALID, "IFD at offset %llu lies outside the file", (unsigned long long)off);
        const uint64_t n = uint_at(head, cb);
        if (n > 65535) return fail(AP_ERR_INVALID, "IFD at offset %llu claims %llu entries", (unsigned long long)off, (unsigned long long)n);
        std::vector<unsigned char> raw((size_t)(n * eb + nb));
        if (!read(off + cb, raw.data(), raw.size()))
            return fail(AP_ERR_INVALID, "IFD at offset %llu (%llu entries) runs past the end of the file", (unsigned long long)off, (unsigned long long)n);
        entries.resize((size_t)n);
        for (uint64_t i = 0; i < n; ++i) {
            const unsigned char* p = raw.data() + i * eb;
            Entry& e = entries[(size_t)i];
            e.tag = (unsigned)uint_at(p, 2);
            e.type = (unsigned)uint_at(p + 2, 2);
            e.count = uint_at(p + 4, t.big ? 8 : 4);
            memcpy(e.value, p + (t.big ? 12 : 8), t.big ? 8 : 4);
        }
        next = uint_at(raw.data() + n * eb, nb);
        return true;
    }

    // one IFD -> a level (tiled = true) or nothing (a stripped image)
    bool level(const std::vector<Entry>& entries, Level& lv, bool& tiled) {
        uint64_t compression = 1, spp = 1, planar = 1, unit = 2, photometric = ~0ull;
        std::vector<uint64_t> bps;
        const Entry *offs = nullptr, *cnts = nullptr, *tables = nullptr, *desc = nullptr, *xres = nullptr, *yres = nullptr;
        tiled = false;
        for (const Entry& e : entries)
            if (e.tag == 322) tiled = true;
        if (!tiled) return true;
        for (const Entry& e : entries) {
            switch (e.tag) {
                case 256: if (!one(e, lv.w, "ImageWidth")) return false; break;
                case 257: if (!one(e, lv.h, "ImageLength")) return false; break;
                case 258: if (!uints(e, 8, bps, "BitsPerSample")) return false; break;
                case 259: if (!one(e, compression, "Compression")) return false; break;
                case 262:                                             // another type or count: the tag counts as absent
                    if ((e.type == 1 || e.type == 3 || e.type == 4) && e.count == 1 && !one(e, photometric, "PhotometricInterpretation")) return false;
                    break;
                case 270: desc = &e; break;
                case 277: if (!one(e, spp, "SamplesPerPixel")) return false; break;
                case 282: xres = &e; break;
                case 283: yres = &e; break;
                case 284: if (!one(e, planar, "PlanarConfiguration")) return false; break;
                case 296: if (!one(e, unit, "ResolutionUnit")) return false; break;
                case 322: if (!one(e, lv.tw, "TileWidth")) return false; break;
                case 323: if (!one(e, lv.th, "TileLength")) return false; break;
                case 324: offs = &e; break;
                case 325: cnts = &e; break;
                case 347: tables = &e; break;
                default: break;
            }
        }
        if (compression != 7) {
            const char* name = compression == 33003 || compression == 33005 ? " (Aperio JPEG 2000)" : compression == 5 ? " (LZW)" :
                               compression == 8 || compression == 32946 ? " (deflate)" : compression == 6 ? " (old-style JPEG)" :
                               compression == 1 ? " (uncompressed)" : "";
            return fail(AP_ERR_UNSUPPORTED, "tiled level with Compression %llu%s: only 7 (JPEG) is read", (unsigned long long)compression, name);
        }
        if (!(spp == 1 || spp == 3)) return fail(AP_ERR_UNSUPPORTED, "SamplesPerPixel %llu: only 1 and 3 are read", (unsigned long long)spp);
        if (bps.empty()) bps.assign(1, 1);                                // TIFF's default is 1 bit
        for (uint64_t b : bps)
            if (b != 8) return fail(AP_ERR_UNSUPPORTED, "BitsPerSample %llu: only 8 is read", (unsigned long long)b);
        if (planar != 1) return fail(AP_ERR_UNSUPPORTED, "PlanarConfiguration %llu: only 1 (chunky) is read", (unsigned long long)planar);
        if (lv.w == 0 || lv.h == 0 || lv.w > 0x7FFFFFFFull || lv.h > 0x7FFFFFFFull)
            return fail(AP_ERR_INVALID, "image size %llu x %llu is empty or overflows", (unsigned long long)lv.w, (unsigned long long)lv.h);
        if (lv.tw == 0 || lv.th == 0 || lv.tw % 16 || lv.th % 16 || lv.tw > 65535 || lv.th > 65535)
            return fail(AP_ERR_INVALID, "tile size %llu x %llu is not a multiple of 16 (or exceeds a JPEG frame)", (unsigned long long)lv.tw, (unsigned long long)lv.th);
        lv.tx = (lv.w + lv.tw - 1) / lv.tw;
        lv.ty = (lv.h + lv.th - 1) / lv.th;
        const uint64_t tiles = lv.tx * lv.ty;                              // both < 2^31 / 16
        if (tiles > kMaxTiles) return fail(AP_ERR_INVALID, "%llu tiles in one level exceed the limit", (unsigned long long)tiles);
        if (!offs || !cnts) return fail(AP_ERR_INVALID, "tiled level without TileOffsets / TileByteCounts");
        if (offs->count != tiles || cnts->count != tiles)
            return fail(AP_ERR_INVALID, "TileOffsets / TileByteCounts hold %llu / %llu values, the %llu x %llu grid needs %llu",
                        (unsigned long long)offs->count, (unsigned long long)cnts->count, (unsigned long long)lv.tx, (unsigned long long)lv.ty,
                        (unsigned long long)tiles);
        if (!uints(*offs, tiles, lv.off, "TileOffsets") || !uints(*cnts, tiles, lv.cnt, "TileByteCounts")) return false;
        for (uint64_t i = 0; i < tiles; ++i) {
            const uint64_t o = lv.off[(size_t)i], c = lv.cnt[(size_t)i];
            if (o == 0 || c == 0) { lv.off[(size_t)i] = lv.cnt[(size_t)i] = 0; continue; }       // a missing tile
            if (o > t.size || c > t.size - o)
                return fail(AP_ERR_INVALID, "tile %llu: %llu bytes at offset %llu lie outside the file (%llu bytes)", (unsigned long long)i,
                            (unsigned long long)c, (unsigned long long)o, (unsigned long long)t.size);
        }
        if (tables) {
            if (!(tables->type == 1 || tables->type == 7)) return fail(AP_ERR_INVALID, "JPEGTables: field type %u", tables->type);
            if (!payload(*tables, kMaxTables, lv.tables, "JPEGTables")) return false;
        }
        if (desc && desc->type == 2) {
            std::vector<unsigned char> buf;
            if (!payload(*desc, kMaxDescription, buf, "ImageDescription")) return false;
            lv.description.assign((const char*)buf.data(), buf.size());
            const size_t nul = lv.description.find('\0');
            if (nul != std::string::npos) lv.description.resize(nul);
        }
        if (xres && !rational(*xres, lv.xres, "XResolution")) return false;
        if (yres && !rational(*yres, lv.yres, "YResolution")) return false;
        lv.resunit = (int)std::min<uint64_t>(unit, 65535);
        // libtiff's rule (tif_jpeg.c: JPEGPreDecode): only Photometric 6 lets libjpeg convert YCbCr; under 2 the components are handed
        // out as R, G, B whatever the stream's markers say.  Any other value, or no tag, keeps libjpeg's inference.
        lv.rgb = spp == 3 && photometric == 2;
        return true;
    }

    // sampling of the level's first present tile, or -1 when the stream is outside ap_jpeg_decode_tiles' subset.  An RGB level
    // (Photometric 2) reports AP_JPEG_RGB or -1, and is refused (false) when that tile has a subsampled component: libtiff rejects
    // such a file ("Improper JPEG sampling factors"), and no route of this reader decodes it as libtiff would.
    bool probe(Level& lv) {
        lv.sampling = -1;
        const bool device = lv.tw == lv.th && lv.tw <= (uint64_t)ap::kJpegDeviceMaxSide;
        if (!device && !lv.rgb) return true;
        for (size_t i = 0; i < lv.off.size(); ++i) {
            if (!lv.cnt[i]) continue;
            std::vector<unsigned char> buf((size_t)lv.cnt[i]);
            if (!read(lv.off[i], buf.data(), lv.cnt[i])) return true;
            int wh[2] = {0, 0}, found = -1;
            char w2[200] = "";
            const int rc = ap::jpeg_mem_coefficients(lv.tables.empty() ? nullptr : lv.tables.data(), lv.tables.size(), buf.data(), buf.size(),
                                                     wh, &found, 0, 0, nullptr, w2, sizeof(w2), lv.colour());
            if (rc != AP_OK && lv.rgb && found == ap::kJpegRgbSubsampled)
                return fail(AP_ERR_UNSUPPORTED, "level tagged PhotometricInterpretation 2 (RGB) holds a subsampled tile: %s", w2);
            if (rc == AP_OK && device && wh[0] == (int)lv.tw && wh[1] == (int)lv.th && lv.rgb == (found == AP_JPEG_RGB))   // RGB-inferred tiles outside an RGB level: -1
                lv.sampling = found;
            return true;
        }
        return true;
    }

    bool parse() {
        struct stat st;
        if (fstat(t.fd, &st) != 0 || st.st_size < 0) return fail(AP_ERR_INVALID, "cannot stat the file");
        t.size = (uint64_t)st.st_size;
        unsigned char head[16];
        if (t.size < 8 || !read(0, head, 8)) return fail(AP_ERR_INVALID, "%llu bytes: too short for a TIFF header", (unsigned long long)t.size);
        if (head[0] == 'I' && head[1] == 'I') t.be = false;
        else if (head[0] == 'M' && head[1] == 'M') t.be = true;
        else return fail(AP_ERR_INVALID, "not a TIFF file (no II / MM byte-order mark)");
        const uint64_t magic = uint_at(head + 2, 2);
        uint64_t next = 0;
        if (magic == 42) {
            t.big = false;
            next = uint_at(head + 4, 4);
        } else if (magic == 43) {
            t.big = true;
            if (!read(0, head, 16)) return fail(AP_ERR_INVALID, "too short for a BigTIFF header");
            if (uint_at(head + 4, 2) != 8 || uint_at(head + 6, 2) != 0) return fail(AP_ERR_INVALID, "BigTIFF header with an offset size other than 8");
            next = uint_at(head + 8, 8);
        } else {
            return fail(AP_ERR_INVALID, "not a TIFF file (magic %llu)", (unsigned long long)magic);
        }
        std::unordered_set<uint64_t> seen;
        std::vector<Entry> entries;
        while (next) {
            if (!seen.insert(next).second) return fail(AP_ERR_INVALID, "the IFD chain returns to offset %llu: a cycle", (unsigned long long)next);
            if (seen.size() > kMaxIfds) return fail(AP_ERR_INVALID, "more than %llu IFDs", (unsigned long long)kMaxIfds);
            uint64_t after = 0;
            if (!ifd(next, entries, after)) return false;
            Level lv;
            bool tiled = false;
            if (!level(entries, lv, tiled)) return false;
            if (tiled) t.levels.push_back(std::move(lv));
            next = after;
        }
        if (t.levels.empty()) return fail(AP_ERR_UNSUPPORTED, "no tiled JPEG level (a stripped TIFF is not read)");
        std::stable_sort(t.levels.begin(), t.levels.end(), [](const Level& a, const Level& b) { return a.w > b.w; });
        for (Level& lv : t.levels)
            if (!probe(lv)) return false;
        return true;
    }
};

bool read_tile(const ap_tiff* t, const Level& lv, size_t id, std::vector<unsigned char>& buf) {
    buf.resize((size_t)lv.cnt[id]);
    return pread_all(t->fd, lv.off[id], buf.data(), lv.cnt[id]);
}

}  // namespace

extern "C" int ap_host_tiff_open(const char* path, ap_tiff** out) {
    AP_REQUIRE(path && out, "ap_host_tiff_open: null pointer");
    *out = nullptr;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    AP_REQUIRE(fd >= 0, "ap_host_tiff_open: cannot open %s", path);
    ap_tiff* t = new ap_tiff;
    t->fd = fd;
    Parser p{*t};
    if (!p.parse()) {
        ap::set_error("ap_host_tiff_open: %s: %s", path, p.why);
        close(fd);
        delete t;
        return p.code;
    }
    *out = t;
    return AP_OK;
}

extern "C" void ap_host_tiff_close(ap_tiff* slide) {
    if (!slide) return;
    if (slide->fd >= 0) close(slide->fd);
    delete slide;
}

extern "C" int ap_host_tiff_info(const ap_tiff* slide, int* levels, double* resolution, int* resolution_unit, char* description,
                                 size_t description_cap, size_t* description_bytes) {
    AP_REQUIRE(slide && levels && resolution && resolution_unit && description_bytes && (description || description_cap == 0),
               "ap_host_tiff_info: null pointer");
    const Level& l0 = slide->levels[0];
    *levels = (int)slide->levels.size();
    resolution[0] = l0.xres;
    resolution[1] = l0.yres;
    *resolution_unit = l0.resunit;
    *description_bytes = l0.description.size();
    if (description_cap) {
        const size_t n = std::min(description_cap - 1, l0.description.size());
        memcpy(description, l0.description.data(), n);
        description[n] = 0;
    }
    return AP_OK;
}

extern "C" int ap_host_tiff_level(const ap_tiff* slide, int level, int64_t* geometry) {
    AP_REQUIRE(slide && geometry, "ap_host_tiff_level: null pointer");
    AP_REQUIRE(level >= 0 && (size_t)level < slide->levels.size(), "ap_host_tiff_level: level %d of %zu", level, slide->levels.size());
    const Level& lv = slide->levels[(size_t)level];
    const int64_t g[8] = {(int64_t)lv.w, (int64_t)lv.h, (int64_t)lv.tw, (int64_t)lv.th, (int64_t)lv.tx, (int64_t)lv.ty, lv.sampling,
                          (int64_t)lv.tables.size()};
    memcpy(geometry, g, sizeof(g));
    return AP_OK;
}

extern "C" int ap_host_tiff_tile_present(const ap_tiff* slide, int level, uint8_t* present) {
    AP_REQUIRE(slide && present, "ap_host_tiff_tile_present: null pointer");
    AP_REQUIRE(level >= 0 && (size_t)level < slide->levels.size(), "ap_host_tiff_tile_present: level %d of %zu", level, slide->levels.size());
    const Level& lv = slide->levels[(size_t)level];
    for (size_t i = 0; i < lv.cnt.size(); ++i) present[i] = lv.cnt[i] ? 1 : 0;
    return AP_OK;
}

extern "C" int ap_host_tiff_read_patches(const ap_tiff* slide, int level, const int64_t* xy, int n, int w, int h, void* dst) {
    AP_REQUIRE(slide && (n == 0 || (xy && dst)) && n >= 0 && w > 0 && h > 0, "ap_host_tiff_read_patches: bad arguments");
    AP_REQUIRE(level >= 0 && (size_t)level < slide->levels.size(), "ap_host_tiff_read_patches: level %d of %zu", level, slide->levels.size());
    AP_REQUIRE((uint64_t)w * (uint64_t)h <= (1ull << 40) / 3 / (uint64_t)(n ? n : 1), "ap_host_tiff_read_patches: %d patches of %d x %d overflow", n, w, h);
    const Level& lv = slide->levels[(size_t)level];
    const int64_t W = (int64_t)lv.w, H = (int64_t)lv.h, tw = (int64_t)lv.tw, th = (int64_t)lv.th;
    const size_t patch_bytes = (size_t)w * h * 3, tile_row = (size_t)tw * 3;
    if (n) memset(dst, 0, patch_bytes * (size_t)n);                       // outside the level and missing tiles: 0
    std::unordered_map<uint64_t, std::vector<unsigned char>> decoded;    // a tile is decoded once per call
    std::vector<unsigned char> stream;
    for (int p = 0; p < n; ++p) {
        const int64_t x0 = xy[2 * p], y0 = xy[2 * p + 1];
        AP_REQUIRE(x0 > -(1ll << 40) && x0 < (1ll << 40) && y0 > -(1ll << 40) && y0 < (1ll << 40), "ap_host_tiff_read_patches: patch %d origin overflows", p);
        // the part of the patch inside the level, in level coordinates
        const int64_t xa = std::max<int64_t>(x0, 0), ya = std::max<int64_t>(y0, 0), xb = std::min<int64_t>(x0 + w, W), yb = std::min<int64_t>(y0 + h, H);
        if (xa >= xb || ya >= yb) continue;
        unsigned char* out = (unsigned char*)dst + (size_t)p * patch_bytes;
        for (int64_t ty = ya / th; ty <= (yb - 1) / th; ++ty)
            for (int64_t tx = xa / tw; tx <= (xb - 1) / tw; ++tx) {
                const uint64_t id = (uint64_t)ty * lv.tx + (uint64_t)tx;
                if (!lv.cnt[(size_t)id]) continue;
                auto it = decoded.find(id);
                if (it == decoded.end()) {
                    char why[200] = "";
                    std::vector<unsigned char> px((size_t)tw * th * 3);
                    int rc = AP_ERR_INVALID;
                    if (!read_tile(slide, lv, (size_t)id, stream)) snprintf(why, sizeof(why), "short read");
                    else rc = ap::jpeg_mem_pixels(lv.tables.empty() ? nullptr : lv.tables.data(), lv.tables.size(), stream.data(), stream.size(),
                                                  (int)tw, (int)th, px.data(), tile_row, why, sizeof(why), lv.colour());
                    if (rc != AP_OK) {
                        ap::set_error("ap_host_tiff_read_patches: level %d tile (%lld, %lld): %s", level, (long long)tx, (long long)ty, why);
                        return rc;
                    }
                    it = decoded.emplace(id, std::move(px)).first;
                }
                const int64_t cx0 = std::max(xa, tx * tw), cx1 = std::min(xb, (tx + 1) * tw);
                const int64_t cy0 = std::max(ya, ty * th), cy1 = std::min(yb, (ty + 1) * th);
                for (int64_t y = cy0; y < cy1; ++y)
                    memcpy(out + ((size_t)(y - y0) * w + (size_t)(cx0 - x0)) * 3,
                           it->second.data() + (size_t)(y - ty * th) * tile_row + (size_t)(cx0 - tx * tw) * 3, (size_t)(cx1 - cx0) * 3);
            }
    }
    return AP_OK;
}

extern "C" int ap_host_tiff_tile_coefficients(const ap_tiff* slide, int level, const int32_t* tile_ids, int m, void* slots) {
    AP_REQUIRE(slide && (m == 0 || (tile_ids && slots)) && m >= 0, "ap_host_tiff_tile_coefficients: bad arguments");
    AP_REQUIRE(level >= 0 && (size_t)level < slide->levels.size(), "ap_host_tiff_tile_coefficients: level %d of %zu", level, slide->levels.size());
    const Level& lv = slide->levels[(size_t)level];
    AP_REQUIRE(lv.sampling >= 0, "ap_host_tiff_tile_coefficients: level %d is outside the device decoder's subset", level);
    const size_t stride = ap_jpeg_slot_bytes_ex((int)lv.tw, lv.sampling);
    AP_REQUIRE(stride, "ap_host_tiff_tile_coefficients: bad side %d or sampling %d", (int)lv.tw, lv.sampling);
    std::vector<unsigned char> stream;
    for (int i = 0; i < m; ++i) {
        const int64_t id = tile_ids[i];
        AP_REQUIRE(id >= 0 && (uint64_t)id < lv.cnt.size(), "ap_host_tiff_tile_coefficients: tile id %lld of %zu", (long long)id, lv.cnt.size());
        const long long tx = (long long)((uint64_t)id % lv.tx), ty = (long long)((uint64_t)id / lv.tx);
        AP_REQUIRE(lv.cnt[(size_t)id], "ap_host_tiff_tile_coefficients: level %d tile (%lld, %lld) is missing", level, tx, ty);
        char why[200] = "";
        int wh[2], found, rc = AP_ERR_INVALID;
        if (!read_tile(slide, lv, (size_t)id, stream)) snprintf(why, sizeof(why), "short read");
        else rc = ap::jpeg_mem_coefficients(lv.tables.empty() ? nullptr : lv.tables.data(), lv.tables.size(), stream.data(), stream.size(), wh,
                                            &found, (int)lv.tw, lv.sampling, (unsigned char*)slots + (size_t)i * stride, why, sizeof(why),
                                            lv.colour());
        if (rc != AP_OK) {
            ap::set_error("ap_host_tiff_tile_coefficients: level %d tile (%lld, %lld): %s", level, tx, ty, why);
            return rc;
        }
    }
    return AP_OK;
}

extern "C" size_t ap_host_tiff_max_tile_bytes(const ap_tiff* slide, int level) {
    if (!slide || level < 0 || (size_t)level >= slide->levels.size()) return 0;
    uint64_t most = 0;
    for (uint64_t c : slide->levels[(size_t)level].cnt) most = std::max(most, c);
    return (size_t)((most + 15) & ~(uint64_t)15);
}

// ap_host_tiff_tile_streams and its _ex twin: one body, one set of messages
static int stage_tiles(const ap_tiff* slide, int level, const int32_t* tile_ids, int m, void* descs, void* arena, size_t arena_cap,
                       size_t* arena_used, int flags) {
    AP_REQUIRE(slide && arena_used && (m == 0 || (tile_ids && descs && arena)) && m >= 0, "ap_host_tiff_tile_streams: bad arguments");
    AP_REQUIRE((((uintptr_t)arena | (uintptr_t)descs) & 15) == 0, "ap_host_tiff_tile_streams: descs and arena must be 16-byte aligned");
    AP_REQUIRE(level >= 0 && (size_t)level < slide->levels.size(), "ap_host_tiff_tile_streams: level %d of %zu", level, slide->levels.size());
    const Level& lv = slide->levels[(size_t)level];
    AP_REQUIRE(lv.sampling >= 0, "ap_host_tiff_tile_streams: level %d is outside the device decoder's subset", level);
    size_t used = 0;
    *arena_used = 0;
    ap::JpegStreamTables tables;
    char twhy[200] = "";
    if (ap::jpeg_stream_tables(lv.tables.data(), lv.tables.size(), &tables, twhy, sizeof(twhy)) != AP_OK) {
        ap::set_error("ap_host_tiff_tile_streams: level %d: %s", level, twhy);
        return AP_ERR_INVALID;
    }
    for (int i = 0; i < m; ++i) {
        const int64_t id = tile_ids[i];
        AP_REQUIRE(id >= 0 && (uint64_t)id < lv.cnt.size(), "ap_host_tiff_tile_streams: tile id %lld of %zu", (long long)id, lv.cnt.size());
        const long long tx = (long long)((uint64_t)id % lv.tx), ty = (long long)((uint64_t)id / lv.tx);
        AP_REQUIRE(lv.cnt[(size_t)id], "ap_host_tiff_tile_streams: level %d tile (%lld, %lld) is missing", level, tx, ty);
        char why[200] = "";
        int rc = AP_ERR_INVALID;
        // the tile's bytes go straight into the arena, where its payload will start; the unstuffing pass then runs in place
        const uint64_t bytes = lv.cnt[(size_t)id];
        unsigned char* at = (unsigned char*)arena + used;
        if (bytes > arena_cap - used) snprintf(why, sizeof(why), "the arena would overflow");
        else if (!pread_all(slide->fd, lv.off[(size_t)id], at, bytes)) snprintf(why, sizeof(why), "short read");
        else rc = ap::jpeg_stream_stage(&tables, at, (size_t)bytes, (int)lv.tw, lv.sampling, (ap::JpegStreamDesc*)descs + i, (unsigned char*)arena,
                                        arena_cap, &used, why, sizeof(why), lv.colour(), flags);
        if (rc != AP_OK) {
            ap::set_error("ap_host_tiff_tile_streams: level %d tile (%lld, %lld): %s", level, tx, ty, why);
            return rc;
        }
        *arena_used = used;
    }
    return AP_OK;
}

extern "C" int ap_host_tiff_tile_streams(const ap_tiff* slide, int level, const int32_t* tile_ids, int m, void* descs, void* arena,
                                         size_t arena_cap, size_t* arena_used) {
    return stage_tiles(slide, level, tile_ids, m, descs, arena, arena_cap, arena_used, 0);
}

extern "C" int ap_host_tiff_tile_streams_ex(const ap_tiff* slide, int level, const int32_t* tile_ids, int m, void* descs, void* arena,
                                            size_t arena_cap, size_t* arena_used, int flags) {
    AP_REQUIRE((flags & ~AP_JPEG_STREAM_RESTART) == 0, "ap_host_tiff_tile_streams_ex: unknown flags %d", flags);
    return stage_tiles(slide, level, tile_ids, m, descs, arena, arena_cap, arena_used, flags);
}
