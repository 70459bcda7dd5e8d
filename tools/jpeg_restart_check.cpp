// Stand-alone driver of the stream route's host parser under AP_JPEG_STREAM_RESTART (atlaspatch_amd/csrc/jpeg_stream_host.cpp) and of the
// restart decode core (atlaspatch_amd/csrc/jpeg_restart_core.h) for sanitizer runs on the CPU, the twin of tools/jpeg_entropy_check.cpp:
// the passes ap_jpeg_entropy_decode_tiles_rst runs on a workgroup for a restart tile are run here with the 256 lanes in a loop, so every
// table entry, payload word and slot address the kernel would touch is touched here first, under AddressSanitizer / UBSan, on exact-size
// heap blocks.  No GPU, no Python, no preload.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip tools/jpeg_restart_check.cpp atlaspatch_amd/csrc/jpeg_stream_host.cpp atlaspatch_amd/csrc/jpeg_host.cpp -ldl \
//         -o jpeg_restart_check
//   ./jpeg_restart_check SCRATCH_FILE FILE.jpg ..      (SCRATCH_FILE: where the damaged variants are written for the file readers;
//                                                        python -m tests.jpeg_restart_streams DIR writes the tests' restart corpus)
//
// Per file: the file as it is (where libjpeg reads it without a warning the slot must equal ap_host_jpeg_coefficients' outside the
// padding, status 0); cut at six depths of the file and of the entropy-coded segment; one byte flipped at eight places of that segment;
// a restart marker deleted, duplicated and renumbered; the staged descriptor with each restart field outside its bounds (interval 0
// beside a count, an interval from the frame's MCU count up to 2^32 - 1 beside count 1, count - 1 / + 1 / 0 / huge, a table offset
// outside the arena or misaligned) and the staged table with entry 0 not 0, two entries equal, two entries swapped, an entry at and
// above payload_bytes.  Every decode runs the lanes in ascending and in descending order, which must agree on status and slot: the tile's
// status is the first error in interval order.  A damaged input must end flagged, refused by the stager, or -- where libjpeg reads the
// same bytes without a warning -- with libjpeg's slot.  A file the stager stages restart free (no DRI, an interval that covers the frame)
// is counted and left to tools/jpeg_entropy_check.cpp. Exits 1 on any disagreement, 0 otherwise.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/atlaspatch_hip.h"
#include "../atlaspatch_amd/csrc/jpeg_restart_core.h"

namespace ap {
static thread_local char g_error[512];
void set_error(const char* fmt, ...) {
    va_list va;
    va_start(va, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, va);
    va_end(va);
}
}  // namespace ap

using namespace ap;

static int g_failures = 0;
static long g_runs = 0, g_flagged = 0, g_refused = 0, g_equal = 0, g_plain = 0, g_unjudged = 0;

// the kernel's body for a restart tile (jpeg_entropy.hip: jpeg_restart_kernel), barriers replaced by the end of a loop over the lanes
static int32_t run_tile(const JpegStreamDesc* desc, const uint8_t* arena, size_t arena_bytes, uint8_t* slot, int side, int sampling, bool ascending) {
    RestartShared* sh = (RestartShared*)malloc(sizeof(RestartShared));
    memset(sh, 0xA5, sizeof(RestartShared));
    RestartTile R;
    restart_tile(desc, arena, arena_bytes, slot, side, sampling, &R);
    const int nl = kEntropyLanes;
    restart_pass0_clear(sh);
    for (int l = 0; l < nl; ++l) { restart_pass0_tables(R, sh, l); entropy_pass0_slot(R.T, l, nl); }
    for (int l = 0; l < nl; ++l) restart_pass_decode(R, sh, ascending ? l : nl - 1 - l, nl);
    const int32_t status = restart_pass_status(R, sh);
    free(sh);
    return status;
}

static bool same_slot(const uint8_t* a, const uint8_t* b, size_t bytes) {
    return !memcmp(a, b, 384) && !memcmp(a + 512, b + 512, bytes - 512);
}

// one staged restart tile in both lane orders; `want`: libjpeg's slot for the same bytes, or null
static void decode_both(const char* what, const JpegStreamDesc* desc, const uint8_t* arena, size_t arena_bytes, int side, int sampling,
                        const uint8_t* want, bool must_pass, bool must_flag) {
    const size_t bytes = ap_jpeg_slot_bytes_ex(side, sampling);
    uint8_t* up = (uint8_t*)malloc(bytes);
    uint8_t* down = (uint8_t*)malloc(bytes);
    memset(up, 0x5A, bytes);
    memset(down, 0x5A, bytes);
    const int32_t a = run_tile(desc, arena, arena_bytes, up, side, sampling, true);
    const int32_t b = run_tile(desc, arena, arena_bytes, down, side, sampling, false);
    g_runs += 2;
    if (a != b || (a == 0 && !same_slot(up, down, bytes))) {
        printf("FAIL %s: lanes ascending give status %d, descending %d%s\n", what, a, b, a == b ? ", other slots" : "");
        ++g_failures;
    }
    if (a == 0 && want && !same_slot(up, want, bytes)) {
        printf("FAIL %s: status 0 and another slot than libjpeg's\n", what);
        ++g_failures;
    }
    if (a == 0 && want) ++g_equal;
    if (a == 0 && !want) ++g_unjudged;                      // e.g. a stream that lacks its EOI only: libjpeg warns, every block is there
    if (a != 0) ++g_flagged;
    if (a < 0 || a > 5) { printf("FAIL %s: status %d\n", what, a); ++g_failures; }
    if (must_pass && want && a != 0) {
        printf("FAIL %s: a stream libjpeg reads without a warning ends with status %d\n", what, a);
        ++g_failures;
    }
    if (must_flag && a == 0 && !(want && same_slot(up, want, bytes))) {
        printf("FAIL %s: a descriptor outside its bounds ends with status 0\n", what);
        ++g_failures;
    }
    free(up);
    free(down);
}

static uint32_t mcu_count(int side, int sampling) {
    JpegGeom g;
    jpeg_geom(side, sampling, &g);
    return (uint32_t)(side / (8 * g.hmax)) * (uint32_t)(side / (8 * g.vmax));
}

static size_t table_bound(int side, int sampling) { return ((size_t)4 * mcu_count(side, sampling) + 15) & ~(size_t)15; }

// a stream in memory: written to a scratch file for the two file readers, staged with AP_JPEG_STREAM_RESTART, decoded
static void check_stream(const char* what, const std::vector<uint8_t>& stream, int side, int sampling, const char* scratch, bool must_pass) {
    FILE* f = fopen(scratch, "wb");
    if (!f || fwrite(stream.data(), 1, stream.size(), f) != stream.size()) { fprintf(stderr, "cannot write %s\n", scratch); exit(3); }
    fclose(f);
    const size_t bytes = ap_jpeg_slot_bytes_ex(side, sampling);
    uint8_t* want = (uint8_t*)malloc(bytes);
    const bool libjpeg_ok = ap_host_jpeg_coefficients(want, &scratch, 1, side, sampling) == AP_OK;
    size_t bound = 0;
    if (ap_host_jpeg_stream_bound(&scratch, 1, &bound) != AP_OK) { fprintf(stderr, "%s\n", g_error); exit(3); }
    bound += table_bound(side, sampling);
    // exact-size blocks: a byte past the arena or the descriptor is a heap-buffer-overflow
    uint8_t* arena = (uint8_t*)aligned_alloc(16, bound);
    JpegStreamDesc* desc = (JpegStreamDesc*)aligned_alloc(16, sizeof(JpegStreamDesc));
    size_t used = 0;
    const int rc = ap_host_jpeg_streams_ex(desc, arena, bound, &used, &scratch, 1, side, sampling, AP_JPEG_STREAM_RESTART);
    if (rc != AP_OK) {
        ++g_refused;
        if (must_pass) { printf("FAIL %s: refused: %s\n", what, g_error); ++g_failures; }
    } else {
        if (desc->restart_interval == 0) {
            ++g_plain;
            if (desc->restart_count || desc->restart_table_offset) { printf("FAIL %s: restart fields of a restart-free tile\n", what); ++g_failures; }
        } else {
            // the decoder is handed exactly the bytes that hold the payload and the table
            uint8_t* packed = (uint8_t*)aligned_alloc(16, used ? used : 16);
            memcpy(packed, arena, used);
            decode_both(what, desc, packed, used, side, sampling, libjpeg_ok ? want : nullptr, must_pass, false);
            free(packed);
        }
        // one byte less than the file and its staged form need: refused, nothing written past the arena
        const size_t need = used > stream.size() ? used : stream.size();
        size_t used2 = 0;
        void* small = nullptr;
        if (posix_memalign(&small, 16, need - 1)) exit(3);
        if (ap_host_jpeg_streams_ex(desc, small, need - 1, &used2, &scratch, 1, side, sampling, AP_JPEG_STREAM_RESTART) == AP_OK) {
            printf("FAIL %s: an arena one byte short was accepted\n", what);
            ++g_failures;
        }
        free(small);
    }
    free(desc);
    free(arena);
    free(want);
}

// where the RSTn markers of the entropy-coded segment that starts at `start` lie
static std::vector<size_t> markers_of(const std::vector<uint8_t>& s, size_t start) {
    std::vector<size_t> at;
    for (size_t i = start; i + 1 < s.size();) {
        if (s[i] != 0xFF) { ++i; continue; }
        const int nx = s[i + 1];
        if (nx == 0x00) i += 2;
        else if (nx == 0xFF) i += 1;
        else if (nx >= 0xD0 && nx <= 0xD7) { at.push_back(i); i += 2; }
        else break;
    }
    return at;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s SCRATCH_FILE FILE.jpg ...\n", argv[0]); return 2; }
    const char* scratch = argv[1];
    for (int i = 2; i < argc; ++i) {
        const char* path = argv[i];
        FILE* f = fopen(path, "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
        std::vector<uint8_t> stream;
        uint8_t chunk[4096];
        for (size_t got; (got = fread(chunk, 1, sizeof(chunk), f)) > 0;) stream.insert(stream.end(), chunk, chunk + got);
        fclose(f);
        int w = 0, h = 0, sampling = -1;
        const int probe = ap_host_jpeg_probe(path, &w, &h, &sampling);
        if (probe == AP_ERR_UNSUPPORTED) { fprintf(stderr, "no usable libjpeg: %s\n", g_error); return 3; }
        if (probe != AP_OK || w != h) { fprintf(stderr, "%s: not a square tile of the subset\n", path); return 2; }
        const int side = w;
        char what[600];
        const long before = g_refused, plain = g_plain;
        check_stream(path, stream, side, sampling, scratch, false);
        if (g_refused != before || g_plain != plain) continue;                    // refused as it is, or a restart-free tile
        snprintf(what, sizeof(what), "%s (must pass)", path);
        check_stream(what, stream, side, sampling, scratch, true);
        // where the entropy-coded segment lies
        size_t sos = 0;
        for (size_t k = 0; k + 3 < stream.size(); ++k)
            if (stream[k] == 0xFF && stream[k + 1] == 0xDA) { sos = k; break; }
        const size_t start = sos + 2 + (((size_t)stream[sos + 2] << 8) | stream[sos + 3]), body = stream.size() - 2 - start;
        for (int d = 1; d <= 6; ++d) {                                            // cut at six depths: headers and entropy data
            const size_t keep_file = stream.size() * (size_t)d / 7, keep_body = start + body * (size_t)d / 7;
            for (size_t keep : {keep_file, keep_body}) {
                std::vector<uint8_t> cut(stream.begin(), stream.begin() + (long)keep);
                snprintf(what, sizeof(what), "%s cut at %zu", path, keep);
                check_stream(what, cut, side, sampling, scratch, false);
            }
        }
        for (int k = 0; k < 8 && body > 0; ++k) {                                 // one flipped byte
            std::vector<uint8_t> bad = stream;
            const size_t at = start + (body - 1) * (size_t)k / 7;
            bad[at] ^= k & 1 ? 0xFF : 0x10;
            snprintf(what, sizeof(what), "%s byte %zu flipped", path, at);
            check_stream(what, bad, side, sampling, scratch, false);
        }
        const std::vector<size_t> marks = markers_of(stream, start);              // a marker deleted, duplicated, renumbered
        if (!marks.empty()) {
            const size_t at = marks[marks.size() / 2];
            std::vector<uint8_t> bad = stream;
            bad.erase(bad.begin() + (long)at, bad.begin() + (long)at + 2);
            snprintf(what, sizeof(what), "%s marker at %zu deleted", path, at);
            check_stream(what, bad, side, sampling, scratch, false);
            bad = stream;
            bad.insert(bad.begin() + (long)at, stream.begin() + (long)at, stream.begin() + (long)at + 2);
            snprintf(what, sizeof(what), "%s marker at %zu duplicated", path, at);
            check_stream(what, bad, side, sampling, scratch, false);
            bad = stream;
            bad[at + 1] = (uint8_t)(0xD0 + ((bad[at + 1] - 0xD0 + 3) & 7));
            snprintf(what, sizeof(what), "%s marker at %zu renumbered", path, at);
            check_stream(what, bad, side, sampling, scratch, false);
        }
        // the staged descriptor and table with each restart field outside its bounds
        FILE* o = fopen(scratch, "wb");
        fwrite(stream.data(), 1, stream.size(), o);
        fclose(o);
        size_t bound = 0, used = 0;
        ap_host_jpeg_stream_bound(&scratch, 1, &bound);
        bound += table_bound(side, sampling);
        uint8_t* arena = (uint8_t*)aligned_alloc(16, bound);
        JpegStreamDesc* desc = (JpegStreamDesc*)aligned_alloc(16, sizeof(JpegStreamDesc));
        if (ap_host_jpeg_streams_ex(desc, arena, bound, &used, &scratch, 1, side, sampling, AP_JPEG_STREAM_RESTART) != AP_OK) {
            printf("FAIL %s: %s\n", path, g_error);
            ++g_failures;
            free(desc);
            free(arena);
            continue;
        }
        uint8_t* packed = (uint8_t*)aligned_alloc(16, used);
        memcpy(packed, arena, used);
        const uint32_t n = desc->restart_count;
        {
            JpegStreamDesc d = *desc;
            d.restart_interval = 0;
            snprintf(what, sizeof(what), "%s restart_interval 0 beside a count", path);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false, true);
        }
        for (uint32_t v : {0u, n - 1, n + 1, 2 * n, 1u << 20, 0x7FFFFFFFu, 0xFFFFFFFFu}) {
            JpegStreamDesc d = *desc;
            d.restart_count = v;
            snprintf(what, sizeof(what), "%s restart_count %u", path, v);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false, true);
        }
        for (uint32_t v : {0x7FFFFFFFu, 0xFFFFFFFFu}) {
            JpegStreamDesc d = *desc;
            d.restart_interval = v;
            snprintf(what, sizeof(what), "%s restart_interval %u", path, v);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false, true);
        }
        // an interval at or above the frame's MCU count beside the count that fits it, 1: the stager stages such a tile restart free, so
        // the decoder refuses it -- above 2^31 the interval would otherwise turn negative as an int and the block count wrap
        const uint32_t mcus = mcu_count(side, sampling);
        for (uint32_t v : {mcus, mcus + 1, 2 * mcus, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xAAAAAB00u, 0xFFFFFFFFu}) {
            JpegStreamDesc d = *desc;
            d.restart_interval = v;
            d.restart_count = 1;
            snprintf(what, sizeof(what), "%s restart_interval %u beside count 1", path, v);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false, true);
        }
        for (uint64_t v : {(uint64_t)used, (uint64_t)used + 16, desc->restart_table_offset + 16 * ((4 * (uint64_t)n + 15) / 16), desc->restart_table_offset + 8,
                           (uint64_t)1 << 40, ~(uint64_t)0, ~(uint64_t)15}) {
            if (v == desc->restart_table_offset) continue;
            JpegStreamDesc d = *desc;
            d.restart_table_offset = v;
            snprintf(what, sizeof(what), "%s restart_table_offset %llu", path, (unsigned long long)v);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false, true);
        }
        uint32_t* table = (uint32_t*)(packed + desc->restart_table_offset);       // little-endian host
        const uint32_t mid = n / 2;
        struct Edit { const char* name; uint32_t at, value; };
        const Edit edits[] = {{"entry 0 = 1", 0, 1},
                              {"an entry equal to its predecessor", mid, table[mid ? mid - 1 : 0]},
                              {"the last entry = payload_bytes", n - 1, desc->payload_bytes},
                              {"an entry = payload_bytes", mid, desc->payload_bytes},
                              {"an entry = 2^32 - 1", mid, 0xFFFFFFFFu},
                              {"the last entry = 2^32 - 1", n - 1, 0xFFFFFFFFu}};
        for (const Edit& e : edits) {
            if (e.at == 0 && e.value == 0) continue;
            const uint32_t keep = table[e.at];
            table[e.at] = e.value;
            snprintf(what, sizeof(what), "%s table: %s", path, e.name);
            decode_both(what, desc, packed, used, side, sampling, nullptr, false, true);
            table[e.at] = keep;
        }
        if (n >= 3) {                                                             // two entries swapped: a decreasing pair
            const uint32_t a = table[mid], b = table[mid + 1 < n ? mid + 1 : mid - 1];
            table[mid] = b;
            table[mid + 1 < n ? mid + 1 : mid - 1] = a;
            snprintf(what, sizeof(what), "%s table: two entries swapped", path);
            decode_both(what, desc, packed, used, side, sampling, nullptr, false, true);
        }
        free(packed);
        free(desc);
        free(arena);
    }
    printf("%d files: %ld decodes, %ld flagged, %ld refused by the stager, %ld equal to libjpeg's slot, %ld staged restart free, "
           "%ld with status 0 where libjpeg warns, %d failures\n",
           argc - 2, g_runs, g_flagged, g_refused, g_equal, g_plain, g_unjudged, g_failures);
    return g_failures ? 1 : 0;
}
