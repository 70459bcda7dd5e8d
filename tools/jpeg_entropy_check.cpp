// Stand-alone driver of the stream route's host parser (atlaspatch_amd/csrc/jpeg_stream_host.cpp) and of the device decoder's core
// (atlaspatch_amd/csrc/jpeg_entropy_core.h) for sanitizer runs on the CPU: the passes ap_jpeg_entropy_decode_tiles runs on a
// workgroup are run here with the 256 lanes in a loop, a pass at a time, so every payload read, table index and slot write the kernel
// would make is made here first, under AddressSanitizer / UBSan, on exact-size heap blocks.  No GPU, no Python, no preload.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip tools/jpeg_entropy_check.cpp atlaspatch_amd/csrc/jpeg_stream_host.cpp atlaspatch_amd/csrc/jpeg_host.cpp -ldl \
//         -o jpeg_entropy_check
//   ./jpeg_entropy_check SCRATCH_FILE FILE.jpg ...      (SCRATCH_FILE: where the damaged variants are written for the file readers)
//
// Per file, at subsequence_bits 32 and at the default: the file as it is (where libjpeg reads it without a warning its slot must
// equal ap_host_jpeg_coefficients' outside the padding, status 0); cut at six depths; one byte flipped at eight places of the
// entropy-coded segment; the staged descriptor with each of its fields (payload length and offset, component count, selectors, code counts) set to values outside its bounds.  A damaged
// input must end flagged, refused, or -- where libjpeg reads the same bytes without a warning -- with libjpeg's slot; both subsequence
// lengths must agree on status, and on the slot when the status is 0.  Exits 1 on any disagreement, 0 otherwise.
// Every file is also asked for under each of the other sampling codes, AP_JPEG_RGB included (a YCbCr file as RGB and an RGB-coded file
// -- Adobe transform 0, or ids 'R' 'G' 'B' -- as 4:4:4 must be refused); an RGB-coded file is staged and decoded at AP_JPEG_RGB.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/atlaspatch_hip.h"
#include "../atlaspatch_amd/csrc/jpeg_entropy_core.h"

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
static long g_runs = 0, g_flagged = 0, g_refused = 0, g_equal = 0;

// the kernel's body (jpeg_entropy.hip), barriers replaced by the end of a loop over the lanes
static int32_t run_tile(const JpegStreamDesc* desc, const uint8_t* arena, size_t arena_bytes, uint8_t* slot, int side, int sampling, int ssb) {
    EntropyShared* sh = (EntropyShared*)malloc(sizeof(EntropyShared));
    memset(sh, 0xA5, sizeof(EntropyShared));
    EntropyTile T;
    entropy_tile(desc, arena, arena_bytes, slot, side, sampling, ssb, &T);
    const int nl = kEntropyLanes;
    const size_t words = arena_bytes / 4 + 1;
    const int max_rounds = (int)(words < (size_t)kEntropyMaxSubseq ? words : (size_t)kEntropyMaxSubseq);
    entropy_pass0_clear(sh);
    for (int l = 0; l < nl; ++l) { entropy_pass0_tables(T, sh, l); entropy_pass0_slot(T, l, nl); }
    for (int l = 0; l < nl; ++l) entropy_pass1(T, sh, l, nl);
    const int rounds = T.S < max_rounds ? T.S : max_rounds;
    std::vector<uint32_t> mask(nl);
    for (int r = 0; r < rounds; ++r) {
        bool any = false;
        for (int l = 0; l < nl; ++l) { mask[l] = entropy_pass2_read(T, sh, l, nl); any = any || mask[l]; }
        if (!any) break;
        for (int l = 0; l < nl; ++l) entropy_pass2_decode(T, sh, l, nl, mask[l]);
    }
    for (int l = 0; l < nl; ++l) entropy_pass3_sum(T, sh, l, nl);
    for (int l = nl - 1; l >= 0; --l) entropy_pass3_scan(T, sh, l, nl);
    for (int l = 0; l < nl; ++l) entropy_pass3_write(T, sh, l, nl);
    for (int l = 0; l < nl; ++l) entropy_pass4_sum(T, sh, l, nl);
    for (int l = nl - 1; l >= 0; --l) entropy_pass4_scan(T, sh, l, nl);
    const int32_t status = entropy_pass5_status(T, sh);
    free(sh);
    return status;
}

static bool same_slot(const uint8_t* a, const uint8_t* b, size_t bytes) {
    return !memcmp(a, b, 384) && !memcmp(a + 512, b + 512, bytes - 512);
}

// one staged tile through both subsequence lengths; `want`: libjpeg's slot for the same bytes, or null
static void decode_both(const char* what, const JpegStreamDesc* desc, const uint8_t* arena, size_t arena_bytes, int side, int sampling,
                        const uint8_t* want, bool must_pass) {
    const size_t bytes = ap_jpeg_slot_bytes_ex(side, sampling);
    uint8_t* s32 = (uint8_t*)malloc(bytes);
    uint8_t* sdef = (uint8_t*)malloc(bytes);
    memset(s32, 0x5A, bytes);
    memset(sdef, 0x5A, bytes);
    const int32_t a = run_tile(desc, arena, arena_bytes, s32, side, sampling, 32);
    const int32_t b = run_tile(desc, arena, arena_bytes, sdef, side, sampling, kEntropyDefaultBits);
    g_runs += 2;
    if (a != b || (a == 0 && !same_slot(s32, sdef, bytes))) {
        printf("FAIL %s: subsequence_bits 32 gives status %d, the default %d%s\n", what, a, b, a == b ? ", other slots" : "");
        ++g_failures;
    }
    if (a == 0 && want && !same_slot(s32, want, bytes)) {
        printf("FAIL %s: status 0 and another slot than libjpeg's\n", what);
        ++g_failures;
    }
    if (a == 0 && want) ++g_equal;
    if (a != 0) ++g_flagged;
    if (must_pass && want && a != 0) {                      // a file libjpeg itself refuses (a damaged one among the arguments) need not pass
        printf("FAIL %s: a stream libjpeg reads without a warning ends with status %d\n", what, a);
        ++g_failures;
    }
    free(s32);
    free(sdef);
}

// a stream in memory: written to a scratch file for the two file readers, staged, decoded
static void check_stream(const char* what, const std::vector<uint8_t>& stream, int side, int sampling, const char* scratch, bool must_pass) {
    FILE* f = fopen(scratch, "wb");
    if (!f || fwrite(stream.data(), 1, stream.size(), f) != stream.size()) { fprintf(stderr, "cannot write %s\n", scratch); exit(3); }
    fclose(f);
    const size_t bytes = ap_jpeg_slot_bytes_ex(side, sampling);
    uint8_t* want = (uint8_t*)malloc(bytes);
    const bool libjpeg_ok = ap_host_jpeg_coefficients(want, &scratch, 1, side, sampling) == AP_OK;
    size_t bound = 0;
    if (ap_host_jpeg_stream_bound(&scratch, 1, &bound) != AP_OK) { fprintf(stderr, "%s\n", g_error); exit(3); }
    // exact-size blocks: a byte past the arena or the descriptor is a heap-buffer-overflow
    uint8_t* arena = (uint8_t*)aligned_alloc(16, bound);
    JpegStreamDesc* desc = (JpegStreamDesc*)aligned_alloc(16, sizeof(JpegStreamDesc));
    size_t used = 0;
    const int rc = ap_host_jpeg_streams(desc, arena, bound, &used, &scratch, 1, side, sampling);
    if (rc != AP_OK) {
        ++g_refused;
        if (must_pass) { printf("FAIL %s: refused: %s\n", what, g_error); ++g_failures; }
    } else {
        // the decoder is handed exactly the bytes that hold payloads
        uint8_t* packed = (uint8_t*)aligned_alloc(16, used ? used : 16);
        memcpy(packed, arena, used);
        decode_both(what, desc, packed, used, side, sampling, libjpeg_ok ? want : nullptr, must_pass);
        free(packed);
    }
    // one byte less than the file needs: refused, nothing written past the arena
    if (bound >= 32) {
        size_t used2 = 0;
        void* small = nullptr;
        if (posix_memalign(&small, 16, stream.size() - 1)) exit(3);
        if (ap_host_jpeg_streams(desc, small, stream.size() - 1, &used2, &scratch, 1, side, sampling) == AP_OK) {
            printf("FAIL %s: an arena one byte short of the file was accepted\n", what);
            ++g_failures;
        }
        free(small);
    }
    free(desc);
    free(arena);
    free(want);
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
        char what[600];
        if (probe != AP_OK || w != h) {
            // outside the subset already at its header: every sampling must refuse it
            for (int s = 0; s <= AP_JPEG_RGB; ++s) { snprintf(what, sizeof(what), "%s as sampling %d", path, s); check_stream(what, stream, 16, s, scratch, false); }
            continue;
        }
        const int side = w;
        JpegGeom g;
        jpeg_geom(side, sampling, &g);
        const bool in_subset = side % (8 * g.hmax) == 0 && side % (8 * g.vmax) == 0 && side <= kJpegDeviceMaxSide;
        // the file as it is; a restart-marker or progressive file is refused by the stager, which check_stream counts
        const size_t before = (size_t)g_refused;
        check_stream(path, stream, side, sampling, scratch, false);
        const bool staged = (size_t)g_refused == before;
        if (staged && !in_subset) { printf("FAIL %s: staged although its side is no multiple of the MCU size\n", path); ++g_failures; }
        for (int s = 0; s <= AP_JPEG_RGB; ++s)
            if (s != sampling) { snprintf(what, sizeof(what), "%s as sampling %d", path, s); check_stream(what, stream, side, s, scratch, false); }
        if (!staged) continue;
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
        // the staged descriptor with each field outside its bounds
        FILE* o = fopen(scratch, "wb");
        fwrite(stream.data(), 1, stream.size(), o);
        fclose(o);
        size_t bound = 0, used = 0;
        ap_host_jpeg_stream_bound(&scratch, 1, &bound);
        uint8_t* arena = (uint8_t*)aligned_alloc(16, bound);
        JpegStreamDesc* desc = (JpegStreamDesc*)aligned_alloc(16, sizeof(JpegStreamDesc));
        if (ap_host_jpeg_streams(desc, arena, bound, &used, &scratch, 1, side, sampling) != AP_OK) { printf("FAIL %s: %s\n", path, g_error); ++g_failures; continue; }
        uint8_t* packed = (uint8_t*)aligned_alloc(16, used ? used : 16);
        memcpy(packed, arena, used);
        const uint32_t n = desc->payload_bytes;
        for (uint32_t v : {0u, 1u, n - 1, n + 1, n + 16, n + 17, (uint32_t)used + 1, 1u << 20, 0x7FFFFFFFu, 0xFFFFFFFFu}) {
            JpegStreamDesc d = *desc;
            d.payload_bytes = v;
            snprintf(what, sizeof(what), "%s payload_bytes %u", path, v);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false);
        }
        for (uint64_t v : {(uint64_t)1, (uint64_t)8, (uint64_t)16, (uint64_t)used, (uint64_t)used + 16, (uint64_t)1 << 40, ~(uint64_t)0, ~(uint64_t)15}) {
            JpegStreamDesc d = *desc;
            d.payload_offset = v;
            snprintf(what, sizeof(what), "%s payload_offset %llu", path, (unsigned long long)v);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false);
        }
        for (uint32_t v : {0u, 2u, 4u, 255u, 0xFFFFFFFFu, desc->ncomp == 1 ? 3u : 1u}) {
            JpegStreamDesc d = *desc;
            d.ncomp = v;
            snprintf(what, sizeof(what), "%s ncomp %u", path, v);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false);
        }
        for (int t = 0; t < 4; ++t) {
            JpegStreamDesc d = *desc;
            memset(d.huff_counts[t], 255, 16);
            snprintf(what, sizeof(what), "%s table %d with 255 codes of every length", path, t);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false);
            d = *desc;
            memset(d.huff_counts[t], 0, 16);
            snprintf(what, sizeof(what), "%s table %d empty", path, t);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false);
            d = *desc;
            memset(d.huff_symbols[t], 0xFF, 256);
            snprintf(what, sizeof(what), "%s table %d with symbols FF", path, t);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false);
        }
        for (int c = 0; c < 3; ++c) {
            JpegStreamDesc d = *desc;
            d.dc_sel[c] = 7;
            d.ac_sel[c] = 255;
            snprintf(what, sizeof(what), "%s selectors of component %d", path, c);
            decode_both(what, &d, packed, used, side, sampling, nullptr, false);
        }
        free(packed);
        free(desc);
        free(arena);
    }
    printf("%d files: %ld decodes, %ld flagged, %ld refused by the stager, %ld equal to libjpeg's slot, %d failures\n", argc - 2, g_runs,
           g_flagged, g_refused, g_equal, g_failures);
    return g_failures ? 1 : 0;
}
