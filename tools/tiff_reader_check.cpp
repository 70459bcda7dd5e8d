// Stand-alone driver of the TIFF reader (atlaspatch_amd/csrc/tiff_host.cpp, with jpeg_host.cpp behind it) for sanitizer runs of the
// HOST code: untrusted files reach the IFD parser, the tile tables, libjpeg's header parser and entropy decoder, the patch
// copy and the slot copy.  CPU only, no device work.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip tools/tiff_reader_check.cpp atlaspatch_amd/csrc/tiff_host.cpp atlaspatch_amd/csrc/jpeg_host.cpp \
//         atlaspatch_amd/csrc/jpeg_stream_host.cpp -ldl -o tiff_reader_check
//   ./tiff_reader_check FILE.tif ...
//
// Every file is opened; an accepted file has, per level, its corner patches (overhanging all four corners, and one in the
// middle) read into exact-size heap blocks, and -- where the level has a sampling -- its first, last and middle tiles read as
// coefficient slots, each into an exact-size block.  Prints one line per file; exits 0 unless an argument is wrong.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/atlaspatch_hip.h"

namespace ap {
static thread_local char g_error[512];
void set_error(const char* fmt, ...) {
    va_list va;
    va_start(va, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, va);
    va_end(va);
}
}  // namespace ap

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s FILE.tif ...\n", argv[0]); return 2; }
    int accepted = 0, refused = 0, patches_ok = 0, patches_failed = 0, slots_ok = 0, slots_failed = 0;
    for (int i = 1; i < argc; ++i) {
        ap_tiff* t = nullptr;
        const int rc = ap_host_tiff_open(argv[i], &t);
        if (rc != AP_OK) {
            ++refused;
            printf("%s: refused (%d): %s\n", argv[i], rc, ap::g_error);
            if (t) { printf("REFUSED WITH A HANDLE\n"); return 1; }
            continue;
        }
        ++accepted;
        int levels = 0, unit = 0;
        double res[2];
        size_t desc_bytes = 0;
        ap_host_tiff_info(t, &levels, res, &unit, nullptr, 0, &desc_bytes);
        char* desc = (char*)malloc(desc_bytes / 2 + 1);                   // a truncating read into an exact-size block
        ap_host_tiff_info(t, &levels, res, &unit, desc, desc_bytes / 2 + 1, &desc_bytes);
        free(desc);
        printf("%s: %d levels", argv[i], levels);
        for (int lv = 0; lv < levels; ++lv) {
            int64_t g[8];
            ap_host_tiff_level(t, lv, g);
            const int64_t tiles = g[4] * g[5];
            unsigned char* present = (unsigned char*)malloc((size_t)tiles);
            ap_host_tiff_tile_present(t, lv, present);
            free(present);
            const int side = 96;
            const int64_t xy[5][2] = {{-40, -40}, {g[0] - 50, -10}, {-10, g[1] - 50}, {g[0] - 50, g[1] - 50}, {g[0] / 2 - 7, g[1] / 2 - 3}};
            unsigned char* px = (unsigned char*)malloc((size_t)5 * side * side * 3);
            (ap_host_tiff_read_patches(t, lv, &xy[0][0], 5, side, side, px) == AP_OK ? patches_ok : patches_failed)++;
            free(px);
            if (g[6] >= 0) {
                const size_t bytes = ap_jpeg_slot_bytes_ex((int)g[2], (int)g[6]);
                const int32_t ids[3] = {0, (int32_t)(tiles - 1), (int32_t)(tiles / 2)};
                for (int k = 0; k < 3; ++k) {
                    unsigned char* slot = (unsigned char*)malloc(bytes);
                    (ap_host_tiff_tile_coefficients(t, lv, &ids[k], 1, slot) == AP_OK ? slots_ok : slots_failed)++;
                    free(slot);
                }
            }
            printf(" | %lld x %lld, tiles %lld x %lld, sampling %lld", (long long)g[0], (long long)g[1], (long long)g[2], (long long)g[3], (long long)g[6]);
        }
        printf("\n");
        ap_host_tiff_close(t);
    }
    printf("%d accepted, %d refused; patch reads %d ok / %d failed; slots %d ok / %d failed\n", accepted, refused, patches_ok, patches_failed,
           slots_ok, slots_failed);
    return 0;
}
