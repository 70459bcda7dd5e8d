// Stand-alone driver of the JPEG coefficient reader (atlaspatch_amd/csrc/jpeg_host.cpp) for sanitizer runs of the HOST code:
// untrusted files reach libjpeg's header parser, its entropy decoder and the slot copy.  CPU only, no device work.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -x hip tools/jpeg_reader_check.cpp atlaspatch_amd/csrc/jpeg_host.cpp -ldl -o jpeg_reader_check
//   ./jpeg_reader_check FILE.jpg ...
//
// Every file is probed, read at the side and sampling its header states into a slot with a red zone of its own (an exact-size
// heap block, so a write past the slot is a heap-buffer-overflow), read again at every other sampling and at a wrong side
// (refusals), and decoded to pixels through ap_host_decode_jpeg_tiles.  Prints one line per file; exits 0 unless an argument is wrong.
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
    if (argc < 2) { fprintf(stderr, "usage: %s FILE.jpg ...\n", argv[0]); return 2; }
    int delivered = 0, refused = 0;
    for (int i = 1; i < argc; ++i) {
        const char* path = argv[i];
        int w = 0, h = 0, sampling = -1;
        const int probe = ap_host_jpeg_probe(path, &w, &h, &sampling);
        if (probe == AP_ERR_UNSUPPORTED) { fprintf(stderr, "no usable libjpeg: %s\n", ap::g_error); return 3; }
        printf("%s: probe %d", path, probe);
        if (probe == AP_OK) printf(" (%d x %d, sampling %d)", w, h, sampling);
        // a header the probe refuses is still offered to the reader at every sampling: it must refuse too
        const int side = probe == AP_OK ? w : 16;
        for (int s = 0; s < 4; ++s)
            for (int sd : {side, side + 8}) {
                const size_t bytes = ap_jpeg_slot_bytes(sd, s);
                unsigned char* slot = (unsigned char*)malloc(bytes);
                memset(slot, 0xA5, bytes);
                const int rc = ap_host_jpeg_coefficients(slot, &path, 1, sd, s);
                if (rc == AP_OK) {
                    ++delivered;
                    printf(" | slot %d/%d ok", sd, s);
                } else {
                    ++refused;
                    for (size_t k = 0; k < bytes; ++k)
                        if (slot[k] != 0xA5) { printf(" | REFUSED SLOT WRITTEN"); break; }
                }
                free(slot);
            }
        if (w > 0 && w == h && w <= 4096) {
            std::vector<unsigned char> rgb((size_t)w * w * 3);
            printf(" | pixels %d", ap_host_decode_jpeg_tiles(rgb.data(), &path, 1, w));
        }
        printf("\n");
    }
    printf("%d slots delivered, %d refusals\n", delivered, refused);
    return 0;
}
