// K0, device half of the stream route: a JPEG tile's Huffman decode on the device (include/atlaspatch_hip.h:
// ap_jpeg_entropy_decode_tiles).  Descriptor + unstuffed payload (jpeg_stream.h) in, the coefficient slot of jpeg_slot.h out, so that
// ap_jpeg_decode_tiles and ap_gather_patches run unchanged behind it.
//
// One workgroup of 256 lanes decodes one tile with the self-synchronising scheme that jpeg_entropy_core.h states and implements; this
// file is the barriers between that header's passes.  Nothing waits on another workgroup: no global atomics, no spinning, no grid
// synchronisation.  The only loop whose length depends on the data is the synchronisation loop; it ends when a round changes nothing
// and in any case after S <= max_rounds rounds, a number the host computes from the arena size.
//
// The bit string is read from global memory (two cached 32-bit words per lane, one new word per 32 bits consumed; the payload of a
// tile is 8 - 44 KB and stays in L2); the decode tables, the per-subsequence states and the scans live in LDS (54.6 KB per
// workgroup, two workgroups per CU).  Measured: on noise-rich 4:2:0 tiles a subsequence of the default length
// holds less than one MCU, the block-in-MCU phase of a guessed state does not re-synchronise, and the loop runs about S rounds: the
// kernel is then as slow as one sequential pass per tile.  The fixes named there are not built.
//
// ap_jpeg_entropy_decode_tiles_rst takes launches that mix such tiles with tiles that carry restart intervals (jpeg_stream.h:
// restart_interval != 0), which are decoded an interval per lane by the passes of jpeg_restart_core.h in a kernel of their own: its LDS
// is the four tables and a few words (under 4 KB), so it keeps an occupancy the 54.6 KB of the kernel above cannot.  The device cannot
// tell the host which kind a tile is without a copy, so both kernels are launched over the n tiles and a workgroup whose tile is
// not of its kind returns on a uniform branch after reading the descriptor's restart fields.  For the other entries the first kernel is instantiated
// without that branch: it is the kernel they always ran.
#include "ap_common.h"
#include "jpeg_entropy_core.h"
#include "jpeg_restart_core.h"

namespace ap {
namespace {

struct EntropyArgs {
    const JpegStreamDesc* descs;
    const uint8_t* arena;
    size_t arena_bytes;
    uint8_t* slots;
    int32_t* status;
    size_t slot_bytes;
    int side, sampling, subsequence_bits, max_rounds;
};

// kMixed: the launch may hold restart tiles, which are jpeg_restart_kernel's
template <bool kMixed>
__global__ __launch_bounds__(kEntropyLanes) void jpeg_entropy_kernel(EntropyArgs a) {
    __shared__ EntropyShared sh;
    const int lane = (int)threadIdx.x, nl = kEntropyLanes, tile = (int)blockIdx.x;
    if (kMixed && restart_fields_set(a.descs + tile)) return;
    EntropyTile T;
    entropy_tile(a.descs + tile, a.arena, a.arena_bytes, a.slots + (size_t)tile * a.slot_bytes, a.side, a.sampling, a.subsequence_bits, &T);
    if (lane == 0) entropy_pass0_clear(&sh);
    __syncthreads();
    entropy_pass0_tables(T, &sh, lane);
    entropy_pass0_slot(T, lane, nl);
    __syncthreads();
    entropy_pass1(T, &sh, lane, nl);
    __syncthreads();
    const int rounds = T.S < a.max_rounds ? T.S : a.max_rounds;
    for (int r = 0; r < rounds; ++r) {
        const uint32_t mask = entropy_pass2_read(T, &sh, lane, nl);
        if (!__syncthreads_or(mask != 0)) break;
        entropy_pass2_decode(T, &sh, lane, nl, mask);
        __syncthreads();
    }
    entropy_pass3_sum(T, &sh, lane, nl);
    __syncthreads();
    entropy_pass3_scan(T, &sh, lane, nl);
    __syncthreads();
    entropy_pass3_write(T, &sh, lane, nl);
    __syncthreads();
    entropy_pass4_sum(T, &sh, lane, nl);
    __syncthreads();
    entropy_pass4_scan(T, &sh, lane, nl);
    if (lane == 0) a.status[tile] = entropy_pass5_status(T, &sh);
}

__global__ __launch_bounds__(kEntropyLanes) void jpeg_restart_kernel(EntropyArgs a) {
    __shared__ RestartShared sh;
    const int lane = (int)threadIdx.x, nl = kEntropyLanes, tile = (int)blockIdx.x;
    if (!restart_fields_set(a.descs + tile)) return;
    RestartTile R;
    restart_tile(a.descs + tile, a.arena, a.arena_bytes, a.slots + (size_t)tile * a.slot_bytes, a.side, a.sampling, &R);
    if (lane == 0) restart_pass0_clear(&sh);
    __syncthreads();
    restart_pass0_tables(R, &sh, lane);
    entropy_pass0_slot(R.T, lane, nl);
    __syncthreads();
    restart_pass_decode(R, &sh, lane, nl);
    __syncthreads();
    if (lane == 0) a.status[tile] = restart_pass_status(R, &sh);
}

// the argument checks and the launch of every entry; `mixed`: restart tiles are decoded by their own kernel
int entropy_launch(const void* descs, const void* arena, size_t arena_bytes, int n, int side, int sampling, void* slots, int32_t* status,
                   int subsequence_bits, ap_stream_t stream, bool mixed) {
    AP_REQUIRE(descs && arena && slots && status, "ap_jpeg_entropy_decode_tiles: null pointer");
    AP_REQUIRE(n >= 0, "ap_jpeg_entropy_decode_tiles: bad n %d", n);
    AP_REQUIRE((((uintptr_t)descs | (uintptr_t)arena | (uintptr_t)slots) & 15) == 0,
               "ap_jpeg_entropy_decode_tiles: descs, arena and slots must be 16-byte aligned");
    JpegGeom g;
    AP_REQUIRE(jpeg_geom(side, sampling, &g), "ap_jpeg_entropy_decode_tiles: bad side %d or sampling %d", side, sampling);
    AP_REQUIRE(side <= kJpegDeviceMaxSide && side % (8 * g.hmax) == 0 && side % (8 * g.vmax) == 0,
               "ap_jpeg_entropy_decode_tiles: side %d is above %d or no multiple of the MCU size", side, kJpegDeviceMaxSide);
    if (subsequence_bits == 0) subsequence_bits = kEntropyDefaultBits;
    AP_REQUIRE(subsequence_bits >= 32 && subsequence_bits % 32 == 0 && subsequence_bits <= (1 << 20),
               "ap_jpeg_entropy_decode_tiles: subsequence_bits %d is no multiple of 32 in [32, 2^20]", subsequence_bits);
    if (n == 0) return AP_OK;
    EntropyArgs a;
    a.descs = (const JpegStreamDesc*)descs;
    a.arena = (const uint8_t*)arena;
    a.arena_bytes = arena_bytes;
    a.slots = (uint8_t*)slots;
    a.status = status;
    a.slot_bytes = g.bytes;
    a.side = side;
    a.sampling = sampling;
    a.subsequence_bits = subsequence_bits;
    // no tile has more subsequences than its payload has words, nor than the state arrays hold: the bound of the synchronisation loop
    const size_t words = arena_bytes / 4 + 1;
    a.max_rounds = (int)(words < (size_t)kEntropyMaxSubseq ? words : (size_t)kEntropyMaxSubseq);
    if (!mixed) {
        hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)n), dim3(kEntropyLanes), 0, (hipStream_t)stream, a);
        AP_HIP_CHECK(hipGetLastError());
        return AP_OK;
    }
    hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)n), dim3(kEntropyLanes), 0, (hipStream_t)stream, a);
    AP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_restart_kernel, dim3((unsigned)n), dim3(kEntropyLanes), 0, (hipStream_t)stream, a);
    AP_HIP_CHECK(hipGetLastError());
    return AP_OK;
}

}  // namespace
}  // namespace ap

extern "C" int ap_jpeg_entropy_decode_tiles_ex(const void* descs, const void* arena, size_t arena_bytes, int n, int side, int sampling,
                                               void* slots, int32_t* status, int subsequence_bits, ap_stream_t stream) {
    return ap::entropy_launch(descs, arena, arena_bytes, n, side, sampling, slots, status, subsequence_bits, stream, false);
}

extern "C" int ap_jpeg_entropy_decode_tiles_rst(const void* descs, const void* arena, size_t arena_bytes, int n, int side, int sampling,
                                                void* slots, int32_t* status, int subsequence_bits, ap_stream_t stream) {
    return ap::entropy_launch(descs, arena, arena_bytes, n, side, sampling, slots, status, subsequence_bits, stream, true);
}

// the four codes this entry was published with; AP_JPEG_RGB stays an unknown sampling here
extern "C" int ap_jpeg_entropy_decode_tiles(const void* descs, const void* arena, size_t arena_bytes, int n, int side, int sampling,
                                            void* slots, int32_t* status, int subsequence_bits, ap_stream_t stream) {
    AP_REQUIRE(sampling != AP_JPEG_RGB, "ap_jpeg_entropy_decode_tiles: bad side %d or sampling %d (AP_JPEG_RGB: ap_jpeg_entropy_decode_tiles_ex)", side, sampling);
    return ap_jpeg_entropy_decode_tiles_ex(descs, arena, arena_bytes, n, side, sampling, slots, status, subsequence_bits, stream);
}
