// The decode core of ap_jpeg_entropy_decode_tiles_rst for a tile WITH restart intervals (jpeg_stream.h: restart_interval != 0), written
// the way jpeg_entropy_core.h is: __host__ __device__ functions for "lane `lane` of `nl`".  The kernel (jpeg_entropy.hip) runs a pass on
// every thread of a workgroup with a barrier behind it; tools/jpeg_restart_check.cpp runs the same functions with the lanes in a loop,
// under AddressSanitizer / UBSan, before any input reaches a GPU.
//
// A restart stream is parallel by construction: interval k starts byte aligned at payload byte table[k], at block 0 of MCU
// k * restart_interval, with the DC predictors at zero.  So there is no guessed state, there are no rounds and there is no DC prefix
// sum; what jpeg_entropy_core.h needs its passes 1 .. 4 for is one pass here:
//   pass 0  as there: the four tables into shared memory, the slot zeroed and the quantisers copied in 16-byte stores
//   pass R  lane l decodes the intervals l, l + nl, ...: the bit reader is opened on the payload with the interval's end as its
//           length (bytes at and behind it read as zero), min(restart_interval, MCUs - k * restart_interval) MCUs are decoded, every
//           coefficient goes to natural[z] of its block and the DC as the accumulated value itself
//   status  the first error in interval order (the minimum of interval << 4 | status), so it does not depend on the lanes' timing
// Every loop is bounded by the interval's block count times 64 symbols (a symbol that is no error moves the zig-zag index on or ends
// the block) and by its bits.  Nothing waits on another lane.
// Memory safety on any input: a table entry is read only below the checked count, from a table that lies inside the arena; a payload
// word is read only below the interval's checked end; a slot address is built from a block index below the frame's count.
#pragma once
#include "jpeg_entropy_core.h"

namespace ap {

struct RestartShared {                      // what one tile's lanes share: LDS on the device, under 4 KB
    HuffTable tab[4];
    uint32_t error;                         // min over the intervals of (interval << 4 | status)
    uint32_t table_error;
    uint8_t natural[64];
};

struct RestartTile {                        // one tile's job, the same on every lane
    EntropyTile T;                          // geometry, selectors, payload: the descriptor checks of entropy_tile as they are
    const uint8_t* table;                   // restart_count little-endian uint32, 16-byte aligned, inside the arena
    uint32_t interval, count;               // MCUs per interval, intervals; count == 0 when the descriptor is refused
    int mcus;
};

// ---- the tile's job from its descriptor: entropy_tile's checks, then the restart fields against the frame and the arena
AP_HD void restart_tile(const JpegStreamDesc* desc, const uint8_t* arena, size_t arena_bytes, uint8_t* slot, int side, int sampling,
                        RestartTile* R) {
    entropy_tile(desc, arena, arena_bytes, slot, side, sampling, kEntropyDefaultBits, &R->T);
    const uint32_t interval = desc->restart_interval, count = desc->restart_count;
    const uint64_t offset = desc->restart_table_offset;
    R->mcus = R->T.total_blocks / R->T.bpm;
    // an interval that covers the frame is staged restart free, so 0 < interval < MCUs <= (976 / 8)^2 here, and with it count <= MCUs:
    // from here on interval, count and every product of one of them with the MCU's block count fit an int
    bool bad = R->T.bad || interval == 0 || count == 0 || (uint64_t)interval >= (uint64_t)R->mcus ||
               (uint64_t)count != ((uint64_t)R->mcus + interval - 1) / interval;
    bad = bad || (offset & 15) || offset > arena_bytes || (((uint64_t)count * 4 + 15) & ~(uint64_t)15) > arena_bytes - offset;
    R->T.bad = bad;
    R->interval = bad ? 0 : interval;
    R->count = bad ? 0 : count;
    R->table = arena + (bad ? 0 : offset);
}

// which of ap_jpeg_entropy_decode_tiles_rst's two kernels a tile is for: a restart-free descriptor has all three fields zero, and one
// with an interval of 0 beside a count or a table offset is this path's to flag
AP_HD bool restart_fields_set(const JpegStreamDesc* desc) {
    return desc->restart_interval != 0 || desc->restart_count != 0 || desc->restart_table_offset != 0;
}

AP_HD uint32_t restart_entry(const RestartTile& R, uint32_t k) {                           // k < R.count
    const uint8_t* e = R.table + 4 * (size_t)k;
    return (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
}

AP_HD void restart_record(RestartShared* sh, uint32_t k, int status) {
    const uint32_t v = (k << 4) | (uint32_t)status;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(&sh->error, v);
#else
    if (v < sh->error) sh->error = v;
#endif
}

// ================================================================== the passes, for lane `lane` of `nl`
// before pass 0, by one lane
AP_HD void restart_pass0_clear(RestartShared* sh) { sh->table_error = 0; }
// pass 0: lanes 0 .. 3 build the four tables, lane 4 the natural-order map and the error word; the slot is entropy_pass0_slot's
AP_HD void restart_pass0_tables(const RestartTile& R, RestartShared* sh, int lane) {
    const EntropyTile& T = R.T;
    if (lane < 4) {
        bool used = false;
        for (int c = 0; c < T.ncomp; ++c) used = used || (lane < 2 ? T.dc[c] == lane : T.ac[c] == lane - 2);
        const bool good = entropy_build_table(T.desc->huff_counts[lane], T.desc->huff_symbols[lane], &sh->tab[lane]);
        if (used && !good) sh->table_error = 1;           // lanes that write all write 1
    } else if (lane == 4) {
        constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
        for (int k = 0; k < 64; ++k) sh->natural[k] = zz[k];
        sh->error = kEntropyNoError;
    }
}

// ---- interval k, whole: its table entries checked, its MCUs decoded into the slot, its first error recorded
AP_HD void restart_decode_interval(const RestartTile& R, RestartShared* sh, uint32_t k) {
    const EntropyTile& T = R.T;
    const uint32_t lo = restart_entry(R, k), hi = k + 1 < R.count ? restart_entry(R, k + 1) : T.nbytes;
    // entry 0 is 0; an entry lies strictly above its predecessor and below payload_bytes (the last interval ends at payload_bytes)
    if ((k == 0 && lo != 0) || lo >= hi || hi > T.nbytes || (k + 1 < R.count && hi >= T.nbytes)) {
        restart_record(sh, k, kEntropyBadDescriptor);
        return;
    }
    const uint32_t first = k * R.interval, left = (uint32_t)R.mcus - first;           // k < count, so first < MCUs
    const int m0 = (int)first, nm = (int)(left < R.interval ? left : R.interval);
    const int nblocks = nm * T.bpm, hv = T.hmax * T.vmax;
    const uint32_t end = hi * 8;
    uint32_t p = lo * 8;
    int blk = m0 * T.bpm, b = 0, z = 0, comp = 0, done_blocks = 0;
    int dc0 = 0, dc1 = 0, dc2 = 0;
    uint32_t base = entropy_block_offset(T, blk, &comp);
    BitReader r;
    r.open(T.payload, hi, p);
    for (int step = 0; step < nblocks * 64; ++step) {
        const int c = b < hv ? 0 : 1 + (b - hv);
        int pos, val;
        bool done;
        int status = entropy_step(r, sh->tab[T.dc[c]], sh->tab[2 + T.ac[c]], p, z, &pos, &val, &done);
        if (status == kEntropyOk && p > end) status = kEntropyExhausted;
        if (status != kEntropyOk) {
            restart_record(sh, k, status);
            return;
        }
        if (pos == 0) {                                                      // the DC difference: the value itself is stored
            int& dc = c == 0 ? dc0 : c == 1 ? dc1 : dc2;
            dc = (int)((uint32_t)dc + (uint32_t)val);
            val = dc;
        }
        if (pos >= 0) *(int16_t*)(T.slot + base + 2u * sh->natural[pos & 63]) = (int16_t)val;
        if (done) {
            ++blk;
            if (++b == T.bpm) b = 0;
            if (++done_blocks == nblocks) break;
            base = entropy_block_offset(T, blk, &comp);
        }
    }
    if (done_blocks < nblocks) restart_record(sh, k, kEntropyExhausted);     // unreachable: 64 symbols complete any block
    else if (end - p >= 8) restart_record(sh, k, kEntropyLeftover);
}

// pass R
AP_HD void restart_pass_decode(const RestartTile& R, RestartShared* sh, int lane, int nl) {
    for (uint32_t k = (uint32_t)lane; k < R.count; k += (uint32_t)nl) restart_decode_interval(R, sh, k);
}

// status, one lane
AP_HD int32_t restart_pass_status(const RestartTile& R, const RestartShared* sh) {
    if (R.T.bad || sh->table_error) return kEntropyBadDescriptor;
    if (sh->error != kEntropyNoError) return (int32_t)(sh->error & 15u);
    return kEntropyOk;
}

}  // namespace ap
