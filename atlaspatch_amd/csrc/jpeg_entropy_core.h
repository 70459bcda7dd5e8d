// The decode core of ap_jpeg_entropy_decode_tiles (jpeg_entropy.hip), as __host__ __device__ functions: the bit reader, one symbol step,
// the state transition, the scan-index -> slot-address map and the passes of one tile, each written for "lane `lane` of `nl`".  The
// kernel runs a pass on every thread of a workgroup with a barrier behind it; tools/jpeg_entropy_check.cpp runs the same functions
// with the lanes in a loop, under AddressSanitizer / UBSan, before any input reaches a GPU.
//
// Self-synchronising parallel Huffman decode (Weissenberger & Schmidt, ICPP 2018 / 2021).  The unstuffed payload is cut into S
// subsequences of `ssb` bits.  The decoder state is (p, b, z): bit position, block-in-MCU index (selects component and tables), zig-zag
// index (0 = "DC next"), packed into one word.  entry[i] is the state subsequence i is decoded from, exit_[i] the state after the
// first symbol that ends at or past its last bit, count[i] the blocks completed on the way.
//   pass 1  every subsequence from the guess (first bit, b = 0, z = 0)
//   pass 2  rounds: entry[i] <- exit_[i - 1]; every subsequence whose entry changed is decoded again.  entry[0] is true by
//           construction, so after round r the first r + 1 subsequences are final: a round that changes nothing ends it, and S rounds
//           always suffice.  A decode that meets an invalid code, a coefficient index past 63 or the end of the bits leaves the
//           state DEAD, which propagates; on a false trajectory that is harmless, a later round replaces it.
//   pass 3  exclusive scan of count -> each subsequence's first block; every subsequence once more, now writing, stopping at the
//           frame's block count.  Errors are recorded here only: this IS the final trajectory.
//   pass 4  per component, prefix sum of the DC differences in scan order (int32, truncated to int16 on store), in place
//   pass 5  status
// Memory safety on any input: a payload word is read only below the checked length, a slot address is built from a block index below
// the frame's count, every table index is masked.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "jpeg_slot.h"
#include "jpeg_stream.h"

#ifndef AP_HD
#define AP_HD __host__ __device__ __forceinline__
#endif

namespace ap {

enum JpegEntropyStatus : int32_t {          // include/atlaspatch_hip.h: AP_JPEG_ENTROPY_*
    kEntropyOk = 0,
    kEntropyBadCode = 1,                    // a bit pattern no code of the table matches
    kEntropyBadIndex = 2,                   // a run that takes the zig-zag index past 63 (libjpeg folds it; this decoder flags it)
    kEntropyExhausted = 3,                  // the bits ran out before the frame's last block
    kEntropyLeftover = 4,                   // whole bytes left over after the last block
    kEntropyBadDescriptor = 5,              // a descriptor field outside its bounds (component count, selectors, tables, offset, length)
};

constexpr int kEntropyLanes = 256;
constexpr int kEntropyMaxSubseq = 4096;     // per tile; a longer payload gets longer subsequences
constexpr uint32_t kEntropyDead = 0xFFFFFFFFu;
constexpr uint32_t kEntropyNoError = 0xFFFFFFFFu;
constexpr int kEntropyDefaultBits = 1024;

struct HuffTable {                          // libjpeg's d_derived_tbl, 8-bit look-ahead
    uint16_t look[256];                     // (length << 8) | symbol for codes of <= 8 bits, 0 = longer
    int32_t maxcode[18];                    // largest code of length l, -1 if none; [17] ends every search
    int32_t valoff[18];                     // symbol index of the first code of length l, minus that code
    uint8_t sym[256];
};

struct EntropyShared {                      // what one tile's lanes share: LDS on the device
    HuffTable tab[4];
    uint32_t entry[kEntropyMaxSubseq], exit_[kEntropyMaxSubseq], count[kEntropyMaxSubseq];
    uint32_t lane_sum[3][kEntropyLanes];
    uint32_t error;                         // min over the final trajectory of (subsequence << 4 | status)
    uint32_t final_p;                       // the bit position behind the frame's last block, kEntropyDead until it is reached
    uint32_t table_error;
    uint8_t natural[64];
};

struct EntropyTile {                        // one tile's job, the same on every lane
    const JpegStreamDesc* desc;
    const uint8_t* payload;                 // 16-byte aligned; words up to the next multiple of 16 behind nbytes are readable
    uint8_t* slot;
    uint32_t nbytes, nbits, ssb;
    int S;
    int ncomp, hmax, vmax, bpm, mcux, total_blocks;
    int wb[3], nblk[3];
    uint32_t off[3], slot_bytes;
    int dc[3], ac[3];
    bool bad;                               // descriptor refused: the passes do nothing
};

AP_HD uint32_t entropy_pack(uint32_t p, int b, int z) { return (p << 9) | ((uint32_t)b << 6) | (uint32_t)z; }

// ---- bit reader: 32 bits from bit p, out of two cached big-endian words; bytes at and behind nbytes read as zero
struct BitReader {
    const uint8_t* d;
    uint32_t nbytes, idx, w0, w1;
    AP_HD uint32_t word(uint32_t j) const {
        if (j >= (nbytes + 3) / 4) return 0;
        const uint32_t w = __builtin_bswap32(((const uint32_t*)d)[j]);
        const uint32_t rem = nbytes - 4 * j;
        return rem >= 4 ? w : w & ~(0xFFFFFFFFu >> (8 * rem));
    }
    AP_HD void open(const uint8_t* data, uint32_t bytes, uint32_t p) {
        d = data; nbytes = bytes; idx = p >> 5; w0 = word(idx); w1 = word(idx + 1);
    }
    AP_HD uint32_t peek(uint32_t p) {
        const uint32_t j = p >> 5;
        if (j != idx) {
            if (j == idx + 1) { w0 = w1; w1 = word(j + 1); }
            else { w0 = word(j); w1 = word(j + 1); }
            idx = j;
        }
        const uint32_t s = p & 31;
        return s ? (w0 << s) | (w1 >> (32 - s)) : w0;
    }
};

// ---- the tables, from the raw DHT form; false when the counts are no canonical code libjpeg would take
AP_HD bool entropy_build_table(const uint8_t* counts, const uint8_t* symbols, HuffTable* t) {
    for (int k = 0; k < 256; ++k) { t->look[k] = 0; t->sym[k] = symbols[k]; }
    int p = 0, last = 0;
    uint32_t code = 0;
    bool good = true;
    for (int l = 1; l <= 16; ++l) if (counts[l - 1]) last = l;
    for (int l = 1; l <= 16; ++l) {
        const int c = counts[l - 1];
        t->valoff[l] = p - (int32_t)code;
        for (int i = 0; i < c; ++i, ++p, ++code) {
            if (p >= 256) { good = false; continue; }
            if (l <= 8) {
                const uint32_t first = (code << (8 - l)) & 255u, span = 1u << (8 - l);
                for (uint32_t k = 0; k < span; ++k) t->look[(first + k) & 255u] = (uint16_t)((l << 8) | symbols[p]);
            }
        }
        t->maxcode[l] = c ? (int32_t)code - 1 : -1;
        if (l <= last && code >= (1u << l)) good = false;
        code <<= 1;
    }
    t->maxcode[0] = -1; t->valoff[0] = 0;
    t->maxcode[17] = 0x7FFFFFFF; t->valoff[17] = 0;
    return good && last > 0;
}

// ---- one symbol: the state (p, b, z) moves on; returns a status; *pos >= 0 when a coefficient (zig-zag index *pos, value *val) was
// coded, *done when the symbol completed a block.  `dc_table` / `ac_table`: the tables of block b's component.
AP_HD int entropy_step(BitReader& r, const HuffTable& dc_table, const HuffTable& ac_table, uint32_t& p, int& z, int* pos, int* val, bool* done) {
    const HuffTable& t = z == 0 ? dc_table : ac_table;
    const uint32_t v = r.peek(p);
    int l, sym;
    const uint32_t lk = t.look[v >> 24];
    if (lk) {
        l = (int)(lk >> 8);
        sym = (int)(lk & 255u);
    } else {
        l = 9;
        while (l <= 16 && (int32_t)(v >> (32 - l)) > t.maxcode[l]) ++l;
        if (l > 16) return kEntropyBadCode;
        sym = t.sym[((int32_t)(v >> (32 - l)) + t.valoff[l]) & 255];
    }
    *pos = -1;
    *done = false;
    int s;
    if (z == 0) {
        s = sym & 15;
        *pos = 0;
        z = 1;
    } else {
        const int run = sym >> 4;
        s = sym & 15;
        if (s == 0) {
            p += (uint32_t)l;
            if (run != 15) { *done = true; z = 0; return kEntropyOk; }      // EOB, as jdhuff.c reads every (r != 15, 0)
            z += 16;
            return z > 63 ? kEntropyBadIndex : kEntropyOk;
        }
        z += run;
        if (z > 63) return kEntropyBadIndex;
        *pos = z;
        ++z;
        if (z == 64) { *done = true; z = 0; }
    }
    int x = 0;
    if (s) {
        x = (int)((v << l) >> (32 - s));                                    // l + s <= 31
        if (x < (1 << (s - 1))) x -= (1 << s) - 1;                          // HUFF_EXTEND
    }
    *val = x;
    p += (uint32_t)(l + s);
    return kEntropyOk;
}

// ---- scan index -> where the block lies in the slot: (component, byte offset of its 64 coefficients)
AP_HD uint32_t entropy_block_offset(const EntropyTile& T, int blk, int* comp) {
    const int m = blk / T.bpm, j = blk - m * T.bpm, my = m / T.mcux, mx = m - my * T.mcux, hv = T.hmax * T.vmax;
    int c, row, col;
    if (j < hv) { c = 0; const int dy = j / T.hmax; row = my * T.vmax + dy; col = mx * T.hmax + (j - dy * T.hmax); }
    else { c = 1 + (j - hv); row = my; col = mx; }
    *comp = c;
    return T.off[c] + (uint32_t)(row * T.wb[c] + col) * 128u;
}
// the k-th block of component c in scan order
AP_HD uint32_t entropy_component_block_offset(const EntropyTile& T, int c, int k) {
    if (c > 0) return T.off[c] + (uint32_t)k * 128u;                         // one block per MCU, MCUs in raster order = block order
    const int hv = T.hmax * T.vmax, m = k / hv, j = k - m * hv, my = m / T.mcux, mx = m - my * T.mcux, dy = j / T.hmax;
    return T.off[0] + (uint32_t)((my * T.vmax + dy) * T.wb[0] + mx * T.hmax + (j - dy * T.hmax)) * 128u;
}

AP_HD void entropy_record(EntropyShared* sh, int i, int status) {
    const uint32_t v = ((uint32_t)i << 4) | (uint32_t)status;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(&sh->error, v);
#else
    if (v < sh->error) sh->error = v;
#endif
}

// ---- subsequence i from entry[i].  !write: exit_[i] and count[i].  write: coefficients into the slot from block `first` on, errors recorded.
AP_HD void entropy_decode_subsequence(const EntropyTile& T, EntropyShared* sh, int i, bool write, int first) {
    const uint32_t e = sh->entry[i];
    if (e == kEntropyDead) {
        if (!write) { sh->exit_[i] = kEntropyDead; sh->count[i] = 0; }
        return;
    }
    uint32_t p = e >> 9;
    int b = (int)((e >> 6) & 7u), z = (int)(e & 63u);
    const uint32_t end = i == T.S - 1 ? T.nbits : (uint32_t)(i + 1) * T.ssb;
    int blk = first, comp = 0;
    uint32_t n = 0, base = 0;
    if (b >= T.bpm) b = 0;                                                   // a state no decode produced
    if (write && blk < T.total_blocks) base = entropy_block_offset(T, blk, &comp);
    BitReader r;
    r.open(T.payload, T.nbytes, p);
    while (p < end) {
        if (write && blk >= T.total_blocks) return;
        const int c = b < T.hmax * T.vmax ? 0 : 1 + (b - T.hmax * T.vmax);
        int pos, val;
        bool done;
        int status = entropy_step(r, sh->tab[T.dc[c]], sh->tab[2 + T.ac[c]], p, z, &pos, &val, &done);
        if (status == kEntropyOk && p > T.nbits) status = kEntropyExhausted;
        if (status != kEntropyOk) {
            if (write) entropy_record(sh, i, status);
            else { sh->exit_[i] = kEntropyDead; sh->count[i] = n; }
            return;
        }
        if (write && pos >= 0) *(int16_t*)(T.slot + base + 2u * sh->natural[pos & 63]) = (int16_t)val;
        if (done) {
            ++n;
            ++blk;
            if (++b == T.bpm) b = 0;
            if (write) {
                if (blk == T.total_blocks) { sh->final_p = p; return; }
                base = entropy_block_offset(T, blk, &comp);
            }
        }
    }
    if (!write) { sh->exit_[i] = entropy_pack(p, b, z); sh->count[i] = n; }
}

// ---- the tile's job from its descriptor; every field is checked, T->bad on a field outside its bounds
AP_HD void entropy_tile(const JpegStreamDesc* desc, const uint8_t* arena, size_t arena_bytes, uint8_t* slot, int side, int sampling,
                        int subsequence_bits, EntropyTile* T) {
    JpegGeom g;
    jpeg_geom(side, sampling, &g);
    T->desc = desc;
    T->slot = slot;
    T->ncomp = g.ncomp; T->hmax = g.hmax; T->vmax = g.vmax;
    T->bpm = g.hmax * g.vmax + (g.ncomp == 3 ? 2 : 0);
    T->mcux = side / (8 * g.hmax);
    T->total_blocks = T->mcux * (side / (8 * g.vmax)) * T->bpm;
    T->slot_bytes = (uint32_t)g.bytes;
    for (int c = 0; c < 3; ++c) {
        T->wb[c] = g.wb[c]; T->nblk[c] = g.wb[c] * g.hb[c]; T->off[c] = (uint32_t)g.off[c];
        T->dc[c] = desc->dc_sel[c] & 1; T->ac[c] = desc->ac_sel[c] & 1;
    }
    const uint64_t offset = desc->payload_offset;
    const uint32_t nbytes = desc->payload_bytes;
    bool bad = desc->ncomp != (uint32_t)g.ncomp || nbytes > kJpegStreamMaxPayload || (offset & 15) || offset > arena_bytes ||
               (((uint64_t)nbytes + 15) & ~(uint64_t)15) > arena_bytes - offset;
    for (int c = 0; c < g.ncomp; ++c) bad = bad || desc->dc_sel[c] > 1 || desc->ac_sel[c] > 1;
    T->bad = bad;
    T->nbytes = bad ? 0 : nbytes;
    T->nbits = T->nbytes * 8;
    T->payload = arena + (bad ? 0 : offset);
    uint32_t ssb = (uint32_t)subsequence_bits;
    const uint32_t least = (T->nbits + kEntropyMaxSubseq - 1) / kEntropyMaxSubseq;
    if (ssb < least) ssb = (least + 31) & ~31u;
    T->ssb = ssb;
    T->S = (int)((T->nbits + ssb - 1) / ssb);
}

// ================================================================== the passes, for lane `lane` of `nl` (nl * 32 >= kEntropyMaxSubseq)
// pass 0a: lanes 0 .. 3 build the four tables; lane 4 the natural-order map and the shared words
AP_HD void entropy_pass0_tables(const EntropyTile& T, EntropyShared* sh, int lane) {
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
        sh->final_p = kEntropyDead;
    }
}
// before pass 0a, by one lane: table_error must be clear before the table lanes may set it
AP_HD void entropy_pass0_clear(EntropyShared* sh) { sh->table_error = 0; }

// pass 0b: the slot -- quantisers, zero padding, zero coefficients -- in 16-byte stores
AP_HD void entropy_pass0_slot(const EntropyTile& T, int lane, int nl) {
    struct alignas(16) V { uint32_t w[4]; };
    const V* q = (const V*)T.desc->quant;
    V* out = (V*)T.slot;
    const uint32_t nv = T.slot_bytes / 16;
    for (uint32_t k = (uint32_t)lane; k < nv; k += (uint32_t)nl) out[k] = k < 24 ? q[k] : V{{0, 0, 0, 0}};
}

AP_HD void entropy_pass1(const EntropyTile& T, EntropyShared* sh, int lane, int nl) {
    for (int i = lane; i < T.S; i += nl) {
        sh->entry[i] = entropy_pack((uint32_t)i * T.ssb, 0, 0);
        entropy_decode_subsequence(T, sh, i, false, 0);
    }
}
// pass 2, first half: take the predecessors' exit states; returns the mask of this lane's subsequences that must be decoded again
AP_HD uint32_t entropy_pass2_read(const EntropyTile& T, EntropyShared* sh, int lane, int nl) {
    uint32_t mask = 0;
    int k = 0;
    for (int i = lane; i < T.S; i += nl, ++k) {
        if (i == 0) continue;
        const uint32_t e = sh->exit_[i - 1];
        if (e != sh->entry[i]) { sh->entry[i] = e; mask |= 1u << k; }
    }
    return mask;
}
AP_HD void entropy_pass2_decode(const EntropyTile& T, EntropyShared* sh, int lane, int nl, uint32_t mask) {
    int k = 0;
    for (int i = lane; i < T.S; i += nl, ++k)
        if (mask >> k & 1u) entropy_decode_subsequence(T, sh, i, false, 0);
}
// pass 3: count -> first block (exclusive scan, in place), in two halves around a barrier, then the writing decode
AP_HD void entropy_pass3_sum(const EntropyTile& T, EntropyShared* sh, int lane, int nl) {
    const int per = (T.S + nl - 1) / nl, lo = lane * per, hi = lo + per < T.S ? lo + per : T.S;
    uint32_t s = 0;
    for (int i = lo; i < hi; ++i) s += sh->count[i];
    sh->lane_sum[0][lane] = s;
}
AP_HD void entropy_pass3_scan(const EntropyTile& T, EntropyShared* sh, int lane, int nl) {
    const int per = (T.S + nl - 1) / nl, lo = lane * per, hi = lo + per < T.S ? lo + per : T.S;
    uint32_t s = 0;
    for (int k = 0; k < lane; ++k) s += sh->lane_sum[0][k];
    for (int i = lo; i < hi; ++i) { const uint32_t c = sh->count[i]; sh->count[i] = s; s += c; }
}
AP_HD void entropy_pass3_write(const EntropyTile& T, EntropyShared* sh, int lane, int nl) {
    for (int i = lane; i < T.S; i += nl) {
        const uint32_t first = sh->count[i];
        if (first < (uint32_t)T.total_blocks) entropy_decode_subsequence(T, sh, i, true, (int)first);
    }
}
// pass 4: DC differences -> DC values, per component in scan order, in two halves around a barrier
AP_HD void entropy_pass4_sum(const EntropyTile& T, EntropyShared* sh, int lane, int nl) {
    for (int c = 0; c < T.ncomp; ++c) {
        const int per = (T.nblk[c] + nl - 1) / nl, lo = lane * per, hi = lo + per < T.nblk[c] ? lo + per : T.nblk[c];
        uint32_t s = 0;
        for (int k = lo; k < hi; ++k) s += (uint32_t)(int32_t) * (const int16_t*)(T.slot + entropy_component_block_offset(T, c, k));
        sh->lane_sum[c][lane] = s;
    }
}
AP_HD void entropy_pass4_scan(const EntropyTile& T, EntropyShared* sh, int lane, int nl) {
    for (int c = 0; c < T.ncomp; ++c) {
        const int per = (T.nblk[c] + nl - 1) / nl, lo = lane * per, hi = lo + per < T.nblk[c] ? lo + per : T.nblk[c];
        uint32_t s = 0;
        for (int k = 0; k < lane; ++k) s += sh->lane_sum[c][k];
        for (int k = lo; k < hi; ++k) {
            int16_t* at = (int16_t*)(T.slot + entropy_component_block_offset(T, c, k));
            s += (uint32_t)(int32_t)*at;
            *at = (int16_t)s;
        }
    }
}
// pass 5, one lane
AP_HD int32_t entropy_pass5_status(const EntropyTile& T, const EntropyShared* sh) {
    if (T.bad || sh->table_error) return kEntropyBadDescriptor;
    if (sh->error != kEntropyNoError) return (int32_t)(sh->error & 15u);
    if (sh->final_p == kEntropyDead) return kEntropyExhausted;
    if (T.nbits - sh->final_p >= 8) return kEntropyLeftover;
    return kEntropyOk;
}

}  // namespace ap
