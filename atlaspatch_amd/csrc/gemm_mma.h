// MFMA fragment / row-statistics / tile-walk helpers of the two GEMM kernels (the epilogue family itself: gemm_epilogue.h).
//
// The persistent kernel's (gemm256.hip) 16-bit product is v_mfma_f32_16x16x32_{f16,bf16}: on MI355X the chip holds a higher clock on this shape than on
// 32x32x16 at equal cycles per FLOP (tools/isa_probes/mfma_shape_probe.hip, profiles/mfma_shape_probe.txt), and the f32
// accumulators of the two shapes are bit-identical for the same operands in ascending k (same probe), which is why the
// 128 x 128 kernel (gemm.hip) can stay on 32x32x16 and still agree with this one bit for bit.
#pragma once
#include "kernel_util.h"
#include "gemm_epilogue.h"

namespace ap {
namespace {

// Operand map of Mma16x16<T>::run(a, b, c): lane l supplies row l & 15 of either operand, k = 8 (l >> 4) + j (j = 0..7 of the Frag), and
// receives c[e] = C[first-operand row 4 (l >> 4) + e][second-operand row l & 15].
// AccMap: the kernels give the WEIGHT fragment as the first operand and cover a 32 (n) x 32 (m) region of the output with 2 x 2
// blocks, block g = nh * 2 + mh.  Element e of block g in lane l is
//     m = mh * 16 + (l & 15),    n = nh * 16 + 4 (l >> 4) + e       -- four consecutive n of one m (what pack4 and the
// 16-byte transposed stores rely on).  m(g) / n(g): the lane's row and first column of block g inside the region.
struct AccMap {
    int l15, q;
    __device__ __forceinline__ explicit AccMap(int lane) : l15(lane & 15), q(lane >> 4) {}
    static __device__ __forceinline__ constexpr int nh(int g) { return g >> 1; }
    static __device__ __forceinline__ constexpr int mh(int g) { return g & 1; }
    __device__ __forceinline__ int m(int g) const { return mh(g) * 16 + l15; }
    __device__ __forceinline__ int n(int g) const { return nh(g) * 16 + q * 4; }
};

// EPI_RESID_STATS element step on 8 packed values: y = T(d + r) (d = the branch output already rounded to T, r = the
// stream), s += sum(y), q += sum(y^2) in f32, ONE chain over the four dwords.
template <typename T> __device__ __forceinline__ u32x4 resid_add_stats(u32x4 d, u32x4 r, float& s, float& q) {
    u32x4 y;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t dk = d[k], rk = r[k];     // (bit_cast of a vector-element lvalue reads element 0: copy first)
        const uint32_t yk = resid_add2<T>(dk, rk);
        y[k] = yk;
        stats2<T>(yk, s, q);
    }
    return y;
}

#define AP_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

struct TileWalk {          // this workgroup's tile list: ids first, first + stride, ... (< end)
    int first, stride, count, tiles_n, tiles_m, group;
    // id -> (row tile, column tile): column groups of `group` tiles, row-major inside a group, so the
    // workgroups of an XCD (consecutive ids) form a (workgroups / group) x group block of tiles.
    __device__ __forceinline__ void rc(int id, int& tr, int& tc) const {
        const int per = group * tiles_m;
        const int grp = id / per, rem = id - grp * per;
        const int left = tiles_n - grp * group;
        const int width = left < group ? left : group;
        tr = rem / width;
        tc = grp * group + (rem - tr * width);
    }
};

}  // namespace
}  // namespace ap
