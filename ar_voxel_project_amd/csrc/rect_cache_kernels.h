// rect_cache_kernels.h -- the table of cached block rectangles (carve_kernels.h, "cached rectangles").
//
// The rectangle arithmetic of the carve (rect_prepare) is a function of a view's matrix, the image
// size, the voxel size and the box.  A rig with calibrated cameras sends the same matrices with
// every batch of masks, so the answers for the boxes the exact kernel forms again and again -- the
// 4 x 4 x 4 blocks of block_tests -- are computed once here and loaded from then on.  An entry is
// bit for bit what the consumer would compute: the kernel below forms exactly block_tests' boxes
// (the clipping to the grid, global_z for slabs and striped slabs) and calls the same rect_prepare.
#pragma once

#include "carve_kernels.h"

namespace arvx {

// the inverse of rec_index: first voxel (slab-local z) of the sub-tile with record index ri
__device__ inline void rec_origin(const CarveParams &p, size_t ri, int &sx0, int &sy0, int &sz0) {
    const int tshift = p.cyShift + p.czShift;
    const int wave = (int)(ri & 3);
    const int tl = (int)((ri >> 2) & ((1u << tshift) - 1u));
    const int ct = (int)(ri >> (tshift + 2));
    const int tx = ct % p.coarseX;
    const int ty = (((ct / p.coarseX) % p.coarseY) << p.cyShift) + (tl & ((1 << p.cyShift) - 1));
    const int tz = ((ct / (p.coarseX * p.coarseY)) << p.czShift) + (tl >> p.cyShift);
    sx0 = tx * kTileX + wave * kSubX;
    sy0 = ty * kTileY;
    sz0 = tz * kTileZ;
}

// entry (view, ri, blk) of the table: block blk (block_tests: j = blk & 3, m = blk >> 2) of the
// sub-tile with record index ri.  false: the rectangle does not fit an entry.
__device__ inline bool rect_cache_block_entry(const CarveParams &p, int view, size_t ri, int blk,
                                              uint32_t &e) {
    int sx0, sy0, sz0;
    rec_origin(p, ri, sx0, sy0, sz0);
    const int j = blk & 3, m = blk >> 2, byi = m >> 1, bzi = m & 1;
    const int x0 = sx0 + 4 * j, y0 = sy0 + 4 * byi, z0 = sz0 + 4 * bzi;
    RectQ q;
    q.code = kClsOut;  // (outside the grid: block_tests does not look, its answer is "outside")
    q.fast = q.base = q.dx = q.dy = 0;
    if (x0 < p.X && y0 < p.Y && z0 < p.Z) {
        const BoxW box = make_box(p.s, x0, min(x0 + 3, p.X - 1), y0, min(y0 + 3, p.Y - 1),
                                  global_z(p, z0), global_z(p, min(z0 + 3, p.Z - 1)));
        float Mr[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) Mr[i] = p.M[12 * view + i];
        q = rect_prepare(Mr, box, p.W, p.H, p.satW);
    }
    const RectBits rb = {p.rcXB, p.rcYB, p.rcDB};
    return rect_pack_block(q, p.satW, rb, e);
}

// CHECK false: writes the table `blk` (nblk entries; a view's are rec_count * 16).  *miss (a
// page-locked word of the host's) is set when a rectangle does not fit its entry: the host then
// gives the table up.  true: recomputes every entry and counts the ones that differ in *bad
// (arvx_selftest_rect_cache).
template <bool CHECK>
__global__ __launch_bounds__(256) void rect_cache_block_kernel(const CarveParams p, uint32_t *__restrict__ blk,
                                                               size_t nblk, long long *miss,
                                                               unsigned long long *bad) {
    const size_t per_view = rec_count(p) << 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nblk; i += stride) {
        const size_t in_view = i % per_view;
        uint32_t e;
        const bool fits = rect_cache_block_entry(p, (int)(i / per_view), in_view >> 4, (int)(in_view & 15), e);
        if (CHECK) {
            if (!fits || blk[i] != e) atomicAdd(bad, 1ull);
        } else {
            blk[i] = e;
            if (!fits) *miss = 1;
        }
    }
}

}  // namespace arvx
