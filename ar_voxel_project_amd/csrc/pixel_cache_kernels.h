// pixel_cache_kernels.h -- the table of cached voxel pixels (carve_kernels.h, table_view_blocks).
//
// The pixel a voxel projects to in a view is a function of the view's matrix, the voxel size, the
// voxel's place in the grid and the grouping of the row sums -- the masks only decide which bit is
// found there.  While a context's cameras stand (the validity of the block rectangles of
// rect_cache_kernels.h, plus the grouping), the exact kernel's projection is therefore computed once,
// here, and read from then on: one byte per (voxel, view), the pixel relative to the origin of the
// cached rectangle of the voxel's 4 x 4 x 4 block.  The kernel below forms the voxels exactly as
// carve_exact_blocks_kernel does (its lane <-> voxel map, global_z for slabs and striped slabs, the
// world coordinates as fp32 products) and runs exact_view_blocks' own arithmetic: row_sum on the
// exact fp64 products, IEEE quotients -- bit for bit the shared-reciprocal quotients wherever the
// kernel may use those (divide2_shared_rcp) --, pixel_tagged.
#pragma once

#include "rect_cache_kernels.h"

namespace arvx {

// The 16 bytes of lane `lane` for (view, ri): byte 4 m + j = the lane's voxel in block j of group
// m = 2 byi + bzi, voxel (4 j + lx, 4 byi + ly, 4 bzi + lz) of the sub-tile; low nibble px - pxlo,
// high nibble py - pylo of the block's entry `ent[4 m + j]`.  Voxels outside the grid and blocks
// whose entry is no rectangle ("outside", "mixed without a look"): 0, never read for a decision.
// false: a pixel of a block with a rectangle lies outside the image or more than 15 pixels from the
// rectangle's origin.
template <bool LEFT>
__device__ inline bool pixel_cache_lane(const CarveParams &p, int view, size_t ri, int lane,
                                        const uint32_t *__restrict__ ent, uint4 &out) {
    int sx0, sy0, sz0;
    rec_origin(p, ri, sx0, sy0, sz0);
    const int lx = lane & 3, ly = (lane >> 2) & 3, lz = lane >> 4;
    const float *Mv = p.M + 12 * view;
    double md[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) md[r][c] = (double)Mv[4 * r + c];
    const float wlim = (float)p.W - 0.5f, hlim = (float)p.H - 0.5f;
    const int xb = p.rcXB, yb = p.rcYB;
    bool fits = true;
    uint32_t w[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int byi = m >> 1, bzi = m & 1;
        const int y = sy0 + 4 * byi + ly, z = sz0 + 4 * bzi + lz;
        const double dwy = (double)((float)y * p.s);
        const double dwz = (double)((float)(-global_z(p, z)) * p.s);
        w[m] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = sx0 + 4 * j + lx;
            const uint32_t e = ent[4 * m + j];
            if (!(e >> (xb + yb)) || x >= p.X || y >= p.Y || z >= p.Z) continue;
            const double dwx = (double)((float)x * p.s);
            float a[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                a[r] = row_sum<LEFT>(md[r][0] * dwy, md[r][1] * dwx, md[r][2] * dwz, md[r][3]);
            const uint32_t pix = pixel_tagged(a[0] / a[2], a[1] / a[2], p.W, wlim, hlim, 0);
            const int at = (int)(pix & 0x7fffffffu);
            const int py = at / p.W, px = at - py * p.W;
            const int ox = px - (int)__builtin_amdgcn_ubfe(e, 0u, (unsigned)xb);
            const int oy = py - (int)__builtin_amdgcn_ubfe(e, (unsigned)xb, (unsigned)yb);
            if (!(pix >> 31) || (unsigned)ox > 15u || (unsigned)oy > 15u) {
                fits = false;
                continue;
            }
            w[m] |= (uint32_t)(ox | (oy << 4)) << (8 * j);
        }
    }
    out = make_uint4(w[0], w[1], w[2], w[3]);
    return fits;
}

// CHECK false: writes the table `tab` (n lanes of 16 bytes; a view's are rec_count * 64) from the
// block table p.rcBlk and sets bit v of miss[v / 64] for every view with a pixel that does not fit:
// such a view stays with the projection, the others are read.  true: recomputes every lane and
// counts the bytes that differ in *bad (arvx_selftest_pixel_cache).
template <bool LEFT, bool CHECK>
__global__ __launch_bounds__(256) void pixel_cache_kernel(const CarveParams p, uint4 *__restrict__ tab, size_t n,
                                                          unsigned long long *miss, unsigned long long *bad) {
    const size_t per_view = rec_count(p) << 6;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int view = (int)(i / per_view);
        const size_t ri = (i % per_view) >> 6;
        uint4 o;
        const bool fits = pixel_cache_lane<LEFT>(p, view, ri, (int)(i & 63),
                                                 p.rcBlk + (((size_t)view * rec_count(p) + ri) << 4), o);
        if (CHECK) {
            const uint4 t = tab[i];
            const uint32_t d[4] = {t.x ^ o.x, t.y ^ o.y, t.z ^ o.z, t.w ^ o.w};
            int nb = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int b = 0; b < 4; ++b) nb += ((d[k] >> (8 * b)) & 0xffu) ? 1 : 0;
            if (nb) atomicAdd(bad, (unsigned long long)nb);
        } else {
            tab[i] = o;
            if (!fits) atomicOr(&miss[view >> 6], 1ull << (view & 63));
        }
    }
}

}  // namespace arvx
