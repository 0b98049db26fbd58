// vote_kernels.h -- the vote carve (arvx_carve_votes, an extension beyond the reference) for gfx950.
//
// The reference's carve empties a voxel at the first view that calls its pixel background
// (src/VoxelCarving.cpp:50-54).  The vote carve counts instead: per voxel bg = the views whose pixel
// is background and in = the views whose pixel lies in the image, and a voxel is emptied only when
// bg > max_misses (arvx.h has the definition).  One launch, one wave per 16 x 8 x 8 sub-tile, as
// carve_fused_kernel:
//   phase 1  lanes = views, 64 per chunk: classify_box of the sub-tile against each view.  A view
//            that sees only background adds 1 to both counts of EVERY voxel, one that sees only
//            foreground adds 1 to `in`, one that does not see the box adds nothing: three wave-wide
//            sums, no voxel is projected.  The rest are the sub-tile's mixed views.
//   phase 2  the mixed views, one after the other: the wave's 1024 voxels are projected in the
//            carve's own arithmetic (row_sum, divide2_shared_rcp under kFastDiv or IEEE `/`,
//            pixel_from_quotients) and the background bit is read.  Row map (subtile_of): a lane
//            holds 4 x-neighbours of 4 z planes, 16 voxels, one packed counter each -- bg in the
//            low half, in in the high half; bg <= in <= V <= 65535, so neither half overflows.
// Without the counts the work stops where the decision is known: a sub-tile whose all-background
// views alone outnumber max_misses is stored carved and seen (the carve's cull, generalised), and
// phase 2 ends at the first ballot that finds every voxel above max_misses (bg > max_misses >= 0
// implies in >= 1: seen).  With the counts every view is counted.
#pragma once

#include "carve_kernels.h"

namespace arvx {

struct VoteCarveParams {
    CarveParams g;     // geometry, views, records; flags bit2: the state is a fresh model (no load)
    uint16_t *bg;      // counts, flat index order, or null (no ARVX_VOTES_COUNTS)
    uint16_t *in;
    int max_misses;
    int cull;          // 0: ARVX_VOTES_NO_CULL -- every voxel is projected in every view
};

// One mixed view on the 16 voxels of every lane: cnt[k][j] += 1 << 16 where the pixel of voxel
// (x + j, y, zb + k) lies in the image, += 1 more where it is background.  The row sums are hoisted
// as in exact_view_blocks: the part of a row that does not change along the inner loop is formed
// once per view (LEFT: (p0[y] + p1[x]), RIGHT: (p1[x] + p2[z]) + p3 per plane), and p1 is an exact
// product, so fma(m1, wx, p) IS round(p1 + p).  The coordinates stay floats and are widened where
// they are used: sixteen counters and twelve hoisted doubles are what the lane has to hold.
template <bool LEFT>
__device__ __forceinline__ void vote_view(const CarveParams &p, const int view, const bool fast,
                                          const float wy, const float (&wx)[4], const float (&wz)[4],
                                          uint32_t (&cnt)[4][4]) {
    const uint32_t *__restrict__ bgv = p.bg + (size_t)view * p.bgWords;
    // the matrix is the same for every lane: through the scalar cache into scalar registers
    // (exact_view_blocks has the reasons)
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 row0, row1, row2;
    const float *Mv = p.M + 12 * view;
    asm volatile(
        "s_load_dwordx4 %0, %3, 0x0\n\t"
        "s_load_dwordx4 %1, %3, 0x10\n\t"
        "s_load_dwordx4 %2, %3, 0x20\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&s"(row0), "=&s"(row1), "=&s"(row2)
        : "s"(Mv)
        : "memory");
    const float mf[3][3] = {{row0.x, row0.y, row0.z}, {row1.x, row1.y, row1.z}, {row2.x, row2.y, row2.z}};
    const double p3[3] = {(double)row0.w, (double)row1.w, (double)row2.w};
    const float wlim = (float)p.W - 0.5f, hlim = (float)p.H - 0.5f;
    // a voxel outside the image reads the always-zero bit behind the view's plane
    const int zero_pix = 32 * (p.bgWords - 1);
    double h[3][4];  // LEFT: p0 + p1[j], for every plane
    double p0[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p0[r] = (double)mf[r][0] * (double)wy;
        if (LEFT) {
#pragma unroll
            for (int j = 0; j < 4; ++j) h[r][j] = fma((double)mf[r][1], (double)wx[j], p0[r]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double p2[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) p2[r] = (double)mf[r][2] * (double)wz[k];
        uint32_t pix[4];  // pixel_tagged
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                if (LEFT)
                    a[r] = (float)((h[r][j] + p2[r]) + p3[r]);
                else
                    a[r] = (float)(p0[r] + (fma((double)mf[r][1], (double)wx[j], p2[r]) + p3[r]));
            }
            float u, v;
            if (fast) {
                divide2_shared_rcp(a[0], a[1], a[2], u, v);
            } else {
                u = a[0] / a[2];
                v = a[1] / a[2];
            }
            pix[j] = pixel_tagged(u, v, p.W, wlim, hlim, zero_pix);
        }
        uint32_t word[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) word[j] = bgv[(pix[j] & 0x7fffffffu) >> 5];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t isbg = __builtin_amdgcn_ubfe(word[j], pix[j], 1u);  // bit pix & 31
            cnt[k][j] += ((pix[j] >> 31) << 16) + isbg;
        }
    }
}

template <bool LEFT>
__global__ __launch_bounds__(256, 4) void carve_votes_kernel(const VoteCarveParams q) {
    const CarveParams &p = q.g;
    // rows of tiles along x dealt to the 8 XCDs cyclically, as carve_fused_kernel
    const unsigned kb = blockIdx.x >> 3;
    const unsigned trow = (kb / p.tilesX) * 8u + (blockIdx.x & 7u);
    if (trow >= (unsigned)(p.tilesY * p.tilesZ)) return;
    const int tx = kb % p.tilesX;
    const int ty = trow % p.tilesY;
    const int tz = trow / p.tilesY;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const SubTile t = subtile_of(p, tx, ty, tz, wave, lane);
    if (t.sx0 >= p.X) return;  // wave-uniform
    uint16_t *const rec = p.rec + rec_index(p, tx, ty, tz, wave) * kRecU16;
    const bool counts = q.bg != nullptr;
    const bool cull = q.cull != 0;
    const bool early = cull && !counts;
    const uint32_t K = (uint32_t)q.max_misses;

    const float wy = (float)t.y * p.s;
    float wx[4], wz[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wx[j] = (float)(t.x + j) * p.s;
#pragma unroll
    for (int k = 0; k < 4; ++k) wz[k] = (float)(-global_z(p, t.zb + k)) * p.s;
    // this lane's voxels inside the grid: bit 4 k + j
    uint32_t okm = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t.lane_ok && t.zb + k < p.Z && t.x + j < p.X) okm |= 1u << (4 * k + j);

    uint32_t cnt[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt[k][j] = 0u;
    uint32_t base = 0u;  // what phase 1 adds to every voxel (wave-uniform), packed like cnt
    bool done = false;   // every voxel of the sub-tile is above max_misses
    const BoxW box = make_box(p.s, t.sx0, t.sx1, t.sy0, t.sy1, global_z(p, t.sz0), global_z(p, t.sz1));

    for (int vc = p.v0; vc < p.v1 && !done; vc += 64) {
        const int myv = vc + lane;
        int cls = kClsOut;
        if (myv < p.v1) {
            if (!cull) {
                // every voxel is projected; the rectangle arithmetic only says whether the shared-
                // reciprocal division is the IEEE one on this box (no table is looked at)
                float Mr[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) Mr[i] = p.M[12 * myv + i];
                cls = kClsMixed | rect_prepare(Mr, box, p.W, p.H, p.satW).fast;
            } else {
                cls = classify_box(p.M + 12 * myv, box, p.W, p.H, p.sat + (size_t)myv * p.satStride,
                                   p.satW);
            }
        }
        const unsigned long long fastdiv = __ballot((cls & kFastDiv) != 0);
        cls &= 3;
        const unsigned long long carved = __ballot(cls == kClsCarved);
        const unsigned long long infg = __ballot(cls == kClsFg);
        unsigned long long mixed = __ballot(cls == kClsMixed);
        base += (uint32_t)__popcll(carved) * 0x10001u + (uint32_t)__popcll(infg) * 0x10000u;
        if (early && (base & 0xffffu) > K) {
            done = true;
            break;
        }
        while (mixed) {
            const int b = __ffsll((long long)mixed) - 1;
            mixed &= mixed - 1;
            vote_view<LEFT>(p, __builtin_amdgcn_readfirstlane(vc + b), (fastdiv >> b) & 1ull, wy, wx, wz, cnt);
            if (early) {
                bool over = true;
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        over = over & (!((okm >> (4 * k + j)) & 1u) | (((base + cnt[k][j]) & 0xffffu) > K));
                if (__all(over)) {
                    done = true;
                    break;
                }
            }
        }
    }

    if (done) {
        subtile_store_done(rec, lane);
        return;
    }
    // occ' = occ && bg <= max_misses, seen' = seen || in >= 1.  (Voxels outside the grid stay as
    // the records keep them, occ 0 seen 1: nothing sets an occupied bit or clears a seen bit.)
    uint32_t st[4];
    subtile_load(p, t, rec, lane, st);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t w = st[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t tot = base + cnt[k][j];
            const uint32_t over = (tot & 0xffffu) > K ? 1u : 0u;
            const uint32_t seen = (tot >> 16) ? 2u : 0u;
            w = (w | (seen << (8 * j))) & ~(over << (8 * j));
        }
        st[k] = w;
    }
    subtile_store(rec, lane, st);
    if (!counts) return;
    // four x-neighbours are four u16 next to each other in either array: one 8-byte store each
    // where rows start at multiples of four voxels (X % 4 == 0), two-byte stores otherwise
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((okm >> (4 * k)) & 1u)) continue;  // (the lane's first x decides: rows are cut at the end)
        const size_t at = (size_t)t.x + (size_t)p.X * ((size_t)t.y + (size_t)p.Y * (size_t)(t.zb + k));
        uint32_t tot[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[j] = base + cnt[k][j];
        if ((p.X & 3) == 0) {
            const uint2 b2 = make_uint2((tot[0] & 0xffffu) | (tot[1] << 16), (tot[2] & 0xffffu) | (tot[3] << 16));
            const uint2 i2 = make_uint2((tot[0] >> 16) | (tot[1] & 0xffff0000u),
                                        (tot[2] >> 16) | (tot[3] & 0xffff0000u));
            *reinterpret_cast<uint2 *>(q.bg + at) = b2;
            *reinterpret_cast<uint2 *>(q.in + at) = i2;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!((okm >> (4 * k + j)) & 1u)) continue;
                q.bg[at + j] = (uint16_t)tot[j];
                q.in[at + j] = (uint16_t)(tot[j] >> 16);
            }
        }
    }
}

}  // namespace arvx
