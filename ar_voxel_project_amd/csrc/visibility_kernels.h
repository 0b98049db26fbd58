// visibility_kernels.h -- the occlusion-aware colour vote for gfx950 (arvx_color_visible; the
// definition is in include/arvx/arvx.h, next to arvx_color).
//
// The colour list is arvx_color's (bitplane_kernels.h compaction, ascending flat index).  Then:
//   vis_clear_kernel        the V depth buffers to +inf, the large-footprint list to empty
//   vis_splat_kernel        one lane per (surface voxel, view), view-major (blockIdx.y = view, so a
//                           workgroup's neighbouring voxels hit neighbouring pixels): the centre's
//                           a2 and the eight corners' quotients, then the footprint's minimum --
//                           small footprints from the lane, large ones appended to a list (when
//                           it is full, swept by the lane's wave instead)
//   vis_splat_large_kernel  one wave per listed footprint, a pixel per lane
//   vis_vote_kernel         color_vote_kernel's loop with the visibility test: the visible and the
//                           unfiltered vote side by side (the fallback costs no second pass), and
//                           the number of views each voxel is visible in
// The depth buffer holds the bits of positive fp32 values (a2 > 0) and +inf: for those, unsigned
// order is float order, so the minimum is a no-return atomicMin on the bits and does not depend on
// the order in which voxels arrive.  Every fp32 operation is rounded on its own (-ffp-contract=off)
// and fp32 '/' is correctly rounded.
#pragma once

#include "color_kernels.h"

namespace arvx {

constexpr uint32_t kDepthInf = 0x7F800000u;  // +inf
constexpr int kSplatLanePixels = 16;  // footprints up to this many pixels are splatted by their lane

// A footprint left to vis_splat_large_kernel: columns c0..c1, rows r0..r1 (inclusive, in the image),
// its view and the bits of its depth.
struct SplatRect {
    uint32_t cols;  // c0 | c1 << 16  (W, H <= kMaxImageDim)
    uint32_t rows;  // r0 | r1 << 16
    uint32_t view;
    uint32_t depth;
};

struct SplatParams {
    const int *index;        // surface voxels (flat index over the grid)
    long long cap;           // entries the launch covers (the list's capacity)
    const long long *n_dev;  // the list's length as the compaction left it on the device
    int X, Y;
    float s;
    int V, W, H;
    const float *M;      // V x 12
    uint32_t *zbuf;      // V x H x W depth bits
    SplatRect *large;    // large footprints
    unsigned *n_large;   // entries appended (may exceed large_cap: those were splatted by their lane)
    unsigned large_cap;
};

__global__ __launch_bounds__(256) void vis_clear_kernel(uint32_t *__restrict__ zbuf, size_t n,
                                                        unsigned *__restrict__ n_large) {
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 == 0) *n_large = 0;
    for (size_t i = i0; i < n; i += (size_t)gridDim.x * 256) zbuf[i] = kDepthInf;
}

// the minimum of one pixel: the load first, so that a voxel behind what the pixel already holds
// sends no atomic (the value only decreases: a stale load can only let a useless atomic through)
__device__ __forceinline__ void splat_min(uint32_t *p, uint32_t d) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > d) atomicMin(p, d);
}

__device__ __forceinline__ void splat_rect(uint32_t *__restrict__ z, int W, int c0, int c1, int r0,
                                           int r1, uint32_t d) {
    for (int r = r0; r <= r1; ++r)
        for (int c = c0; c <= c1; ++c) splat_min(z + (size_t)r * W + c, d);
}

// one footprint (packed as in SplatRect) by a whole wave: its pixels row-major across the lanes
__device__ __forceinline__ void sweep_rect(uint32_t *__restrict__ z, int W, uint32_t cols, uint32_t rows,
                                           uint32_t d, int lane) {
    const int c0 = (int)(cols & 0xFFFFu), c1 = (int)(cols >> 16);
    const int r0 = (int)(rows & 0xFFFFu), r1 = (int)(rows >> 16);
    const int wc = c1 - c0 + 1;
    const int area = wc * (r1 - r0 + 1);
    for (int k = lane; k < area; k += 64) {
        const int r = r0 + k / wc, c = c0 + k % wc;
        splat_min(z + (size_t)r * W + c, d);
    }
}

// The footprint of voxel i in view v (definition step 2): false if the voxel does not splat there
// or its footprint misses the image; else the inclusive columns / rows packed as in SplatRect and
// the bits of the centre's a2.
template <bool LEFT>
__device__ __forceinline__ bool splat_footprint(const SplatParams &p, const float *__restrict__ Mv, int i,
                                                uint32_t &cols, uint32_t &rows, uint32_t &d) {
    const int x = i % p.X;
    const int y = (i / p.X) % p.Y;
    const int z = i / (p.X * p.Y);
    // the centre: only its a2 counts here (the splat's test and its depth)
    float a[3];
    project_rows<LEFT>(Mv, p.s, x, y, z, a);
    const float a2 = a[2];
    if (!(a2 > 0.f)) return false;
    // the corners: each world coordinate takes two values, so the products of a row do too; the
    // sums are formed per corner in the row's grouping
    const float s = p.s;
    const float w0[2] = {((float)y + 0.5f * -1.f) * s, ((float)y + 0.5f * 1.f) * s};
    const float w1[2] = {((float)x + 0.5f * -1.f) * s, ((float)x + 0.5f * 1.f) * s};
    const float w2[2] = {-(((float)z + 0.5f * -1.f) * s), -(((float)z + 0.5f * 1.f) * s)};
    double P0[3][2], P1[3][2], P2[3][2], P3[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            P0[r][k] = (double)Mv[4 * r] * (double)w0[k];
            P1[r][k] = (double)Mv[4 * r + 1] * (double)w1[k];
            P2[r][k] = (double)Mv[4 * r + 2] * (double)w2[k];
        }
        P3[r] = (double)Mv[4 * r + 3];
    }
    float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int kx = c & 1, ky = (c >> 1) & 1, kz = c >> 2;
        const float c0 = row_sum<LEFT>(P0[0][ky], P1[0][kx], P2[0][kz], P3[0]);
        const float c1 = row_sum<LEFT>(P0[1][ky], P1[1][kx], P2[1][kz], P3[1]);
        const float c2 = row_sum<LEFT>(P0[2][ky], P1[2][kx], P2[2][kz], P3[2]);
        const float qu = c0 / c2, qv = c1 / c2;
        ok &= (c2 > 0.f) & isfinite(qu) & isfinite(qv);
        umin = fminf(umin, qu);
        umax = fmaxf(umax, qu);
        vmin = fminf(vmin, qv);
        vmax = fmaxf(vmax, qv);
    }
    if (!ok) return false;
    // footprint: round (half away from zero) of the extremes, clipped to the image
    const float cu0 = roundf(umin), cu1 = roundf(umax), rv0 = roundf(vmin), rv1 = roundf(vmax);
    if (cu1 < 0.f || rv1 < 0.f || cu0 > (float)(p.W - 1) || rv0 > (float)(p.H - 1)) return false;
    const int col0 = (int)fmaxf(cu0, 0.f), col1 = (int)fminf(cu1, (float)(p.W - 1));
    const int row0 = (int)fmaxf(rv0, 0.f), row1 = (int)fminf(rv1, (float)(p.H - 1));
    if (col0 > col1 || row0 > row1) return false;  // (never: the extremes are ordered)
    cols = (uint32_t)col0 | ((uint32_t)col1 << 16);
    rows = (uint32_t)row0 | ((uint32_t)row1 << 16);
    d = __float_as_uint(a2);
    return true;
}

// One lane per (list entry, view): blockIdx.y is the view, the x grid strides over the list (its
// length is on the device).  Footprints of up to kSplatLanePixels pixels are splatted by their
// lane; larger ones go to the list that vis_splat_large_kernel sweeps, a wave per footprint.  When
// that list is full, the lane's own wave sweeps them, one after the other, 64 pixels a step: no
// lane ever walks a large footprint alone.
template <bool LEFT>
__global__ __launch_bounds__(256) void vis_splat_kernel(const SplatParams p) {
    const long long n = (p.n_dev && *p.n_dev < p.cap) ? *p.n_dev : p.cap;
    const int v = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const float *__restrict__ Mv = p.M + 12 * v;
    uint32_t *__restrict__ zv = p.zbuf + (size_t)v * p.W * p.H;
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
        const long long t = base + threadIdx.x;
        uint32_t cols = 0, rows = 0, d = 0;
        bool wide = false;  // large, and the list had no room
        if (t < n && splat_footprint<LEFT>(p, Mv, p.index[t], cols, rows, d)) {
            const int c0 = (int)(cols & 0xFFFFu), c1 = (int)(cols >> 16);
            const int r0 = (int)(rows & 0xFFFFu), r1 = (int)(rows >> 16);
            if ((c1 - c0 + 1) * (r1 - r0 + 1) <= kSplatLanePixels) {
                splat_rect(zv, p.W, c0, c1, r0, r1, d);
            } else {
                const unsigned k = atomicAdd(p.n_large, 1u);
                if (k < p.large_cap)
                    p.large[k] = SplatRect{cols, rows, (uint32_t)v, d};
                else
                    wide = true;
            }
        }
        // (every lane of the wave gets here: the loop bound is uniform over the workgroup)
        unsigned long long m = __ballot(wide);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            sweep_rect(zv, p.W, (uint32_t)__shfl((int)cols, l), (uint32_t)__shfl((int)rows, l),
                       (uint32_t)__shfl((int)d, l), lane);
        }
    }
}

// one wave per listed footprint, its pixels row-major across the lanes; a fixed grid that strides
// over the list (its length is on the device).  The number of footprints the splat wanted to list
// goes to `need` (a page-locked host word, read at the call's synchronisation): the next call
// sizes the list from it.
__global__ __launch_bounds__(256) void vis_splat_large_kernel(const SplatRect *__restrict__ large,
                                                              const unsigned *__restrict__ n_large,
                                                              unsigned large_cap, uint32_t *__restrict__ zbuf,
                                                              int W, int H, long long *__restrict__ need) {
    const int lane = threadIdx.x & 63;
    const unsigned waves = gridDim.x * 4;
    const unsigned wanted = *n_large;
    if (blockIdx.x == 0 && threadIdx.x == 0) *need = (long long)wanted;
    const unsigned n = min(wanted, large_cap);
    for (unsigned f = blockIdx.x * 4 + (threadIdx.x >> 6); f < n; f += waves) {
        const SplatRect e = large[f];
        sweep_rect(zbuf + (size_t)e.view * W * H, W, e.cols, e.rows, e.depth, lane);
    }
}

struct VisVoteParams {
    VoteParams vote;          // the colour pass's own parameters (zglob0 = 0: a whole grid)
    const uint32_t *zbuf;     // V x H x W depth bits
    float tol;                // >= 0, finite or +inf
    int *views;               // per entry: views in which the voxel is visible
};

// color_vote_kernel with the visibility test: per sample, visible iff the centre is inside the
// image (the sample exists), a2 > 0 and a2 <= Z_v[pix] + tol.  The unfiltered vote runs beside the
// visible one; a voxel visible in no view takes the unfiltered colour, and `has` / `depth` are
// always the unfiltered ones (arvx_color's).
template <bool LEFT>
__global__ __launch_bounds__(256) void vis_vote_kernel(const VisVoteParams q) {
    const VoteParams &p = q.vote;
    __shared__ double s_M[kVoteLdsViews * 12];
    const bool lds = p.V <= kVoteLdsViews;  // (uniform)
    if (lds) {
        for (int k = threadIdx.x; k < p.V * 12; k += 256) s_M[k] = (double)p.M[k];
        __syncthreads();
    }
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.n || (p.n_dev && t >= *p.n_dev)) return;
    const int i = p.index[t];
    const int x = i % p.X;
    const int y = (i / p.X) % p.Y;
    const int z = p.zglob0 + i / (p.X * p.Y);
    const float w0 = (float)y * p.s, w1 = (float)x * p.s, w2 = (float)(-z) * p.s;
    const double d0w = (double)w0, d1w = (double)w1, d2w = (double)w2;
    const float wlim = (float)p.W - 0.5f, hlim = (float)p.H - 0.5f;
    const size_t plane = (size_t)p.W * p.H;
    // all samples (the fallback) | the visible ones
    unsigned sr = 0, sg = 0, sb = 0, n = 0;
    float best = 0.f, br = 0.f, bgc = 0.f, bb = 0.f;
    double best_sum = 0.0;
    unsigned vr = 0, vg = 0, vb = 0, nv = 0;
    float vbest = 0.f, vbr = 0.f, vbg = 0.f, vbb = 0.f;
    double vbest_sum = 0.0;
    for (int v = 0; v < p.V; ++v) {
        float a[3];
        if (lds) {
            const double *Md = s_M + 12 * v;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                a[r] = row_sum<LEFT>(Md[4 * r] * d0w, Md[4 * r + 1] * d1w, Md[4 * r + 2] * d2w, Md[4 * r + 3]);
        } else {
            const float *__restrict__ Mv = p.M + 12 * v;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                a[r] = row_sum<LEFT>((double)Mv[4 * r] * d0w, (double)Mv[4 * r + 1] * d1w,
                                     (double)Mv[4 * r + 2] * d2w, (double)Mv[4 * r + 3]);
        }
        float qu, qv;
        const bool tame = fabsf(a[2]) >= 0x1p-60f && fabsf(a[2]) <= 0x1p60f && fabsf(a[0]) <= 0x1p60f &&
                          fabsf(a[1]) <= 0x1p60f;
        if (__all(tame)) {
            divide2_shared_rcp(a[0], a[1], a[2], qu, qv);
        } else {
            qu = a[0] / a[2];
            qv = a[1] / a[2];
        }
        int pix;
        if (!pixel_from_quotients(qu, qv, p.W, wlim, hlim, pix)) continue;
        const uint8_t *img = p.images + ((size_t)v * plane + pix) * 3;
        const unsigned b = img[0], g = img[1], r = img[2];
        const float *__restrict__ c = p.campos + 3 * v;
        const double e0 = (double)(c[0] - w0), e1 = (double)(c[1] - w1), e2 = (double)(c[2] - w2);
        const double e3 = (double)(1.f - 1.f);
        const double sum = ((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3;
        // (the square root only where it can decide: color_vote_kernel)
        if (n == 0 || sum < best_sum) {
            const float depth = (float)sqrt(sum);
            if (n == 0 || depth < best) {
                best = depth;
                br = (float)r;
                bgc = (float)g;
                bb = (float)b;
            }
            best_sum = sum;
        }
        sr += r;
        sg += g;
        sb += b;
        ++n;
        const float zb = __uint_as_float(q.zbuf[(size_t)v * plane + pix]);
        if (!(a[2] > 0.f) || !(a[2] <= zb + q.tol)) continue;
        if (nv == 0 || sum < vbest_sum) {
            const float depth = (float)sqrt(sum);
            if (nv == 0 || depth < vbest) {
                vbest = depth;
                vbr = (float)r;
                vbg = (float)g;
                vbb = (float)b;
            }
            vbest_sum = sum;
        }
        vr += r;
        vg += g;
        vb += b;
        ++nv;
    }
    p.has[t] = n ? 1 : 0;
    p.depth[t] = best;
    q.views[t] = (int)nv;
    if (nv) {  // the visible samples' vote
        n = nv;
        sr = vr;
        sg = vg;
        sb = vb;
        br = vbr;
        bgc = vbg;
        bb = vbb;
    }
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    if (n) {
        if (p.mode == 0) {
            o0 = br;
            o1 = bgc;
            o2 = bb;
        } else {
            const float fn = (float)n;
            o0 = roundf((float)sr / fn);
            o1 = roundf((float)sg / fn);
            o2 = roundf((float)sb / fn);
        }
    }
    p.rgba[t] = make_float4(o0, o1, o2, n ? 1.f : 0.f);
}

}  // namespace arvx
