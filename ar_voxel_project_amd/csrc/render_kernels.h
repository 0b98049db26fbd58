// render_kernels.h -- the welded mesh's vertex voxels drawn into a camera view for gfx950
// (arvx_render; the definition is in include/arvx/arvx.h, after the smoothing block).
//
// The vertex list is arvx_mc_mesh_welded's (ascending flat index, its colours beside it).  Then:
//   render_clear_kernel        the W x H keys to all-ones, the large-footprint list and the
//                              agreement counters to empty
//   render_splat_kernel        one lane per vertex voxel: splat_footprint (visibility_kernels.h) with
//                              the caller's camera, then the footprint's minimum -- small
//                              footprints from the lane, large ones appended to a list (when it is
//                              full, swept by the lane's wave instead)
//   render_splat_large_kernel  one wave per listed footprint, a pixel per lane
//   render_resolve_kernel      one lane per pixel: the key's index and depth, the winner's colour
//   render_agreement_kernel    covered pixels against a view's background bit plane
// A key is bits(a2) << 32 | k.  a2 is a positive fp32, for which unsigned order of the bits is
// float order: the 64-bit unsigned minimum is the nearest voxel and, among equally near ones, the
// one with the least k.  It is a no-return atomicMin and does not depend on the order in which
// voxels arrive.  All stores are ordinary vector stores.
#pragma once

#include "visibility_kernels.h"

namespace arvx {

constexpr unsigned long long kRenderEmpty = ~0ull;  // no voxel covers the pixel

// The list's header (64 bytes in front of the footprints): the entries appended, then the three
// agreement counters.
struct RenderHeader {
    unsigned n_large;
    unsigned pad;
    unsigned long long counts[3];
};

struct RenderSplatParams {
    const int *index;  // the welded mesh's vertex voxels (flat index over the grid)
    long long n;       // how many
    int X, Y;
    float s;
    int W, H;
    SelftestMatrix M;  // the camera, row-major 3 x 4
    unsigned long long *keys;  // H x W
    SplatRect *large;  // large footprints; `view` holds the vertex's k
    unsigned *n_large;  // entries appended (may exceed large_cap: those were splatted by their lane)
    unsigned large_cap;
};

__global__ __launch_bounds__(256) void render_clear_kernel(unsigned long long *__restrict__ keys, size_t n,
                                                           RenderHeader *__restrict__ head) {
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 == 0) {
        head->n_large = 0;
        head->counts[0] = head->counts[1] = head->counts[2] = 0;
    }
    for (size_t i = i0; i < n; i += (size_t)gridDim.x * 256) keys[i] = kRenderEmpty;
}

// splat_min on a key: the load first, so that a voxel behind what the pixel already holds sends no
// atomic (the value only decreases: a stale load can only let a useless atomic through)
__device__ __forceinline__ void key_min(unsigned long long *p, unsigned long long key) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(p, key);
}

__device__ __forceinline__ unsigned long long render_key(uint32_t d, uint32_t k) {
    return ((unsigned long long)d << 32) | k;
}

// one footprint (packed as in SplatRect) by a whole wave: its pixels row-major across the lanes
__device__ __forceinline__ void sweep_key_rect(unsigned long long *__restrict__ keys, int W, uint32_t cols,
                                               uint32_t rows, unsigned long long key, int lane) {
    const int c0 = (int)(cols & 0xFFFFu), c1 = (int)(cols >> 16);
    const int r0 = (int)(rows & 0xFFFFu), r1 = (int)(rows >> 16);
    const int wc = c1 - c0 + 1;
    const int area = wc * (r1 - r0 + 1);
    for (int j = lane; j < area; j += 64) {
        const int r = r0 + j / wc, c = c0 + j % wc;
        key_min(keys + (size_t)r * W + c, key);
    }
}

// One lane per vertex voxel; the grid strides over the list.  Footprints of up to kSplatLanePixels
// pixels are splatted by their lane; larger ones go to the list that render_splat_large_kernel
// sweeps, a wave per footprint.  When that list is full, the lane's own wave sweeps them, one
// after the other, 64 pixels a step (as vis_splat_kernel).
template <bool LEFT>
__global__ __launch_bounds__(256) void render_splat_kernel(const RenderSplatParams p) {
    SplatParams sp{};  // (splat_footprint reads the grid, the voxel size and the image size)
    sp.X = p.X;
    sp.Y = p.Y;
    sp.s = p.s;
    sp.W = p.W;
    sp.H = p.H;
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * 256; base < p.n; base += (long long)gridDim.x * 256) {
        const long long t = base + threadIdx.x;
        uint32_t cols = 0, rows = 0, d = 0;
        bool wide = false;  // large, and the list had no room
        if (t < p.n && splat_footprint<LEFT>(sp, p.M.m, p.index[t], cols, rows, d)) {
            const int c0 = (int)(cols & 0xFFFFu), c1 = (int)(cols >> 16);
            const int r0 = (int)(rows & 0xFFFFu), r1 = (int)(rows >> 16);
            if ((c1 - c0 + 1) * (r1 - r0 + 1) <= kSplatLanePixels) {
                const unsigned long long key = render_key(d, (uint32_t)t);
                for (int r = r0; r <= r1; ++r)
                    for (int c = c0; c <= c1; ++c) key_min(p.keys + (size_t)r * p.W + c, key);
            } else {
                const unsigned k = atomicAdd(p.n_large, 1u);
                if (k < p.large_cap)
                    p.large[k] = SplatRect{cols, rows, (uint32_t)t, d};
                else
                    wide = true;
            }
        }
        // (every lane of the wave gets here: the loop bound is uniform over the workgroup)
        unsigned long long m = __ballot(wide);
        const long long wave_t0 = base + (threadIdx.x - lane);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            sweep_key_rect(p.keys, p.W, (uint32_t)__shfl((int)cols, l), (uint32_t)__shfl((int)rows, l),
                           render_key((uint32_t)__shfl((int)d, l), (uint32_t)(wave_t0 + l)), lane);
        }
    }
}

// one wave per listed footprint; a fixed grid that strides over the list (its length is on the
// device).  The number of footprints the splat wanted to list goes to `need` (a page-locked host
// word, read at the next synchronisation of a render call): the renders after that size their
// lists from it.
__global__ __launch_bounds__(256) void render_splat_large_kernel(const SplatRect *__restrict__ large,
                                                                 const unsigned *__restrict__ n_large,
                                                                 unsigned large_cap,
                                                                 unsigned long long *__restrict__ keys, int W,
                                                                 long long *__restrict__ need) {
    const int lane = threadIdx.x & 63;
    const unsigned waves = gridDim.x * 4;
    const unsigned wanted = *n_large;
    if (blockIdx.x == 0 && threadIdx.x == 0) *need = (long long)wanted;
    const unsigned n = min(wanted, large_cap);
    for (unsigned f = blockIdx.x * 4 + (threadIdx.x >> 6); f < n; f += waves) {
        const SplatRect e = large[f];
        sweep_key_rect(keys, W, e.cols, e.rows, render_key(e.depth, e.view), lane);
    }
}

__device__ __forceinline__ uint8_t render_channel(float c) {
    return (uint8_t)roundf(fminf(fmaxf(c, 0.f), 255.f));
}

// One lane per pixel.  bgr holds the background already (the caller's image or zeros): only the
// covered pixels are written.
__global__ __launch_bounds__(256) void render_resolve_kernel(const unsigned long long *__restrict__ keys,
                                                             size_t npix, const float *__restrict__ rgb,
                                                             int *__restrict__ id, float *__restrict__ depth,
                                                             uint8_t *__restrict__ bgr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long key = keys[i];
    if (key == kRenderEmpty) {
        id[i] = -1;
        depth[i] = INFINITY;
        return;
    }
    const uint32_t k = (uint32_t)key;
    id[i] = (int)k;
    depth[i] = __uint_as_float((uint32_t)(key >> 32));
    const float *__restrict__ c = rgb + 3 * (size_t)k;
    bgr[3 * i] = render_channel(c[2]);
    bgr[3 * i + 1] = render_channel(c[1]);
    bgr[3 * i + 2] = render_channel(c[0]);
}

// One lane per pixel, so a wave holds 64 consecutive pixels starting at a multiple of 64: their
// coverage by __ballot against the two 32-bit words of the view's background plane (bit i of word
// i / 32 = pixel i is background).  counts: covered and foreground, covered and background,
// uncovered and foreground -- reduced per workgroup, one atomicAdd per counter per workgroup.
__global__ __launch_bounds__(256) void render_agreement_kernel(const int *__restrict__ id, size_t npix,
                                                               const uint32_t *__restrict__ bg,
                                                               unsigned long long *__restrict__ counts) {
    __shared__ unsigned s_n[4][3];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < npix;
    const unsigned long long in = __ballot(valid);
    const unsigned long long cov = __ballot(valid && id[i] >= 0);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        unsigned long long back = 0;
        if (in) {  // (the plane has a word more than the pixels need: both words exist)
            const size_t g = i >> 6;
            back = (unsigned long long)bg[2 * g] | ((unsigned long long)bg[2 * g + 1] << 32);
        }
        s_n[wave][0] = (unsigned)__popcll(cov & ~back);
        s_n[wave][1] = (unsigned)__popcll(cov & back);
        s_n[wave][2] = (unsigned)__popcll(in & ~cov & ~back);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned n = s_n[0][threadIdx.x] + s_n[1][threadIdx.x] + s_n[2][threadIdx.x] + s_n[3][threadIdx.x];
        if (n) atomicAdd(counts + threadIdx.x, (unsigned long long)n);
    }
}

// the counters into the page-locked words the host reads at the call's synchronisation
__global__ void render_counts_out_kernel(const unsigned long long *__restrict__ counts,
                                         long long *__restrict__ out) {
    if (threadIdx.x < 3) out[threadIdx.x] = (long long)counts[threadIdx.x];
}

}  // namespace arvx
