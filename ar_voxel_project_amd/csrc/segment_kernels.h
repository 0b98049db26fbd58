// segment_kernels.h -- silhouettes from the photographs (arvx_segment_views; definition in
// include/arvx/arvx.h): a per-pixel rule, box opening and closing, speck removal and hole filling,
// all on bit planes of the images, and the views' flat background plane out of the result.
//
// The work planes are BitGrids (bitplane_kernels.h) with X = W, Y = H, Z = views: rows of whole
// 64-bit words, bit x & 63 of word x >> 6 = 1 iff pixel (x, y) is FOREGROUND, the bits behind a row's
// last pixel 0 in every plane a kernel leaves.
//
//   seg_rule_kernel      image bytes (and plate bytes) -> the raw foreground plane, four pixels per
//                        lane from three aligned 4-byte loads, sixteen lanes per word
//   seg_count_kernel     foreground pixels per view (a count word per view and step)
//   seg_combine_kernel   out = AND / OR of n copies of a plane, each shifted by a whole number of
//                        pixels along x and y; pixels outside the image read as the operation's
//                        identity -- foreground for an erosion, background for a dilation, which is
//                        the border rule of the definition.  One launch with n = 2 r + 1 is a row or
//                        a column pass of radius r; launches with n = 2 double a window (host side)
//   seg_init_kernel      L[p] = the first pixel of p's run inside its word, for the pixels of the
//                        labelled kind (foreground, background or both); -1 elsewhere
//   seg_link_kernel      unions with the backward neighbours: foreground under 8-connectivity,
//                        background under 4; nothing crosses a view (comp_unite, components_kernels.h)
//   seg_roots_kernel     (next launch) L[p] = p's root
//   seg_area_kernel      per root its pixels, and bit 31: the component touches the image border
//   seg_best_kernel      per view the largest component that passes min_area: size << 32 | ~label
//   seg_specks_kernel    step 4 applied in place; the two counts, added by the roots' own lanes
//   seg_holes_kernel     step 5 applied in place; likewise
//   seg_publish_kernel   the flat background plane of views_bits_kernel: bit y * W + x, every word
//                        behind the pixels 0; a thread per 32-bit word
//   seg_bytes_kernel     a view's final plane as bytes (arvx_segment_download)
//
// Pixels are numbered p = (view * H + y) * W + x inside a batch of views: below 2^31 by the host's
// choice of the batch.  seg_init, seg_link, seg_specks and seg_holes run one lane per BIT of a padded row:
// 64 lanes = one word, which every lane reads from the same address and __ballot writes.
// No kernel waits for another workgroup.
#pragma once

#include "components_kernels.h"

namespace arvx {

constexpr int kSegRange = 0, kSegPlate = 1;  // ARVX_SEGMENT_RANGE / _PLATE

// the bits of word xw of a row that are pixels
__device__ __forceinline__ unsigned long long seg_valid(const BitGrid &g, int xw) {
    const int left = g.X - 64 * xw;
    return left >= 64 ? ~0ull : (1ull << left) - 1ull;
}

// twelve bytes from any address: four aligned words, shifted into place (the first and the last hold
// a byte of the twelve, so no load leaves the words the image occupies)
__device__ __forceinline__ void seg_load12(const uint8_t *p, uint32_t w[3]) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t *q = (const uint32_t *)(a & ~(uintptr_t)3);
    const int sh = (int)(a & 3) * 8;
    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
    if (sh == 0) {
        w[0] = d0;
        w[1] = d1;
        w[2] = d2;
    } else {
        const uint32_t d3 = q[3];
        w[0] = (d0 >> sh) | (d1 << (32 - sh));
        w[1] = (d1 >> sh) | (d2 << (32 - sh));
        w[2] = (d2 >> sh) | (d3 << (32 - sh));
    }
}

struct SegRule {
    int rule;
    uint32_t lo, hi;  // B | G << 8 | R << 16
    int threshold;
};

__device__ __forceinline__ bool seg_foreground(const SegRule &r, const uint8_t *p, const uint8_t *plate) {
    if (r.rule == kSegRange) {
        bool bg = true;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            bg = bg && (uint32_t)p[c] >= ((r.lo >> (8 * c)) & 0xffu) && (uint32_t)p[c] <= ((r.hi >> (8 * c)) & 0xffu);
        return !bg;
    }
    int d = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int e = (int)p[c] - (int)plate[c];
        d = max(d, e < 0 ? -e : e);
    }
    return d > r.threshold;
}

// sixteen lanes per word, four pixels per lane.  plate_stride: bytes between the views' plates (0: one
// plate for all)
__global__ __launch_bounds__(256) void seg_rule_kernel(const uint8_t *__restrict__ images,
                                                       const uint8_t *__restrict__ plates, size_t plate_stride,
                                                       const BitGrid g, const SegRule r,
                                                       unsigned long long *__restrict__ out) {
    const size_t nwords = (size_t)g.XW * g.Y * g.Z;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t wi = t >> 4;
    const int q = (int)(t & 15);
    unsigned long long nib = 0ull;
    if (wi < nwords) {
        const int xw = (int)(wi % g.XW);
        const size_t row = wi / g.XW;  // view * H + y
        const int x = 64 * xw + 4 * q;
        if (x < g.X) {
            const size_t view = row / g.Y;
            const size_t in_view = (row % g.Y) * (size_t)g.X + x;
            const uint8_t *src = images + (row * (size_t)g.X + x) * 3;
            const uint8_t *pl = r.rule == kSegPlate ? plates + view * plate_stride + in_view * 3 : nullptr;
            if (x + 3 < g.X) {
                uint32_t a[3], b[3] = {0u, 0u, 0u};
                seg_load12(src, a);
                if (pl) seg_load12(pl, b);
                const uint8_t *pa = reinterpret_cast<const uint8_t *>(a);
                const uint8_t *pb = reinterpret_cast<const uint8_t *>(b);
#pragma unroll
                for (int j = 0; j < 4; ++j) nib |= (seg_foreground(r, pa + 3 * j, pb + 3 * j) ? 1ull : 0ull) << j;
            } else {
                for (int j = 0; x + j < g.X; ++j)
                    nib |= (seg_foreground(r, src + 3 * j, pl ? pl + 3 * j : src) ? 1ull : 0ull) << j;
            }
        }
    }
    unsigned long long word = nib << (4 * q);
    word |= __shfl_xor(word, 1);
    word |= __shfl_xor(word, 2);
    word |= __shfl_xor(word, 4);
    word |= __shfl_xor(word, 8);
    if (q == 0 && wi < nwords) out[wi] = word;
}

// grid (words of a view / 256, views); counts: 8 words per view, this step's at `slot`
__global__ __launch_bounds__(256) void seg_count_kernel(const unsigned long long *__restrict__ plane,
                                                        const BitGrid g, unsigned long long *__restrict__ counts,
                                                        int slot) {
    const size_t per_view = (size_t)g.XW * g.Y;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    int n = w < per_view ? __popcll(plane[blockIdx.y * per_view + w]) : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(counts + 8 * (size_t)blockIdx.y + slot, (unsigned long long)n);
}

// word xw of row y of view z as if the plane were shifted: bit b = pixel (64 xw + b + sx, y + sy);
// pixels outside the image read as `fill` (0 or ~0)
__device__ __forceinline__ unsigned long long seg_shifted(const unsigned long long *__restrict__ plane,
                                                          const BitGrid &g, unsigned long long fill, int xw,
                                                          int y, int z, int sx, int sy) {
    const int yy = y + sy;
    if (yy < 0 || yy >= g.Y) return fill;
    const unsigned long long *row = plane + ((size_t)z * g.Y + yy) * g.XW;
    const int o = 64 * xw + sx;
    const int k = o >> 6, sh = o & 63;  // (arithmetic shift: floor)
    const auto word = [&](int j) -> unsigned long long {
        if (j < 0 || j >= g.XW) return fill;
        return row[j] | (fill & ~seg_valid(g, j));
    };
    const unsigned long long lo = word(k);
    if (sh == 0) return lo;
    return (lo >> sh) | (word(k + 1) << (64 - sh));
}

// one word per thread: out = op over i < n of the plane shifted by (sx0 + i dsx, sy0 + i dsy)
__global__ __launch_bounds__(256) void seg_combine_kernel(const unsigned long long *__restrict__ in,
                                                          unsigned long long *__restrict__ out, const BitGrid g,
                                                          int op_and, int n, int sx0, int dsx, int sy0, int dsy) {
    const size_t nwords = (size_t)g.XW * g.Y * g.Z;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const int xw = (int)(w % g.XW);
    const size_t row = w / g.XW;
    const int y = (int)(row % g.Y), z = (int)(row / g.Y);
    const unsigned long long fill = op_and ? ~0ull : 0ull;
    unsigned long long acc = fill;
    for (int i = 0; i < n; ++i) {
        const unsigned long long s = seg_shifted(in, g, fill, xw, y, z, sx0 + i * dsx, sy0 + i * dsy);
        acc = op_and ? acc & s : acc | s;
    }
    out[w] = acc & seg_valid(g, xw);
}

// ---- labelling: one lane per bit of the padded rows ---------------------------------------------

struct SegLane {
    bool live;  // a pixel
    size_t wi;  // its word
    int b, x, y, z;
    int p;      // (z * H + y) * W + x
};
__device__ __forceinline__ SegLane seg_lane(const BitGrid &g) {
    SegLane l;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    l.wi = t >> 6;
    l.b = (int)(t & 63);
    const int xw = (int)(l.wi % g.XW);
    const size_t row = l.wi / g.XW;
    l.x = 64 * xw + l.b;
    l.y = (int)(row % g.Y);
    l.z = (int)(row / g.Y);
    l.live = l.wi < (size_t)g.XW * g.Y * g.Z && l.x < g.X;
    l.p = l.live ? (int)(row * (size_t)g.X + l.x) : -1;
    return l;
}

// 1 / 0: the pixel's bit; -1: outside the image
__device__ __forceinline__ int seg_bit(const unsigned long long *__restrict__ plane, const BitGrid &g, int x,
                                       int y, int z) {
    if (x < 0 || x >= g.X || y < 0 || y >= g.Y) return -1;
    return (int)((plane[((size_t)z * g.Y + y) * g.XW + (x >> 6)] >> (x & 63)) & 1ull);
}

// which: 1 the foreground is labelled, 2 the background, 3 both
__global__ __launch_bounds__(256) void seg_init_kernel(const unsigned long long *__restrict__ plane,
                                                       const BitGrid g, int which, int *__restrict__ L) {
    const SegLane l = seg_lane(g);
    if (!l.live) return;
    const unsigned long long w = plane[l.wi];
    const bool fg = (w >> l.b) & 1ull;
    int v = -1;
    if (which & (fg ? 1 : 2)) {
        // the pixels of the other kind below b: the run starts behind the highest of them
        const unsigned long long other = (fg ? ~w : w) & ((1ull << l.b) - 1ull);
        const int start = other ? 64 - __clzll((long long)other) : 0;
        v = l.p - (l.b - start);
    }
    L[l.p] = v;
}

__global__ __launch_bounds__(256) void seg_link_kernel(const unsigned long long *__restrict__ plane,
                                                       const BitGrid g, int which, int *__restrict__ L) {
    const SegLane l = seg_lane(g);
    if (!l.live) return;
    const int c = seg_bit(plane, g, l.x, l.y, l.z);
    if (!(which & (c ? 1 : 2))) return;
    // x - 1: inside a word the run is one tree already
    const bool left = seg_bit(plane, g, l.x - 1, l.y, l.z) == c;
    if (l.b == 0 && left) comp_unite(L, l.p, l.p - 1);
    // y - 1: where x - 1 has the pixel's kind in both rows, its lane makes the same union
    const bool up = seg_bit(plane, g, l.x, l.y - 1, l.z) == c;
    if (up && !(left && seg_bit(plane, g, l.x - 1, l.y - 1, l.z) == c)) comp_unite(L, l.p, l.p - g.X);
    if (c == 1) {
        // the two backward diagonals, only where neither pixel between them is foreground (they unite
        // the pair by row and column steps otherwise)
        if (!left && !up && seg_bit(plane, g, l.x - 1, l.y - 1, l.z) == 1) comp_unite(L, l.p, l.p - g.X - 1);
        if (!up && seg_bit(plane, g, l.x + 1, l.y, l.z) != 1 && seg_bit(plane, g, l.x + 1, l.y - 1, l.z) == 1)
            comp_unite(L, l.p, l.p - g.X + 1);
    }
}

// one pixel per thread; the links are final (they were made in the launch before)
__global__ __launch_bounds__(256) void seg_roots_kernel(int *__restrict__ L, int n) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)n || comp_load(L + p) < 0) return;
    const int root = comp_find(L, (int)p);
    if (root != (int)p) __hip_atomic_store(L + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr unsigned kSegBorder = 0x80000000u;  // of an area word: a pixel of the component is on the border

// One pixel per thread, workgroups of 1024.  A component that covers most of the image -- the background
// around a silhouette -- would take one atomic per wave on ONE word; so the pixels of the workgroup's
// least root (the component that began first and still reaches here: the large one, as a rule) are
// counted in LDS and added once per workgroup, and only the other roots go out wave by wave, the lanes
// that share one adding once.  area: zeroed, one word per pixel, used at the roots.
constexpr int kSegAreaBlock = 1024;
__global__ __launch_bounds__(kSegAreaBlock) void seg_area_kernel(const int *__restrict__ L, int n, int W, int H,
                                                                 unsigned *__restrict__ area) {
    __shared__ int s_root;
    __shared__ unsigned s_count, s_border;
    const size_t p = (size_t)blockIdx.x * kSegAreaBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) {
        s_root = 0x7fffffff;
        s_count = 0u;
        s_border = 0u;
    }
    __syncthreads();
    int root = -1;
    bool border = false;
    if (p < (size_t)n) {
        root = L[p];
        const int x = (int)(p % W), y = (int)((p / W) % H);
        border = x == 0 || x == W - 1 || y == 0 || y == H - 1;
    }
    if (root >= 0) atomicMin(&s_root, root);
    __syncthreads();
    const int shared_root = s_root;
    const bool mine = root >= 0 && root == shared_root;
    const unsigned long long mm = __ballot(mine), mmb = __ballot(mine && border);
    if (lane == 0 && mm) {
        atomicAdd(&s_count, (unsigned)__popcll(mm));
        if (mmb) atomicOr(&s_border, 1u);
    }
    unsigned long long todo = __ballot(root >= 0 && !mine);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(root, lead);
        const bool same = root == r0;
        const unsigned long long m = __ballot(same);
        const unsigned long long mb = __ballot(same && border);
        if (lane == lead) {
            atomicAdd(area + r0, (unsigned)__popcll(m));
            if (mb) atomicOr(area + r0, kSegBorder);
        }
        todo &= ~m;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_count) {
        atomicAdd(area + shared_root, s_count);
        if (s_border) atomicOr(area + shared_root, kSegBorder);
    }
}

__device__ __forceinline__ unsigned long long seg_key(unsigned size, int root) {
    return ((unsigned long long)size << 32) | (uint32_t)~root;
}

// best: one word per view of the batch, zeroed
__global__ __launch_bounds__(256) void seg_best_kernel(const int *__restrict__ L, const unsigned *__restrict__ area,
                                                       int n, int view_pixels, long long min_area,
                                                       unsigned long long *__restrict__ best) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)n || L[p] != (int)p) return;
    const unsigned size = area[p] & ~kSegBorder;
    if ((long long)size >= min_area) atomicMax(best + p / view_pixels, seg_key(size, (int)p));
}

// Step 4 in place.  counts: the batch's first view's eight words; [4] components removed, [5] their pixels
__global__ __launch_bounds__(256) void seg_specks_kernel(unsigned long long *__restrict__ plane, const BitGrid g,
                                                         const int *__restrict__ L,
                                                         const unsigned *__restrict__ area, long long min_area,
                                                         int largest, const unsigned long long *__restrict__ best,
                                                         unsigned long long *__restrict__ counts) {
    const SegLane l = seg_lane(g);
    bool keep = false;
    if (l.live && ((plane[l.wi] >> l.b) & 1ull)) {
        const int root = L[l.p];
        const unsigned size = area[root] & ~kSegBorder;
        keep = (long long)size >= min_area && (!largest || seg_key(size, root) == best[l.z]);
        if (!keep && root == l.p) {
            atomicAdd(counts + 8 * (size_t)l.z + 4, 1ull);
            atomicAdd(counts + 8 * (size_t)l.z + 5, (unsigned long long)size);
        }
    }
    const unsigned long long word = __ballot(keep);
    if (l.b == 0 && l.wi < (size_t)g.XW * g.Y * g.Z) plane[l.wi] = word;
}

// Step 5 in place.  counts: [6] holes filled, [7] their pixels
__global__ __launch_bounds__(256) void seg_holes_kernel(unsigned long long *__restrict__ plane, const BitGrid g,
                                                        const int *__restrict__ L,
                                                        const unsigned *__restrict__ area, long long max_hole,
                                                        unsigned long long *__restrict__ counts) {
    const SegLane l = seg_lane(g);
    const bool in = l.wi < (size_t)g.XW * g.Y * g.Z;
    const unsigned long long w = in ? plane[l.wi] : 0ull;
    bool fill = false;
    if (l.live && !((w >> l.b) & 1ull)) {
        const int root = L[l.p];
        const unsigned a = area[root];
        const unsigned size = a & ~kSegBorder;
        fill = !(a & kSegBorder) && (max_hole < 0 || (long long)size <= max_hole);
        if (fill && root == l.p) {
            atomicAdd(counts + 8 * (size_t)l.z + 6, 1ull);
            atomicAdd(counts + 8 * (size_t)l.z + 7, (unsigned long long)size);
        }
    }
    const unsigned long long add = __ballot(fill);
    if (l.b == 0 && in) plane[l.wi] = w | add;
}

// grid (bgWords / 256, views): one 32-bit word of the flat plane per thread, padding included -- the
// pixels 32 j .. 32 j + 31, which lie in one work row or, where rows end inside the word, in several
__global__ __launch_bounds__(256) void seg_publish_kernel(const unsigned long long *__restrict__ plane,
                                                          const BitGrid g, uint32_t *__restrict__ bg, int bgWords) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= (size_t)bgWords) return;
    const int z = blockIdx.y;
    const size_t i = 32 * j;
    uint32_t out = 0u;
    if (i < (size_t)g.X * g.Y) {
        int y = (int)(i / g.X), x = (int)(i % g.X);
        for (int filled = 0; filled < 32 && y < g.Y; x = 0, ++y) {
            const int take = min(32 - filled, g.X - x);
            const unsigned long long *row = plane + ((size_t)z * g.Y + y) * g.XW;
            const int k = x >> 6, sh = x & 63;
            unsigned long long w = row[k] >> sh;
            if (sh + take > 64) w |= row[k + 1] << (64 - sh);  // (the pixels go on in the next word of the row)
            const uint32_t mask = take == 32 ? 0xffffffffu : (1u << take) - 1u;
            out |= (~(uint32_t)w & mask) << filled;
            filled += take;
        }
    }
    bg[(size_t)z * bgWords + j] = out;
}

__global__ __launch_bounds__(256) void seg_bytes_kernel(const unsigned long long *__restrict__ plane, const BitGrid g,
                                                        int z, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.X * g.Y) return;
    out[i] = seg_bit(plane, g, (int)(i % g.X), (int)(i / g.X), z) == 1 ? 255 : 0;
}

}  // namespace arvx
