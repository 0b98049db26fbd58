// components_kernels.h -- connected components of the occupied voxels (arvx_components,
// arvx_components_keep; definition in include/arvx/arvx.h): label equivalence, union-find by least
// flat index, on the occupancy bit plane of bitplane_kernels.h.
//
//   comp_init_kernel      L[i] = the first voxel of i's run inside its 64-bit word; -1 where empty
//   comp_link_kernel      unions every occupied voxel with its occupied "backward" neighbours (flat
//                         index below its own: 3 under connectivity 6, 13 under 26), but for the
//                         unions that others are certain to make
//   comp_roots_kernel     (next launch) L[i] = i's root; the plane of the roots, counted per chunk
//                         for the ordered compaction (bit_compact_counted_kernel): the list of
//                         roots IS the table's labels, ascending
//   comp_sizes_kernel     size[k] += voxels whose root is the k-th root
//   comp_best_kernel      the largest component: one 64-bit max of size << 32 | ~label
//   comp_decide_kernel    keep[k] by the rule of arvx_components_keep; the two counts
//   comp_remove_kernel    the plane of the voxels whose component goes (rec_andnot_bitgrid_kernel
//                         takes it off the records)
//   comp_publish_kernel   the two counts into the host's count words
//
// The invariant: L[i] <= i for every occupied voxel, L[i] is a voxel of i's component, and L[i] only
// ever decreases.  So every walk up the parents is bounded by a strictly decreasing index, the root
// of a tree is its least index, and once every adjacent pair has been united a component is one
// tree whose root is the label of the definition.  No thread waits for another: a union that loses
// its race learns so from what its atomicMin returned and goes on from there.
//
// Visibility inside the link launch: parents are read with relaxed agent-scope atomic loads, which
// may still return an older -- larger -- parent than the one another XCD has just stored.  Any value
// L[i] ever held satisfies the invariant, so a stale parent only lengthens the walk; a voxel is taken
// for a root, and hung under another, only by the value the atomicMin on it returned.  The compress
// pass runs in the next launch and relies on that boundary for the links.
#pragma once

#include "bitplane_kernels.h"

namespace arvx {

__device__ __forceinline__ int comp_load(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of a's tree as far as this thread can see: each hop reads L[a] < a
__device__ __forceinline__ int comp_find(const int *__restrict__ L, int a) {
    for (;;) {
        const int p = comp_load(L + a);
        if (p >= a || p < 0) return a;  // (p == a: a root; the other two never happen among occupied voxels)
        a = p;
    }
}

// One tree out of a's and b's.  Each round hangs the larger root under the smaller with an
// atomicMin; if the larger one was no root any more, the atomic returned its parent -- below it --
// and the round starts again from there: max(a, b) strictly decreases.
__device__ __forceinline__ void comp_unite(int *__restrict__ L, int a, int b) {
    for (;;) {
        a = comp_find(L, a);
        b = comp_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(L + a, b);
        if (old == a) return;  // a was a root: it hangs under b now
        // a had the parent `old` < a: L[a] = min(old, b) now, and old's and b's trees are still to be united
        a = old;
    }
}

__device__ __forceinline__ bool comp_occ(const unsigned long long *__restrict__ occ, const BitGrid &g,
                                         int x, int y, int z) {
    if (x < 0 || x >= g.X || y < 0 || y >= g.Y || z < 0 || z >= g.Z) return false;
    return (occ[((size_t)z * g.Y + y) * g.XW + (x >> 6)] >> (x & 63)) & 1ull;
}

// one thread per voxel, flat index order
__global__ __launch_bounds__(256) void comp_init_kernel(const unsigned long long *__restrict__ occ,
                                                        const BitGrid g, int *__restrict__ L) {
    const size_t n = (size_t)g.X * g.Y * g.Z;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % g.X);
    const size_t row = i / g.X;
    const unsigned long long w = occ[row * g.XW + (x >> 6)];
    const int b = x & 63;
    int v = -1;
    if ((w >> b) & 1ull) {
        // the empty voxels of the word below b: the run starts behind the highest of them
        const unsigned long long below = ~w & ((1ull << b) - 1ull);
        const int start = below ? 64 - __clzll((long long)below) : 0;
        v = (int)i - (b - start);
    }
    L[i] = v;
}

template <int kConn>
__global__ __launch_bounds__(256) void comp_link_kernel(const unsigned long long *__restrict__ occ,
                                                        const BitGrid g, int *__restrict__ L) {
    const size_t n = (size_t)g.X * g.Y * g.Z;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % g.X);
    const size_t row = i / g.X;
    const int y = (int)(row % g.Y), z = (int)(row / g.Y);
    if (!comp_occ(occ, g, x, y, z)) return;
    const int plane = g.X * g.Y;
    // x - 1: inside a word the run is one tree already (comp_init_kernel)
    const bool left = comp_occ(occ, g, x - 1, y, z);
    if ((x & 63) == 0 && left) comp_unite(L, (int)i, (int)i - 1);
    // y - 1 and z - 1: where x - 1 is occupied in both rows, its thread makes the same union
    const bool down = comp_occ(occ, g, x, y - 1, z), back = comp_occ(occ, g, x, y, z - 1);
    if (down && !(left && comp_occ(occ, g, x - 1, y - 1, z))) comp_unite(L, (int)i, (int)i - g.X);
    if (back && !(left && comp_occ(occ, g, x - 1, y, z - 1))) comp_unite(L, (int)i, (int)i - plane);
    if (kConn == 26) {
        // The ten diagonal neighbours.  Two voxels that share an edge also meet through either of the
        // two other voxels of their 2 x 2 square, two that share a corner through any of the six
        // other voxels of their 2 x 2 x 2 cube -- by face and edge steps, which are united on their
        // own account: a diagonal is united only where all of those are empty.
        const bool right = comp_occ(occ, g, x + 1, y, z);
#pragma unroll
        for (int dx = -1; dx <= 1; dx += 2) {  // (x + dx, y - 1, z)
            const bool side = dx < 0 ? left : right;
            if (!side && !down && comp_occ(occ, g, x + dx, y - 1, z)) comp_unite(L, (int)i, (int)i - g.X + dx);
        }
        const bool up = comp_occ(occ, g, x, y + 1, z);
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {  // (x + dx, y + dy, z - 1)
                if (dx == 0 && dy == 0) continue;
                if (!comp_occ(occ, g, x + dx, y + dy, z - 1)) continue;
                bool bridge = back;
                if (dx != 0) bridge = bridge || (dx < 0 ? left : right);
                if (dy != 0) bridge = bridge || (dy < 0 ? down : up);
                if (dx != 0 && dy != 0)
                    bridge = bridge || comp_occ(occ, g, x + dx, y + dy, z) || comp_occ(occ, g, x + dx, y, z - 1) ||
                             comp_occ(occ, g, x, y + dy, z - 1);
                if (!bridge) comp_unite(L, (int)i, (int)i - plane + dy * g.X + dx);
            }
    }
}

// One word per thread (the grid covers whole waves: chunk_count_add).  Every voxel of the word gets
// its root; other threads of this launch store roots over parents meanwhile, and either is a voxel
// of the tree at or below the one that was read.
__global__ __launch_bounds__(256) void comp_roots_kernel(const unsigned long long *__restrict__ occ,
                                                         const BitGrid g, int *__restrict__ L,
                                                         unsigned long long *__restrict__ roots,
                                                         int *__restrict__ counts) {
    const size_t nwords = (size_t)g.XW * g.Y * g.Z;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long r = 0ull;
    if (w < nwords) {
        unsigned long long b = occ[w];
        const int first = (int)((w / g.XW) * g.X) + (int)(w % g.XW) * 64;
        while (b) {
            const int k = __ffsll((long long)b) - 1;
            b &= b - 1ull;
            const int i = first + k;
            const int root = comp_find(L, i);
            if (root == i) r |= 1ull << k;
            else __hip_atomic_store(L + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        roots[w] = r;
    }
    chunk_count_add(counts, w, __popcll(r));
}

// the place of root r in the table (the ordered compaction of the roots' plane)
__device__ __forceinline__ int comp_rank(const SparseWord *__restrict__ rank, const BitGrid &g, int r) {
    return sparse_find(SparseList{rank}, g.XW, r % g.X, (size_t)(r / g.X));
}

// One word per thread.  The voxels of a word mostly share a root, and so do the words of a wave: a
// word's runs but the last are added on their own, the last runs of a wave root by root -- one add
// per distinct root (64 rounds at the most).  Nothing is counted unless the whole table fitted
// (*total <= cap): the call runs again then.
__global__ __launch_bounds__(256) void comp_sizes_kernel(const unsigned long long *__restrict__ occ,
                                                         const BitGrid g, const int *__restrict__ L,
                                                         const SparseWord *__restrict__ rank,
                                                         const long long *__restrict__ total, long long cap,
                                                         int *__restrict__ size) {
    const size_t nwords = (size_t)g.XW * g.Y * g.Z;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (*total > cap) return;  // (the same for every thread)
    const int lane = threadIdx.x & 63;
    int run_root = -1, run = 0;
    if (w < nwords) {
        unsigned long long b = occ[w];
        const int first = (int)((w / g.XW) * g.X) + (int)(w % g.XW) * 64;
        while (b) {
            const int k = __ffsll((long long)b) - 1;
            b &= b - 1ull;
            const int root = L[first + k];
            if (root != run_root) {
                if (run) {
                    const int at = comp_rank(rank, g, run_root);
                    if (at >= 0) atomicAdd(size + at, run);
                }
                run_root = root;
                run = 0;
            }
            ++run;
        }
    }
    unsigned long long todo = __ballot(run > 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(run_root, lead);
        const bool same = run > 0 && run_root == r0;
        int v = same ? run : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (lane == lead) {
            const int at = comp_rank(rank, g, r0);
            if (at >= 0) atomicAdd(size + at, v);
        }
        todo &= ~__ballot(same);
    }
}

// ctl: [0] the greatest size << 32 | ~label, [1] components kept, [2] voxels removed
__global__ __launch_bounds__(256) void comp_best_kernel(const int *__restrict__ label,
                                                        const int *__restrict__ size,
                                                        const long long *__restrict__ total, long long cap,
                                                        unsigned long long *__restrict__ ctl) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (*total > cap || k >= *total) return;
    atomicMax(ctl, ((unsigned long long)(uint32_t)size[k] << 32) | (uint32_t)~label[k]);
}

__global__ __launch_bounds__(256) void comp_decide_kernel(const int *__restrict__ label,
                                                          const int *__restrict__ size,
                                                          const long long *__restrict__ total, long long cap,
                                                          long long min_voxels, int largest,
                                                          unsigned long long *__restrict__ ctl,
                                                          uint8_t *__restrict__ keep) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (*total > cap || k >= *total) return;
    const unsigned long long key = ((unsigned long long)(uint32_t)size[k] << 32) | (uint32_t)~label[k];
    const bool kept = (long long)size[k] >= min_voxels && (!largest || key == ctl[0]);
    keep[k] = kept ? 1 : 0;
    if (kept) atomicAdd(ctl + 1, 1ull);
    else atomicAdd(ctl + 2, (unsigned long long)size[k]);
}

// One word per thread: the voxels whose component goes.  An attempt whose table did not fit removes
// nothing (an all-zero plane).
__global__ __launch_bounds__(256) void comp_remove_kernel(const unsigned long long *__restrict__ occ,
                                                          const BitGrid g, const int *__restrict__ L,
                                                          const SparseWord *__restrict__ rank,
                                                          const uint8_t *__restrict__ keep,
                                                          const long long *__restrict__ total, long long cap,
                                                          unsigned long long *__restrict__ plane) {
    const size_t nwords = (size_t)g.XW * g.Y * g.Z;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    unsigned long long out = 0ull;
    if (*total <= cap) {
        unsigned long long b = occ[w];
        const int first = (int)((w / g.XW) * g.X) + (int)(w % g.XW) * 64;
        int run_root = -1;
        bool go = false;
        while (b) {
            const int k = __ffsll((long long)b) - 1;
            b &= b - 1ull;
            const int root = L[first + k];
            if (root != run_root) {
                run_root = root;
                const int at = comp_rank(rank, g, root);
                go = at >= 0 && keep[at] == 0;
            }
            if (go) out |= 1ull << k;
        }
    }
    plane[w] = out;
}

__global__ void comp_publish_kernel(const unsigned long long *__restrict__ ctl, long long *__restrict__ kept_host,
                                    long long *__restrict__ removed_host) {
    __hip_atomic_store(kept_host, (long long)ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(removed_host, (long long)ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace arvx
