// mc_decimate_kernels.h -- vertex clustering of the welded mesh (arvx_mc_mesh_decimate; the
// definition is in include/arvx/arvx.h).
//
// The welded mesh of the device (mc_weld_kernels.h) has its vertices on the lattice, in (z, y, x)
// order, and the vertex plane with its SparseWord ranks is kept.  A cluster is a cube of cell^3
// voxels, so
//   - the non-empty clusters are a bit plane over the cluster grid, gathered from the vertex plane,
//     and their ordered compaction is the decimated vertex list with its own ranks;
//   - the members of a cluster, ascending, are the set bits of its box's rows in (z, y, x) order, and
//     the bits of one word are consecutive vertex indices from the word's rank on;
//   - the corners of a face are corners of ONE marching-cubes cell, so their clusters lie pairwise at
//     Chebyshev distance <= 1: a face with three distinct clusters is named by its least cluster
//     (the anchor) and an unordered pair of the anchor's 13 forward neighbours -- kDecSlots slots per
//     decimated vertex, no hash and no sort.
//   mc_decimate_plane_kernel    per word of the cluster plane: gather, write, chunk counts
//   (bit_compact_counted_kernel: the cluster list and its ranks)
//   mc_decimate_vertex_kernel   per decimated vertex: the fp32 sums over its members in order
//   mc_decimate_map_kernel      per welded vertex: its decimated index
//   mc_decimate_claim_kernel    per face with three distinct clusters: atomicMin of t into its slot
//   mc_decimate_flag_kernel     per face: 1 when its slot holds its own t
//   (scan_lookback_kernel over the flags)
//   mc_decimate_write_kernel    per surviving face: its record, in ascending t
// No float atomics: every sum runs in one thread in the order the definition gives, every fp32
// operation rounded on its own (the library builds with -ffp-contract=off, fp32 '/' is IEEE).
#pragma once

#include "bitplane_kernels.h"
#include "mc_smooth_kernels.h"

namespace arvx {

constexpr int kDecSlots = 78;  // unordered pairs of 13 forward neighbours

struct DecGrid {
    int X, Y, Z, XW;      // the voxel grid and the words of a vertex-plane row
    int cell;             // 1 .. 64
    int CX, CY, CZ, CXW;  // the cluster grid (ceil(X / cell) ...) and the words of a cluster-plane row
};

// Word w of the cluster plane: bit j of word (cxw, cy, cz) is set when a vertex lies in cluster
// (64 cxw + j, cy, cz).  The 64 clusters of a word cover 64 * cell voxels of a row: the `cell`
// vertex-plane words from cxw * cell on (a cluster may straddle two of them), in cell * cell rows.
// Every vertex-plane word is read by one thread.  counts[chunk] += the word's set bits.  The grid
// covers whole workgroups.
__global__ __launch_bounds__(256) void mc_decimate_plane_kernel(const unsigned long long *__restrict__ vtx,
                                                                const DecGrid d,
                                                                unsigned long long *__restrict__ out,
                                                                int *__restrict__ counts) {
    const size_t nwords = (size_t)d.CXW * d.CY * d.CZ;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long acc = 0ull;
    if (w < nwords) {
        const int cxw = (int)(w % d.CXW);
        const size_t crow = w / d.CXW;
        const int cy = (int)(crow % d.CY), cz = (int)(crow / d.CY);
        const int y0 = cy * d.cell, y1 = min(y0 + d.cell, d.Y);
        const int z0 = cz * d.cell, z1 = min(z0 + d.cell, d.Z);
        for (int k = 0; k < d.cell; ++k) {
            const int xw = cxw * d.cell + k;
            if (xw >= d.XW) break;
            unsigned long long a = 0ull;  // the box's rows of this word, OR-ed
            for (int z = z0; z < z1; ++z)
                for (int y = y0; y < y1; ++y) a |= vtx[((size_t)z * d.Y + y) * d.XW + xw];
            // bit b of `a` is voxel 64 k + b of the word's range: cluster (64 k + b) / cell
            while (a) {
                const int b = __ffsll((long long)a) - 1;
                const int j = (64 * k + b) / d.cell;
                acc |= 1ull << j;
                const int end = (j + 1) * d.cell - 64 * k;  // first bit of the next cluster
                if (end >= 64) break;
                a &= ~0ull << end;
            }
        }
        out[w] = acc;
    }
    chunk_count_add(counts, w, __popcll(acc));
}

// Decimated vertex k (cidx[k]: its cluster's flat index, ascending): the members of the cluster --
// the welded vertices in its box, (z, y, x) order = ascending index --, pos[3k..] = the sum of their
// q from +0 in that order, divided by their count; rgb likewise from col; members[k] = the count.
// vtx: the vertex plane's ranks; V: welded vertices; n_cap: room in cidx and the outputs; n_dev: the
// cluster list's length on the device
__global__ __launch_bounds__(256) void mc_decimate_vertex_kernel(const int *__restrict__ cidx, long long n_cap,
                                                                 const long long *__restrict__ n_dev,
                                                                 const DecGrid d, const SparseList vtx,
                                                                 long long V, const float *__restrict__ q,
                                                                 const float *__restrict__ col,
                                                                 float *__restrict__ pos, float *__restrict__ rgb,
                                                                 int *__restrict__ members) {
    const long long n = *n_dev < n_cap ? *n_dev : n_cap;
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    int cx, cy, cz;
    mc_smooth_xyz(cidx[k], d.CX, d.CY, cx, cy, cz);
    const int x0 = cx * d.cell, x1 = min(x0 + d.cell, d.X);  // [x0, x1)
    const int y0 = cy * d.cell, y1 = min(y0 + d.cell, d.Y);
    const int z0 = cz * d.cell, z1 = min(z0 + d.cell, d.Z);
    const int wlo = x0 >> 6, whi = (x1 - 1) >> 6;  // at most two words: cell <= 64
    float sx = 0.f, sy = 0.f, sz = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
    int cnt = 0;
    for (int z = z0; z < z1; ++z)
        for (int y = y0; y < y1; ++y) {
            const size_t row = (size_t)z * d.Y + y;
            for (int xw = wlo; xw <= whi; ++xw) {
                const SparseWord e = sparse_word(vtx, row * d.XW + xw);
                const int lo = max(x0 - 64 * xw, 0), hi = min(x1 - 64 * xw, 64);  // bits [lo, hi)
                const unsigned long long below = (1ull << lo) - 1ull;
                const unsigned long long upto = hi == 64 ? ~0ull : (1ull << hi) - 1ull;
                const int m = __popcll(e.bits & upto & ~below);
                long long i = (long long)e.rank + __popcll(e.bits & below);  // the first member here
                for (int j = 0; j < m; ++j, ++i) {
                    if (i < 0 || i >= V) break;  // (never: the ranks index the vertex list)
                    sx = sx + q[3 * i];
                    sy = sy + q[3 * i + 1];
                    sz = sz + q[3 * i + 2];
                    sr = sr + col[3 * i];
                    sg = sg + col[3 * i + 1];
                    sb = sb + col[3 * i + 2];
                    ++cnt;
                }
            }
        }
    const float f = (float)cnt;  // (>= 1: the cluster's bit came from a vertex)
    pos[3 * k] = sx / f;
    pos[3 * k + 1] = sy / f;
    pos[3 * k + 2] = sz / f;
    rgb[3 * k] = sr / f;
    rgb[3 * k + 1] = sg / f;
    rgb[3 * k + 2] = sb / f;
    members[k] = cnt;
}

// map[i] = the decimated index of welded vertex i (index[i]: its flat voxel index): the rank of its
// cluster in the cluster plane (clu)
__global__ __launch_bounds__(256) void mc_decimate_map_kernel(const int *__restrict__ index, long long V,
                                                              const DecGrid d, const SparseList clu,
                                                              int *__restrict__ map) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    int x, y, z;
    mc_smooth_xyz(index[i], d.X, d.Y, x, y, z);
    map[i] = sparse_find(clu, d.CXW, x / d.cell, (size_t)(z / d.cell) * d.CY + y / d.cell);
}

// the 13 forward neighbours of a cluster, in (dz, dy, dx) order: 0 .. 12, or -1 for any other offset
__device__ __forceinline__ int mc_decimate_forward(int dx, int dy, int dz) {
    if (dx < -1 || dx > 1 || dy < -1 || dy > 1 || dz < -1 || dz > 1) return -1;
    return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) - 14;  // (the centre and what lies before it: < 0)
}

// Face t mapped: m[0..2] its decimated corners.  Returns its slot in the table (anchor * kDecSlots +
// pair), -1 for a face with two equal mapped corners, -2 for what cannot be (an index outside the
// lists, clusters further apart than one): such a face is dropped.
__device__ __forceinline__ long long mc_decimate_slot(const unsigned *__restrict__ faces, long long t, long long V,
                                                      const int *__restrict__ map, const int *__restrict__ cidx,
                                                      long long n, const DecGrid &d, int m[3]) {
    const unsigned v[3] = {faces[6 * t], faces[6 * t + 1], faces[6 * t + 2]};
    if (v[0] >= V || v[1] >= V || v[2] >= V) return -2;
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = map[v[k]];
    if (m[0] < 0 || m[1] < 0 || m[2] < 0 || m[0] >= n || m[1] >= n || m[2] >= n) return -2;
    if (m[0] == m[1] || m[1] == m[2] || m[0] == m[2]) return -1;
    const int a = min(m[0], min(m[1], m[2])), c = max(m[0], max(m[1], m[2]));
    const int b = m[0] ^ m[1] ^ m[2] ^ a ^ c;
    int ax, ay, az, bx, by, bz, cx, cy, cz;
    mc_smooth_xyz(cidx[a], d.CX, d.CY, ax, ay, az);
    mc_smooth_xyz(cidx[b], d.CX, d.CY, bx, by, bz);
    mc_smooth_xyz(cidx[c], d.CX, d.CY, cx, cy, cz);
    const int fb = mc_decimate_forward(bx - ax, by - ay, bz - az);
    const int fc = mc_decimate_forward(cx - ax, cy - ay, cz - az);  // (b < c: fb < fc)
    if (fb < 0 || fc <= fb) return -2;
    return (long long)a * kDecSlots + fb * (25 - fb) / 2 + (fc - fb - 1);
}

// slots (all ones): per face with three distinct mapped corners, the least t of its corner set
__global__ __launch_bounds__(256) void mc_decimate_claim_kernel(const unsigned *__restrict__ faces, long long T,
                                                                long long V, const int *__restrict__ map,
                                                                const int *__restrict__ cidx, long long n_cap,
                                                                const long long *__restrict__ n_dev,
                                                                const DecGrid d, unsigned *__restrict__ slots) {
    const long long n = *n_dev < n_cap ? *n_dev : n_cap;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int m[3];
    const long long s = mc_decimate_slot(faces, t, V, map, cidx, n, d, m);
    if (s >= 0) atomicMin(slots + s, (unsigned)t);
}

// flags[t] = 1 when face t survives: its slot holds its own t
__global__ __launch_bounds__(256) void mc_decimate_flag_kernel(const unsigned *__restrict__ faces, long long T,
                                                               long long V, const int *__restrict__ map,
                                                               const int *__restrict__ cidx, long long n_cap,
                                                               const long long *__restrict__ n_dev,
                                                               const DecGrid d, const unsigned *__restrict__ slots,
                                                               int *__restrict__ flags) {
    const long long n = *n_dev < n_cap ? *n_dev : n_cap;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int m[3];
    const long long s = mc_decimate_slot(faces, t, V, map, cidx, n, d, m);
    flags[t] = (s >= 0 && slots[s] == (unsigned)t) ? 1 : 0;
}

// the surviving faces' records {map[i0], map[i1], map[i2], r, g, b} at their offsets (cap: room in out)
__global__ __launch_bounds__(256) void mc_decimate_write_kernel(const unsigned *__restrict__ faces, long long T,
                                                                long long V, const int *__restrict__ map,
                                                                const int *__restrict__ flags,
                                                                const int *__restrict__ off, long long cap,
                                                                unsigned *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T || !flags[t]) return;
    const long long o = off[t];
    if (o < 0 || o >= cap) return;  // (never: at most T survive)
#pragma unroll
    for (int k = 0; k < 3; ++k) out[6 * o + k] = (unsigned)map[faces[6 * t + k]];  // (a survivor's corners are in range)
#pragma unroll
    for (int k = 3; k < 6; ++k) out[6 * o + k] = faces[6 * t + k];
}

}  // namespace arvx
