// mesh_relax_kernels.h -- Taubin smoothing and vertex normals on ANY indexed triangle mesh
// (arvx_mesh_relax, arvx_mesh_relax_triangles; the definition is arvx_mc_mesh_smooth's, in
// include/arvx/arvx.h).
//
// mc_smooth_kernels.h gets its adjacency from the lattice.  Here a vertex may have any valence, a
// face may come more than once and may repeat a corner, so the neighbour CSR and the incidence CSR
// are counted, filled in arrival order and then put in order row by row:
//   mesh_relax_count_kernel      per face: a neighbour slot per ordered pair (u, w) of its DISTINCT
//                                corners (at most 6; (i, i, j) gives one to i and one to j) and,
//                                for a face with three distinct corners, one incidence per corner
//   (scan_lookback_kernel        both offset arrays; V + 1 counts whose last is 0)
//   mesh_relax_fill_kernel       per face: the same slots, taken by atomics (the counts count down
//                                to 0)
//   mesh_relax_rows_kernel       per vertex: a row of at most kRelaxLaneRow slots is sorted -- and a
//                                neighbour row made unique -- by its lane in a column of LDS, as
//                                mc_smooth_sort_kernel does; a longer row is listed
//   mesh_relax_long_rows_kernel  per listed row, one workgroup: a row of at most kRelaxBlockRow
//                                slots in LDS, a longer one in place in global memory; the same
//                                sorting network and the same unique pass either way
// A neighbour row is NOT compacted after the unique pass: row i is [off[i], off[i] + degree[i]),
// which mesh_relax_step_kernel reads.  The incidence rows keep their length, so
// mc_smooth_cross_kernel and mc_smooth_normal_kernel run on them as they are.
// Faces with a repeated corner have c_t = (+-0, +-0, +-0), which changes no sum that starts at +0,
// so they have no incidences (as in mc_smooth_kernels.h).  No result depends on the order the
// atomics arrive in: the rows are sorted, and every sum is one lane's, in row order.
#pragma once

#include "mc_smooth_kernels.h"

namespace arvx {

constexpr int kRelaxLaneRow = 48;      // slots a lane sorts in its LDS column (mc_smooth_sort_kernel's row)
constexpr int kRelaxBlockRow = 8192;   // slots a workgroup sorts in LDS (32 KiB); longer rows: global memory

// the distinct corners of face t, in corner order; 0 for a face that indexes no vertex (never)
__device__ __forceinline__ int mesh_relax_corners(const unsigned *__restrict__ faces, long long t, long long V,
                                                  unsigned &d0, unsigned &d1, unsigned &d2) {
    const unsigned a = faces[6 * t], b = faces[6 * t + 1], c = faces[6 * t + 2];
    d0 = d1 = d2 = a;
    if (a >= V || b >= V || c >= V) return 0;
    int n = 1;
    if (b != a) {
        d1 = b;
        n = 2;
    }
    if (c != a && c != b) {
        if (n == 1) d1 = c;
        else d2 = c;
        ++n;
    }
    return n;
}

// ncount, icount (zeroed): neighbour slots and incidences per vertex
__global__ __launch_bounds__(256) void mesh_relax_count_kernel(const unsigned *__restrict__ faces, long long T,
                                                               long long V, int *__restrict__ ncount,
                                                               int *__restrict__ icount) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    unsigned d[3];
    const int n = mesh_relax_corners(faces, t, V, d[0], d[1], d[2]);
    if (n < 2) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= n) break;
        atomicAdd(ncount + d[k], n - 1);
        if (n == 3) atomicAdd(icount + d[k], 1);
    }
}

// every slot the count kernel counted, taken in arrival order (ncount, icount: the counts; they
// count down to 0); ncap, icap: entries of nbr and inc
__global__ __launch_bounds__(256) void mesh_relax_fill_kernel(const unsigned *__restrict__ faces, long long T,
                                                              long long V, int *__restrict__ ncount,
                                                              int *__restrict__ icount,
                                                              const int *__restrict__ noff,
                                                              const int *__restrict__ ioff, long long ncap,
                                                              long long icap, unsigned *__restrict__ nbr,
                                                              unsigned *__restrict__ inc) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    unsigned d[3];
    const int n = mesh_relax_corners(faces, t, V, d[0], d[1], d[2]);
    if (n < 2) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= n) break;
        long long o = (long long)noff[d[k]] + atomicSub(ncount + d[k], n - 1) - (n - 1);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            if (m == k || m >= n) continue;
            if (o >= 0 && o < ncap) nbr[o] = d[m];
            ++o;
        }
        if (n == 3) {
            const long long p = (long long)ioff[d[k]] + atomicSub(icount + d[k], 1) - 1;
            if (p >= 0 && p < icap) inc[p] = (unsigned)t;
        }
    }
}

// Rows of at most kRelaxLaneRow slots, a lane each: ascending, and with Unique each entry once, the
// row's new length to degree[i] (the row is not moved).  A longer row goes to the list (rows: its
// vertex; *n_rows (zeroed): their number; room for every row that can be that long).
template <bool Unique>
__global__ __launch_bounds__(256) void mesh_relax_rows_kernel(const int *__restrict__ off, long long V,
                                                              long long cap, unsigned *__restrict__ list,
                                                              int *__restrict__ degree, int *__restrict__ rows,
                                                              int *__restrict__ n_rows, int rows_cap) {
    __shared__ unsigned s_row[kRelaxLaneRow][256];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    int o, o1;
    mc_smooth_row(off, i, cap, o, o1);
    const int n = o1 - o;
    if (n > kRelaxLaneRow) {
        const int r = atomicAdd(n_rows, 1);
        if (r < rows_cap) rows[r] = (int)i;  // (always: the list has room for cap / kRelaxLaneRow rows)
        return;
    }
    int m = n;
    if (n > 1) {
        unsigned *col = &s_row[0][threadIdx.x];
        for (int k = 0; k < n; ++k) col[k * 256] = list[o + k];
        mc_smooth_sort_row(col, 256, n);
        if (Unique) {
            m = 1;
            for (int k = 1; k < n; ++k) {
                const unsigned e = col[k * 256];
                if (e != col[(m - 1) * 256]) col[m++ * 256] = e;
            }
        }
        for (int k = 0; k < m; ++k) list[o + k] = col[k * 256];
    }
    if (Unique) degree[i] = m;
}

// a[0 .. n) ascending, by the 256 threads of a workgroup: the bitonic network in the form whose
// comparators all point the same way (the first step of every merge compares mirrored places), so
// that places n and above count as +infinity without existing.  a: LDS or global memory.
__device__ __forceinline__ void mesh_relax_sort_block(unsigned *a, int n) {
    unsigned half = 1;  // half the power of two that holds n
    while (2 * half < (unsigned)n) half *= 2;
    for (unsigned k = 2; (k >> 1) < (unsigned)n; k <<= 1) {
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned t = threadIdx.x; t < half; t += 256) {
                const unsigned lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const unsigned hi = j == (k >> 1) ? lo ^ (k - 1) : lo | j;
                if (hi < (unsigned)n) {
                    const unsigned x = a[lo], y = a[hi];
                    if (x > y) {
                        a[lo] = y;
                        a[hi] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// the distinct values of the ascending a[0 .. n), in order, to out; their number.  out may be a:
// an entry goes to a place at or before its own, and a tile of 256 is read before any of it is
// written.  s_cnt: four ints of LDS
__device__ __forceinline__ int mesh_relax_unique_block(const unsigned *a, int n, unsigned *out, int *s_cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int t0 = 0; t0 < n; t0 += 256) {
        const int k = t0 + (int)threadIdx.x;
        unsigned v = 0;
        bool first = false;
        if (k < n) {
            v = a[k];
            first = k == 0 || a[k > 0 ? k - 1 : 0] != v;  // (no address below a[0] is ever formed)
        }
        const unsigned long long b = __ballot(first);
        if (lane == 0) s_cnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = s_cnt[w];
            if (w < wave) before += c;
            total += c;
        }
        if (first) out[base + before + __popcll(b & ((1ull << lane) - 1ull))] = v;
        base += total;
        __syncthreads();
    }
    return base;
}

// The listed rows, a workgroup each (the grid strides over the list): sorted, with Unique made
// unique and degree[i] written.
template <bool Unique>
__global__ __launch_bounds__(256) void mesh_relax_long_rows_kernel(const int *__restrict__ off, long long V,
                                                                   long long cap, unsigned *list,
                                                                   int *__restrict__ degree,
                                                                   const int *__restrict__ rows,
                                                                   const int *__restrict__ n_rows, int rows_cap) {
    __shared__ unsigned s_row[kRelaxBlockRow];
    __shared__ int s_cnt[4];
    const int nr = min(*n_rows, rows_cap);
    for (int r = blockIdx.x; r < nr; r += gridDim.x) {
        const long long i = rows[r];
        if (i < 0 || i >= V) continue;  // (never)
        int o, o1;
        mc_smooth_row(off, i, cap, o, o1);
        const int n = o1 - o;
        unsigned *row = list + o;
        const bool lds = n <= kRelaxBlockRow;
        if (lds)
            for (int k = threadIdx.x; k < n; k += 256) s_row[k] = row[k];
        __syncthreads();
        // (the two memories each through a call of their own, never through one pointer that may be
        // either: such a pointer makes every access a flat one, and a flat access whose base register
        // lies below LDS offset 0 -- a[k - 1] for k = 0, before its instruction offset is added --
        // leaves the LDS aperture)
        int m = n;
        if (lds) {
            mesh_relax_sort_block(s_row, n);
            if (Unique) m = mesh_relax_unique_block(s_row, n, row, s_cnt);
            else
                for (int k = threadIdx.x; k < n; k += 256) row[k] = s_row[k];
        } else {
            mesh_relax_sort_block(row, n);
            if (Unique) m = mesh_relax_unique_block(row, n, row, s_cnt);
        }
        if (Unique && threadIdx.x == 0) degree[i] = m;
        __syncthreads();
    }
}

// mc_smooth_step_kernel on rows [off[i], off[i] + degree[i]); cap: entries of nbr
__global__ __launch_bounds__(256) void mesh_relax_step_kernel(const float *__restrict__ in, long long V,
                                                              const int *__restrict__ off,
                                                              const int *__restrict__ degree, long long cap,
                                                              const unsigned *__restrict__ nbr, float f,
                                                              float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const float px = in[3 * i], py = in[3 * i + 1], pz = in[3 * i + 2];
    int o0, o1;
    mc_smooth_row(off, i, cap, o0, o1);
    const int n = degree[i];
    o1 = n < 0 || n > o1 - o0 ? o0 : o0 + n;  // (never out of its row)
    if (o1 == o0) {
        out[3 * i] = px;
        out[3 * i + 1] = py;
        out[3 * i + 2] = pz;
        return;
    }
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int o = o0; o < o1; ++o) {
        size_t j = nbr[o];
        if (j >= (size_t)V) j = (size_t)i;  // (never: the list holds vertex indices)
        sx = sx + in[3 * j];
        sy = sy + in[3 * j + 1];
        sz = sz + in[3 * j + 2];
    }
    const float k = (float)(o1 - o0);
    const float dx = sx / k - px, dy = sy / k - py, dz = sz / k - pz;
    out[3 * i] = px + f * dx;
    out[3 * i + 1] = py + f * dy;
    out[3 * i + 2] = pz + f * dz;
}

}  // namespace arvx
