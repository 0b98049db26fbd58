// mc_smooth_kernels.h -- Taubin smoothing and vertex normals on the welded mesh
// (arvx_mc_mesh_smooth; the definition is in include/arvx/arvx.h).
//
// The welded mesh of the device (mc_weld_kernels.h) has its vertices on the lattice, and the
// corners of a face are corners of ONE marching-cubes cell: every neighbour of a vertex lies at
// Chebyshev distance 1.  So the neighbour set of a vertex is a 26-bit mask over the offsets, and
// with the bits in (dz, dy, dx) order ascending bit order is ascending vertex index (vertices are
// in (z, y, x) order).  The neighbour list of a vertex is then its mask's bits, in bit order, each
// turned into a vertex index by a rank in the vertex plane (mc_weld_rank): no hash and no sort.
//
// Once per welded mesh (the CSRs; row i is [off[i], off[i + 1]), the scans run over V + 1 counts
// whose last is 0):
//   mc_smooth_adjacency_kernel   per face: neighbour bits of its corner pairs (atomicOr) and, for
//                                a face with three distinct corners, one incidence per corner
//                                (atomicAdd)
//   mc_smooth_degree_kernel      per vertex: popcount of its mask
//   mc_smooth_neighbours_kernel  per vertex: the neighbour CSR, ranks in bit order
//   mc_smooth_incidence_kernel   per face: its index into each corner's row (atomicSub)
//   mc_smooth_sort_kernel        per vertex: its row in ascending face order
// Per call:
//   mc_smooth_step_kernel        one Jacobi step p' = p + f (mean(neighbours) - p), per vertex
//   mc_smooth_cross_kernel       per face: c_t = (q2 - q0) x (q1 - q0), outward
//   mc_smooth_normal_kernel      per vertex: sum of c_t in ascending t, normalised
// Faces with a repeated corner have c_t = (+-0, +-0, +-0), which changes no sum that starts at +0,
// so they have no incidences.  Every fp32 operation is rounded on its own: the library builds
// with -ffp-contract=off, and fp32 '/' and sqrtf are correctly rounded by default.
#pragma once

#include "bitplane_kernels.h"
#include "mc_weld_kernels.h"

namespace arvx {

constexpr int kSmoothSortRow = 48;  // incidences a row sorts in LDS (a vertex has at most 40)

// bit of offset (dx, dy, dz) in {-1, 0, 1}^3 \ {0} in a neighbour mask: (dz, dy, dx) order
__device__ __forceinline__ int mc_smooth_bit(int dx, int dy, int dz) {
    const int b = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1);
    return b < 13 ? b : b - 1;
}

__device__ __forceinline__ void mc_smooth_xyz(int flat, int X, int Y, int &x, int &y, int &z) {
    x = flat % X;
    const int row = flat / X;
    y = row % Y;
    z = row / Y;
}

// faces: the welded mesh's records {i0, i1, i2, r, g, b}; index: flat voxel index per vertex;
// masks (zeroed): neighbour bits per vertex; counts (zeroed): incidences per vertex
__global__ __launch_bounds__(256) void mc_smooth_adjacency_kernel(const unsigned *__restrict__ faces,
                                                                  long long T, long long V,
                                                                  const int *__restrict__ index, int X, int Y,
                                                                  unsigned *__restrict__ masks,
                                                                  int *__restrict__ counts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const unsigned v[3] = {faces[6 * t], faces[6 * t + 1], faces[6 * t + 2]};
    if (v[0] >= V || v[1] >= V || v[2] >= V) return;  // (never: the faces index the vertex list)
    int x[3], y[3], z[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) mc_smooth_xyz(index[v[k]], X, Y, x[k], y[k], z[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = k, b = k == 2 ? 0 : k + 1;
        if (v[a] == v[b]) continue;
        const int dx = x[b] - x[a], dy = y[b] - y[a], dz = z[b] - z[a];
        // (the corners of a face are corners of one cell: |d| <= 1 always)
        if (dx < -1 || dx > 1 || dy < -1 || dy > 1 || dz < -1 || dz > 1) continue;
        atomicOr(masks + v[a], 1u << mc_smooth_bit(dx, dy, dz));
        atomicOr(masks + v[b], 1u << mc_smooth_bit(-dx, -dy, -dz));
    }
    if (v[0] != v[1] && v[1] != v[2] && v[0] != v[2]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(counts + v[k], 1);
    }
}

// degree[i] = neighbours of vertex i for i < V; degree[V] = 0 (the scan's end entry)
__global__ __launch_bounds__(256) void mc_smooth_degree_kernel(const unsigned *__restrict__ masks, long long V,
                                                               int *__restrict__ degree) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < V) degree[i] = __popc(masks[i]);
    else if (i == V) degree[V] = 0;
}

// row i of the neighbour CSR: the vertex indices of mask i's bits, in bit order (= ascending).
// vtx: the vertex plane's SparseList; cap: room in nbr
__global__ __launch_bounds__(256) void mc_smooth_neighbours_kernel(const unsigned *__restrict__ masks, long long V,
                                                                   const int *__restrict__ index, int X, int Y,
                                                                   const SparseList vtx,
                                                                   const int *__restrict__ off, long long cap,
                                                                   unsigned *__restrict__ nbr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    int x, y, z;
    mc_smooth_xyz(index[i], X, Y, x, y, z);
    unsigned m = masks[i];
    long long o = off[i];
    while (m) {
        int b = __ffs(m) - 1;
        m &= m - 1u;
        if (b >= 13) ++b;  // (the centre has no bit)
        const int dx = b % 3 - 1, dy = (b / 3) % 3 - 1, dz = b / 9 - 1;
        unsigned r = mc_weld_rank(vtx, X, Y, x + dx, y + dy, z + dz);
        if (r >= (unsigned long long)V) r = (unsigned)i;  // (cannot happen: a corner is a vertex)
        if (o < cap) nbr[o] = r;
        ++o;
    }
}

// each face with three distinct corners takes one place in each corner's row (counts: the
// incidences per vertex; they count down to 0)
__global__ __launch_bounds__(256) void mc_smooth_incidence_kernel(const unsigned *__restrict__ faces, long long T,
                                                                  long long V,
                                                                  int *__restrict__ counts,
                                                                  const int *__restrict__ off, long long cap,
                                                                  unsigned *__restrict__ inc) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const unsigned v[3] = {faces[6 * t], faces[6 * t + 1], faces[6 * t + 2]};
    if (v[0] >= V || v[1] >= V || v[2] >= V) return;
    if (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long o = (long long)off[v[k]] + atomicSub(counts + v[k], 1) - 1;
        if (o >= 0 && o < cap) inc[o] = (unsigned)t;
    }
}

// row i of a CSR of `cap` entries: [o0, o1) (the scans cannot leave a row outside the list; one
// that was would be empty)
__device__ __forceinline__ void mc_smooth_row(const int *off, long long i, long long cap, int &o0, int &o1) {
    o0 = off[i];
    o1 = off[i + 1];
    if (o0 < 0 || o1 < o0 || o1 > cap) o0 = o1 = 0;
}

// insertion sort of a[0], a[s], ..., a[(n - 1) s]
__device__ __forceinline__ void mc_smooth_sort_row(unsigned *a, int s, int n) {
    for (int k = 1; k < n; ++k) {
        const unsigned e = a[k * s];
        int j = k - 1;
        while (j >= 0 && a[j * s] > e) {
            a[(j + 1) * s] = a[j * s];
            --j;
        }
        a[(j + 1) * s] = e;
    }
}

// every row of the incidence CSR in ascending face order: in LDS (column per lane, no bank
// conflicts); a row longer than kSmoothSortRow -- none on a marching-cubes mesh -- in place
__global__ __launch_bounds__(256) void mc_smooth_sort_kernel(const int *__restrict__ off, long long V,
                                                             long long cap, unsigned *__restrict__ inc) {
    __shared__ unsigned s_row[kSmoothSortRow][256];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    int o, o1;
    mc_smooth_row(off, i, cap, o, o1);
    const int n = o1 - o;
    if (n <= 1) return;
    if (n > kSmoothSortRow) {
        mc_smooth_sort_row(inc + o, 1, n);
        return;
    }
    unsigned *col = &s_row[0][threadIdx.x];
    for (int k = 0; k < n; ++k) col[k * 256] = inc[o + k];
    mc_smooth_sort_row(col, 256, n);
    for (int k = 0; k < n; ++k) inc[o + k] = col[k * 256];
}

// one smoothing step with factor f (Jacobi: in and out are different buffers, 3V floats each);
// cap: entries of nbr
__global__ __launch_bounds__(256) void mc_smooth_step_kernel(const float *__restrict__ in, long long V,
                                                             const int *__restrict__ off, long long cap,
                                                             const unsigned *__restrict__ nbr, float f,
                                                             float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const float px = in[3 * i], py = in[3 * i + 1], pz = in[3 * i + 2];
    int o0, o1;
    mc_smooth_row(off, i, cap, o0, o1);
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

// c_t = a x b with a = q[i2] - q[i0], b = q[i1] - q[i0]: the negated cross product of the mesh's
// own winding, which points into the model
__global__ __launch_bounds__(256) void mc_smooth_cross_kernel(const unsigned *__restrict__ faces, long long T,
                                                              const float *__restrict__ q, long long V,
                                                              float *__restrict__ cross) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    size_t i0 = faces[6 * t], i1 = faces[6 * t + 1], i2 = faces[6 * t + 2];
    if (i0 >= (size_t)V || i1 >= (size_t)V || i2 >= (size_t)V) i0 = i1 = i2 = 0;  // (never)
    const float ax = q[3 * i2] - q[3 * i0], ay = q[3 * i2 + 1] - q[3 * i0 + 1], az = q[3 * i2 + 2] - q[3 * i0 + 2];
    const float bx = q[3 * i1] - q[3 * i0], by = q[3 * i1 + 1] - q[3 * i0 + 1], bz = q[3 * i1 + 2] - q[3 * i0 + 2];
    cross[3 * t] = ay * bz - az * by;
    cross[3 * t + 1] = az * bx - ax * bz;
    cross[3 * t + 2] = ax * by - ay * bx;
}

// n_i = sum of c_t over row i (ascending t) from +0; the unit normal n / |n|, or 0 when |n| == 0
// (cap: entries of inc; T: faces in cross)
__global__ __launch_bounds__(256) void mc_smooth_normal_kernel(const int *__restrict__ off, long long V,
                                                               long long cap, const unsigned *__restrict__ inc,
                                                               const float *__restrict__ cross, long long T,
                                                               float *__restrict__ normals) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    int o0, o1;
    mc_smooth_row(off, i, cap, o0, o1);
    for (int o = o0; o < o1; ++o) {
        const size_t t = inc[o];
        if (t >= (size_t)T) continue;  // (never: the list holds face indices)
        nx = nx + cross[3 * t];
        ny = ny + cross[3 * t + 1];
        nz = nz + cross[3 * t + 2];
    }
    const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (l == 0.f) {
        nx = ny = nz = 0.f;
    } else {
        nx = nx / l;
        ny = ny / l;
        nz = nz / l;
    }
    normals[3 * i] = nx;
    normals[3 * i + 1] = ny;
    normals[3 * i + 2] = nz;
}

}  // namespace arvx
