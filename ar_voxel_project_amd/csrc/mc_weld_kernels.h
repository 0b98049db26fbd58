// mc_weld_kernels.h -- the mesh of mc_mesh_kernels.h with shared vertices (arvx_mc_mesh_welded).
//
// On the device every w is 0 or 1, so every vertex of the unwelded mesh snaps to an occupied voxel
// at the end of a cut edge: a voxel that is occupied and has an empty 6-neighbour (outside the grid
// counts as empty).  Conversely every such voxel is the model end of a cut edge, and Bourke's table
// uses every cut edge of a cell.  The distinct vertices are therefore exactly the set bits of the
// surface plane of the occupancy the cell walk reads (bit_surface_count_kernel over the records,
// closure fills included), and sorted by (z, y, x) -- Model::flatten order, x fastest -- the index
// of a vertex is its rank in that plane: the ordered compaction's SparseWord gives it with one
// 16-byte load and a popcount.  No hash and no sort.
//   mc_weld_tri_kernel     the cell walk of mc_mesh_kernel; per triangle three ranks instead of
//                          nine floats: 24 bytes out instead of 60
//   mc_weld_vertex_kernel  per vertex: its position and (optionally) its voxel's colour
#pragma once

#include "bitplane_kernels.h"
#include "mc_mesh_kernels.h"

namespace arvx {

// index of voxel (x, y, z) in the vertex list (whole grid: z is global)
__device__ __forceinline__ unsigned mc_weld_rank(const SparseList &vtx, int X, int Y, int x, int y, int z) {
    const int XW = (X + 63) >> 6;
    return (unsigned)sparse_find(vtx, XW, x, (size_t)z * Y + y);
}

// mc_mesh_kernel with indexed faces.  Per wave, through LDS (A and the launch geometry are
// mc_mesh_kernel's):
//   A  lane = cell: the cell's triangles as packed descriptors (mc_cell_descriptors);
//   B  lane = triangle: the three rank lookups, the two voxel-colour lookups and the face colour;
//   C  the wave's range streams out in whole lines: 24 bytes of face record per triangle,
//      {i0, i1, i2, r, g, b} -- the C++ layer's Triangle.
// n_cap: room in `cells`; n_dev: the cell list's length on the device; tri_cap: room for triangles
__global__ __launch_bounds__(256) void mc_weld_tri_kernel(const McMeshParams p, const SparseList vtx,
                                                          const int4 *__restrict__ cells, long long n_cap,
                                                          const long long *__restrict__ n_dev, long long tri_cap,
                                                          const int *__restrict__ tri_offset,
                                                          unsigned *__restrict__ faces) {
    // per wave and triangle: A writes {x + 1 | (y + 1) << 16, z + 1 | offset bits << 16}, B
    // replaces them with the face record {i0, i1, i2, r, g, b}
    __shared__ uint32_t s_tri[4][64 * kMeshMaxTris][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = *n_dev < n_cap ? *n_dev : n_cap;
    const long long c0 = ((long long)blockIdx.x * 4 + wave) * 64;
    if (c0 >= n) return;  // (no workgroup-wide barrier below: a wave only touches its own part)
    const long long c = c0 + lane;
    const long long clast = (c0 + 63 < n - 1) ? c0 + 63 : n - 1;
    const long long base = tri_offset[c0];
    const int ntri = (int)(tri_offset[clast] - base) + kMcTri.n[cells[clast].w & 255];
    uint32_t(*mine)[6] = s_tri[wave];
    if (c < n) mc_cell_descriptors(cells[c], (int)(tri_offset[c] - base), mine);  // ---- A
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's LDS writes have landed
    __builtin_amdgcn_wave_barrier();
    const int X = p.g.X, Y = p.g.Y;
    for (int t = lane; t < ntri; t += 64) {  // ---- B
        const uint32_t w0 = mine[t][0], w1 = mine[t][1];
        const int x = (int)(w0 & 0xffffu) - 1, y = (int)(w0 >> 16) - 1, z = (int)(w1 & 0xffffu) - 1;
        const unsigned bits = w1 >> 16;
        int vx[3], vy[3], vz[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            vx[v] = x + (int)((bits >> (3 * v)) & 1u);
            vy[v] = y + (int)((bits >> (3 * v + 1)) & 1u);
            vz[v] = z + (int)((bits >> (3 * v + 2)) & 1u);
        }
        const float3 q0 = mc_voxel_rgb(p, vx[0], vy[0], vz[0]);
        const float3 q1 = mc_voxel_rgb(p, vx[1], vy[1], vz[1]);  // col[2] = col[1], :506
#pragma unroll
        for (int v = 0; v < 3; ++v) mine[t][v] = mc_weld_rank(vtx, X, Y, vx[v], vy[v], vz[v]);
        mine[t][3] = mc_mean3(q0.x, q1.x, q1.x);
        mine[t][4] = mc_mean3(q0.y, q1.y, q1.y);
        mine[t][5] = mc_mean3(q0.z, q1.z, q1.z);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    unsigned *fo = faces + 6 * base;  // ---- C
    for (int i = lane; i < 6 * ntri; i += 64) {
        const int t = i / 6, f = i - 6 * t;
        if (base + t >= tri_cap) continue;  // (no room: the caller repeats the launch with more)
        fo[i] = mine[t][f];
    }
}

// Vertex k of the list (index[k]: its flat voxel index, ascending): verts[3k..3k+2] = x, y, z
// (voxel units) and, when rgb is not null, rgb[3k..3k+2] = the voxel's colour as mc_mesh_kernel
// reads it (mc_voxel_rgb).  One vertex per lane; a wave's 64 vertices leave as 768 consecutive
// bytes per array (lane i stores component i % 3 of vertex i / 3, handed over by a lane shuffle).
// n_cap: room in `index` and the outputs; n_dev: the list's length on the device
__global__ __launch_bounds__(256) void mc_weld_vertex_kernel(const McMeshParams p,
                                                             const int *__restrict__ index, long long n_cap,
                                                             const long long *__restrict__ n_dev,
                                                             float *__restrict__ verts,
                                                             float *__restrict__ rgb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = *n_dev < n_cap ? *n_dev : n_cap;
    const long long k0 = ((long long)blockIdx.x * 4 + wave) * 64;
    if (k0 >= n) return;
    const long long k = k0 + lane;
    const int cnt = (int)(n - k0 < 64 ? n - k0 : 64);
    const int X = p.g.X, Y = p.g.Y;
    const int flat = k < n ? index[k] : 0;
    const int x = flat % X, row = flat / X;
    const int y = row % Y, z = row / Y;
    float3 c = make_float3(0.f, 0.f, 0.f);
    if (rgb && k < n) c = mc_voxel_rgb(p, x, y, z);
    float *vo = verts + 3 * k0;
    float *co = rgb ? rgb + 3 * k0 : nullptr;
#pragma unroll
    for (int r = 0; r < 3; ++r) {  // (every lane takes part in the shuffles)
        const int i = lane + 64 * r, j = i / 3, comp = i - 3 * j;
        const int sx = __shfl(x, j), sy = __shfl(y, j), sz = __shfl(z, j);
        if (i < 3 * cnt) vo[i] = (float)(comp == 0 ? sx : comp == 1 ? sy : sz);
        if (co) {
            const float cx = __shfl(c.x, j), cy = __shfl(c.y, j), cz = __shfl(c.z, j);
            if (i < 3 * cnt) co[i] = comp == 0 ? cx : comp == 1 ? cy : cz;
        }
    }
}

}  // namespace arvx
