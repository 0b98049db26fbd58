// mc_refine_kernels.h -- the marching-cubes mesh with one vertex per cut edge, placed where the
// edge leaves the visual hull (arvx_mc_mesh_refined; arvx.h has the definition).
//
// A cut edge is a lattice edge with exactly one occupied end.  Its lower end q lies in
// [-1, X) x [-1, Y) x [-1, Z) and its axis a in {0, 1, 2}; the vertices are sorted by
// (((q.z+1)(Y+1) + (q.y+1))(X+1) + (q.x+1)) * 3 + a.  That key is the flat index of bit
// 3 (q.x+1) + a of row (q.y+1, q.z+1) of a bit plane with 3 (X+1) bits per row, (Y+1)(Z+1) rows:
// the EDGE PLANE, in the layout of bitplane_kernels.h.  So the ordered compaction of that plane is
// the vertex list (its entries are the keys), and a vertex's index is the rank of its bit: the
// compaction's SparseWord gives it with one 16-byte load and a popcount, as mc_weld ranks its
// vertex plane.  No hash and no sort.
//   mc_refine_plane_kernel   the edge plane from the occupancy plane, with its chunk counts
//   mc_refine_tri_kernel     the cell walk of mc_mesh_kernel; per triangle the ranks of its three
//                            cut edges and mc_mesh_kernel's face colour: 24-byte face records
//   mc_refine_vertex_kernel  per cut edge: the inside tests of its ends, the bisection, the vertex,
//                            its colour, and the edge's description
#pragma once

#include "bitplane_kernels.h"
#include "mc_mesh_kernels.h"

namespace arvx {

// the edge plane over the lower ends of an X x Y x Z grid
__host__ __device__ __forceinline__ BitGrid refine_edge_grid(int X, int Y, int Z) {
    return BitGrid{3 * (X + 1), Y + 1, Z + 1, (3 * (X + 1) + 63) / 64};
}

// bits x0 .. x0 + 31 of row (y, z) of an occupancy plane; x0 >= -1; zeros outside the grid (the
// plane's padding bits are zero)
__device__ __forceinline__ uint32_t refine_occ_window(const unsigned long long *__restrict__ occ,
                                                      const BitGrid &g, int x0, int y, int z) {
    if (y < 0 || y >= g.Y || z < 0 || z >= g.Z) return 0u;
    const int xs = x0 + 64;  // (a zero word stands before the row)
    const int wi = (xs >> 6) - 1, sh = xs & 63;
    unsigned long long v = bit_word(occ, g, wi, y, z) >> sh;
    if (sh) v |= bit_word(occ, g, wi + 1, y, z) << (64 - sh);
    return (uint32_t)v;
}

// bit i of v (i < 21) to bit 3 i
__device__ __forceinline__ unsigned long long refine_spread3(uint32_t v) {
    unsigned long long x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
// bits 3 i + a of the result: bit i of cx, cy, cz for a = 0, 1, 2 (i < 21)
__device__ __forceinline__ unsigned long long refine_interleave3(uint32_t cx, uint32_t cy, uint32_t cz) {
    return refine_spread3(cx) | (refine_spread3(cy) << 1) | (refine_spread3(cz) << 2);
}

// edge = occ XOR occ shifted one step along the axis, the three axes of a lower end interleaved;
// counts[chunk] += its set bits.  One word of the edge plane per thread; a word covers at most 23
// lower ends of one row, so three 32-bit windows of the occupancy (the row, the next row along y,
// the next along z) hold everything it reads: their XORs, interleaved three bits per lower end and
// shifted to where the word starts inside its first lower end.  The grid covers whole workgroups.
__global__ __launch_bounds__(256) void mc_refine_plane_kernel(const unsigned long long *__restrict__ occ,
                                                              const BitGrid g, const BitGrid eg,
                                                              unsigned long long *__restrict__ out,
                                                              int *__restrict__ counts) {
    const size_t nwords = (size_t)eg.XW * eg.Y * eg.Z;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long e = 0ull;
    if (w < nwords) {
        const int xw = (int)(w % eg.XW);
        const size_t row = w / eg.XW;
        const int qy = (int)(row % eg.Y) - 1, qz = (int)(row / eg.Y) - 1;
        // the word's first bit, its lower end (q.x + 1), and the axis that bit belongs to
        const int j0 = 64 * xw, p0 = j0 / 3, r = j0 - 3 * p0;
        const uint32_t w0 = refine_occ_window(occ, g, p0 - 1, qy, qz);
        const uint32_t wy = refine_occ_window(occ, g, p0 - 1, qy + 1, qz);
        const uint32_t wz = refine_occ_window(occ, g, p0 - 1, qy, qz + 1);
        // bit i: lower end p0 + i.  (Lower ends past X read zeros in every window: no cut, and the
        // word's padding bits stay clear.)
        const uint32_t cx = w0 ^ (w0 >> 1), cy = w0 ^ wy, cz = w0 ^ wz;
        // lower ends p0 .. p0 + 10 fill bits -r .. 32 - r, p0 + 11 .. p0 + 22 the bits from 33 - r on
        const unsigned long long lo = refine_interleave3(cx & 0x7ffu, cy & 0x7ffu, cz & 0x7ffu);
        const unsigned long long hi = refine_interleave3((cx >> 11) & 0xfffu, (cy >> 11) & 0xfffu, (cz >> 11) & 0xfffu);
        e = (lo >> r) | (hi << (33 - r));
        out[w] = e;
    }
    chunk_count_add(counts, w, __popcll(e));
}

// index of the cut edge between corners ca and cb of the cell at (x, y, z) in the vertex list
__device__ __forceinline__ unsigned mc_refine_rank(const SparseList &edges, const BitGrid &eg, int x, int y,
                                                   int z, int ca, int cb) {
    constexpr unsigned kCx = 0x99u, kCy = 0xCCu, kCz = 0xF0u;  // corner offsets (mc_cell_descriptors)
    const int ax = (kCx >> ca) & 1, ay = (kCy >> ca) & 1, az = (kCz >> ca) & 1;
    const int bx = (kCx >> cb) & 1, by = (kCy >> cb) & 1, bz = (kCz >> cb) & 1;
    const int axis = ax != bx ? 0 : ay != by ? 1 : 2;
    const int qx = x + min(ax, bx), qy = y + min(ay, by), qz = z + min(az, bz);  // the lower end
    return (unsigned)sparse_find(edges, eg.XW, 3 * (qx + 1) + axis, (size_t)(qz + 1) * eg.Y + (qy + 1));
}

// mc_mesh_kernel with one index per cut edge.  Per wave, through LDS (the launch geometry and the
// triangle offsets are mc_mesh_kernel's):
//   A  lane = cell: per triangle {x + 1 | (y + 1) << 16, z + 1 | its three edge numbers << 16, cube index};
//   B  lane = triangle: the three rank lookups; the colours of the occupied ends of the first two
//      edges and mc_mesh_kernel's face colour of them;
//   C  the wave's range streams out in whole lines, 24 bytes of face record per triangle.
__global__ __launch_bounds__(256) void mc_refine_tri_kernel(const McMeshParams p, const SparseList edges,
                                                            const BitGrid eg, const int4 *__restrict__ cells,
                                                            long long n_cap, const long long *__restrict__ n_dev,
                                                            long long tri_cap, const int *__restrict__ tri_offset,
                                                            unsigned *__restrict__ faces) {
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
    if (c < n) {  // ---- A
        const int4 cell = cells[c];
        const int idx = cell.w & 255, nt = kMcTri.n[idx], t0 = (int)(tri_offset[c] - base);
        const uint4 rw = *reinterpret_cast<const uint4 *>(kMcTri.e[idx]);  // 16 edge numbers
        const unsigned long long elo = (unsigned long long)rw.x | ((unsigned long long)rw.y << 32),
                                 ehi = (unsigned long long)rw.z | ((unsigned long long)rw.w << 32);
        for (int k = 0; k < nt; ++k) {
            uint32_t e3 = 0;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const int j = 3 * k + v;
                e3 |= (uint32_t)((j < 8 ? elo >> (8 * j) : ehi >> (8 * (j - 8))) & 15ull) << (4 * v);
            }
            mine[t0 + k][0] = (uint32_t)(cell.x + 1) | ((uint32_t)(cell.y + 1) << 16);
            mine[t0 + k][1] = (uint32_t)(cell.z + 1) | (e3 << 16);
            mine[t0 + k][2] = (uint32_t)idx;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's LDS writes have landed
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < ntri; t += 64) {  // ---- B
        constexpr unsigned kCx = 0x99u, kCy = 0xCCu, kCz = 0xF0u;
        const uint32_t w0 = mine[t][0], w1 = mine[t][1];
        const int idx = (int)mine[t][2];
        const int x = (int)(w0 & 0xffffu) - 1, y = (int)(w0 >> 16) - 1, z = (int)(w1 & 0xffffu) - 1;
        unsigned rank[3];
        float3 q[2];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const int e = (int)((w1 >> (16 + 4 * v)) & 15u);
            const int a = e & 7, b = mc::kSecondCorner[e];  // e % 8 and its partner
            rank[v] = mc_refine_rank(edges, eg, x, y, z, a, b);
            if (v < 2) {  // col[2] = col[1], as mc_mesh_kernel
                const int cn = ((idx >> a) & 1) ? b : a;  // the corner that is in the model
                q[v] = mc_voxel_rgb(p, x + (int)((kCx >> cn) & 1u), y + (int)((kCy >> cn) & 1u),
                                    z + (int)((kCz >> cn) & 1u));
            }
        }
        mine[t][0] = rank[0];
        mine[t][1] = rank[1];
        mine[t][2] = rank[2];
        mine[t][3] = mc_mean3(q[0].x, q[1].x, q[1].x);
        mine[t][4] = mc_mean3(q[0].y, q[1].y, q[1].y);
        mine[t][5] = mc_mean3(q[0].z, q[1].z, q[1].z);
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

// what the bisection reads of the views
struct RefineViews {
    const float *M;      // V x 12
    const uint32_t *bg;  // V x bgWords, bit = 1 where the mask pixel is background
    int V, W, H, bgWords;
    float s;
};

// inside(p) of arvx.h for the lanes with `active` set: no view in which p projects into the image
// onto a background pixel.  The loop over views is the wave's: v is the same in every lane, so the
// matrix comes through scalar loads, and it ends when every lane of the wave has met a background
// pixel (or the views).  The arithmetic is the carve's with float coordinates: fp32 world
// coordinates, fp64 products summed in the context's grouping and rounded to fp32, IEEE quotients,
// pixel_from_quotients.  A plane word is read only for a pixel inside the image.
template <bool LEFT>
__device__ __forceinline__ bool refine_inside(const RefineViews &vw, bool active, float px, float py, float pz) {
    const double w0 = (double)(py * vw.s), w1 = (double)(px * vw.s), w2 = (double)((-pz) * vw.s);
    const float wlim = (float)vw.W - 0.5f, hlim = (float)vw.H - 0.5f;
    bool in = active;
    for (int v = 0; v < vw.V; ++v) {
        if (!__any(in)) break;
        const float *__restrict__ Mv = vw.M + 12 * v;
        float a[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            a[r] = row_sum<LEFT>((double)Mv[4 * r] * w0, (double)Mv[4 * r + 1] * w1, (double)Mv[4 * r + 2] * w2,
                                 (double)Mv[4 * r + 3]);
        int pix;
        const bool seen = pixel_from_quotients(a[0] / a[2], a[1] / a[2], vw.W, wlim, hlim, pix);
        if (in && seen) {
            const uint32_t word = vw.bg[(size_t)v * vw.bgWords + ((unsigned)pix >> 5)];
            if ((word >> (pix & 31)) & 1u) in = false;
        }
    }
    return in;
}

// Vertex k of the list (index[k]: its key, ascending).  One cut edge per lane: which end is
// occupied, the inside tests of both ends, `bisections` steps along a silhouette edge (wave-uniform
// trip count; lanes whose edge is no silhouette edge sit them out), and
//   verts[3k..]  the occupied end with n / 2^(B+1) added towards the empty end along the axis
//   rgb[3k..]    the occupied end's colour as mc_mesh_kernel reads it (mc_voxel_rgb)
//   edges[4k..]  the occupied end and the direction (0 +x, 1 -x, 2 +y, 3 -y, 4 +z, 5 -z; + 8: no
//                silhouette edge)
//   cut[k]       n
// Every coordinate is exact in fp32 (sides <= 4096, B <= 10).  With vw.V == 0 (only B == 0 gets
// here without views) no edge is a silhouette edge's business: n = 1 either way.
// n_cap: room in `index` and the outputs; n_dev: the list's length on the device
template <bool LEFT>
__global__ __launch_bounds__(256) void mc_refine_vertex_kernel(const McMeshParams p, const RefineViews vw,
                                                               const unsigned long long *__restrict__ occ,
                                                               const BitGrid g, const int *__restrict__ index,
                                                               long long n_cap, const long long *__restrict__ n_dev,
                                                               int bisections, float *__restrict__ verts,
                                                               float *__restrict__ rgb, int *__restrict__ edges,
                                                               int *__restrict__ cut) {
    const long long n = *n_dev < n_cap ? *n_dev : n_cap;
    const long long k0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (k0 >= n) return;  // (wave-uniform)
    const long long k = k0 + (threadIdx.x & 63);
    const bool live = k < n;
    const int key = live ? index[k] : 0;
    const int axis = key % 3, pt = key / 3;
    const int qx = pt % (g.X + 1) - 1, row = pt / (g.X + 1);
    const int qy = row % (g.Y + 1) - 1, qz = row / (g.Y + 1) - 1;
    // the occupied end A: the lower end q if it is occupied, else the upper end
    const bool low = qx >= 0 && qy >= 0 && qz >= 0 && plane_bit(occ, g.X, g.Y, qx, qy, qz);
    const int up = low ? 0 : 1;
    const int Ax = qx + (axis == 0 ? up : 0), Ay = qy + (axis == 1 ? up : 0), Az = qz + (axis == 2 ? up : 0);
    const float sgn = low ? 1.f : -1.f;  // towards the empty end E
    // (a step t along the axis: the other two components get + 0, which changes nothing)
    const float fx = (float)Ax, fy = (float)Ay, fz = (float)Az;
    const float ux = axis == 0 ? sgn : 0.f, uy = axis == 1 ? sgn : 0.f, uz = axis == 2 ? sgn : 0.f;
    const bool inA = refine_inside<LEFT>(vw, live, fx, fy, fz);
    const bool inE = refine_inside<LEFT>(vw, live && inA, fx + ux, fy + uy, fz + uz);
    const bool sil = vw.V > 0 && inA && !inE;
    const float scale = (float)(1 << bisections);
    int lo = 0, hi = 1 << bisections;
    for (int b = 0; b < bisections; ++b) {
        const int mid = (lo + hi) >> 1;
        const float t = (float)mid / scale;
        if (refine_inside<LEFT>(vw, live && sil, fx + ux * t, fy + uy * t, fz + uz * t)) lo = mid;
        else hi = mid;
    }
    const int nn = sil ? lo + hi : 1 << bisections;
    if (!live) return;
    const float t = (float)nn / (2.f * scale);
    const float3 c = mc_voxel_rgb(p, Ax, Ay, Az);
    verts[3 * k] = fx + ux * t, verts[3 * k + 1] = fy + uy * t, verts[3 * k + 2] = fz + uz * t;
    rgb[3 * k] = c.x, rgb[3 * k + 1] = c.y, rgb[3 * k + 2] = c.z;
    *reinterpret_cast<int4 *>(edges + 4 * k) = make_int4(Ax, Ay, Az, 2 * axis + up + (sil ? 0 : 8));
    cut[k] = nn;
}

}  // namespace arvx
