// mesh_color_kernels.h -- a held mesh's vertices coloured from the photographs for gfx950: per view a
// depth buffer of the mesh's own triangles, then a vote per vertex over the views that see it
// (arvx_mesh_color; the definition is in include/arvx/arvx.h, after the triangle render's block).
//
// The depth pass is the triangle render's (render_mesh_kernels.h) over a BATCH of views per launch:
// the same device functions -- mesh_project, mesh_tri_setup, mesh_edges / mesh_weights through
// mesh_pixel -- fed with the view's slice of the projected vertices and of the keys, so that a view's
// keys are the keys arvx_render_mesh_view would leave, by construction.  Only the keys are written: no
// class counts, no images.
//   mesh_color_project_kernel  one lane per (vertex, view of the batch): 16 bytes each
//   mesh_color_raster_kernel   one lane per (triangle, view): boxes of up to kMeshLanePixels pixels are
//                              swept by the lane, larger ones appended to the batch's list (when it is
//                              full, swept by the lane's wave instead)
//   mesh_color_large_kernel    one wave per listed (triangle, view)
//   mesh_color_vote_kernel     one lane per vertex: the views in ascending order, the projection once
//                              more, the nearest key, the background bit, four pixels, integer sums
//   mesh_color_depth_kernel    a view's keys as the fp32 depth image
// All stores are ordinary vector stores; the key minimum is render_kernels.h's key_min.
#pragma once

#include "render_mesh_kernels.h"

namespace arvx {

// The header (64 bytes in front of the list of large boxes): the entries the batch appended, the most
// any batch of the call wanted to append, the vertices some view sees.
struct MeshColorHeader {
    unsigned n_large;
    unsigned most;
    unsigned long long coloured;
};

struct MeshColorParams {
    RenderMeshParams mesh;     // the source; proj and keys: those of the batch's first view; M, rgb, head unused
    const SelftestMatrix *M;   // the context's V cameras
    int view0, nviews;         // the batch
    MeshColorHeader *head;
};

// the mesh as view b of the batch sees it: its slice of the projected vertices and of the keys
__device__ __forceinline__ RenderMeshParams mesh_color_view(const MeshColorParams &p, unsigned b) {
    RenderMeshParams q = p.mesh;
    q.proj = p.mesh.proj + (size_t)b * (size_t)p.mesh.V;
    q.keys = p.mesh.keys + (size_t)b * ((size_t)p.mesh.W * p.mesh.H);
    return q;
}

// grid: (vertices / 256, views of the batch)
template <bool LEFT>
__global__ __launch_bounds__(256) void mesh_color_project_kernel(const MeshColorParams p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.mesh.V || (int)blockIdx.y >= p.nviews) return;
    const SelftestMatrix M = p.M[p.view0 + (int)blockIdx.y];
    const float *__restrict__ v = p.mesh.verts;
    mesh_vertex_store(p.mesh.proj + (size_t)blockIdx.y * (size_t)p.mesh.V, (size_t)i,
                      mesh_project<LEFT>(M, p.mesh.s, v[3 * i], v[3 * i + 1], v[3 * i + 2]));
}

// grid: (workgroups that stride over the faces, views of the batch)
__global__ __launch_bounds__(256) void mesh_color_raster_kernel(const MeshColorParams p) {
    if ((int)blockIdx.y >= p.nviews) return;
    const RenderMeshParams q = mesh_color_view(p, blockIdx.y);
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * 256; base < q.T; base += (long long)gridDim.x * 256) {
        const long long t = base + threadIdx.x;
        bool wide = false;  // large, and the list had no room
        if (t < q.T) {
            MeshTri tri;
            if (mesh_tri_setup(q, t, tri) == kMeshDrawn) {
                if ((tri.c1 - tri.c0 + 1) * (tri.r1 - tri.r0 + 1) <= kMeshLanePixels) {
                    for (int r = tri.r0; r <= tri.r1; ++r)
                        for (int c = tri.c0; c <= tri.c1; ++c) (void)mesh_pixel(q, tri, (uint32_t)t, c, r);
                } else {
                    const unsigned k = atomicAdd(&p.head->n_large, 1u);
                    if (k < q.large_cap)
                        q.large[k] = SplatRect{(uint32_t)tri.c0 | ((uint32_t)tri.c1 << 16),
                                               (uint32_t)tri.r0 | ((uint32_t)tri.r1 << 16), (uint32_t)t, blockIdx.y};
                    else
                        wide = true;
                }
            }
        }
        // (every lane of the wave gets here: the loop bound is uniform over the workgroup)
        unsigned long long m = __ballot(wide);
        const long long wave_t0 = base + (threadIdx.x - lane);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            MeshTri tri;
            (void)mesh_tri_setup(q, wave_t0 + l, tri);  // (kMeshDrawn: lane l found it so)
            (void)mesh_sweep_wave(q, tri, (uint32_t)(wave_t0 + l), lane);
        }
    }
}

// One wave per listed (triangle, view); a fixed grid that strides over the list.  The most any batch
// of the call wanted to list goes to `need` (a page-locked host word, read at the call's
// synchronisation): the next call sizes its list from it.
__global__ __launch_bounds__(256) void mesh_color_large_kernel(const MeshColorParams p, long long *__restrict__ need) {
    const int lane = threadIdx.x & 63;
    const unsigned waves = gridDim.x * 4;
    const unsigned wanted = p.head->n_large;
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (the batches follow each other on the stream)
        const unsigned most = max(p.head->most, wanted);
        p.head->most = most;
        *need = (long long)most;
    }
    const unsigned n = min(wanted, p.mesh.large_cap);
    for (unsigned f = blockIdx.x * 4 + (threadIdx.x >> 6); f < n; f += waves) {
        const uint32_t t = p.mesh.large[f].view;
        const unsigned b = p.mesh.large[f].depth;
        if (b >= (unsigned)p.nviews || (long long)t >= p.mesh.T) continue;  // (never: the raster listed it)
        const RenderMeshParams q = mesh_color_view(p, b);
        MeshTri tri;
        if (mesh_tri_setup(q, t, tri) != kMeshDrawn) continue;  // (never)
        (void)mesh_sweep_wave(q, tri, t, lane);
    }
}

struct MeshVoteParams {
    const float *verts, *col;  // Vn x 3 each: the source's positions and its own colours
    long long Vn;
    float s;
    int V, W, H;
    const SelftestMatrix *M;          // V cameras
    const unsigned long long *keys;   // V x H x W
    const uint32_t *bg;               // the views' background bit planes (null: the flag is not set)
    int bgWords;
    const uint8_t *images;            // V x H x W x 3, BGR
    int average;
    float tol;
    float *rgb;                       // Vn x 3
    int *views;                       // Vn
    unsigned long long *coloured;
};

template <bool LEFT>
__global__ __launch_bounds__(256) void mesh_color_vote_kernel(const MeshVoteParams p) {
    __shared__ unsigned s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int n = 0;
    if (i < p.Vn) {
        const float px = p.verts[3 * i], py = p.verts[3 * i + 1], pz = p.verts[3 * i + 2];
        const size_t npix = (size_t)p.W * p.H;
        unsigned long long sum[3] = {0, 0, 0};  // AVERAGE: the sums; CLOSEST: the nearest view's S
        float best = INFINITY;
        for (int v = 0; v < p.V; ++v) {
            const SelftestMatrix M = p.M[v];
            const MeshVertex q = mesh_project<LEFT>(M, p.s, px, py, pz);
            if (!q.valid || q.fx < 0 || q.fy < 0 || q.fx > 16 * (p.W - 1) || q.fy > 16 * (p.H - 1)) continue;
            const size_t pix = (size_t)((q.fy + 8) >> 4) * p.W + (size_t)((q.fx + 8) >> 4);
            const unsigned long long key = p.keys[(size_t)v * npix + pix];
            const float a2 = __uint_as_float(q.a2);
            const float D = key == kRenderEmpty ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
            if (!(a2 <= D + p.tol)) continue;
            if (p.bg && ((p.bg[(size_t)v * p.bgWords + (pix >> 5)] >> (pix & 31)) & 1u)) continue;
            ++n;
            if (!p.average && !(a2 < best)) continue;
            best = a2;
            const int c0 = q.fx >> 4, r0 = q.fy >> 4;
            const unsigned wx = (unsigned)(q.fx & 15), wy = (unsigned)(q.fy & 15);
            const int c1 = min(c0 + 1, p.W - 1), r1 = min(r0 + 1, p.H - 1);
            const uint8_t *__restrict__ img = p.images + (size_t)v * npix * 3;
            const uint8_t *p00 = img + ((size_t)r0 * p.W + c0) * 3, *p01 = img + ((size_t)r0 * p.W + c1) * 3;
            const uint8_t *p10 = img + ((size_t)r1 * p.W + c0) * 3, *p11 = img + ((size_t)r1 * p.W + c1) * 3;
            const unsigned w00 = (16 - wx) * (16 - wy), w01 = wx * (16 - wy), w10 = (16 - wx) * wy, w11 = wx * wy;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {  // (r, g, b of pixels stored B, G, R)
                const unsigned S = w00 * p00[2 - ch] + w01 * p01[2 - ch] + w10 * p10[2 - ch] + w11 * p11[2 - ch];
                sum[ch] = p.average ? sum[ch] + S : S;
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float out;
            if (n == 0) out = p.col[3 * i + ch];
            else if (p.average) out = (float)((double)sum[ch] / (double)(256ull * (unsigned long long)n));
            else out = (float)(uint32_t)sum[ch] / 256.0f;
            p.rgb[3 * i + ch] = out;
        }
        p.views[i] = n;
    }
    const unsigned long long seen = __ballot(n > 0);
    if ((threadIdx.x & 63) == 0 && seen) atomicAdd(&s_n, (unsigned)__popcll(seen));
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(p.coloured, (unsigned long long)s_n);
}

// a view's keys as its depth image: +inf where no triangle covers the pixel
__global__ __launch_bounds__(256) void mesh_color_depth_kernel(const unsigned long long *__restrict__ keys, size_t npix,
                                                               float *__restrict__ depth) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long key = keys[i];
    depth[i] = key == kRenderEmpty ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
}

}  // namespace arvx
