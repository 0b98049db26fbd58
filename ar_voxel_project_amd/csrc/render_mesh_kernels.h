// render_mesh_kernels.h -- a mesh's triangles drawn into a camera view for gfx950: a z-buffered
// rasteriser (arvx_render_mesh, arvx_render_triangles; the definition is in include/arvx/arvx.h,
// after the render's block).
//
// The mesh is V positions (fp32 voxel coordinates), V colours and T face records {i0, i1, i2, r, g,
// b}: the layout every mesh of the context has.  Then, after render_clear_kernel (render_kernels.h):
//   render_mesh_project_kernel  one lane per vertex: refine_inside's projection with the caller's
//                               camera, the two quotients, the validity test and the position in
//                               sixteenths of a pixel -- 16 bytes per vertex, gathered by the rest
//   render_mesh_raster_kernel   one lane per triangle: its class, its pixel box; boxes of up to
//                               kMeshLanePixels pixels are swept by the lane, larger ones appended
//                               to a list (when it is full, swept by the lane's wave instead)
//   render_mesh_large_kernel    one wave per listed triangle, a pixel of its box per lane
//   render_mesh_resolve_kernel  one lane per pixel: the winner's edge functions once more, its
//                               depth, the interpolated colour (or, instantiated with
//                               MeshTextureColour, the face's texel), the face's shade
// With a near plane set (arvx_ctx_set_render_near) the raster, large and resolve kernels launched are
// those of render_mesh_clip_kernels.h instead; the ones here have no clip path.
// Coverage is decided by three 64-bit integer edge functions of 28.4 fixed-point corners: exact, so
// two faces that share an edge agree about its pixels.  A key is bits(depth) << 32 | t with depth a
// positive fp32: its 64-bit unsigned minimum (key_min, a no-return atomicMin) is the nearest
// triangle and, among equally near ones, the least t, in whatever order triangles arrive.  The class
// counts are reduced per workgroup.  All stores are ordinary vector stores.
#pragma once

#include <float.h>

#include "render_kernels.h"

namespace arvx {

constexpr int kMeshLanePixels = 64;    // pixel boxes up to this size are swept by their lane
constexpr float kMeshMaxPixel = 32768.f;  // |qu|, |qv| of a valid vertex: |fx| <= 2^19

// The triangle render's header (64 bytes in front of its list): the entries appended, then the four
// class counts.
enum MeshClass { kMeshDrawn, kMeshEmpty, kMeshFlat, kMeshRefused, kMeshClasses };
struct RenderMeshHeader {
    unsigned n_large;
    unsigned pad;
    unsigned long long classes[kMeshClasses];
};

// A projected vertex: fx, fy in sixteenths of a pixel, the bits of a2, and whether it is VALID.
struct MeshVertex {
    int fx, fy;
    uint32_t a2;
    int valid;
};

struct RenderMeshParams {
    const float *verts;     // V x 3, voxel coordinates
    const float *rgb;       // V x 3
    const unsigned *faces;  // T x 6: i0, i1, i2, r, g, b
    long long V, T;
    float s;
    int W, H;
    SelftestMatrix M;  // the camera, row-major 3 x 4
    MeshVertex *proj;  // V
    unsigned long long *keys;  // H x W
    SplatRect *large;  // listed triangles: their pixel box, `view` holds t
    RenderMeshHeader *head;
    unsigned large_cap;
    float light[3];
    int lit;
    // near-plane clipping (render_mesh_clip_kernels.h; read by its kernels only): the plane, > 0, and
    // the four clip counts
    float near;
    unsigned long long *clip;
};

// Step 1 of the definition for the point (px, py, pz) under camera M: the one place it is computed
// (the mesh colours' kernels, mesh_color_kernels.h, project with it too).
template <bool LEFT>
__device__ __forceinline__ void mesh_project_rows(const SelftestMatrix &M, float s, float px, float py, float pz,
                                                  float (&a)[3]) {
    const double w0 = (double)(py * s), w1 = (double)(px * s), w2 = (double)((-pz) * s);
#pragma unroll
    for (int r = 0; r < 3; ++r)
        a[r] = row_sum<LEFT>((double)M.m[4 * r] * w0, (double)M.m[4 * r + 1] * w1, (double)M.m[4 * r + 2] * w2,
                             (double)M.m[4 * r + 3]);
}

template <bool LEFT>
__device__ __forceinline__ MeshVertex mesh_project(const SelftestMatrix &M, float s, float px, float py, float pz) {
    float a[3];
    mesh_project_rows<LEFT>(M, s, px, py, pz, a);
    const float qu = a[0] / a[2], qv = a[1] / a[2];
    const bool valid = a[2] >= FLT_MIN && isfinite(qu) && isfinite(qv) && fabsf(qu) <= kMeshMaxPixel &&
                       fabsf(qv) <= kMeshMaxPixel;
    MeshVertex out{0, 0, __float_as_uint(a[2]), valid ? 1 : 0};
    if (valid) {
        out.fx = (int)roundf(qu * 16.0f);
        out.fy = (int)roundf(qv * 16.0f);
    }
    return out;
}

__device__ __forceinline__ void mesh_vertex_store(MeshVertex *__restrict__ proj, size_t i, const MeshVertex &v) {
    *reinterpret_cast<int4 *>(proj + i) = make_int4(v.fx, v.fy, (int)v.a2, v.valid);
}

template <bool LEFT>
__global__ __launch_bounds__(256) void render_mesh_project_kernel(const RenderMeshParams p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.V) return;
    mesh_vertex_store(p.proj, (size_t)i,
                      mesh_project<LEFT>(p.M, p.s, p.verts[3 * i], p.verts[3 * i + 1], p.verts[3 * i + 2]));
}

// What a triangle's sweep and its resolve need: the corners, the doubled area's sign, 1 / a2 per
// corner, and the pixel box.
struct MeshTri {
    int x0, y0, x1, y1, x2, y2;
    long long A;  // positive (the sign is in `neg`)
    bool neg;
    double iz0, iz1, iz2;
    int c0, c1, r0, r1;
};

__device__ __forceinline__ MeshVertex mesh_vertex(const MeshVertex *__restrict__ proj, size_t i) {
    const int4 v = *reinterpret_cast<const int4 *>(proj + i);
    return MeshVertex{v.x, v.y, (uint32_t)v.z, v.w};
}

// a * b - c * d of differences of fixed-point coordinates: each below 2^21 in magnitude, exact in int64
__device__ __forceinline__ long long mesh_det(int a, int b, int c, int d) {
    return (long long)a * b - (long long)c * d;
}

// Steps 2 and 3 for the corners already in `tri`: kMeshFlat, kMeshEmpty for an empty pixel box, or
// kMeshDrawn with A, its sign and the box set.
__device__ __forceinline__ int mesh_tri_box(const RenderMeshParams &p, MeshTri &tri) {
    const long long A = mesh_det(tri.x1 - tri.x0, tri.y2 - tri.y0, tri.x2 - tri.x0, tri.y1 - tri.y0);
    if (A == 0) return kMeshFlat;
    tri.neg = A < 0;
    tri.A = tri.neg ? -A : A;
    const int xmin = min(tri.x0, min(tri.x1, tri.x2)), xmax = max(tri.x0, max(tri.x1, tri.x2));
    const int ymin = min(tri.y0, min(tri.y1, tri.y2)), ymax = max(tri.y0, max(tri.y1, tri.y2));
    // (an arithmetic shift is the floor; + 15 first makes it the ceiling)
    tri.c0 = max((xmin + 15) >> 4, 0);
    tri.c1 = min(xmax >> 4, p.W - 1);
    tri.r0 = max((ymin + 15) >> 4, 0);
    tri.r1 = min(ymax >> 4, p.H - 1);
    // (most triangles of a fine mesh lie between the pixel centres: they end here, before the divisions)
    if (tri.c0 > tri.c1 || tri.r0 > tri.r1) return kMeshEmpty;
    return kMeshDrawn;
}

// The class of triangle t as far as its corners decide it: kMeshRefused, kMeshFlat, kMeshEmpty for one
// whose pixel box is empty, or kMeshDrawn for a triangle with an area and a box (it may still turn
// out kMeshEmpty); only then is `tri` complete.
__device__ __forceinline__ int mesh_tri_setup(const RenderMeshParams &p, long long t, MeshTri &tri) {
    size_t i0 = p.faces[6 * t], i1 = p.faces[6 * t + 1], i2 = p.faces[6 * t + 2];
    if (i0 >= (size_t)p.V || i1 >= (size_t)p.V || i2 >= (size_t)p.V) return kMeshRefused;  // (never)
    const MeshVertex v0 = mesh_vertex(p.proj, i0), v1 = mesh_vertex(p.proj, i1), v2 = mesh_vertex(p.proj, i2);
    if (!(v0.valid && v1.valid && v2.valid)) return kMeshRefused;
    tri.x0 = v0.fx, tri.y0 = v0.fy, tri.x1 = v1.fx, tri.y1 = v1.fy, tri.x2 = v2.fx, tri.y2 = v2.fy;
    if (const int cls = mesh_tri_box(p, tri); cls != kMeshDrawn) return cls;
    tri.iz0 = 1.0 / (double)__uint_as_float(v0.a2);
    tri.iz1 = 1.0 / (double)__uint_as_float(v1.a2);
    tri.iz2 = 1.0 / (double)__uint_as_float(v2.a2);
    return kMeshDrawn;
}

// The edge functions at pixel (c, r), signed so that the inside is >= 0; true when it is COVERED.
__device__ __forceinline__ bool mesh_edges(const MeshTri &tri, int c, int r, long long &e0, long long &e1,
                                           long long &e2) {
    const int px = 16 * c, py = 16 * r;  // (|px|, |py| < 2^18)
    e0 = mesh_det(tri.x1 - px, tri.y2 - py, tri.x2 - px, tri.y1 - py);
    e1 = mesh_det(tri.x2 - px, tri.y0 - py, tri.x0 - px, tri.y2 - py);
    e2 = mesh_det(tri.x0 - px, tri.y1 - py, tri.x1 - px, tri.y0 - py);
    if (tri.neg) e0 = -e0, e1 = -e1, e2 = -e2;
    return e0 >= 0 && e1 >= 0 && e2 >= 0;
}

// t_i = E_i / a2_i and their sum: the weights of the perspective-correct interpolation
__device__ __forceinline__ double mesh_weights(const MeshTri &tri, long long e0, long long e1, long long e2,
                                               double &t0, double &t1, double &t2) {
    t0 = (double)e0 * tri.iz0;
    t1 = (double)e1 * tri.iz1;
    t2 = (double)e2 * tri.iz2;
    return (t0 + t1) + t2;
}

// one pixel of triangle t's box: true when it is covered (then its key has gone to the pixel)
__device__ __forceinline__ bool mesh_pixel(const RenderMeshParams &p, const MeshTri &tri, uint32_t t, int c, int r) {
    long long e0, e1, e2;
    if (!mesh_edges(tri, c, r, e0, e1, e2)) return false;
    double t0, t1, t2;
    const double S = mesh_weights(tri, e0, e1, e2, t0, t1, t2);
    const float depth = (float)((double)tri.A / S);
    key_min(p.keys + (size_t)r * p.W + c, render_key(__float_as_uint(depth), t));
    return true;
}

// a triangle's box by a whole wave, its pixels row-major across the lanes; true (in every lane) when
// some pixel is covered
__device__ __forceinline__ bool mesh_sweep_wave(const RenderMeshParams &p, const MeshTri &tri, uint32_t t, int lane) {
    const int wc = tri.c1 - tri.c0 + 1;
    const int area = wc * (tri.r1 - tri.r0 + 1);  // (at most 2^28)
    bool any = false;
    for (int j = lane; j < area; j += 64) any |= mesh_pixel(p, tri, t, tri.c0 + j % wc, tri.r0 + j / wc);
    return __any(any);
}

// the wave's class counts into the workgroup's, the workgroup's into the header: s_n is zeroed before
// and a barrier stands between the waves' adds and this
__device__ __forceinline__ void mesh_classes_out(unsigned (&s_n)[kMeshClasses], RenderMeshHeader *head) {
    __syncthreads();
    if (threadIdx.x < kMeshClasses && s_n[threadIdx.x])
        atomicAdd(head->classes + threadIdx.x, (unsigned long long)s_n[threadIdx.x]);
}

// One lane per triangle; the grid strides over the faces.  A listed triangle is counted by
// render_mesh_large_kernel, every other one here.
__global__ __launch_bounds__(256) void render_mesh_raster_kernel(const RenderMeshParams p) {
    __shared__ unsigned s_n[kMeshClasses];
    if (threadIdx.x < kMeshClasses) s_n[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned mine[kMeshClasses] = {0, 0, 0, 0};  // (wave sweeps are counted by lane 0)
    for (long long base = (long long)blockIdx.x * 256; base < p.T; base += (long long)gridDim.x * 256) {
        const long long t = base + threadIdx.x;
        bool wide = false;  // large, and the list had no room
        if (t < p.T) {
            MeshTri tri;
            int cls = mesh_tri_setup(p, t, tri);
            if (cls == kMeshDrawn) {
                if ((tri.c1 - tri.c0 + 1) * (tri.r1 - tri.r0 + 1) <= kMeshLanePixels) {
                    bool any = false;
                    for (int r = tri.r0; r <= tri.r1; ++r)
                        for (int c = tri.c0; c <= tri.c1; ++c) any |= mesh_pixel(p, tri, (uint32_t)t, c, r);
                    if (!any) cls = kMeshEmpty;
                } else {
                    cls = -1;  // counted where it is swept
                    const unsigned k = atomicAdd(&p.head->n_large, 1u);
                    if (k < p.large_cap)
                        p.large[k] = SplatRect{(uint32_t)tri.c0 | ((uint32_t)tri.c1 << 16),
                                               (uint32_t)tri.r0 | ((uint32_t)tri.r1 << 16), (uint32_t)t, 0u};
                    else
                        wide = true;
                }
            }
#pragma unroll
            for (int k = 0; k < kMeshClasses; ++k) mine[k] += cls == k ? 1u : 0u;
        }
        // (every lane of the wave gets here: the loop bound is uniform over the workgroup)
        unsigned long long m = __ballot(wide);
        const long long wave_t0 = base + (threadIdx.x - lane);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            MeshTri tri;
            (void)mesh_tri_setup(p, wave_t0 + l, tri);  // (kMeshDrawn: lane l listed it)
            const bool any = mesh_sweep_wave(p, tri, (uint32_t)(wave_t0 + l), lane);
            if (lane == 0) {
                mine[kMeshDrawn] += any ? 1u : 0u;
                mine[kMeshEmpty] += any ? 0u : 1u;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kMeshClasses; ++k)
        if (mine[k]) atomicAdd(&s_n[k], mine[k]);
    mesh_classes_out(s_n, p.head);
}

// One wave per listed triangle; a fixed grid that strides over the list (its length is on the
// device).  The number of triangles the raster wanted to list goes to `need` (a page-locked host
// word, read at the next synchronisation of a render call): the renders after that size their
// lists from it.
__global__ __launch_bounds__(256) void render_mesh_large_kernel(const RenderMeshParams p, long long *__restrict__ need) {
    __shared__ unsigned s_n[kMeshClasses];
    if (threadIdx.x < kMeshClasses) s_n[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned waves = gridDim.x * 4;
    const unsigned wanted = p.head->n_large;
    if (blockIdx.x == 0 && threadIdx.x == 0) *need = (long long)wanted;
    const unsigned n = min(wanted, p.large_cap);
    unsigned drawn = 0, empty = 0;
    for (unsigned f = blockIdx.x * 4 + (threadIdx.x >> 6); f < n; f += waves) {
        const uint32_t t = p.large[f].view;
        MeshTri tri;
        if (mesh_tri_setup(p, t, tri) != kMeshDrawn) continue;  // (never: the raster listed it)
        if (mesh_sweep_wave(p, tri, t, lane)) ++drawn;
        else ++empty;
    }
    if (lane == 0) {
        if (drawn) atomicAdd(&s_n[kMeshDrawn], drawn);
        if (empty) atomicAdd(&s_n[kMeshEmpty], empty);
    }
    mesh_classes_out(s_n, p.head);
}

// l of the definition: the length of a vector, every operation rounded on its own
__device__ __forceinline__ float mesh_length(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// Step 5's v of the winner t before the light, per channel r, g, b: the vertex colours interpolated.
// (MeshTextureColour, mesh_texture_kernels.h, is the other Colour of the resolve kernel.)
struct MeshVertexColour {
    __device__ __forceinline__ void operator()(const RenderMeshParams &p, uint32_t, size_t i0, size_t i1, size_t i2,
                                               double t0, double t1, double t2, double S, float (&v)[3]) const {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double n = (t0 * (double)p.rgb[3 * i0 + ch] + t1 * (double)p.rgb[3 * i1 + ch]) +
                             t2 * (double)p.rgb[3 * i2 + ch];
            v[ch] = (float)(n / S);
        }
    }
};

// The winner t of pixel i with its weights (w0, w1, w2, S): its id and depth, step 5's colour and
// shade.  bgr holds the background already (the caller's image or zeros).
template <class Colour>
__device__ __forceinline__ void mesh_pixel_out(const RenderMeshParams &p, size_t i, unsigned long long key, double w0,
                                               double w1, double w2, double S, int *__restrict__ id,
                                               float *__restrict__ depth, uint8_t *__restrict__ bgr,
                                               const Colour &colour) {
    const uint32_t t = (uint32_t)key;
    id[i] = (int)t;
    depth[i] = __uint_as_float((uint32_t)(key >> 32));
    const size_t i0 = p.faces[6 * (size_t)t], i1 = p.faces[6 * (size_t)t + 1], i2 = p.faces[6 * (size_t)t + 2];
    float shade = 1.f;
    if (p.lit) {
        const float *__restrict__ q = p.verts;
        const float ax = q[3 * i2] - q[3 * i0], ay = q[3 * i2 + 1] - q[3 * i0 + 1], az = q[3 * i2 + 2] - q[3 * i0 + 2];
        const float bx = q[3 * i1] - q[3 * i0], by = q[3 * i1 + 1] - q[3 * i0 + 1], bz = q[3 * i1 + 2] - q[3 * i0 + 2];
        const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const float l = mesh_length(cx, cy, cz), m = mesh_length(p.light[0], p.light[1], p.light[2]);
        const float d = (cx * p.light[0] + cy * p.light[1]) + cz * p.light[2];
        const float f = (l == 0.f || m == 0.f) ? 1.f : fminf(fabsf(d) / (l * m), 1.f);
        shade = 0.25f + 0.75f * f;
    }
    float v[3];
    colour(p, t, i0, i1, i2, w0, w1, w2, S, v);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        if (p.lit) v[ch] = shade * v[ch];
    bgr[3 * i] = render_channel(v[2]);
    bgr[3 * i + 1] = render_channel(v[1]);
    bgr[3 * i + 2] = render_channel(v[0]);
}

// One lane per pixel: only the covered pixels are written.
template <class Colour>
__global__ __launch_bounds__(256) void render_mesh_resolve_kernel(const RenderMeshParams p, size_t npix,
                                                                  int *__restrict__ id, float *__restrict__ depth,
                                                                  uint8_t *__restrict__ bgr, const Colour colour) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long key = p.keys[i];
    const uint32_t t = (uint32_t)key;
    MeshTri tri;
    if (key == kRenderEmpty || (long long)t >= p.T || mesh_tri_setup(p, t, tri) != kMeshDrawn) {
        id[i] = -1;
        depth[i] = INFINITY;
        return;
    }
    long long e0, e1, e2;
    (void)mesh_edges(tri, (int)(i % (size_t)p.W), (int)(i / (size_t)p.W), e0, e1, e2);
    double t0, t1, t2;
    const double S = mesh_weights(tri, e0, e1, e2, t0, t1, t2);
    mesh_pixel_out(p, i, key, t0, t1, t2, S, id, depth, bgr, colour);
}

}  // namespace arvx
