// render_mesh_clip_kernels.h -- the triangle render with a near plane for gfx950
// (arvx_ctx_set_render_near; the definition is in include/arvx/arvx.h, in the triangle render's block).
//
// With the plane off the context launches render_mesh_kernels.h's raster, large and resolve kernels,
// which have no clip path; with it on, the three kernels here take their places (the clear and the
// projection are shared):
//   render_mesh_clip_raster_kernel   one lane per face: a face with every corner in front goes the way
//                                    it goes without a plane; a STRADDLING face projects its corners
//                                    once more (proj keeps no a0, a1), clips, and sets up its one or
//                                    two pieces.  Pieces whose boxes hold up to kMeshLanePixels pixels
//                                    together are swept by the lane; otherwise the FACE is listed (or,
//                                    with a full list, swept by the lane's wave): a face's pieces are
//                                    always swept in one place, which therefore knows the face's class
//   render_mesh_clip_large_kernel    one wave per listed face: its triangle or its pieces
//   render_mesh_clip_resolve_kernel  one lane per pixel: the winner's piece is the least one that
//                                    covers the pixel with exactly the key's depth; its weights go
//                                    through the piece's B to the face's corners
// A straddling face is held rotated: Q0, Q1, Q2 = P_r, P_{r+1}, P_{r+2}, so that every index below is a
// compile-time one; the weights are turned back at the end.  All stores are ordinary vector stores.
#pragma once

#include "render_mesh_kernels.h"

namespace arvx {

// arvx_render_mesh_clip_stats' four counts, behind the list of large pixel boxes
enum MeshClipCount { kClipBehind, kClipStraddle, kClipPieces, kClipDrawn, kClipCounts };

// What mesh_clip_face says of a face beside a number of pieces (1 or 2)
constexpr int kClipWhole = 0;  // every corner in front: the triangle as it is without a plane
constexpr int kClipNone = -1;  // no corner in front

// A straddling face's polygon of 3 or 4 corners: positions, VALID, 1 / a2 and the weights B towards
// Q0, Q1, Q2.  Piece 0 is (0, 1, 2), piece 1 (0, 2, 3).
struct MeshClipPoly {
    int r;  // the rotation: Q_j = P_{(r + j) % 3}
    int fx[4], fy[4], valid[4];
    double iz[4];
    float B[4][3];
};

template <class T>
__device__ __forceinline__ void mesh_rotate(T &x0, T &x1, T &x2, int r) {
    const T a = x0, b = x1, c = x2;
    x0 = r == 0 ? a : r == 1 ? b : c;
    x1 = r == 0 ? b : r == 1 ? c : a;
    x2 = r == 0 ? c : r == 1 ? a : b;
}

// slot SLOT of the polygon: the original corner Q_J
template <int SLOT, int J>
__device__ __forceinline__ void mesh_clip_corner(MeshClipPoly &poly, const MeshVertex &v) {
    poly.fx[SLOT] = v.fx, poly.fy[SLOT] = v.fy, poly.valid[SLOT] = v.valid;
    poly.iz[SLOT] = 1.0 / (double)__uint_as_float(v.a2);
#pragma unroll
    for (int j = 0; j < 3; ++j) poly.B[SLOT][j] = j == J ? 1.f : 0.f;
}

// slot SLOT of the polygon: the clipped vertex of the edge Q_CA Q_CB (one end in front), computed from
// the end with the lower vertex index to the other, whichever face asks
template <int SLOT, int CA, int CB>
__device__ __forceinline__ void mesh_clip_vertex(MeshClipPoly &poly, const float (&qa)[3], size_t ia,
                                                 const float (&qb)[3], size_t ib, float n) {
    const bool sw = ib < ia;  // (lo is b)
    const double lo0 = (double)(sw ? qb[0] : qa[0]), hi0 = (double)(sw ? qa[0] : qb[0]);
    const double lo1 = (double)(sw ? qb[1] : qa[1]), hi1 = (double)(sw ? qa[1] : qb[1]);
    const double lo2 = (double)(sw ? qb[2] : qa[2]), hi2 = (double)(sw ? qa[2] : qb[2]);
    const double t = ((double)n - lo2) / (hi2 - lo2);
    const float c0 = (float)(lo0 + t * (hi0 - lo0));
    const float c1 = (float)(lo1 + t * (hi1 - lo1));
    const float qu = c0 / n, qv = c1 / n;
    const bool valid = isfinite(qu) && isfinite(qv) && fabsf(qu) <= kMeshMaxPixel && fabsf(qv) <= kMeshMaxPixel;
    poly.fx[SLOT] = valid ? (int)roundf(qu * 16.0f) : 0;
    poly.fy[SLOT] = valid ? (int)roundf(qv * 16.0f) : 0;
    poly.valid[SLOT] = valid ? 1 : 0;
    poly.iz[SLOT] = 1.0 / (double)n;
    const float b_hi = (float)t, b_lo = (float)(1.0 - t);
#pragma unroll
    for (int j = 0; j < 3; ++j) poly.B[SLOT][j] = j == CA ? (sw ? b_hi : b_lo) : j == CB ? (sw ? b_lo : b_hi) : 0.f;
}

// Face t against the plane: kClipWhole, kClipNone, or the number of pieces with `poly` complete.
template <bool LEFT>
__device__ __forceinline__ int mesh_clip_face(const RenderMeshParams &p, long long t, MeshClipPoly &poly) {
    size_t i0 = p.faces[6 * t], i1 = p.faces[6 * t + 1], i2 = p.faces[6 * t + 2];
    if (i0 >= (size_t)p.V || i1 >= (size_t)p.V || i2 >= (size_t)p.V) return kClipWhole;  // (never; refused there)
    MeshVertex v0 = mesh_vertex(p.proj, i0), v1 = mesh_vertex(p.proj, i1), v2 = mesh_vertex(p.proj, i2);
    const float n = p.near;
    // (a NaN is behind)
    const bool f0 = __uint_as_float(v0.a2) >= n, f1 = __uint_as_float(v1.a2) >= n, f2 = __uint_as_float(v2.a2) >= n;
    const int front = (int)f0 + (int)f1 + (int)f2;
    if (front == 3) return kClipWhole;
    if (front == 0) return kClipNone;
    // one in front: Q0 is that corner; two in front: Q2 is the corner behind
    const int r = front == 1 ? (f0 ? 0 : f1 ? 1 : 2) : (!f2 ? 0 : !f0 ? 1 : 2);
    poly.r = r;
    mesh_rotate(i0, i1, i2, r);
    mesh_rotate(v0, v1, v2, r);
    const float *__restrict__ q = p.verts;
    float a0[3], a1[3], a2[3];
    mesh_project_rows<LEFT>(p.M, p.s, q[3 * i0], q[3 * i0 + 1], q[3 * i0 + 2], a0);
    mesh_project_rows<LEFT>(p.M, p.s, q[3 * i1], q[3 * i1 + 1], q[3 * i1 + 2], a1);
    mesh_project_rows<LEFT>(p.M, p.s, q[3 * i2], q[3 * i2 + 1], q[3 * i2 + 2], a2);
    mesh_clip_corner<0, 0>(poly, v0);
    if (front == 1) {
        mesh_clip_vertex<1, 0, 1>(poly, a0, i0, a1, i1, n);
        mesh_clip_vertex<2, 2, 0>(poly, a2, i2, a0, i0, n);
        // (slot 3 belongs to piece 1, which this face has not: set so that no select reads garbage)
        poly.fx[3] = poly.fy[3] = poly.valid[3] = 0;
        poly.iz[3] = 0.0;
        poly.B[3][0] = poly.B[3][1] = poly.B[3][2] = 0.f;
        return 1;
    }
    mesh_clip_corner<1, 1>(poly, v1);
    mesh_clip_vertex<2, 1, 2>(poly, a1, i1, a2, i2, n);
    mesh_clip_vertex<3, 2, 0>(poly, a2, i2, a0, i0, n);
    return 2;
}

// The piece of polygon slots (0, B, C) as a triangle of its own: its class as mesh_tri_setup gives it
template <int B, int C>
__device__ __forceinline__ int mesh_clip_piece_of(const RenderMeshParams &p, const MeshClipPoly &poly, MeshTri &tri) {
    if (!(poly.valid[0] && poly.valid[B] && poly.valid[C])) return kMeshRefused;
    tri.x0 = poly.fx[0], tri.y0 = poly.fy[0];
    tri.x1 = poly.fx[B], tri.y1 = poly.fy[B];
    tri.x2 = poly.fx[C], tri.y2 = poly.fy[C];
    if (const int cls = mesh_tri_box(p, tri); cls != kMeshDrawn) return cls;
    tri.iz0 = poly.iz[0], tri.iz1 = poly.iz[B], tri.iz2 = poly.iz[C];
    return kMeshDrawn;
}

__device__ __forceinline__ int mesh_clip_piece(const RenderMeshParams &p, const MeshClipPoly &poly, int k,
                                               MeshTri &tri) {
    return k == 0 ? mesh_clip_piece_of<1, 2>(p, poly, tri) : mesh_clip_piece_of<2, 3>(p, poly, tri);
}

// w_j = (t_0 * B_0j + t_1 * B_1j) + t_2 * B_2j of piece k, turned back to the face's corner order
__device__ __forceinline__ void mesh_clip_weights(const MeshClipPoly &poly, int k, double t0, double t1, double t2,
                                                  double &w0, double &w1, double &w2) {
    double w[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double b0 = (double)poly.B[0][j];
        const double b1 = (double)(k == 0 ? poly.B[1][j] : poly.B[2][j]);
        const double b2 = (double)(k == 0 ? poly.B[2][j] : poly.B[3][j]);
        w[j] = (t0 * b0 + t1 * b1) + t2 * b2;
    }
    // (corner j of the face is Q_{(j - r) mod 3})
    const int r = poly.r;
    w0 = r == 0 ? w[0] : r == 1 ? w[2] : w[1];
    w1 = r == 0 ? w[1] : r == 1 ? w[0] : w[2];
    w2 = r == 0 ? w[2] : r == 1 ? w[1] : w[0];
}

// A straddling face's pieces by a whole wave (t and poly are uniform over it): the face's class and,
// added to `drawn`, its DRAWN pieces -- the same in every lane.
__device__ __forceinline__ int mesh_clip_sweep_wave(const RenderMeshParams &p, const MeshClipPoly &poly, int pieces,
                                                    uint32_t t, int lane, unsigned &drawn) {
    int best = kMeshRefused;
    for (int k = 0; k < pieces; ++k) {
        MeshTri tri;
        int cls = mesh_clip_piece(p, poly, k, tri);
        if (cls == kMeshDrawn) {
            if (mesh_sweep_wave(p, tri, t, lane)) ++drawn;
            else cls = kMeshEmpty;
        }
        best = min(best, cls);
    }
    return best;
}

// Face t by a whole wave, whichever kind it is (t is uniform over the wave): its class
template <bool LEFT>
__device__ __forceinline__ int mesh_clip_face_wave(const RenderMeshParams &p, uint32_t t, int lane, unsigned &drawn) {
    MeshClipPoly poly;
    const int pieces = mesh_clip_face<LEFT>(p, t, poly);
    if (pieces > 0) return mesh_clip_sweep_wave(p, poly, pieces, t, lane, drawn);
    MeshTri tri;
    const int cls = mesh_tri_setup(p, t, tri);  // (kMeshDrawn: the raster listed it)
    if (cls != kMeshDrawn) return cls;
    return mesh_sweep_wave(p, tri, t, lane) ? kMeshDrawn : kMeshEmpty;
}

// the workgroup's clip counts into the render's: as mesh_classes_out
__device__ __forceinline__ void mesh_clip_counts_out(unsigned (&s_c)[kClipCounts], unsigned long long *clip) {
    __syncthreads();
    if (threadIdx.x < kClipCounts && s_c[threadIdx.x]) atomicAdd(clip + threadIdx.x, (unsigned long long)s_c[threadIdx.x]);
}

// One lane per face; the grid strides over the faces.  A listed face is counted by
// render_mesh_clip_large_kernel, every other one here; behind, straddling and pieces made are all
// counted here.
template <bool LEFT>
__global__ __launch_bounds__(256) void render_mesh_clip_raster_kernel(const RenderMeshParams p) {
    __shared__ unsigned s_n[kMeshClasses], s_c[kClipCounts];
    if (threadIdx.x < kMeshClasses) s_n[threadIdx.x] = 0;
    if (threadIdx.x < kClipCounts) s_c[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned mine[kMeshClasses] = {0, 0, 0, 0};  // (wave sweeps are counted by lane 0)
    unsigned clip[kClipCounts] = {0, 0, 0, 0};
    for (long long base = (long long)blockIdx.x * 256; base < p.T; base += (long long)gridDim.x * 256) {
        const long long t = base + threadIdx.x;
        bool wide = false;  // large, and the list had no room
        if (t < p.T) {
            MeshClipPoly poly;
            const int pieces = mesh_clip_face<LEFT>(p, t, poly);
            int cls;
            int c0 = 0, c1 = 0, r0 = 0, r1 = 0;  // the box to list
            bool large = false;
            if (pieces == kClipWhole) {
                MeshTri tri;
                cls = mesh_tri_setup(p, t, tri);
                if (cls == kMeshDrawn) {
                    if ((tri.c1 - tri.c0 + 1) * (tri.r1 - tri.r0 + 1) <= kMeshLanePixels) {
                        bool any = false;
                        for (int r = tri.r0; r <= tri.r1; ++r)
                            for (int c = tri.c0; c <= tri.c1; ++c) any |= mesh_pixel(p, tri, (uint32_t)t, c, r);
                        if (!any) cls = kMeshEmpty;
                    } else {
                        large = true;
                        c0 = tri.c0, c1 = tri.c1, r0 = tri.r0, r1 = tri.r1;
                    }
                }
            } else if (pieces == kClipNone) {
                cls = kMeshRefused;
                ++clip[kClipBehind];
            } else {
                ++clip[kClipStraddle];
                clip[kClipPieces] += (unsigned)pieces;
                // the pieces' boxes together (each at most 2^28 pixels)
                long long area = 0;
                c0 = p.W, c1 = -1, r0 = p.H, r1 = -1;
                for (int k = 0; k < pieces; ++k) {
                    MeshTri tri;
                    if (mesh_clip_piece(p, poly, k, tri) != kMeshDrawn) continue;
                    area += (long long)(tri.c1 - tri.c0 + 1) * (tri.r1 - tri.r0 + 1);
                    c0 = min(c0, tri.c0), c1 = max(c1, tri.c1), r0 = min(r0, tri.r0), r1 = max(r1, tri.r1);
                }
                if (area <= kMeshLanePixels) {
                    cls = kMeshRefused;
                    for (int k = 0; k < pieces; ++k) {
                        MeshTri tri;
                        int ck = mesh_clip_piece(p, poly, k, tri);
                        if (ck == kMeshDrawn) {
                            bool any = false;
                            for (int r = tri.r0; r <= tri.r1; ++r)
                                for (int c = tri.c0; c <= tri.c1; ++c) any |= mesh_pixel(p, tri, (uint32_t)t, c, r);
                            if (any) ++clip[kClipDrawn];
                            else ck = kMeshEmpty;
                        }
                        cls = min(cls, ck);
                    }
                } else {
                    large = true;
                }
            }
            if (large) {
                cls = -1;  // counted where it is swept
                const unsigned k = atomicAdd(&p.head->n_large, 1u);
                if (k < p.large_cap)
                    p.large[k] = SplatRect{(uint32_t)c0 | ((uint32_t)c1 << 16), (uint32_t)r0 | ((uint32_t)r1 << 16),
                                           (uint32_t)t, (uint32_t)pieces};
                else
                    wide = true;
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
            unsigned drawn = 0;
            const int cls = mesh_clip_face_wave<LEFT>(p, (uint32_t)(wave_t0 + l), lane, drawn);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < kMeshClasses; ++k) mine[k] += cls == k ? 1u : 0u;
                clip[kClipDrawn] += drawn;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kMeshClasses; ++k)
        if (mine[k]) atomicAdd(&s_n[k], mine[k]);
#pragma unroll
    for (int k = 0; k < kClipCounts; ++k)
        if (clip[k]) atomicAdd(&s_c[k], clip[k]);
    mesh_classes_out(s_n, p.head);
    mesh_clip_counts_out(s_c, p.clip);
}

// One wave per listed face, as render_mesh_large_kernel.
template <bool LEFT>
__global__ __launch_bounds__(256) void render_mesh_clip_large_kernel(const RenderMeshParams p,
                                                                     long long *__restrict__ need) {
    __shared__ unsigned s_n[kMeshClasses], s_c[kClipCounts];
    if (threadIdx.x < kMeshClasses) s_n[threadIdx.x] = 0;
    if (threadIdx.x < kClipCounts) s_c[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned waves = gridDim.x * 4;
    const unsigned wanted = p.head->n_large;
    if (blockIdx.x == 0 && threadIdx.x == 0) *need = (long long)wanted;
    const unsigned n = min(wanted, p.large_cap);
    unsigned mine[kMeshClasses] = {0, 0, 0, 0};
    unsigned drawn = 0;
    for (unsigned f = blockIdx.x * 4 + (threadIdx.x >> 6); f < n; f += waves) {
        const uint32_t t = p.large[f].view;
        if ((long long)t >= p.T) continue;  // (never: the raster listed it)
        const int cls = mesh_clip_face_wave<LEFT>(p, t, lane, drawn);
#pragma unroll
        for (int k = 0; k < kMeshClasses; ++k) mine[k] += cls == k ? 1u : 0u;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kMeshClasses; ++k)
            if (mine[k]) atomicAdd(&s_n[k], mine[k]);
        if (drawn) atomicAdd(&s_c[kClipDrawn], drawn);
    }
    mesh_classes_out(s_n, p.head);
    mesh_clip_counts_out(s_c, p.clip);
}

// One lane per pixel, as render_mesh_resolve_kernel.
template <class Colour, bool LEFT>
__global__ __launch_bounds__(256) void render_mesh_clip_resolve_kernel(const RenderMeshParams p, size_t npix,
                                                                       int *__restrict__ id,
                                                                       float *__restrict__ depth,
                                                                       uint8_t *__restrict__ bgr, const Colour colour) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long key = p.keys[i];
    const uint32_t t = (uint32_t)key;
    const int c = (int)(i % (size_t)p.W), r = (int)(i / (size_t)p.W);
    bool found = false;
    double w0 = 0, w1 = 0, w2 = 0, S = 0;
    if (key != kRenderEmpty && (long long)t < p.T) {
        MeshClipPoly poly;
        const int pieces = mesh_clip_face<LEFT>(p, t, poly);
        MeshTri tri;
        long long e0, e1, e2;
        if (pieces == kClipWhole) {
            if (mesh_tri_setup(p, t, tri) == kMeshDrawn) {
                (void)mesh_edges(tri, c, r, e0, e1, e2);
                S = mesh_weights(tri, e0, e1, e2, w0, w1, w2);
                found = true;
            }
        } else {
            // the least piece that covers the pixel with exactly the winner's depth
            for (int k = 0; k < pieces && !found; ++k) {
                if (mesh_clip_piece(p, poly, k, tri) != kMeshDrawn) continue;
                if (c < tri.c0 || c > tri.c1 || r < tri.r0 || r > tri.r1) continue;
                if (!mesh_edges(tri, c, r, e0, e1, e2)) continue;
                double t0, t1, t2;
                S = mesh_weights(tri, e0, e1, e2, t0, t1, t2);
                if (__float_as_uint((float)((double)tri.A / S)) != (uint32_t)(key >> 32)) continue;
                mesh_clip_weights(poly, k, t0, t1, t2, w0, w1, w2);
                found = true;
            }
        }
    }
    if (!found) {
        id[i] = -1;
        depth[i] = INFINITY;
        return;
    }
    mesh_pixel_out(p, i, key, w0, w1, w2, S, id, depth, bgr, colour);
}

}  // namespace arvx
