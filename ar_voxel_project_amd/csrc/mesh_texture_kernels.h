// mesh_texture_kernels.h -- a held mesh's faces textured from the photographs for gfx950: an atlas with
// one small triangle of texels per face, sampled from the view that sees the face's three corners and
// shows it largest (arvx_mesh_texture; the definition is in include/arvx/arvx.h, after the mesh
// colours' block).
//
// The depth pass is arvx_mesh_color's (mesh_color_kernels.h), run by the same host code.  Then:
//   mesh_texture_visible_kernel  one lane per vertex: the vote kernel's visibility test in every view,
//                                a bit per view -- ceil(V / 32) words per vertex, word-major
//   mesh_texture_select_kernel   one lane per face: the AND of its corners' words, the three corners
//                                projected once more in the surviving views only, the greatest |A|;
//                                the textured faces are counted per workgroup (the one atomic)
//   mesh_texture_fill_kernel     one lane per four consecutive texels of the atlas taken as one flat
//                                array: 12 bytes, three dword stores, so a wave writes 768 contiguous
//                                bytes whatever the resolution -- a mesh of many small cells and one
//                                of few large cells are the same stream of texels.  A texel finds
//                                its cell, half and local coordinates by multiplications with the
//                                launch's reciprocals (TextureLayout), its face's record is read again
//                                only when the face changes within the lane.  The last one to three
//                                texels of the atlas are stored as bytes.
// render_mesh_resolve_kernel (render_mesh_kernels.h) reads the atlas through TextureLayout when it is
// instantiated for a textured draw.  All stores are ordinary vector stores.
#pragma once

#include "mesh_color_kernels.h"

namespace arvx {

struct MeshVisibleParams {
    const float *verts;  // Vn x 3
    long long Vn;
    float s;
    int V, W, H, words;  // words = ceil(V / 32)
    const SelftestMatrix *M;
    const unsigned long long *keys;  // V x H x W
    const uint32_t *bg;              // null: the flag is not set
    int bgWords;
    float tol;
    uint32_t *bits;  // words x Vn
};

template <bool LEFT>
__global__ __launch_bounds__(256) void mesh_texture_visible_kernel(const MeshVisibleParams p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.Vn) return;
    const float px = p.verts[3 * i], py = p.verts[3 * i + 1], pz = p.verts[3 * i + 2];
    const size_t npix = (size_t)p.W * p.H;
    for (int w = 0; w < p.words; ++w) {
        uint32_t word = 0;
        const int v1 = min(32 * w + 32, p.V);
        for (int v = 32 * w; v < v1; ++v) {
            const SelftestMatrix M = p.M[v];
            const MeshVertex q = mesh_project<LEFT>(M, p.s, px, py, pz);
            if (!q.valid || q.fx < 0 || q.fy < 0 || q.fx > 16 * (p.W - 1) || q.fy > 16 * (p.H - 1)) continue;
            const size_t pix = (size_t)((q.fy + 8) >> 4) * p.W + (size_t)((q.fx + 8) >> 4);
            const unsigned long long key = p.keys[(size_t)v * npix + pix];
            const float D = key == kRenderEmpty ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
            if (!(__uint_as_float(q.a2) <= D + p.tol)) continue;
            if (p.bg && ((p.bg[(size_t)v * p.bgWords + (pix >> 5)] >> (pix & 31)) & 1u)) continue;
            word |= 1u << (v & 31);
        }
        p.bits[(size_t)w * (size_t)p.Vn + (size_t)i] = word;
    }
}

struct MeshSelectParams {
    const float *verts;
    const unsigned *faces;  // T x 6
    long long Vn, T;
    float s;
    int V, words;
    const SelftestMatrix *M;
    const uint32_t *bits;
    int *face_view;  // T
    unsigned long long *textured;
};

template <bool LEFT>
__global__ __launch_bounds__(256) void mesh_texture_select_kernel(const MeshSelectParams p) {
    __shared__ unsigned s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    int best = -1;
    if (t < p.T) {
        const size_t i0 = p.faces[6 * t], i1 = p.faces[6 * t + 1], i2 = p.faces[6 * t + 2];
        if (i0 < (size_t)p.Vn && i1 < (size_t)p.Vn && i2 < (size_t)p.Vn) {  // (always)
            const float *__restrict__ q = p.verts;
            long long most = 0;
            for (int w = 0; w < p.words; ++w) {
                const size_t o = (size_t)w * (size_t)p.Vn;
                uint32_t m = p.bits[o + i0] & p.bits[o + i1] & p.bits[o + i2];
                while (m) {  // (ascending views: a later view wins only with a greater area)
                    const int v = 32 * w + __ffs((int)m) - 1;
                    m &= m - 1;
                    const SelftestMatrix M = p.M[v];
                    const MeshVertex a = mesh_project<LEFT>(M, p.s, q[3 * i0], q[3 * i0 + 1], q[3 * i0 + 2]);
                    const MeshVertex b = mesh_project<LEFT>(M, p.s, q[3 * i1], q[3 * i1 + 1], q[3 * i1 + 2]);
                    const MeshVertex c = mesh_project<LEFT>(M, p.s, q[3 * i2], q[3 * i2 + 1], q[3 * i2 + 2]);
                    long long A = mesh_det(b.fx - a.fx, c.fy - a.fy, c.fx - a.fx, b.fy - a.fy);
                    if (A < 0) A = -A;
                    if (A > most) most = A, best = v;
                }
            }
        }
        p.face_view[t] = best;
    }
    const unsigned long long seen = __ballot(best >= 0);
    if ((threadIdx.x & 63) == 0 && seen) atomicAdd(&s_n, (unsigned)__popcll(seen));
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(p.textured, (unsigned long long)s_n);
}

// Step 1 of the definition: where a texel lies.  The divisions by cw and ch are multiplications with
// floor(2^32 / d) + 1: exact for every n < 2^32 / d, and x < 2^14, y < 2^15, d <= 256.
struct TextureLayout {
    int R, AW, AH, cw, ch, per_row;
    long long T;
    uint32_t inv_cw, inv_ch;
};

__host__ __device__ inline TextureLayout texture_layout(long long T, int R, int AW) {
    TextureLayout l{};
    l.R = R, l.AW = AW, l.T = T;
    l.cw = R + 3, l.ch = R + 2;
    l.per_row = AW / l.cw;
    const long long cells = (T + 1) / 2;
    l.AH = (int)((cells + l.per_row - 1) / l.per_row) * l.ch;
    l.inv_cw = (uint32_t)(0x100000000ull / (unsigned)l.cw) + 1u;
    l.inv_ch = (uint32_t)(0x100000000ull / (unsigned)l.ch) + 1u;
    return l;
}

__host__ __device__ inline uint32_t texture_div(uint32_t n, uint32_t inv) {
    return (uint32_t)(((unsigned long long)n * inv) >> 32);
}

// the atlas texel of local texel (i, j) of face f
__host__ __device__ inline void texture_texel(const TextureLayout &l, long long f, int i, int j, int &x, int &y) {
    const long long k = f >> 1;
    x = (int)(k % l.per_row) * l.cw, y = (int)(k / l.per_row) * l.ch;
    if (f & 1) x += l.cw - 1 - i, y += l.ch - 1 - j;
    else x += i, y += j;
}

// the face and the local texel of atlas texel (x, y); false where the texel belongs to no face
__device__ __forceinline__ bool texture_owner(const TextureLayout &l, uint32_t x, uint32_t y, long long &f, int &i,
                                              int &j) {
    const uint32_t kc = texture_div(x, l.inv_cw), kr = texture_div(y, l.inv_ch);
    if (kc >= (uint32_t)l.per_row) return false;  // the padding columns
    i = (int)(x - kc * (uint32_t)l.cw), j = (int)(y - kr * (uint32_t)l.ch);
    f = 2 * ((long long)kr * l.per_row + kc);
    if (i + j > l.R + 1) i = l.cw - 1 - i, j = l.ch - 1 - j, ++f;
    return f < l.T;  // (the unused cells, and the second half of the last cell of an odd T)
}

// Step 6 of the definition: the resolve kernel's Colour of a textured draw -- the texel nearest to the
// pixel's perspective-correct position in the face, as a float per channel r, g, b.
struct MeshTextureColour {
    const uint8_t *atlas;
    TextureLayout lay;
    __device__ __forceinline__ void operator()(const RenderMeshParams &, uint32_t t, size_t, size_t, size_t, double,
                                               double t1, double t2, double S, float (&v)[3]) const {
        const int i = min(max((int)floor((t1 / S) * (double)lay.R + 0.5), 0), lay.R);
        const int j = min(max((int)floor((t2 / S) * (double)lay.R + 0.5), 0), lay.R);
        int x, y;
        texture_texel(lay, (long long)t, i, j, x, y);
        const uint8_t *__restrict__ texel = atlas + ((size_t)y * lay.AW + x) * 3;
        v[0] = (float)texel[2], v[1] = (float)texel[1], v[2] = (float)texel[0];
    }
};

struct MeshFillParams {
    const float *verts, *col;  // Vn x 3 each
    const unsigned *faces;
    long long Vn;
    float s;
    int W, H;
    const SelftestMatrix *M;
    const uint8_t *images;  // V x H x W x 3, BGR
    const int *face_view;
    TextureLayout lay;
    uint8_t *atlas;  // AH x AW x 3
};

// b0 * a0 + b1 * a1 + b2 * a2 over R, as steps 3 and 4 write it
__device__ __forceinline__ float texture_blend(int b0, int b1, int b2, float a0, float a1, float a2, double R) {
    return (float)((((double)b0 * (double)a0 + (double)b1 * (double)a1) + (double)b2 * (double)a2) / R);
}

template <bool LEFT>
__global__ __launch_bounds__(256) void mesh_texture_fill_kernel(const MeshFillParams p) {
    const TextureLayout l = p.lay;
    const size_t ntex = (size_t)l.AW * (size_t)l.AH;
    const size_t first = 4 * ((size_t)blockIdx.x * 256 + threadIdx.x);
    if (first >= ntex) return;
    const double R = (double)l.R;
    uint32_t y = (uint32_t)(first / (size_t)l.AW), x = (uint32_t)(first - (size_t)y * l.AW);
    uint32_t texel[4] = {0, 0, 0, 0};  // B | G << 8 | R << 16 each (indexed by unrolled loops only: registers)
    long long cur = -1;                // the face whose record the lane holds
    int view = -1;
    size_t i0 = 0, i1 = 0, i2 = 0;
    SelftestMatrix M{};
    const int n = (int)min((size_t)4, ntex - first);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        long long f;
        int i, j;
        if (k < n && texture_owner(l, x, y, f, i, j)) {
            if (f != cur) {
                cur = f;
                i0 = p.faces[6 * f], i1 = p.faces[6 * f + 1], i2 = p.faces[6 * f + 2];
                view = p.face_view[f];
                if (i0 >= (size_t)p.Vn || i1 >= (size_t)p.Vn || i2 >= (size_t)p.Vn) i0 = i1 = i2 = 0, view = -1;  // (never)
                if (view >= 0) M = p.M[view];
            }
            const int b1 = i, b2 = j, b0 = l.R - i - j;
            bool sampled = false;
            if (view >= 0) {
                const float *__restrict__ q = p.verts;
                const float qx = texture_blend(b0, b1, b2, q[3 * i0], q[3 * i1], q[3 * i2], R);
                const float qy = texture_blend(b0, b1, b2, q[3 * i0 + 1], q[3 * i1 + 1], q[3 * i2 + 1], R);
                const float qz = texture_blend(b0, b1, b2, q[3 * i0 + 2], q[3 * i1 + 2], q[3 * i2 + 2], R);
                const MeshVertex pr = mesh_project<LEFT>(M, p.s, qx, qy, qz);
                if (pr.valid) {
                    sampled = true;
                    const int fx = min(max(pr.fx, 0), 16 * (p.W - 1)), fy = min(max(pr.fy, 0), 16 * (p.H - 1));
                    const int c0 = fx >> 4, r0 = fy >> 4;
                    const unsigned wx = (unsigned)(fx & 15), wy = (unsigned)(fy & 15);
                    const int c1 = min(c0 + 1, p.W - 1), r1 = min(r0 + 1, p.H - 1);
                    const uint8_t *__restrict__ img = p.images + (size_t)view * ((size_t)p.W * p.H) * 3;
                    const uint8_t *p00 = img + ((size_t)r0 * p.W + c0) * 3, *p01 = img + ((size_t)r0 * p.W + c1) * 3;
                    const uint8_t *p10 = img + ((size_t)r1 * p.W + c0) * 3, *p11 = img + ((size_t)r1 * p.W + c1) * 3;
                    const unsigned w00 = (16 - wx) * (16 - wy), w01 = wx * (16 - wy), w10 = (16 - wx) * wy, w11 = wx * wy;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch)  // (B, G, R as the image stores them; S + 128 < 2^16)
                        texel[k] |= ((w00 * p00[ch] + w01 * p01[ch] + w10 * p10[ch] + w11 * p11[ch] + 128u) >> 8) << (8 * ch);
                }
            }
            if (!sampled) {
                const float *__restrict__ c = p.col;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    texel[k] |= (uint32_t)render_channel(texture_blend(b0, b1, b2, c[3 * i0 + ch], c[3 * i1 + ch],
                                                                       c[3 * i2 + ch], R))
                                << (8 * (2 - ch));
            }
        }
        if (++x == (uint32_t)l.AW) x = 0, ++y;
    }
    if (n == 4) {
        uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(p.atlas + 3 * first);  // (12 * lane: aligned)
        dst[0] = texel[0] | (texel[1] << 24);
        dst[1] = (texel[1] >> 8) | (texel[2] << 16);
        dst[2] = (texel[2] >> 16) | (texel[3] << 8);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < n) {
                uint8_t *__restrict__ dst = p.atlas + 3 * (first + k);
                dst[0] = (uint8_t)texel[k], dst[1] = (uint8_t)(texel[k] >> 8), dst[2] = (uint8_t)(texel[k] >> 16);
            }
    }
}

}  // namespace arvx
