// A mesh's texture atlas on the host (an extension beyond the reference): what arvx::textureMesh
// (include/arvx/marching_cubes.hpp) returns, the atlas layout of arvx_mesh_texture's definition
// (include/arvx/arvx.h) in plain integers, and a Wavefront OBJ writer.  Standard C++ only: nothing in
// this header needs the device or the library.
#ifndef ARVX_MESH_TEXTURE_HPP_
#define ARVX_MESH_TEXTURE_HPP_

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

namespace arvx {

struct MeshTexture {
    std::vector<uint8_t> atlas;      // AH x AW x 3, B, G, R; row 0 is the top row
    std::vector<int32_t> face_view;  // per face the view it was sampled from, or -1
    std::vector<float> face_uv;      // per face three corners (u, v), v downwards as in the atlas
    int64_t faces = 0, textured = 0;
    int width = 0, height = 0, resolution = 0;
};

// Step 1 of the definition: cells of (R + 3) x (R + 2) texels, two faces each.
struct MeshTextureLayout {
    int R = 0, AW = 0, AH = 0, cw = 0, ch = 0, per_row = 0;
    int64_t T = 0;
    MeshTextureLayout(int64_t faces, int resolution, int atlas_width)
        : R(resolution), AW(atlas_width), cw(resolution + 3), ch(resolution + 2), T(faces) {
        per_row = cw > 0 ? AW / cw : 0;
        const int64_t cells = (T + 1) / 2;
        AH = per_row > 0 ? (int)((cells + per_row - 1) / per_row) * ch : 0;
    }
    bool valid() const { return R >= 1 && R <= 253 && per_row >= 1 && AW <= 16384 && AH <= 32768 && T >= 0; }
    // the atlas texel of local texel (i, j) of face f: i, j >= 0, i + j <= R + 1
    void texel(int64_t f, int i, int j, int &x, int &y) const {
        const int64_t k = f >> 1;
        x = (int)(k % per_row) * cw;
        y = (int)(k / per_row) * ch;
        if (f & 1) {
            x += cw - 1 - i;
            y += ch - 1 - j;
        } else {
            x += i;
            y += j;
        }
    }
    // the face that owns atlas texel (x, y) and its local texel, or -1: padding, an unused cell or the
    // second half of the last cell of an odd T
    int64_t owner(int x, int y, int &i, int &j) const {
        const int kc = x / cw, kr = y / ch;
        if (x < 0 || y < 0 || x >= AW || y >= AH || kc >= per_row) return -1;
        i = x - kc * cw;
        j = y - kr * ch;
        int64_t f = 2 * ((int64_t)kr * per_row + kc);
        if (i + j > R + 1) {
            i = cw - 1 - i;
            j = ch - 1 - j;
            ++f;
        }
        return f < T ? f : -1;
    }
    // face_uv as arvx_mesh_texture_download computes it: 6 T floats
    std::vector<float> uv() const {
        std::vector<float> out(6 * (size_t)T);
        for (int64_t f = 0; f < T; ++f)
            for (int k = 0; k < 3; ++k) {
                int x, y;
                texel(f, k == 1 ? R : 0, k == 2 ? R : 0, x, y);
                out[6 * (size_t)f + 2 * k] = ((float)x + 0.5f) / (float)AW;
                out[6 * (size_t)f + 2 * k + 1] = ((float)y + 0.5f) / (float)AH;
            }
        return out;
    }
};

// Writes `path` (Wavefront OBJ: v, then per face three vt -- v flipped to OBJ's bottom-up convention --
// and f a/ta b/tb c/tc with 1-based indices, and mtllib), beside it <stem>.mtl with map_Kd and
// <stem>.ppm, the atlas as a binary PPM (R, G, B).  verts: 3 floats per vertex; faces: the first three
// of every `face_stride` unsigned are a face's vertex indices (6 for the library's face records).
inline bool writeOBJ(const std::string &path, const float *verts, size_t nv, const unsigned *faces, size_t nt,
                     size_t face_stride, const MeshTexture &tex) {
    if (tex.face_uv.size() != 6 * nt || tex.atlas.size() != (size_t)tex.width * (size_t)tex.height * 3) return false;
    const size_t dot = path.find_last_of('.'), slash = path.find_last_of("/\\");
    const std::string stem = dot != std::string::npos && (slash == std::string::npos || dot > slash) ? path.substr(0, dot) : path;
    const std::string base = slash == std::string::npos ? stem : stem.substr(slash + 1);
    {
        std::ofstream ppm(stem + ".ppm", std::ios::binary);
        ppm << "P6\n" << tex.width << " " << tex.height << "\n255\n";
        std::vector<uint8_t> row((size_t)tex.width * 3);
        for (int y = 0; y < tex.height; ++y) {
            const uint8_t *src = tex.atlas.data() + (size_t)y * row.size();
            for (size_t p = 0; p < row.size(); p += 3) {
                row[p] = src[p + 2];
                row[p + 1] = src[p + 1];
                row[p + 2] = src[p];
            }
            ppm.write((const char *)row.data(), (std::streamsize)row.size());
        }
        if (!ppm) return false;
    }
    {
        std::ofstream mtl(stem + ".mtl");
        mtl << "newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd " << base << ".ppm\n";
        if (!mtl) return false;
    }
    std::ofstream obj(path);
    obj << "mtllib " << base << ".mtl\nusemtl atlas\n";
    char line[128];
    for (size_t i = 0; i < nv; ++i) {
        std::snprintf(line, sizeof line, "v %.9g %.9g %.9g\n", (double)verts[3 * i], (double)verts[3 * i + 1],
                      (double)verts[3 * i + 2]);
        obj << line;
    }
    for (size_t k = 0; k < 3 * nt; ++k) {
        const float v = 1.0f - tex.face_uv[2 * k + 1];
        std::snprintf(line, sizeof line, "vt %.9g %.9g\n", (double)tex.face_uv[2 * k], (double)v);
        obj << line;
    }
    for (size_t t = 0; t < nt; ++t) {
        const unsigned *f = faces + t * face_stride;
        std::snprintf(line, sizeof line, "f %u/%zu %u/%zu %u/%zu\n", f[0] + 1, 3 * t + 1, f[1] + 1, 3 * t + 2, f[2] + 1,
                      3 * t + 3);
        obj << line;
    }
    obj.flush();
    return obj.good();
}

}  // namespace arvx
#endif
