// test_render_mesh_clip_host.cpp -- arvx::setRenderNear, arvx::renderNear, arvx::renderMeshClipStats
// and both arvx::renderMesh overloads under a near plane (include/arvx/marching_cubes.hpp) on a scene
// from a file, for tests/test_render_mesh_clip_gpu.py.
//
//   test_render_mesh_clip_host <scene> <out> <bisections> <near> <M0> ... <M11>
//   scene: tests/cpp/test_host.cpp's scene file (test_render_mesh_host.cpp describes it)
//   near, M: floats as strtof reads them (hexadecimal floats are exact); M is the camera, which may
//          stand inside the mesh
//   out:   two renders, each W*H*3 bytes of bgr, W*H floats of depth, W*H ints of id, each followed by
//          its four clip counts (int64)
//   The model is carved with the scene's views and meshed by marchingCubesMeshRefined.  The first
//   render is renderMesh(ARVX_MESH_REFINED) from M with a light at the camera; the second is the
//   SimpleMesh overload on the mesh the call returned.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <vector>

#include "arvx/marching_cubes.hpp"

using arvx::Model;

static void write_view(std::ofstream &o, const arvx::RenderedView &r, const arvx::RenderClipStats &st) {
    o.write((const char *)r.bgr.data(), (std::streamsize)r.bgr.size());
    o.write((const char *)r.depth.data(), (std::streamsize)(r.depth.size() * sizeof(float)));
    o.write((const char *)r.id.data(), (std::streamsize)(r.id.size() * sizeof(int32_t)));
    const int64_t n[4] = {st.behind, st.straddling, st.pieces, st.piecesDrawn};
    o.write((const char *)n, sizeof n);
}

int main(int argc, char **argv) {
    if (argc < 17) {
        std::fprintf(stderr, "usage: test_render_mesh_clip_host <scene> <out> <bisections> <near> <M0> ... <M11>\n");
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    int32_t hd[7] = {0, 0, 0, 0, 0, 0, 0};
    f.read((char *)hd, sizeof hd);
    const int X = hd[0], Y = hd[1], Z = hd[2], V = hd[3], W = hd[4], H = hd[5], C = hd[6];
    float s = 0.f;
    f.read((char *)&s, 4);
    arvx::Intrinsics intr;
    f.read((char *)intr.K, 36);
    std::vector<arvx::View> views((size_t)V);
    for (auto &v : views) f.read((char *)v.pose, 48);
    std::vector<uint8_t> masks((size_t)V * H * W * C), images((size_t)V * H * W * 3), st0((size_t)X * Y * Z);
    f.read((char *)masks.data(), (std::streamsize)masks.size());
    f.read((char *)images.data(), (std::streamsize)images.size());
    f.read((char *)st0.data(), (std::streamsize)st0.size());
    if (!f) {
        std::fprintf(stderr, "short scene file\n");
        return 2;
    }
    for (int i = 0; i < V; ++i) {
        views[(size_t)i].mask = {masks.data() + (size_t)i * H * W * C, W, H, C, (size_t)W * C};
        views[(size_t)i].image = {images.data() + (size_t)i * H * W * 3, W, H, 3, (size_t)W * 3};
    }
    const int bisections = std::atoi(argv[3]);
    const float near = std::strtof(argv[4], nullptr);
    float M[12];
    for (int k = 0; k < 12; ++k) M[k] = std::strtof(argv[5 + k], nullptr);
    try {
        Model model(X, Y, Z, s);
        arvx::carve(intr, model, views);
        const float light[3] = {M[9], M[8], -M[10]};
        const arvx::SimpleMesh mesh = arvx::marchingCubesMeshRefined(intr, &model, views, bisections);
        if (arvx::renderNear(&model) != 0.f) return 4;  // (off by default)
        arvx::setRenderNear(&model, near);
        // an invalid plane throws and leaves the setting
        const float bad[3] = {-near, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
        for (float b : bad) {
            bool threw = false;
            try {
                arvx::setRenderNear(&model, b);
            } catch (const arvx::Error &) {
                threw = true;
            }
            if (!threw) return 5;
        }
        if (arvx::renderNear(&model) != near) return 6;
        std::ofstream o(argv[2], std::ios::binary);
        const arvx::RenderedView a = arvx::renderMesh(&model, ARVX_MESH_REFINED, M, W, H, nullptr, light);
        write_view(o, a, arvx::renderMeshClipStats(&model));
        const arvx::RenderedView b = arvx::renderMesh(&model, mesh, M, W, H, nullptr, light);
        write_view(o, b, arvx::renderMeshClipStats(&model));
        if (!o) return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
    return 0;
}
