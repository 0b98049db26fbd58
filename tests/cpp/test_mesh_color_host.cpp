// test_mesh_color_host.cpp -- arvx::colorMesh and arvx::renderMesh with ARVX_MESH_IMAGE_COLORS
// (include/arvx/marching_cubes.hpp) on a scene from a file, for tests/test_mesh_color_cpp_gpu.py.
//
//   test_mesh_color_host <scene> <out> <bisections> <view> <mode> <tolerance in voxel edges> <flags>
//   scene: tests/cpp/test_host.cpp's scene file -- int32 X, Y, Z, V, W, H, C; float s; float K[9];
//          V * (float pose[12]); V*H*W*C mask bytes; V*H*W*3 image bytes; X*Y*Z initial state bytes
//   out:   int64 Vn, int64 coloured, 3 Vn floats of rgb, Vn ints of views, then one render: W*H*3 bytes
//          of bgr, W*H floats of depth, W*H ints of id
//   The model is carved with the scene's views, meshed by marchingCubesMeshRefined and coloured by
//   colorMesh(ARVX_MESH_REFINED); the render is renderMesh(ARVX_MESH_REFINED | ARVX_MESH_IMAGE_COLORS)
//   from view <view> over its image with a light at the camera.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "arvx/marching_cubes.hpp"

using arvx::Model;

int main(int argc, char **argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: test_mesh_color_host <scene> <out> <bisections> <view> <mode> <tol> <flags>\n");
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
    const int bisections = std::atoi(argv[3]), view = std::atoi(argv[4]), mode = std::atoi(argv[5]);
    const float tolerance = (float)std::atof(argv[6]) * s;
    const unsigned flags = (unsigned)std::atoi(argv[7]);
    if (view < 0 || view >= V) return 2;
    try {
        Model model(X, Y, Z, s);
        arvx::carve(intr, model, views);
        float M[12];
        arvx::detail::check(arvx_compose_projection(intr.K, views[(size_t)view].pose, M), "arvx_compose_projection");
        const float light[3] = {M[9], M[8], -M[10]};
        const uint8_t *bg = images.data() + (size_t)view * H * W * 3;
        const int drawn = ARVX_MESH_REFINED | ARVX_MESH_IMAGE_COLORS;
        const arvx::SimpleMesh mesh = arvx::marchingCubesMeshRefined(intr, &model, views, bisections);
        bool threw = false;
        try {  // no image colours yet
            (void)arvx::renderMesh(&model, drawn, M, W, H, bg, light);
        } catch (const arvx::Error &) {
            threw = true;
        }
        if (!threw) return 4;
        const arvx::MeshColors col = arvx::colorMesh(intr, &model, views, ARVX_MESH_REFINED, mode, tolerance, flags);
        const size_t Vn = col.views.size();
        if (Vn != mesh.GetVertices().size()) return 5;
        const arvx::RenderedView r = arvx::renderMesh(&model, drawn, M, W, H, bg, light);
        std::ofstream o(argv[2], std::ios::binary);
        const int64_t head[2] = {(int64_t)Vn, col.coloured};
        o.write((const char *)head, sizeof head);
        o.write((const char *)col.rgb.data(), (std::streamsize)(col.rgb.size() * sizeof(float)));
        o.write((const char *)col.views.data(), (std::streamsize)(col.views.size() * sizeof(int32_t)));
        o.write((const char *)r.bgr.data(), (std::streamsize)r.bgr.size());
        o.write((const char *)r.depth.data(), (std::streamsize)(r.depth.size() * sizeof(float)));
        o.write((const char *)r.id.data(), (std::streamsize)(r.id.size() * sizeof(int32_t)));
        if (!o) return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
    return 0;
}
