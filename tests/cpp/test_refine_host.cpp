// test_refine_host.cpp -- arvx::marchingCubesMeshRefined (include/arvx/marching_cubes.hpp) on a scene
// from a file, for tests/test_mc_refine_gpu.py.
//
//   test_refine_host <scene> <out> <bisections> <fractional>
//   scene: tests/cpp/test_host.cpp's scene file -- int32 X, Y, Z, V, W, H, C; float s; float K[9];
//          V * (float pose[12]); V*H*W*C mask bytes; V*H*W*3 image bytes; X*Y*Z initial state bytes
//   out:   int64 Vr, T; 3 Vr floats of positions; 6 T uints of face records
//   The model is carved with the scene's views and meshed with the same views.  fractional != 0: one
//   occupied voxel gets w = 0.5 first, the call must throw, and nothing is written (exit status 0
//   when it threw, 4 when it did not).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "arvx/marching_cubes.hpp"

using arvx::Model;
using arvx::Vec4f;

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: test_refine_host <scene> <out> <bisections> <fractional>\n");
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
    const bool fractional = std::atoi(argv[4]) != 0;
    try {
        Model model(X, Y, Z, s);
        for (int z = 0; z < Z; ++z)
            for (int y = 0; y < Y; ++y)
                for (int x = 0; x < X; ++x) {
                    const uint8_t b = st0[(size_t)x + (size_t)X * (y + (size_t)Y * z)];
                    if (!(b & 1)) model.set(x, y, z, Vec4f(0, 0, 0, 0));
                    if (b & 2) model.see(x, y, z);
                }
        arvx::carve(intr, model, views);
        if (fractional) {
            bool set = false;
            for (int z = 0; z < Z && !set; ++z)
                for (int y = 0; y < Y && !set; ++y)
                    for (int x = 0; x < X && !set; ++x)
                        if (model.get(x, y, z).w() != 0.f) {
                            model.set(x, y, z, Vec4f(1, 2, 3, 0.5f));
                            set = true;
                        }
            if (!set) return 5;
            try {
                (void)arvx::marchingCubesMeshRefined(intr, &model, views, bisections);
            } catch (const arvx::Error &e) {
                std::printf("refused: %s\n", e.what());
                return 0;
            }
            return 4;
        }
        const arvx::SimpleMesh mesh = arvx::marchingCubesMeshRefined(intr, &model, views, bisections);
        const int64_t n[2] = {(int64_t)mesh.GetVertices().size(), (int64_t)mesh.GetTriangles().size()};
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char *)n, sizeof n);
        if (n[0]) o.write((const char *)mesh.GetVertices()[0].data(), (std::streamsize)(n[0] * 12));
        if (n[1]) o.write((const char *)&mesh.GetTriangles()[0].idx0, (std::streamsize)(n[1] * 24));
        if (!o) return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
    return 0;
}
