// test_mesh_relax_host.cpp -- arvx::relaxMesh, both overloads (include/arvx/marching_cubes.hpp), on a
// scene from a file, for tests/test_mesh_relax_cpp_gpu.py.
//
//   test_mesh_relax_host <scene> <out> <bisections> <iterations> <lambda> <mu>
//   scene: tests/cpp/test_host.cpp's scene file -- int32 X, Y, Z, V, W, H, C; float s; float K[9];
//          V * (float pose[12]); V*H*W*C mask bytes; V*H*W*3 image bytes; X*Y*Z initial state bytes
//   out:   int64 Vn, int64 T, then 6 T uints of face records, 3 Vn floats of positions and 3 Vn floats of
//          normals from relaxMesh(model, ARVX_MESH_REFINED), and the same two arrays from
//          relaxMesh(model, <the refined mesh as a SimpleMesh>)
//   The model is carved with the scene's views and meshed by marchingCubesMeshRefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "arvx/marching_cubes.hpp"

using arvx::Model;

int main(int argc, char **argv) {
    if (argc < 7) {
        std::fprintf(stderr, "usage: test_mesh_relax_host <scene> <out> <bisections> <iterations> <lambda> <mu>\n");
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
    const int bisections = std::atoi(argv[3]), iterations = std::atoi(argv[4]);
    const float lambda = (float)std::atof(argv[5]), mu = (float)std::atof(argv[6]);
    try {
        Model model(X, Y, Z, s);
        arvx::carve(intr, model, views);
        bool threw = false;
        try {  // no refined mesh yet
            (void)arvx::relaxMesh(&model, ARVX_MESH_REFINED, iterations, lambda, mu);
        } catch (const arvx::Error &) {
            threw = true;
        }
        if (!threw) return 4;
        const arvx::SimpleMesh refined = arvx::marchingCubesMeshRefined(intr, &model, views, bisections);
        std::vector<float> n1, n2;
        const arvx::SimpleMesh a = arvx::relaxMesh(&model, ARVX_MESH_REFINED, iterations, lambda, mu, &n1);
        const arvx::SimpleMesh b = arvx::relaxMesh(&model, refined, iterations, lambda, mu, &n2);
        const size_t Vn = refined.GetVertices().size(), T = refined.GetTriangles().size();
        if (a.GetVertices().size() != Vn || b.GetVertices().size() != Vn || a.GetTriangles().size() != T ||
            b.GetTriangles().size() != T || n1.size() != 3 * Vn || n2.size() != 3 * Vn || Vn == 0 || T == 0)
            return 5;
        std::ofstream o(argv[2], std::ios::binary);
        const int64_t head[2] = {(int64_t)Vn, (int64_t)T};
        o.write((const char *)head, sizeof head);
        o.write((const char *)&a.GetTriangles()[0].idx0, (std::streamsize)(T * sizeof(arvx::Triangle)));
        o.write((const char *)a.GetVertices()[0].data(), (std::streamsize)(3 * Vn * sizeof(float)));
        o.write((const char *)n1.data(), (std::streamsize)(3 * Vn * sizeof(float)));
        o.write((const char *)b.GetVertices()[0].data(), (std::streamsize)(3 * Vn * sizeof(float)));
        o.write((const char *)n2.data(), (std::streamsize)(3 * Vn * sizeof(float)));
        if (!o) return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
    return 0;
}
