// arvx_mesh_weld_time.cpp -- wall-clock of the drop-in mesh calls on one model: marchingCubesMesh
// (the reference's mesh, three fresh vertices per triangle) against marchingCubesMeshWelded (shared
// vertices), both with the mesh on the host, after the pipeline of src/main.cpp:262-303 (carve,
// average colour, handleUnseen, closure).  Driven by tools/mesh_weld_time.py.
//
//   arvx_mesh_weld_time <scene file> <X> <Y> <Z> <voxel size> [rounds]
//   (scene file: tests/cpp/test_host.cpp; the grid in it is ignored)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "arvx/marching_cubes.hpp"
#include "arvx/postprocessing.hpp"
#include "arvx/voxel_carving.hpp"

using Clock = std::chrono::steady_clock;
static double ms(Clock::time_point a, Clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}
static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char **argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: arvx_mesh_weld_time <scene> X Y Z size [rounds]\n");
        return 2;
    }
    const int X = atoi(argv[2]), Y = atoi(argv[3]), Z = atoi(argv[4]);
    const float size = (float)atof(argv[5]);
    const int rounds = argc > 6 ? std::max(1, atoi(argv[6])) : 9;
    std::ifstream f(argv[1], std::ios::binary);
    int32_t hd[7];
    f.read((char *)hd, sizeof hd);
    const int V = hd[3], W = hd[4], H = hd[5], C = hd[6];
    float s_unused;
    f.read((char *)&s_unused, 4);
    arvx::Intrinsics intr;
    f.read((char *)intr.K, 36);
    std::vector<arvx::View> views(V);
    for (auto &v : views) f.read((char *)v.pose, 48);
    std::vector<uint8_t> masks((size_t)V * H * W * C), images((size_t)V * H * W * 3);
    f.read((char *)masks.data(), masks.size());
    f.read((char *)images.data(), images.size());
    if (!f) {
        std::fprintf(stderr, "short scene file\n");
        return 2;
    }
    for (int i = 0; i < V; ++i) {
        views[i].mask = {masks.data() + (size_t)i * H * W * C, W, H, C, (size_t)W * C};
        views[i].image = {images.data() + (size_t)i * H * W * 3, W, H, 3, (size_t)W * 3};
    }
    std::cout.setstate(std::ios::failbit);  // the LOG lines of the entry points
    arvx::Model model(X, Y, Z, size);
    arvx::carve(intr, model, views);
    arvx::reconstructAvgColor(intr, model, views);
    model.handleUnseen();
    arvx::applyClosure(&model, 3);
    std::vector<double> plain, welded;
    size_t T = 0, nv = 0, Tw = 0;
    for (int r = 0; r < rounds + 1; ++r) {  // (round 0: warm-up, not counted)
        auto t0 = Clock::now();
        {
            arvx::SimpleMesh m = arvx::marchingCubesMesh(&model, 0.5f);
            T = m.GetTriangles().size();
        }
        auto t1 = Clock::now();
        {
            arvx::SimpleMesh m = arvx::marchingCubesMeshWelded(&model, 0.5f);
            nv = m.GetVertices().size();
            Tw = m.GetTriangles().size();
        }
        auto t2 = Clock::now();
        if (r) {
            plain.push_back(ms(t0, t1));
            welded.push_back(ms(t1, t2));
        }
    }
    if (Tw != T) {
        std::fprintf(stderr, "welded mesh has %zu triangles, the mesh %zu\n", Tw, T);
        return 1;
    }
    std::fprintf(stderr,
                 "drop-in %dx%dx%d: marchingCubesMesh %.3f ms (%zu triangles, %.1f MB) | "
                 "marchingCubesMeshWelded %.3f ms (%zu vertices, %.1f MB)  [median of %d]\n",
                 X, Y, Z, median(plain), T, 60.0 * T / 1e6, median(welded), nv,
                 (12.0 * nv + 24.0 * T) / 1e6, rounds);
    return 0;
}
