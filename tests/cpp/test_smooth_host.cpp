// test_smooth_host.cpp -- arvx::smoothMesh (include/arvx/marching_cubes.hpp) on a welded mesh from a
// file, for tests/test_mc_smooth_cpu.py: no GPU is touched.
//
//   test_smooth_host <in> <out>
//   in:  int64 V, int64 T, int32 iterations, float32 lambda, float32 mu, then 3V float32
//        (positions), then 3T uint32 (faces)
//   out: 3V float32 (smoothed positions), then 3V float32 (unit vertex normals)
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "arvx/marching_cubes.hpp"

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: test_smooth_host <in> <out>\n");
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    int64_t V = 0, T = 0;
    int32_t iterations = 0;
    float lambda = 0.f, mu = 0.f;
    f.read((char *)&V, 8);
    f.read((char *)&T, 8);
    f.read((char *)&iterations, 4);
    f.read((char *)&lambda, 4);
    f.read((char *)&mu, 4);
    std::vector<float> v((size_t)V * 3);
    std::vector<uint32_t> faces((size_t)T * 3);
    f.read((char *)v.data(), v.size() * 4);
    f.read((char *)faces.data(), faces.size() * 4);
    if (!f) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    arvx::SimpleMesh mesh;
    for (int64_t i = 0; i < V; ++i) mesh.AddVertex(arvx::Vec3f(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
    for (int64_t t = 0; t < T; ++t) mesh.AddFace(faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]);
    arvx::HostVector<arvx::Vec3f> normals;
    const arvx::SimpleMesh smoothed = arvx::smoothMesh(mesh, iterations, lambda, mu, &normals);
    if ((int64_t)smoothed.GetVertices().size() != V || (int64_t)normals.size() != V ||
        (int64_t)smoothed.GetTriangles().size() != T)
        return 1;
    std::ofstream o(argv[2], std::ios::binary);
    for (const arvx::Vec3f &p : smoothed.GetVertices()) o.write((const char *)p.data(), 12);
    for (const arvx::Vec3f &n : normals) o.write((const char *)n.data(), 12);
    return o ? 0 : 1;
}
