// test_decimate_host.cpp -- arvx::decimateMesh (include/arvx/marching_cubes.hpp) on a welded mesh
// from a file, for tests/test_mc_decimate_cpu.py: no GPU is touched.
//
//   test_decimate_host <in> <out>
//   in:  int64 V, int64 T, int32 cell, int32 smoothed (0 / 1), then 3V float32 (lattice positions),
//        then -- if smoothed -- 3V float32 (smoothed positions), then 6T uint32 (face records)
//   out: int64 Vd, int64 Td, then 3Vd float32 (positions), 6Td uint32 (face records), Vd int32
//        (members), V int32 (map)
//   stdout: the time of the decimateMesh call alone (tools/decimate_time.py reads it)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "arvx/marching_cubes.hpp"

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: test_decimate_host <in> <out>\n");
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    int64_t V = 0, T = 0;
    int32_t cell = 0, has_smoothed = 0;
    f.read((char *)&V, 8);
    f.read((char *)&T, 8);
    f.read((char *)&cell, 4);
    f.read((char *)&has_smoothed, 4);
    std::vector<float> v((size_t)V * 3), q(has_smoothed ? (size_t)V * 3 : 0);
    std::vector<uint32_t> faces((size_t)T * 6);
    f.read((char *)v.data(), v.size() * 4);
    f.read((char *)q.data(), q.size() * 4);
    f.read((char *)faces.data(), faces.size() * 4);
    if (!f) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    arvx::SimpleMesh mesh, smoothed;
    for (int64_t i = 0; i < V; ++i) mesh.AddVertex(arvx::Vec3f(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
    for (int64_t t = 0; t < T; ++t)
        mesh.AddFace(faces[6 * t], faces[6 * t + 1], faces[6 * t + 2], faces[6 * t + 3], faces[6 * t + 4],
                     faces[6 * t + 5]);
    if (has_smoothed)
        for (int64_t i = 0; i < V; ++i) smoothed.AddVertex(arvx::Vec3f(q[3 * i], q[3 * i + 1], q[3 * i + 2]));
    std::vector<int32_t> members, map;
    const auto t0 = std::chrono::steady_clock::now();
    const arvx::SimpleMesh out = arvx::decimateMesh(mesh, cell, has_smoothed ? &smoothed : nullptr, &members, &map);
    std::printf("decimateMesh %.3f ms\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    const int64_t Vd = (int64_t)out.GetVertices().size(), Td = (int64_t)out.GetTriangles().size();
    if ((int64_t)members.size() != Vd || (int64_t)map.size() != V) return 1;
    std::ofstream o(argv[2], std::ios::binary);
    o.write((const char *)&Vd, 8);
    o.write((const char *)&Td, 8);
    for (const arvx::Vec3f &p : out.GetVertices()) o.write((const char *)p.data(), 12);
    for (const arvx::Triangle &t : out.GetTriangles()) o.write((const char *)&t.idx0, 24);
    o.write((const char *)members.data(), members.size() * 4);
    o.write((const char *)map.data(), map.size() * 4);
    return o ? 0 : 1;
}
