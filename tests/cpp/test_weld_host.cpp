// test_weld_host.cpp -- arvx::weldMesh (include/arvx/marching_cubes.hpp) on a mesh from a file, for
// tests/test_mc_weld_cpu.py: no GPU is touched.
//
//   test_weld_host <in> <out> [off]
//   in:  int64 T, then 9T float32 (triangle t: vertices 3t, 3t+1, 3t+2), then 3T uint32 (r, g, b)
//   out: int64 V, int64 T, then 3V float32 (welded vertices), then 6T uint32 (i0, i1, i2, r, g, b)
//   off: the welded mesh as SimpleMesh::WriteMesh writes it (scale 1, no translation)
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "arvx/marching_cubes.hpp"

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: test_weld_host <in> <out> [off]\n");
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    int64_t T = 0;
    f.read((char *)&T, 8);
    std::vector<float> v((size_t)T * 9);
    std::vector<uint32_t> rgb((size_t)T * 3);
    f.read((char *)v.data(), v.size() * 4);
    f.read((char *)rgb.data(), rgb.size() * 4);
    if (!f) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    arvx::SimpleMesh mesh;
    for (int64_t t = 0; t < T; ++t) {
        unsigned int h[3];
        for (int k = 0; k < 3; ++k) {
            const float *p = &v[(size_t)(3 * t + k) * 3];
            h[k] = mesh.AddVertex(arvx::Vec3f(p[0], p[1], p[2]));
        }
        mesh.AddFace(h[0], h[1], h[2], rgb[3 * t], rgb[3 * t + 1], rgb[3 * t + 2]);
    }
    const arvx::SimpleMesh &welded = arvx::weldMesh(mesh);
    static_assert(sizeof(arvx::Triangle) == 24, "six packed uints");
    const int64_t nv = (int64_t)welded.GetVertices().size(), nt = (int64_t)welded.GetTriangles().size();
    std::ofstream o(argv[2], std::ios::binary);
    o.write((const char *)&nv, 8);
    o.write((const char *)&nt, 8);
    for (const arvx::Vec3f &p : welded.GetVertices()) {
        const float q[3] = {p.x(), p.y(), p.z()};
        o.write((const char *)q, 12);
    }
    if (nt) o.write((const char *)welded.GetTriangles().data(), (std::streamsize)(nt * 24));
    if (!o) return 1;
    if (argc > 3) {
        arvx::SimpleMesh copy = welded;
        if (!copy.WriteMesh(argv[3])) return 1;
    }
    return 0;
}
