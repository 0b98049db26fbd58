// test_morph_host.cpp -- arvx::signedDistance and arvx::morph (include/arvx/postprocessing.hpp) on a
// Model built from a file, for tests/test_distance_gpu.py.
//
//   test_morph_host <in> <out> <op> <radius_voxels> <border_occupied>
//   in:  int32 X, Y, Z, then X*Y*Z state bytes (bit0 occupied, bit1 seen), flat index x + X*(y + Y*z)
//   out: X*Y*Z int32 (the field of the model as given), int64 (morph's return value), X*Y*Z int32
//        (the field after the op, border empty), then X*Y*Z bytes (bit0: get().w != 0, bit1: visited)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "arvx/postprocessing.hpp"

using arvx::Model;
using arvx::Vec3i;
using arvx::Vec4f;

int main(int argc, char **argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: test_morph_host <in> <out> <op> <radius_voxels> <border_occupied>\n");
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    int32_t dims[3] = {0, 0, 0};
    f.read((char *)dims, sizeof dims);
    const int X = dims[0], Y = dims[1], Z = dims[2];
    std::vector<uint8_t> st((size_t)X * Y * Z);
    f.read((char *)st.data(), (std::streamsize)st.size());
    if (!f) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    const int op = std::atoi(argv[3]);
    const float radius = (float)std::atof(argv[4]);
    const bool border_occupied = std::atoi(argv[5]) != 0;
    try {
        Model model(X, Y, Z, 0.01f);
        for (int z = 0; z < Z; ++z)
            for (int y = 0; y < Y; ++y)
                for (int x = 0; x < X; ++x) {
                    const uint8_t b = st[(size_t)x + (size_t)X * (y + (size_t)Y * z)];
                    if (!(b & 1)) model.set(x, y, z, Vec4f(0, 0, 0, 0));
                    if (b & 2) model.see(x, y, z);
                }
        const std::vector<int32_t> before = arvx::signedDistance(model, border_occupied);
        const int64_t changed = arvx::morph(model, op, radius);
        const std::vector<int32_t> after = arvx::signedDistance(model);
        std::vector<uint8_t> out(st.size());
        for (int z = 0; z < Z; ++z)
            for (int y = 0; y < Y; ++y)
                for (int x = 0; x < X; ++x)
                    out[(size_t)x + (size_t)X * (y + (size_t)Y * z)] =
                        (uint8_t)((model.get(x, y, z).w() != 0.f ? 1 : 0) | (model.visited(Vec3i(x, y, z)) ? 2 : 0));
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char *)before.data(), (std::streamsize)(before.size() * 4));
        o.write((const char *)&changed, 8);
        o.write((const char *)after.data(), (std::streamsize)(after.size() * 4));
        o.write((const char *)out.data(), (std::streamsize)out.size());
        if (!o) return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
    return 0;
}
