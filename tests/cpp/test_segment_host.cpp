// test_segment_host.cpp -- arvx::segmentViews (include/arvx/segmentation.hpp) on a scene from a file,
// for tests/test_segment_cpp_gpu.py.
//
//   test_segment_host <scene> <out> <rule> <a> <b> <open> <close> <min_area> <largest> <max_hole>
//   scene: tests/cpp/test_host.cpp's scene file -- int32 X, Y, Z, V, W, H, C; float s; float K[9];
//          V * (float pose[12]); V*H*W*C mask bytes; V*H*W*3 image bytes; X*Y*Z initial state bytes
//   rule:  0 -- background where a <= every channel <= b; 1 -- foreground where a channel differs by
//          more than a from a plate whose every byte is b (one plate for all views)
//   out:   V*H*W bytes of masks, V*8 int64 of counts, X*Y*Z bytes of the state carve() left
//   The scene's own masks are not used: the views' masks are those segmentViews made of the images.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "arvx/segmentation.hpp"

int main(int argc, char **argv) {
    if (argc < 11) {
        std::fprintf(stderr, "usage: test_segment_host <scene> <out> <rule> <a> <b> <open> <close> <min_area> "
                             "<largest> <max_hole>\n");
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
    std::vector<uint8_t> masks((size_t)V * H * W * C), images((size_t)V * H * W * 3);
    f.read((char *)masks.data(), (std::streamsize)masks.size());
    f.read((char *)images.data(), (std::streamsize)images.size());
    if (!f) {
        std::fprintf(stderr, "short scene file\n");
        return 2;
    }
    for (int i = 0; i < V; ++i) views[(size_t)i].image = {images.data() + (size_t)i * H * W * 3, W, H, 3, (size_t)W * 3};
    const int rule = std::atoi(argv[3]), a = std::atoi(argv[4]), b = std::atoi(argv[5]);
    arvx::SegmentParams p = arvx::referenceSegmentParams();
    if (p.rule != ARVX_SEGMENT_RANGE || p.lo[0] != 120 || p.hi[2] != 255 || p.open_radius || p.close_radius ||
        p.min_area || p.max_hole || p.flags)
        return 4;  // (the reference's rule: src/Segmentation.h:10-11, no cleaning)
    std::vector<uint8_t> plate;
    std::vector<arvx::Image> plates;
    if (rule == 0) {
        for (int c = 0; c < 3; ++c) {
            p.lo[c] = (uint8_t)a;
            p.hi[c] = (uint8_t)b;
        }
    } else {
        p.rule = ARVX_SEGMENT_PLATE;
        p.threshold = a;
        plate.assign((size_t)H * W * 3, (uint8_t)b);
        plates.push_back({plate.data(), W, H, 3, (size_t)W * 3});
    }
    p.open_radius = std::atoi(argv[6]);
    p.close_radius = std::atoi(argv[7]);
    p.min_area = std::atoll(argv[8]);
    p.flags = std::atoi(argv[9]) ? ARVX_SEGMENT_LARGEST : 0u;
    p.max_hole = std::atoll(argv[10]);
    try {
        arvx::Model model(X, Y, Z, s);
        arvx::SegmentedMasks seg;
        arvx::segmentViews(model, views, p, plates, seg);
        if (seg.width != W || seg.height != H || (int)seg.masks.size() != V) return 5;
        for (int i = 0; i < V; ++i)
            if (views[(size_t)i].mask.data != seg.masks[(size_t)i].data() || views[(size_t)i].mask.channels != 1) return 6;
        arvx::carve(intr, model, views);
        std::ofstream o(argv[2], std::ios::binary);
        for (const auto &m : seg.masks) o.write((const char *)m.data(), (std::streamsize)m.size());
        for (const auto &n : seg.counts) o.write((const char *)n.data(), (std::streamsize)sizeof n);
        const std::vector<uint8_t> st = model.byte_state();
        o.write((const char *)st.data(), (std::streamsize)st.size());
        return o ? 0 : 3;
    } catch (const arvx::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
