// segmentation.hpp -- silhouettes from the photographs, on the device (header only, C++17, links
// libarvx.so).  An extension beyond the reference, whose `-c=4` (src/Segmentation.h:4-12) is an RGB
// range test on the host: here the rule -- that range test, or a comparison against a background
// plate -- and the cleaning of the masks (opening, closing, specks, holes; the definition is in
// include/arvx/arvx.h, arvx_segment_views) run on the model's device context.
//
//   SegmentParams             arvx_segment_params with the reference's rule as its default
//   referenceSegmentParams()  the reference's rule: background 120..255 in every channel, no cleaning
//   segmentViews(...)         runs the stage and points every view's mask at the result, so that
//                             carve, carveVotes, fastCarve and the colour functions take the views
//                             unchanged
#ifndef ARVX_SEGMENTATION_HPP
#define ARVX_SEGMENTATION_HPP

#include <array>
#include <cstring>
#include <vector>

#include "arvx/voxel_carving.hpp"

namespace arvx {

struct SegmentParams : arvx_segment_params {
    SegmentParams() {
        std::memset(static_cast<arvx_segment_params *>(this), 0, sizeof(arvx_segment_params));
        rule = ARVX_SEGMENT_RANGE;
        for (int c = 0; c < 3; ++c) {  // src/Segmentation.h:10-11
            lo[c] = 120;
            hi[c] = 255;
        }
    }
};

inline SegmentParams referenceSegmentParams() { return SegmentParams(); }

// The masks segmentViews made: one channel, 255 foreground, tightly packed.  The views point into
// it: it has to outlive their use.
struct SegmentedMasks {
    int width = 0, height = 0;
    std::vector<std::vector<uint8_t>> masks;
    std::vector<std::array<int64_t, 8>> counts;  // arvx_segment_counts, per view
};

// Segments views[i].image (BGR, one size and stride) on model's context, downloads the masks into
// `out` and points views[i].mask at them.  plates: none (RANGE), one for all views or one per view,
// of the images' size and stride.  The cameras bound meanwhile are views[i].M where the caller gave
// it, the pose otherwise: the masks do not depend on them, and whatever carves or colours next binds
// the views again.  The context's colour list goes, as with any new views.
inline void segmentViews(Model &model, std::vector<View> &views, const SegmentParams &params,
                         const std::vector<Image> &plates, SegmentedMasks &out) {
    auto fail = [](const char *msg) {
        std::cerr << "LOG(ERR) - GPU: " << msg << std::endl;
        throw Error(ARVX_ERR_INVALID, msg);
    };
    if (views.empty()) fail("no views");
    const int V = (int)views.size();
    const Image &i0 = views[0].image;
    std::vector<float> M((size_t)V * 12), cam((size_t)V * 3);
    std::vector<const uint8_t *> imgs(V), pls(plates.size());
    for (int i = 0; i < V; ++i) {
        const Image &im = views[i].image;
        if (!im.data || im.channels != 3 || im.width != i0.width || im.height != i0.height || im.stride != i0.stride)
            fail("segmentViews: the images must be BGR u8 of one size and stride");
        imgs[i] = im.data;
        std::memcpy(&M[12 * (size_t)i], views[i].has_M ? views[i].M : views[i].pose, 12 * sizeof(float));
        cam[3 * (size_t)i] = views[i].pose[3];
        cam[3 * (size_t)i + 1] = views[i].pose[7];
        cam[3 * (size_t)i + 2] = views[i].pose[11];
    }
    for (size_t i = 0; i < plates.size(); ++i) {
        const Image &pl = plates[i];
        if (!pl.data || pl.channels != 3 || pl.width != i0.width || pl.height != i0.height || pl.stride != i0.stride)
            fail("segmentViews: the plates must have the images' size and stride");
        pls[i] = pl.data;
    }
    arvx_ctx *ctx = model.device();
    detail::check(arvx_segment_views(ctx, V, M.data(), cam.data(), imgs.data(), i0.width, i0.height, i0.stride,
                                     pls.empty() ? nullptr : pls.data(), (int)pls.size(), &params),
                  "arvx_segment_views");
    model.set_colors_on_device(false);
    out.width = i0.width;
    out.height = i0.height;
    out.masks.assign(V, std::vector<uint8_t>((size_t)i0.width * i0.height));
    out.counts.assign(V, {});
    for (int i = 0; i < V; ++i) {
        detail::check(arvx_segment_download(ctx, i, out.masks[i].data()), "arvx_segment_download");
        detail::check(arvx_segment_counts(ctx, i, out.counts[i].data()), "arvx_segment_counts");
        views[i].mask = {out.masks[i].data(), i0.width, i0.height, 1, (size_t)i0.width};
    }
}

}  // namespace arvx
#endif
