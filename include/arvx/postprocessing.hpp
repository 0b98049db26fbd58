// postprocessing.hpp -- the reference's applyClosure(Model*, int kernelSize)
// (src/Postprocessing3d.h:10, src/Postprocessing3d.cpp:4-100) over the GPU library.
//
// Same name, arguments, return value and log lines.  As in the reference the
// result is one dilation with a kernelSize^3 box (its erosion half tests w < 0
// and never fires); new voxels get the mean RGBA of their occupied
// neighbours.  Limitation: explicit colours must have w == 1 (every colour the
// reference's own pipeline produces has).  Runs on the model's own device context: state and
// the colour list of the colour pass are already there (src/main.cpp:282-299).
//
// dropFloaters(Model&, ...) -- an extension beyond the reference: the connected components of the
// carved model (arvx_components_keep), for the clumps of voxels that the false foreground specks of
// a few silhouettes leave in mid-air.
#ifndef ARVX_POSTPROCESSING_HPP
#define ARVX_POSTPROCESSING_HPP

#include <cmath>
#include <cstdint>
#include <vector>

#include "arvx/voxel_carving.hpp"

namespace arvx {

inline int applyClosure(Model *model, int kernelSize) {
    std::cout << "LOG - PP: starting postprocessing." << std::endl;
    if (kernelSize % 2 != 1) {
        std::cerr << "Invalid kernel size for post processing, skipping..." << std::endl;
        return -1;
    }
    detail::timing(kStagePostProcessing, true);
    arvx_ctx *ctx = model->device();
    // painted voxels: when the paint is exactly "not seen" (handleUnseen was the last thing that
    // touched the state) the device derives it itself; otherwise the byte plane carries it (bit2)
    const bool painted = model->painted();
    if (painted && !model->paint_is_unseen()) {
        const std::vector<uint8_t> st = model->byte_state();
        detail::check(arvx_state_upload(ctx, st.data()), "arvx_state_upload");
        model->set_colors_on_device(false);
    }
    if (!model->colors_on_device()) {
        std::vector<int64_t> idx;
        std::vector<float> rgb;
        if (!model->sorted_colors(idx, rgb)) {
            std::cerr << "LOG(ERR) - GPU: applyClosure needs explicit colours with w == 1"
                      << std::endl;
            throw Error(ARVX_ERR_INVALID, "explicit colour with w != 1");
        }
        detail::check(arvx_colors_upload(ctx, (int64_t)idx.size(), idx.data(), rgb.data()),
                      "arvx_colors_upload");
        model->set_colors_on_device(true);
    }
    std::cout << "LOG - PP: starting dilution." << std::endl;
    detail::check(arvx_closure(ctx, kernelSize, (painted && model->paint_is_unseen()) ? 1 : 0),
                  "arvx_closure");
    int64_t n = 0;
    detail::check(arvx_closure_count(ctx, &n), "arvx_closure_count");
    // straight into the model's own arrays (recycled page-locked memory, host_pool.hpp)
    HostVector<int> fidx((size_t)n);
    HostVector<Vec4f> frgba((size_t)n);
    if (n) detail::check(arvx_closure_download32(ctx, fidx.data(), frgba[0].data()),
                         "arvx_closure_download32");
    std::cout << "LOG - PP: starting erosion." << std::endl;  // a no-op in the reference too
    // the filled voxels: occupied on the device already, with their colours on the host now;
    // the context keeps its closure result, so the model goes back to "host is current" and a
    // second closure starts from a fresh upload
    model->device_changed_keep_paint();
    model->set_closure_list(std::move(fidx), std::move(frgba), true);
    model->closure_applied();
    detail::timing(kStagePostProcessing, false);
    std::cout << "LOG - PP: postprocessing completed." << std::endl;
    return 0;
}

// Extension beyond the reference: drops the floaters of a carved model, between the carve and the
// colour pass (arvx_components_keep).  A connected component of occupied voxels (connectivity 6 or
// 26) stays iff it has at least min_voxels voxels and -- with largest_only -- is the largest one (the
// one with the least flat index among equals); the voxels of the others become empty and keep their
// seen bits.  Runs on the model's own device context, as photoCarve does: the model's current state
// goes there first if the host holds it, and the result stays on the device until somebody reads
// the model on the host.  Returns the voxels removed.
inline int64_t dropFloaters(Model &model, int64_t min_voxels = 1, bool largest_only = true, int connectivity = 6) {
    std::cout << "LOG - PP: dropping floaters." << std::endl;
    detail::timing(kStagePostProcessing, true);
    arvx_ctx *ctx = model.device();
    int64_t kept = 0, removed = 0;
    detail::check(arvx_components_keep(ctx, connectivity, min_voxels, largest_only ? ARVX_COMPONENTS_LARGEST : 0u,
                                       &kept, &removed),
                  "arvx_components_keep");
    model.device_changed();
    detail::timing(kStagePostProcessing, false);
    std::cout << "LOG - PP: floaters dropped (" << kept << " components kept, " << removed << " voxels removed)."
              << std::endl;
    return removed;
}

// Extension beyond the reference: erosion, dilation, opening or closing (ARVX_MORPH_*) of the model
// by a ball of radius_voxels voxels (arvx_morph with radius_sq = floor(radius_voxels^2)), next to
// dropFloaters: an opening removes what is thinner than the ball -- fins, spurs, one-voxel bridges --
// and what it cuts loose, dropFloaters drops.  Voxels that leave the model keep their seen bits;
// voxels that join it carry no colour until a colour pass gives them one.  Runs on the model's own
// device context with the same hand-over as dropFloaters.  Returns the voxels removed plus added.
inline int64_t morph(Model &model, int op, float radius_voxels) {
    static const char *const kNames[] = {"erosion", "dilation", "opening", "closing"};
    if (op < ARVX_MORPH_ERODE || op > ARVX_MORPH_CLOSE) throw Error(ARVX_ERR_INVALID, "morph: op must be 0..3");
    if (!(radius_voxels >= 0.f)) throw Error(ARVX_ERR_INVALID, "morph: radius_voxels must be >= 0");
    const double r2 = std::floor((double)radius_voxels * (double)radius_voxels);
    if (r2 >= (double)ARVX_DISTANCE_INF) throw Error(ARVX_ERR_INVALID, "morph: radius_voxels too large");
    const int64_t radius_sq = (int64_t)r2;
    std::cout << "LOG - PP: starting " << kNames[op] << " (squared radius " << radius_sq << ")." << std::endl;
    detail::timing(kStagePostProcessing, true);
    arvx_ctx *ctx = model.device();
    int64_t removed = 0, added = 0;
    detail::check(arvx_morph(ctx, op, radius_sq, &removed, &added), "arvx_morph");
    model.device_changed();
    detail::timing(kStagePostProcessing, false);
    std::cout << "LOG - PP: " << kNames[op] << " completed (" << removed << " voxels removed, " << added
              << " voxels added)." << std::endl;
    return removed + added;
}

// Extension beyond the reference: the signed squared Euclidean distance of every voxel of the model
// to the nearest voxel of the other kind (arvx_distance; definition in arvx/arvx.h), flat index order
// x + X*(y + Y*z): positive on occupied voxels, negative on empty ones, +-ARVX_DISTANCE_INF where
// there is no such voxel.  border_occupied: the lattice points outside the grid are no empty sites.
// The model is unchanged.
inline std::vector<int32_t> signedDistance(Model &model, bool border_occupied = false) {
    arvx_ctx *ctx = model.device();
    int64_t n = 0;
    detail::check(arvx_ctx_voxels(ctx, &n), "arvx_ctx_voxels");
    std::vector<int32_t> out((size_t)n);
    detail::check(arvx_distance(ctx, border_occupied ? ARVX_DISTANCE_BORDER_OCCUPIED : 0u), "arvx_distance");
    detail::check(arvx_distance_download(ctx, out.data()), "arvx_distance_download");
    return out;
}

}  // namespace arvx
#endif
