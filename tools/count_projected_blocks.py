#!/usr/bin/env python3
"""Counts what the exact carve kernel projects: per carve of the sphere scene the items, their
listed views, the (item, view) pairs that reach exact_view_blocks, the 4 x 4 x 4 blocks their
rectangles left open (`need`) and the (block, view) passes actually projected (`did`).
EXPERIMENTS.md round 8: the share of the kernel a table of cached pixels could replace.

Needs the experiment build, which carries the counters (flags bit8):
    ARVX_COUNT_BLOCKS=1 ARVX_LIB_PATH=ar_voxel_project_amd/lib/libarvx_experiments.so \
        python tools/count_projected_blocks.py [grid] [views]   (GPU required)
Three fresh carves under the same cameras with the table of pixels switched off: computed
rectangles, the block table's build, the block table read -- the counts of the three must agree (the
table changes where the rectangles come from, not them)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ar_voxel_project_amd import capi, synthetic  # noqa: E402


def main():
    if not os.environ.get("ARVX_COUNT_BLOCKS") or "experiments" not in capi.LIB_PATH:
        raise SystemExit(__doc__)
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    V = int(sys.argv[2]) if len(sys.argv) > 2 else 36
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    sc = synthetic.sphere_scene(N, V)
    d_masks = torch.from_numpy(sc.masks).to(dev)
    torch.cuda.synchronize()
    with capi.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_stream(stream.cuda_stream)
        ctx.set_pixel_cache_limit(0)  # (the counters sit in the projection: keep every view on it)
        for carve in range(3):
            ctx.reset()
            ctx.set_views_device(sc.M, d_masks.data_ptr(), sc.W, sc.H, 1, campos=sc.campos)
            ctx.carve(0)
            st = ctx.stats()
            path = ctx.last_carve_path()
            pairs, did = st["open_voxels_in_slices"], st["slices_evaluated"]
            print(json.dumps({
                "grid": N, "views": V, "carve": carve, "path": path,
                "items": st["subtiles"], "listed_views": st["subtile_views_mixed"],
                "pairs_in_exact_view_blocks": pairs, "blocks_need": st["mixed_pairs_uniform"],
                "blocks_projected": did, "projected_per_pair": did / max(1, pairs)}))


if __name__ == "__main__":
    main()
