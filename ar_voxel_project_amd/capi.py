"""ctypes binding of libarvx.so (include/arvx/arvx.h).

This is plumbing: every call goes straight to the C-ABI, which launches the
gfx950 kernels.  There is no Python or CPU fallback -- if the shared library is
missing or the GPU is unusable the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ARVX_LIB_PATH: A/B another build of the library on the same box (tools/ab_compare.sh)
LIB_PATH = os.environ.get("ARVX_LIB_PATH") or os.path.join(_HERE, "lib", "libarvx.so")

OCC = 1
SEEN = 2
CARVE_NO_CULL = 1
CARVE_STATS = 2
CARVE_FUSED = 8
CARVE_STREAM = 16
CARVE_FILTER = 64
CARVE_NO_STREAM = 32
# the large grids' kernel choice on a grid of any size (include/arvx/arvx.h: path flags)
CARVE_DENSE_CLASSIFY = 128
CARVE_WHOLE_ITEMS = 256
# bits of Context.last_carve_path()["bits"] (ARVX_PATH_*)
PATH_DENSE_CLASSIFY = 1
PATH_ITEM_SHARING = 2
PATH_FRESH = 4
PATH_LAZY_CODES = 8
PATH_FUSED = 16
PATH_BRUTE_FORCE = 32
PATH_STREAM = 64
PATH_RECT_BLOCKS = 128
PATH_PIXEL_TABLE = 256
# bits of Context.last_fast_carve_path()["bits"] (ARVX_FLOOD_*)
FLOOD_PREPASS = 1
FLOOD_FRESH = 2
VOTES_COUNTS = 1
VOTES_NO_CULL = 2
COMPONENTS_LARGEST = 1
DISTANCE_BORDER_OCCUPIED = 1
DISTANCE_INF = 2147483647
MORPH_ERODE = 0
MORPH_DILATE = 1
MORPH_OPEN = 2
MORPH_CLOSE = 3
DECIMATE_LATTICE = 0
DECIMATE_SMOOTHED = 1
MESH_WELDED = 0
MESH_SMOOTHED = 1
MESH_DECIMATED = 2
MESH_REFINED = 3
MESH_RELAXED = 5  # mesh_relax()'s product: its base's faces and colours, the relaxed positions
MESH_IMAGE_COLORS = 0x100  # OR-ed into `source` of the render_mesh family: draw mesh_color()'s colours
MESH_COLOR_FOREGROUND = 1  # flags of mesh_color
MESH_TEXTURED = 0x400  # OR-ed into `source` of the render_mesh family: draw mesh_texture()'s atlas
MESH_TEXTURE_FOREGROUND = 1  # flags of mesh_texture
SEGMENT_RANGE = 0  # rules of segment_views
SEGMENT_PLATE = 1
SEGMENT_LARGEST = 1  # flags of segment_views
# test plumbing: flags OR-ed into every carve of this process, e.g. ARVX_CARVE_EXTRA_FLAGS=16 runs a
# whole test module with the streaming carve forced on every fresh model (the library itself reads
# no environment variable)
_EXTRA_CARVE_FLAGS = int(os.environ.get("ARVX_CARVE_EXTRA_FLAGS", "0"))
COLOR_CLOSEST = 0
COLOR_AVERAGE = 1

# every symbol include/arvx/arvx.h declares
SYMBOLS = [
    "arvx_version", "arvx_last_error", "arvx_device_count", "arvx_projection_assoc",
    "arvx_ctx_create_slab_halo",
    "arvx_set_projection_assoc", "arvx_ctx_set_projection_assoc", "arvx_ctx_projection_assoc",
    "arvx_selftest_project", "arvx_selftest_depth", "arvx_selftest_view_tables",
    "arvx_ctx_create", "arvx_ctx_create_slab", "arvx_ctx_create_striped", "arvx_ctx_destroy",
    "arvx_ctx_set_stream", "arvx_ctx_set_exchange_stream", "arvx_ctx_synchronize", "arvx_ctx_voxels",
    "arvx_compose_projection", "arvx_set_views", "arvx_set_views_device",
    "arvx_set_images", "arvx_state_reset", "arvx_state_upload",
    "arvx_state_download", "arvx_state_device_ptr", "arvx_state_upload_halo",
    "arvx_state_upload_planes", "arvx_state_download_planes", "arvx_state_packet_geometry",
    "arvx_state_download_packets", "arvx_host_register",
    "arvx_host_unregister", "arvx_handle_unseen", "arvx_undistort", "arvx_undistort_device",
    "arvx_pack_occupancy", "arvx_pack_occupancy_global", "arvx_carve", "arvx_carve_views", "arvx_fast_carve",
    "arvx_color", "arvx_surface_count", "arvx_surface_download",
    "arvx_surface_depth_download", "arvx_color_samples",
    "arvx_color_visible", "arvx_surface_visible_download", "arvx_view_depth_download",
    "arvx_photo_carve", "arvx_carve_votes", "arvx_votes_download",
    "arvx_components", "arvx_components_download", "arvx_components_labels_download",
    "arvx_components_keep",
    "arvx_distance", "arvx_distance_download", "arvx_morph",
    "arvx_colors_upload", "arvx_closure", "arvx_closure_count", "arvx_closure_download",
    "arvx_closure_download32",
    "arvx_mc_cells", "arvx_mc_cells_download", "arvx_mc_mesh", "arvx_mc_mesh_download",
    "arvx_mc_mesh_download_faces", "arvx_mc_mesh_welded", "arvx_mc_mesh_welded_download",
    "arvx_mc_mesh_smooth", "arvx_mc_mesh_smooth_download",
    "arvx_mc_mesh_decimate", "arvx_mc_mesh_decimate_download",
    "arvx_mc_mesh_refined", "arvx_mc_mesh_refined_download",
    "arvx_render", "arvx_render_view", "arvx_render_download", "arvx_render_agreement",
    "arvx_render_mesh", "arvx_render_mesh_view", "arvx_render_mesh_agreement", "arvx_render_triangles",
    "arvx_render_mesh_stats", "arvx_selftest_render_mesh_list", "arvx_selftest_compute_units",
    "arvx_ctx_set_render_near", "arvx_ctx_render_near", "arvx_render_mesh_clip_stats",
    "arvx_mesh_color", "arvx_mesh_color_count", "arvx_mesh_color_download", "arvx_mesh_color_depth_download",
    "arvx_selftest_mesh_color_batch",
    "arvx_mesh_texture", "arvx_mesh_texture_info", "arvx_mesh_texture_download",
    "arvx_mesh_relax", "arvx_mesh_relax_info", "arvx_mesh_relax_download", "arvx_mesh_relax_triangles",
    "arvx_occupancy_packet_words", "arvx_occupancy_compress", "arvx_occupancy_expand",
    "arvx_occupancy_expand_striped", "arvx_occupancy_pack_compress", "arvx_occupancy_expand_striped_others",
    "arvx_export_model", "arvx_get_stats", "arvx_last_carve_path", "arvx_last_fast_carve_path",
    "arvx_selftest_divide",
    "arvx_selftest_round",
    "arvx_ctx_set_rect_cache_limit", "arvx_selftest_rect_cache",
    "arvx_ctx_set_pixel_cache_limit", "arvx_pixel_cache_views", "arvx_selftest_pixel_cache",
    "arvx_ctx_set_view_window", "arvx_view_window", "arvx_view_window_host",
    "arvx_selftest_fill_view_tables", "arvx_selftest_view_table_raw",
    "arvx_segment_views", "arvx_segment_views_device", "arvx_segment_download", "arvx_segment_counts",
    "arvx_selftest_segment_batch",
]


class ArvxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"arvx error {code}: {msg}")
        self.code = code


class SegmentParams(C.Structure):
    """arvx_segment_params (include/arvx/arvx.h)."""
    _fields_ = [
        ("rule", C.c_int32),
        ("lo", C.c_uint8 * 3),
        ("hi", C.c_uint8 * 3),
        ("reserved", C.c_uint8 * 2),
        ("threshold", C.c_int32),
        ("open_radius", C.c_int32),
        ("close_radius", C.c_int32),
        ("flags", C.c_uint32),
        ("min_area", C.c_int64),
        ("max_hole", C.c_int64),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("subtiles", C.c_uint64),
        ("subtiles_carved", C.c_uint64),
        ("subtile_views_mixed", C.c_uint64),
        ("subtile_views_total", C.c_uint64),
        ("surface_voxels", C.c_uint64),
        ("reserved", C.c_uint64 * 3),
        ("host_total_fallbacks", C.c_uint64),
    ]


_libs: dict = {}
ASSOC_RIGHT, ASSOC_LEFT = 0, 1  # grouping of the M*world row sums (include/arvx/arvx.h)


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load libarvx.so (built in-tree by ar_voxel_project_amd.build), or another build
    of it at `path` (A/B builds)."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or make -C ar_voxel_project_amd/csrc); there is no CPU fallback")
    # torch (device memory / streams / torch.distributed in bench and tests) ships its
    # own HIP runtime; it must be loaded BEFORE libarvx.so pulls in /opt/rocm's, or a
    # later `import torch` finds "No HIP GPUs".  libarvx itself does not use torch.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    p = C.c_void_p
    f32p = C.POINTER(C.c_float)
    u8p = C.POINTER(C.c_uint8)
    lib.arvx_version.restype = C.c_int
    if hasattr(lib, "arvx_projection_assoc"):
        lib.arvx_projection_assoc.restype = C.c_int
    lib.arvx_last_error.restype = C.c_char_p
    lib.arvx_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.arvx_ctx_create.argtypes = [C.POINTER(p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
    lib.arvx_ctx_create_slab.argtypes = [C.POINTER(p), C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_float, C.c_int, C.c_int]
    lib.arvx_ctx_create_striped.argtypes = [C.POINTER(p), C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_float, C.c_int, C.c_int]
    lib.arvx_ctx_destroy.argtypes = [p]
    lib.arvx_ctx_set_stream.argtypes = [p, p]
    if hasattr(lib, "arvx_ctx_set_exchange_stream"):
        lib.arvx_ctx_set_exchange_stream.argtypes = [p, p]
    lib.arvx_ctx_synchronize.argtypes = [p]
    lib.arvx_ctx_voxels.argtypes = [p, C.POINTER(C.c_int64)]
    lib.arvx_compose_projection.argtypes = [f32p, f32p, f32p]
    lib.arvx_set_views.argtypes = [p, C.c_int, f32p, f32p, C.POINTER(C.c_void_p), C.c_int,
                                   C.c_int, C.c_int, C.c_size_t]
    lib.arvx_set_views_device.argtypes = [p, C.c_int, f32p, f32p, p, C.c_int, C.c_int, C.c_int]
    lib.arvx_set_images.argtypes = [p, C.POINTER(C.c_void_p), C.c_size_t]
    lib.arvx_state_reset.argtypes = [p]
    lib.arvx_state_upload.argtypes = [p, u8p]
    lib.arvx_state_download.argtypes = [p, u8p]
    lib.arvx_state_device_ptr.argtypes = [p, C.POINTER(p), C.POINTER(C.c_size_t)]
    if hasattr(lib, "arvx_state_upload_planes"):
        lib.arvx_state_upload_planes.argtypes = [p, C.c_void_p, C.c_void_p]
        lib.arvx_state_download_planes.argtypes = [p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "arvx_state_download_packets"):
        lib.arvx_state_packet_geometry.argtypes = [p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.arvx_state_download_packets.argtypes = [p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.arvx_host_register.argtypes = [C.c_void_p, C.c_size_t]
        lib.arvx_host_unregister.argtypes = [C.c_void_p]
        lib.arvx_handle_unseen.argtypes = [p]
    lib.arvx_state_upload_halo.argtypes = [p, u8p, u8p]
    lib.arvx_pack_occupancy.argtypes = [p, p]
    lib.arvx_pack_occupancy_global.argtypes = [p, p]
    lib.arvx_carve.argtypes = [p, C.c_uint]
    lib.arvx_carve_views.argtypes = [p, C.c_int, C.c_int, C.c_uint]
    lib.arvx_fast_carve.argtypes = [p]
    lib.arvx_color.argtypes = [p, C.c_int]
    lib.arvx_surface_count.argtypes = [p, C.POINTER(C.c_int64)]
    lib.arvx_surface_download.argtypes = [p, C.POINTER(C.c_int64), f32p]
    lib.arvx_surface_depth_download.argtypes = [p, f32p]
    lib.arvx_colors_upload.argtypes = [p, C.c_int64, C.POINTER(C.c_int64), f32p]
    lib.arvx_closure.argtypes = [p, C.c_int, C.c_int]
    lib.arvx_closure_count.argtypes = [p, C.POINTER(C.c_int64)]
    lib.arvx_closure_download.argtypes = [p, C.POINTER(C.c_int64), f32p]
    lib.arvx_export_model.argtypes = [p, f32p, C.c_int]
    lib.arvx_get_stats.argtypes = [p, C.POINTER(Stats)]
    if hasattr(lib, "arvx_last_carve_path"):
        lib.arvx_last_carve_path.argtypes = [p, C.POINTER(C.c_uint32)]
    if hasattr(lib, "arvx_last_fast_carve_path"):
        lib.arvx_last_fast_carve_path.argtypes = [p, C.POINTER(C.c_uint32)]
    ab_build = bool(os.environ.get("ARVX_LIB_PATH"))  # an older build may lack newer symbols
    if hasattr(lib, "arvx_selftest_divide") or not ab_build:
        lib.arvx_selftest_divide.argtypes = [p, C.c_int64, f32p, f32p, f32p, f32p]
    if hasattr(lib, "arvx_selftest_round") or not ab_build:
        lib.arvx_selftest_round.argtypes = [p, C.POINTER(C.c_int64)]
    if hasattr(lib, "arvx_selftest_rect_cache") or not ab_build:
        lib.arvx_ctx_set_rect_cache_limit.argtypes = [p, C.c_uint64]
        lib.arvx_selftest_rect_cache.argtypes = [p, C.POINTER(C.c_int64)]
    if hasattr(lib, "arvx_ctx_set_pixel_cache_limit") or not ab_build:
        lib.arvx_ctx_set_pixel_cache_limit.argtypes = [p, C.c_uint64]
    if hasattr(lib, "arvx_pixel_cache_views") or not ab_build:
        lib.arvx_pixel_cache_views.argtypes = [p, C.POINTER(C.c_uint64), C.c_int]
    if hasattr(lib, "arvx_selftest_pixel_cache") or not ab_build:
        lib.arvx_selftest_pixel_cache.argtypes = [p, C.POINTER(C.c_int64)]
    if hasattr(lib, "arvx_view_window") or not ab_build:
        lib.arvx_ctx_set_view_window.argtypes = [p, C.c_int]
        lib.arvx_view_window.argtypes = [p, C.c_int, C.POINTER(C.c_int)]
        lib.arvx_view_window_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, f32p, C.c_int, C.c_int,
                                              C.POINTER(C.c_int)]
        lib.arvx_selftest_fill_view_tables.argtypes = [p, C.c_int]
        lib.arvx_selftest_view_table_raw.argtypes = [p, C.c_int, C.c_void_p]
    if hasattr(lib, "arvx_mc_cells") or not ab_build:
        lib.arvx_mc_cells.argtypes = [p, C.POINTER(C.c_int64)]
        lib.arvx_mc_cells_download.argtypes = [p, C.POINTER(C.c_int32)]
    if hasattr(lib, "arvx_occupancy_compress") or not ab_build:
        lib.arvx_occupancy_packet_words.argtypes = [C.c_int64, C.c_int64]
        lib.arvx_occupancy_compress.argtypes = [p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        lib.arvx_occupancy_expand.argtypes = [p, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                              C.c_int64, C.c_void_p, C.c_void_p]
        if hasattr(lib, "arvx_occupancy_expand_striped") or not ab_build:
            lib.arvx_occupancy_expand_striped.argtypes = [p, C.c_void_p, C.c_int, C.c_int64,
                                                          C.c_int64, C.c_int64, C.c_void_p,
                                                          C.c_void_p]
        if hasattr(lib, "arvx_occupancy_pack_compress"):
            lib.arvx_occupancy_pack_compress.argtypes = [p, C.c_void_p, C.c_int64, C.c_void_p]
            lib.arvx_occupancy_expand_striped_others.argtypes = [p, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                                                 C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    if hasattr(lib, "arvx_mc_mesh_smooth"):
        lib.arvx_mc_mesh_smooth.argtypes = [p, C.c_int, C.c_float, C.c_float]
        lib.arvx_mc_mesh_smooth_download.argtypes = [p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "arvx_mc_mesh_decimate"):
        lib.arvx_mc_mesh_decimate.argtypes = [p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.arvx_mc_mesh_decimate_download.argtypes = [p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
    if hasattr(lib, "arvx_mc_mesh_refined"):
        lib.arvx_mc_mesh_refined.argtypes = [p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.arvx_mc_mesh_refined_download.argtypes = [p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p]
    if hasattr(lib, "arvx_color_visible"):
        lib.arvx_color_visible.argtypes = [p, C.c_int, C.c_float]
        lib.arvx_surface_visible_download.argtypes = [p, C.POINTER(C.c_int32)]
        lib.arvx_view_depth_download.argtypes = [p, C.c_int, f32p]
    if hasattr(lib, "arvx_photo_carve"):
        lib.arvx_photo_carve.argtypes = [p, C.c_float, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int64)]
    if hasattr(lib, "arvx_carve_votes"):
        lib.arvx_carve_votes.argtypes = [p, C.c_int, C.c_uint]
        lib.arvx_votes_download.argtypes = [p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "arvx_components"):
        lib.arvx_components.argtypes = [p, C.c_int, C.POINTER(C.c_int64)]
        lib.arvx_components_download.argtypes = [p, C.c_void_p, C.c_void_p]
        lib.arvx_components_labels_download.argtypes = [p, C.c_void_p]
        lib.arvx_components_keep.argtypes = [p, C.c_int, C.c_int64, C.c_uint, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64)]
    if hasattr(lib, "arvx_distance"):
        lib.arvx_distance.argtypes = [p, C.c_uint]
        lib.arvx_distance_download.argtypes = [p, C.c_void_p]
        lib.arvx_morph.argtypes = [p, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if hasattr(lib, "arvx_render"):
        lib.arvx_render.argtypes = [p, f32p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.arvx_render_view.argtypes = [p, C.c_int]
        lib.arvx_render_download.argtypes = [p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.arvx_render_agreement.argtypes = [p, C.c_int, C.POINTER(C.c_int64)]
    if hasattr(lib, "arvx_render_mesh") or not ab_build:
        lib.arvx_render_mesh.argtypes = [p, C.c_int, f32p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.arvx_render_mesh_view.argtypes = [p, C.c_int, C.c_int, C.c_void_p]
        lib.arvx_render_mesh_agreement.argtypes = [p, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        lib.arvx_render_triangles.argtypes = [p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, f32p,
                                              C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.arvx_render_mesh_stats.argtypes = [p, C.POINTER(C.c_int64)]
        lib.arvx_selftest_render_mesh_list.argtypes = [p, C.c_int64]
    if hasattr(lib, "arvx_ctx_set_render_near") or not ab_build:
        lib.arvx_ctx_set_render_near.argtypes = [p, C.c_float]
        lib.arvx_ctx_render_near.argtypes = [p, C.POINTER(C.c_float)]
        lib.arvx_render_mesh_clip_stats.argtypes = [p, C.POINTER(C.c_int64)]
    if hasattr(lib, "arvx_selftest_compute_units") or not ab_build:
        lib.arvx_selftest_compute_units.argtypes = [p, C.c_int]
    if hasattr(lib, "arvx_mesh_color") or not ab_build:
        lib.arvx_mesh_color.argtypes = [p, C.c_int, C.c_int, C.c_float, C.c_uint, C.POINTER(C.c_int64)]
        lib.arvx_mesh_color_count.argtypes = [p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.arvx_mesh_color_download.argtypes = [p, C.c_void_p, C.c_void_p]
        lib.arvx_mesh_color_depth_download.argtypes = [p, C.c_int, C.c_void_p]
        lib.arvx_selftest_mesh_color_batch.argtypes = [p, C.c_int]
    if hasattr(lib, "arvx_mesh_texture") or not ab_build:
        lib.arvx_mesh_texture.argtypes = [p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint, C.POINTER(C.c_int64)]
        lib.arvx_mesh_texture_info.argtypes = [p, C.POINTER(C.c_int64)]
        lib.arvx_mesh_texture_download.argtypes = [p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "arvx_mesh_relax") or not ab_build:
        lib.arvx_mesh_relax.argtypes = [p, C.c_int, C.c_int, C.c_float, C.c_float]
        lib.arvx_mesh_relax_info.argtypes = [p, C.POINTER(C.c_int64)]
        lib.arvx_mesh_relax_download.argtypes = [p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.arvx_mesh_relax_triangles.argtypes = [p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                                  C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "arvx_segment_views") or not ab_build:
        sp = C.POINTER(SegmentParams)
        lib.arvx_segment_views.argtypes = [p, C.c_int, f32p, f32p, C.c_void_p, C.c_int, C.c_int, C.c_size_t,
                                           C.c_void_p, C.c_int, sp]
        lib.arvx_segment_views_device.argtypes = [p, C.c_int, f32p, f32p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_int, sp]
        lib.arvx_segment_download.argtypes = [p, C.c_int, C.c_void_p]
        lib.arvx_segment_counts.argtypes = [p, C.c_int, C.POINTER(C.c_int64)]
        lib.arvx_selftest_segment_batch.argtypes = [p, C.c_int]
    for name in SYMBOLS:
        if ab_build and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        if name == "arvx_occupancy_packet_words":
            fn.restype = C.c_int64
        elif name not in ("arvx_last_error",):
            fn.restype = C.c_int
    _libs[path] = lib
    return lib


def occupancy_packet_words(n_words64: int, cap_words64: int) -> int:
    """64-bit words of one compressed-occupancy packet (header + room for cap mixed words)."""
    return int(load_library().arvx_occupancy_packet_words(n_words64, cap_words64))


def _check(rc: int, lib: Optional[C.CDLL] = None) -> None:
    if rc != 0:
        lib = lib or load_library()
        raise ArvxError(rc, lib.arvx_last_error().decode("utf-8", "replace"))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def compose_projection(K, Rt) -> np.ndarray:
    """M = K * Rt as the reference's `intr * pose` (fp32, unfused, left to right)."""
    K = _f32(K).reshape(9)
    Rt = _f32(Rt).reshape(12)
    M = np.empty(12, np.float32)
    _check(load_library().arvx_compose_projection(_fp(K), _fp(Rt), _fp(M)))
    return M.reshape(3, 4)


def headlight(M) -> np.ndarray:
    """The viewing direction of the camera M (3 x 4, world -> pixel) along the voxel axes x, y, z, for the
    `light` of render_mesh: (m21, m20, -m22), the third row of M reordered, because world = (y * s, x * s,
    -z * s)."""
    M = _f32(M).reshape(3, 4)
    return np.array([M[2, 1], M[2, 0], -M[2, 2]], np.float32)


def view_window_host(X: int, Y: int, Z: int, voxel_size: float, M, W: int, H: int) -> Tuple[int, int, int, int]:
    """(first row, last row, first column, last column), inclusive, of the part of a view's
    summed-area table that the one-launch view derivation writes for a grid of X x Y x Z voxels
    under the camera M (3 x 4): arvx_view_window_host, host arithmetic only."""
    M = _f32(M).reshape(12)
    rect = (C.c_int * 4)()
    _check(load_library().arvx_view_window_host(X, Y, Z, C.c_float(voxel_size), _fp(M), W, H, rect))
    return tuple(int(r) for r in rect)


def stripe_planes(Z: int, world: int, rank: int) -> np.ndarray:
    """Global z of the planes a striped context holds, in local order."""
    groups = np.arange(rank, Z // 8, world)
    return (groups[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)


class Context:
    """One voxel grid (or Z slab) on one GPU: thin wrapper of arvx_ctx."""

    def __init__(self, X: int, Y: int, Z: int, voxel_size: float, device: int = 0,
                 z_range: Optional[Sequence[int]] = None,
                 stripes: Optional[Sequence[int]] = None, lib_path: Optional[str] = None,
                 assoc: Optional[int] = None, halo: int = 1):
        """z_range=(z0,z1): contiguous slab.  stripes=(world, rank): 8-plane groups
        rank, rank+world, ... (load-balanced multi-GPU split).  lib_path: another build of
        the library (A/B).  assoc: ASSOC_LEFT / ASSOC_RIGHT, the grouping of the M*world row
        sums of this context (default: the library's, arvx_projection_assoc).  halo: planes a
        slab keeps (and recomputes) beyond its own on each inner side: arvx_ctx_create_slab_halo."""
        self._lib = load_library(lib_path)
        self._h = C.c_void_p()
        self.X, self.Y, self.Z = int(X), int(Y), int(Z)
        self.voxel_size = float(np.float32(voxel_size))
        if stripes is not None:
            world, rank = int(stripes[0]), int(stripes[1])
            self._ck(self._lib.arvx_ctx_create_striped(C.byref(self._h), device, X, Y, Z,
                                                     C.c_float(voxel_size), world, rank))
            self.planes = stripe_planes(Z, world, rank)
            self.z_range = None
        else:
            z0, z1 = (0, Z) if z_range is None else (int(z_range[0]), int(z_range[1]))
            self.z_range = (z0, z1)
            self._lib.arvx_ctx_create_slab_halo.argtypes = [
                C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                C.c_int, C.c_int]
            self._ck(self._lib.arvx_ctx_create_slab_halo(C.byref(self._h), device, X, Y, Z,
                                                       C.c_float(voxel_size), z0, z1, int(halo)))
            self.planes = np.arange(z0, z1)
        nz = len(self.planes)  # global z of every local plane
        self.shape = (nz, Y, X)  # numpy view of the state plane: [z][y][x]
        self.nvox = nz * Y * X
        self._keep = []
        if assoc is not None:
            self.set_assoc(assoc)

    def set_assoc(self, assoc: int) -> None:
        self._lib.arvx_ctx_set_projection_assoc.argtypes = [C.c_void_p, C.c_int]
        self._ck(self._lib.arvx_ctx_set_projection_assoc(self._h, int(assoc)))

    @property
    def assoc(self) -> int:
        a = C.c_int()
        self._lib.arvx_ctx_projection_assoc.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        self._ck(self._lib.arvx_ctx_projection_assoc(self._h, C.byref(a)))
        return a.value

    def selftest_project(self, M, voxel_size, xyz):
        """(rows (n, 3), uv (n, 2)): the fp32 rows of M * toWord(x, y, z) and the quotients, as
        the kernels compute them with this context's grouping."""
        xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
        n = len(xyz)
        out = np.empty(5 * n, np.float32)
        M = np.ascontiguousarray(M, np.float32).reshape(12)
        self._lib.arvx_selftest_project.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_float,
                                                    C.c_void_p, C.c_void_p]
        self._ck(self._lib.arvx_selftest_project(self._h, n, M.ctypes.data, C.c_float(voxel_size),
                                                 xyz.ctypes.data, out.ctypes.data))
        return out[:3 * n].reshape(n, 3), out[3 * n:].reshape(n, 2)

    def selftest_view_tables(self, view: int, W: int, H: int):
        """(background bit plane as a (H, W) bool array, summed-area table as (H + 1, W + 1)
        uint16) of one view, as derived by set_views (include/arvx/arvx.h)."""
        self._lib.arvx_selftest_view_tables.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                        C.POINTER(C.c_int)]
        ld = C.c_int()
        self._ck(self._lib.arvx_selftest_view_tables(self._h, view, None, None, C.byref(ld)))
        bits = np.zeros((W * H + 31) // 32, np.uint32)
        table = np.zeros((H + 1, ld.value), np.uint16)
        self._ck(self._lib.arvx_selftest_view_tables(self._h, view, bits.ctypes.data, table.ctypes.data,
                                                     C.byref(ld)))
        bg = np.unpackbits(bits.view(np.uint8), bitorder="little")[:W * H].reshape(H, W).astype(bool)
        return bg, table[:, :W + 1].copy()

    def selftest_depth(self, campos, voxel_size, xyz):
        xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
        out = np.empty(len(xyz), np.float32)
        c = np.ascontiguousarray(campos, np.float32).reshape(3)
        self._lib.arvx_selftest_depth.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_float,
                                                  C.c_void_p, C.c_void_p]
        self._ck(self._lib.arvx_selftest_depth(self._h, len(xyz), c.ctypes.data,
                                               C.c_float(voxel_size), xyz.ctypes.data,
                                               out.ctypes.data))
        return out

    def _ck(self, rc: int) -> None:
        _check(rc, self._lib)

    def close(self) -> None:
        if self._h:
            self._lib.arvx_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- views --
    def set_views(self, M, masks, campos=None) -> None:
        """M: (V,3,4) float32. masks: (V,H,W) or (V,H,W,C) uint8 host array."""
        M = _f32(M).reshape(-1, 12)
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        if masks.ndim == 3:
            masks = masks[..., None]
        V, H, W, Cn = masks.shape
        assert M.shape[0] == V
        ptrs = (C.c_void_p * V)(*[masks[i].ctypes.data for i in range(V)])
        cp = None
        if campos is not None:
            campos = _f32(campos).reshape(V, 3)
            cp = _fp(campos)
        self._ck(self._lib.arvx_set_views(self._h, V, _fp(M), cp, ptrs, W, H, Cn, W * Cn))
        self.V, self.W, self.H = V, W, H

    def set_views_device(self, M, dev_masks_ptr: int, W: int, H: int, Cn: int,
                         campos=None) -> None:
        M = _f32(M).reshape(-1, 12)
        V = M.shape[0]
        cp = None
        if campos is not None:
            campos = _f32(campos).reshape(V, 3)
            cp = _fp(campos)
        self._keep = [M, campos]
        self._ck(self._lib.arvx_set_views_device(self._h, V, _fp(M), cp,
                                               C.c_void_p(dev_masks_ptr), W, H, Cn))
        self.V, self.W, self.H = V, W, H

    def set_images(self, images) -> None:
        """images: (V,H,W,3) uint8 BGR, undistorted."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        V, H, W, Cn = images.shape
        assert Cn == 3 and V == self.V and H == self.H and W == self.W
        ptrs = (C.c_void_p * V)(*[images[i].ctypes.data for i in range(V)])
        self._ck(self._lib.arvx_set_images(self._h, ptrs, W * 3))

    # -- silhouettes from the photographs --
    @staticmethod
    def _segment_params(rule, lo, hi, threshold, open_radius, close_radius, min_area, largest, max_hole):
        sp = SegmentParams()
        sp.rule = int(rule)
        for c in range(3):
            sp.lo[c], sp.hi[c] = int(lo[c]), int(hi[c])
        sp.threshold = int(threshold)
        sp.open_radius, sp.close_radius = int(open_radius), int(close_radius)
        sp.flags = SEGMENT_LARGEST if largest else 0
        sp.min_area, sp.max_hole = int(min_area), int(max_hole)
        return sp

    def segment_views(self, M, images, campos=None, plates=None, rule: int = SEGMENT_RANGE,
                      lo=(120, 120, 120), hi=(255, 255, 255), threshold: int = 0, open_radius: int = 0,
                      close_radius: int = 0, min_area: int = 0, largest: bool = False, max_hole: int = 0,
                      params: Optional[SegmentParams] = None) -> None:
        """arvx_segment_views: the views from the photographs.  M: (V,3,4) float32; images: (V,H,W,3)
        uint8 BGR, left resident as set_images would; plates (rule SEGMENT_PLATE): (H,W,3), (1,H,W,3)
        or (V,H,W,3).  The rule and the cleaning steps are those of include/arvx/arvx.h; the defaults
        are the reference's range rule (background 120..255) without cleaning.  `params`: a ready
        SegmentParams instead of the keywords."""
        M = _f32(M).reshape(-1, 12)
        images = np.ascontiguousarray(images, dtype=np.uint8)
        V, H, W, Cn = images.shape
        assert Cn == 3 and M.shape[0] == V
        ptrs = (C.c_void_p * V)(*[images[i].ctypes.data for i in range(V)])
        pp, n_plates = None, 0
        if plates is not None:
            plates = np.ascontiguousarray(plates, dtype=np.uint8).reshape(-1, H, W, 3)
            n_plates = len(plates)
            pp = (C.c_void_p * n_plates)(*[plates[i].ctypes.data for i in range(n_plates)])
        cp = None
        if campos is not None:
            campos = _f32(campos).reshape(V, 3)
            cp = _fp(campos)
        sp = params if params is not None else self._segment_params(
            rule, lo, hi, threshold, open_radius, close_radius, min_area, largest, max_hole)
        self._ck(self._lib.arvx_segment_views(self._h, V, _fp(M), cp, ptrs, W, H, W * 3, pp, n_plates,
                                              C.byref(sp)))
        self.V, self.W, self.H = V, W, H

    def segment_views_device(self, M, dev_images_ptr: int, W: int, H: int, campos=None, dev_plates_ptr: int = 0,
                             plate_count: int = 0, params: Optional[SegmentParams] = None, **kw) -> None:
        """arvx_segment_views_device: as segment_views, the images (and plates) tightly packed in device
        memory; no host synchronisation.  Keywords as segment_views."""
        M = _f32(M).reshape(-1, 12)
        V = M.shape[0]
        cp = None
        if campos is not None:
            campos = _f32(campos).reshape(V, 3)
            cp = _fp(campos)
        if params is None:
            d = dict(rule=SEGMENT_RANGE, lo=(120, 120, 120), hi=(255, 255, 255), threshold=0, open_radius=0,
                     close_radius=0, min_area=0, largest=False, max_hole=0)
            d.update(kw)
            params = self._segment_params(**d)
        self._keep = [M, campos]
        self._ck(self._lib.arvx_segment_views_device(
            self._h, V, _fp(M), cp, C.c_void_p(dev_images_ptr), W, H,
            C.c_void_p(dev_plates_ptr) if dev_plates_ptr else None, int(plate_count), C.byref(params)))
        self.V, self.W, self.H = V, W, H

    def segment_mask(self, view: int) -> np.ndarray:
        """arvx_segment_download: the final mask of a view, (H, W) uint8, 255 foreground."""
        self._ck(self._lib.arvx_segment_counts(self._h, int(view), (C.c_int64 * 8)()))  # (refused before any buffer)
        out = np.empty((self.H, self.W), np.uint8)
        self._ck(self._lib.arvx_segment_download(self._h, int(view), out.ctypes.data))
        return out

    def segment_counts(self, view: int) -> np.ndarray:
        """arvx_segment_counts: foreground pixels after the rule, the closing, the specks and the holes;
        speck components and pixels removed; hole components and pixels filled."""
        out = (C.c_int64 * 8)()
        self._ck(self._lib.arvx_segment_counts(self._h, int(view), out))
        return np.array(list(out), np.int64)

    def selftest_segment_batch(self, views_per_batch: int) -> None:
        """Views per labelling batch of segment_views from the next call on (0: the default bound)."""
        self._ck(self._lib.arvx_selftest_segment_batch(self._h, int(views_per_batch)))

    # -- state --
    def reset(self) -> None:
        self._ck(self._lib.arvx_state_reset(self._h))

    def upload_state(self, state) -> None:
        state = np.ascontiguousarray(state, dtype=np.uint8).reshape(-1)
        assert state.size == self.nvox
        self._ck(self._lib.arvx_state_upload(self._h, state.ctypes.data_as(C.POINTER(C.c_uint8))))

    def download_state(self) -> np.ndarray:
        out = np.empty(self.nvox, np.uint8)
        self._ck(self._lib.arvx_state_download(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.reshape(self.shape)

    def plane_words(self) -> int:
        return ((self.X + 31) // 32) * self.Y * len(self.planes)

    def download_planes(self, occ=None, seen=None):
        """(occ, seen) bit planes, uint32, rows padded to 32-bit words (into the caller's arrays,
        e.g. page-locked ones, when given)."""
        n = self.plane_words()
        if occ is None:
            occ, seen = np.empty(n, np.uint32), np.empty(n, np.uint32)
        assert occ.size == seen.size == n and occ.dtype == seen.dtype == np.uint32
        self._ck(self._lib.arvx_state_download_planes(self._h, occ.ctypes.data, seen.ctypes.data))
        return occ, seen

    def packet_geometry(self):
        """(n, H): 64-bit words per plane of the owned voxels, header words of a state packet."""
        n, h = C.c_int64(), C.c_int64()
        self._ck(self._lib.arvx_state_packet_geometry(self._h, C.byref(n), C.byref(h)))
        return int(n.value), int(h.value)

    def download_packets(self, occ=None, seen=None):
        """The owned voxels' occupancy and seen planes as compressed packets (arvx.h:
        arvx_state_download_packets) -> (occ_packet, seen_packet, occ_need, seen_need), uint64
        arrays of header + capacity words.  occ / seen: the caller's buffers (e.g. page-locked
        ones); too small a buffer is reported through need > capacity and the caller asks again."""
        n, H = self.packet_geometry()
        if occ is None:
            occ = np.empty(H + max(4096, n // 16), np.uint64)
        if seen is None:
            seen = np.empty(H + max(4096, n // 64), np.uint64)
        for _ in range(2):
            on, sn = C.c_int64(), C.c_int64()
            self._ck(self._lib.arvx_state_download_packets(self._h, occ.ctypes.data, occ.size - H,
                                                           seen.ctypes.data, seen.size - H,
                                                           C.byref(on), C.byref(sn)))
            if on.value <= occ.size - H and sn.value <= seen.size - H:
                break
            if on.value > occ.size - H:
                occ = np.empty(H + on.value, np.uint64)
            if sn.value > seen.size - H:
                seen = np.empty(H + sn.value, np.uint64)
        return occ, seen, int(on.value), int(sn.value)

    def upload_planes(self, occ, seen) -> None:
        occ = np.ascontiguousarray(occ, np.uint32)
        seen = np.ascontiguousarray(seen, np.uint32)
        assert occ.size == seen.size == self.plane_words()
        self._ck(self._lib.arvx_state_upload_planes(self._h, occ.ctypes.data, seen.ctypes.data))

    def undistort(self, images, K, dist) -> np.ndarray:
        """cv::undistort on (V,H,W[,C]) uint8 images; returns the same shape."""
        im = np.ascontiguousarray(images, np.uint8)
        shape = im.shape
        if im.ndim == 3:
            im = im[..., None]
        V, H, W, Cn = im.shape
        out = np.empty_like(im)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        dist = np.ascontiguousarray(dist, np.float64).reshape(-1)
        sp = (C.c_void_p * V)(*[im[i].ctypes.data for i in range(V)])
        dp = (C.c_void_p * V)(*[out[i].ctypes.data for i in range(V)])
        self._lib.arvx_undistort.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int,
                                             C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                             C.c_int, C.POINTER(C.c_void_p)]
        self._ck(self._lib.arvx_undistort(self._h, V, sp, W, H, Cn, W * Cn, K.ctypes.data,
                                          dist.ctypes.data if dist.size else None, dist.size, dp))
        return out.reshape(shape)

    def handle_unseen(self) -> None:
        self._ck(self._lib.arvx_handle_unseen(self._h))

    def state_device_ptr(self) -> int:
        ptr = C.c_void_p()
        n = C.c_size_t()
        self._ck(self._lib.arvx_state_device_ptr(self._h, C.byref(ptr), C.byref(n)))
        return int(ptr.value)

    def upload_halo(self, below=None, above=None) -> None:
        def ptr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
            assert a.size == self.X * self.Y
            self._keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_uint8))
        self._ck(self._lib.arvx_state_upload_halo(self._h, ptr(below), ptr(above)))

    def pack_occupancy(self, dev_words_ptr: int) -> None:
        self._ck(self._lib.arvx_pack_occupancy(self._h, C.c_void_p(dev_words_ptr)))

    def pack_occupancy_global(self, dev_global_words_ptr: int) -> None:
        self._ck(self._lib.arvx_pack_occupancy_global(self._h, C.c_void_p(dev_global_words_ptr)))

    # -- compressed occupancy exchange (device pointers; see include/arvx/arvx.h) --
    def occupancy_compress(self, dev_words_ptr: int, n_words64: int, dev_packet_ptr: int,
                           cap_words64: int) -> None:
        self._ck(self._lib.arvx_occupancy_compress(self._h, C.c_void_p(dev_words_ptr), n_words64,
                                                 C.c_void_p(dev_packet_ptr), cap_words64))

    def occupancy_expand(self, dev_packets_ptr: int, world: int, self_rank: int, n_words64: int,
                         cap_words64: int, dev_full_ptr: int, dev_overflow_ptr: int) -> None:
        self._ck(self._lib.arvx_occupancy_expand(self._h, C.c_void_p(dev_packets_ptr), world,
                                               self_rank, n_words64, cap_words64,
                                               C.c_void_p(dev_full_ptr),
                                               C.c_void_p(dev_overflow_ptr)))

    def occupancy_expand_striped(self, dev_packets_ptr: int, world: int, n_words64: int,
                                 cap_words64: int, words_per_group: int, dev_full_ptr: int,
                                 dev_overflow_ptr: int) -> None:
        self._ck(self._lib.arvx_occupancy_expand_striped(
            self._h, C.c_void_p(dev_packets_ptr), world, n_words64, cap_words64, words_per_group,
            C.c_void_p(dev_full_ptr), C.c_void_p(dev_overflow_ptr)))

    def occupancy_pack_compress(self, dev_packet_ptr: int, cap_words64: int, dev_full_ptr: int = 0) -> None:
        """The context's planes -> their packet, straight from the state; with dev_full_ptr the
        rank's own words also go to their place in the whole grid's plane."""
        self._ck(self._lib.arvx_occupancy_pack_compress(self._h, C.c_void_p(dev_packet_ptr), cap_words64,
                                                      C.c_void_p(dev_full_ptr)))

    def occupancy_expand_striped_others(self, dev_packets_ptr: int, world: int, self_rank: int,
                                        n_words64: int, cap_words64: int, words_per_group: int,
                                        dev_full_ptr: int, dev_overflow_ptr: int) -> None:
        self._ck(self._lib.arvx_occupancy_expand_striped_others(
            self._h, C.c_void_p(dev_packets_ptr), world, self_rank, n_words64, cap_words64,
            words_per_group, C.c_void_p(dev_full_ptr), C.c_void_p(dev_overflow_ptr)))

    def set_stream(self, stream_ptr: int) -> None:
        self._ck(self._lib.arvx_ctx_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_exchange_stream(self, stream_ptr: int) -> None:
        """pack_occupancy*, occupancy_compress / _expand* launch on this stream (0: the
        context's); the caller orders it against the context's stream with events."""
        self._ck(self._lib.arvx_ctx_set_exchange_stream(self._h, C.c_void_p(stream_ptr)))

    def synchronize(self) -> None:
        self._ck(self._lib.arvx_ctx_synchronize(self._h))

    # -- hot path --
    def carve(self, flags: int = 0) -> None:
        self._ck(self._lib.arvx_carve(self._h, flags | _EXTRA_CARVE_FLAGS))

    def carve_views(self, first: int, count: int, flags: int = 0) -> None:
        self._ck(self._lib.arvx_carve_views(self._h, first, count, flags | _EXTRA_CARVE_FLAGS))

    def last_carve_path(self) -> dict:
        """Which kernels the last carve of this context launched (PATH_* bits) and how much work
        its pre-passes handed on: coarse tiles listed, workgroups of the dense classify kernel
        (0: the other kernel ran), sub-tiles queued for the exact kernel.  Synchronises."""
        out = (C.c_uint32 * 4)()
        self._ck(self._lib.arvx_last_carve_path(self._h, out))
        return {"bits": int(out[0]), "listed": int(out[1]), "dense_grid": int(out[2]),
                "items": int(out[3])}

    def fast_carve(self) -> None:
        self._ck(self._lib.arvx_fast_carve(self._h))

    def last_fast_carve_path(self) -> dict:
        """How the last greedy carve of this context grew its component: FLOOD_* bits, the tiles
        its whole-tile pre-pass seeded (0 without one), the launches of its step kernel and its
        rows of tiles.  All zero before the first greedy carve.  Synchronises."""
        out = (C.c_uint32 * 4)()
        self._ck(self._lib.arvx_last_fast_carve_path(self._h, out))
        return {"bits": int(out[0]), "seeded": int(out[1]), "launches": int(out[2]),
                "tile_rows": int(out[3])}

    def color(self, mode: int) -> None:
        self._ck(self._lib.arvx_color(self._h, mode))

    def surface(self):
        n = C.c_int64()
        self._ck(self._lib.arvx_surface_count(self._h, C.byref(n)))
        idx = np.empty(n.value, np.int64)
        rgb = np.empty((n.value, 3), np.float32)
        if n.value:
            self._ck(self._lib.arvx_surface_download(
                self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), _fp(rgb)))
        return idx, rgb

    def surface_depth(self) -> np.ndarray:
        n = C.c_int64()
        self._ck(self._lib.arvx_surface_count(self._h, C.byref(n)))
        d = np.empty(n.value, np.float32)
        if n.value:
            self._ck(self._lib.arvx_surface_depth_download(self._h, _fp(d)))
        return d

    def color_visible(self, mode: int, tolerance: float) -> None:
        """arvx_color_visible: the colour vote over the views in which each voxel is visible
        (per-view depth buffers of the surface; tolerance in world units, >= 0, may be inf)."""
        self._ck(self._lib.arvx_color_visible(self._h, int(mode), float(tolerance)))

    def photo_carve(self, max_std: float, min_views: int = 2, tolerance: Optional[float] = None,
                    max_iterations: int = 32) -> Tuple[int, int]:
        """arvx_photo_carve: removes the surface voxels whose visible views disagree in colour
        (summed channel variance above max_std^2 over at least min_views views), until an iteration
        removes nothing or after max_iterations.  tolerance: the visibility test's, in world units
        (None: 3 voxel edges).  -> (iterations run, voxels removed)."""
        if tolerance is None:
            tolerance = np.float32(3) * np.float32(self.voxel_size)
        it = C.c_int()
        removed = C.c_int64()
        self._ck(self._lib.arvx_photo_carve(self._h, float(max_std), int(min_views), float(tolerance),
                                            int(max_iterations), C.byref(it), C.byref(removed)))
        return it.value, removed.value

    def carve_votes(self, max_misses: int, counts: bool = False, cull: bool = True) -> None:
        """arvx_carve_votes: empties the voxels that more than max_misses views see as background
        (max_misses = 0: the plain carve).  counts: keep the per-voxel counts for votes(); cull =
        False: project every voxel in every view."""
        flags = (VOTES_COUNTS if counts else 0) | (0 if cull else VOTES_NO_CULL)
        self._ck(self._lib.arvx_carve_votes(self._h, int(max_misses), flags))

    def votes(self) -> Tuple[np.ndarray, np.ndarray]:
        """arvx_votes_download: (background, inside), uint16 per voxel in flat index order -- the views
        that see the voxel as background / whose image it projects into, of the last
        carve_votes(..., counts=True)."""
        bg = np.empty(self.nvox, np.uint16)
        inside = np.empty(self.nvox, np.uint16)
        self._ck(self._lib.arvx_votes_download(self._h, bg.ctypes.data, inside.ctypes.data))
        return bg, inside

    def components(self, connectivity: int = 6) -> Tuple[np.ndarray, np.ndarray]:
        """arvx_components + arvx_components_download: labels the occupied voxels' connected
        components (connectivity 6 or 26) -> (labels, sizes), int32 each, labels ascending; a label
        is the least flat index of its component.  The state is unchanged."""
        n = C.c_int64()
        self._ck(self._lib.arvx_components(self._h, int(connectivity), C.byref(n)))
        labels = np.empty(n.value, np.int32)
        sizes = np.empty(n.value, np.int32)
        self._ck(self._lib.arvx_components_download(self._h, labels.ctypes.data, sizes.ctypes.data))
        return labels, sizes

    def component_labels(self) -> np.ndarray:
        """arvx_components_labels_download: int32 per voxel in flat index order, the label of its
        component in the last components(), -1 where empty."""
        out = np.empty(self.nvox, np.int32)
        self._ck(self._lib.arvx_components_labels_download(self._h, out.ctypes.data))
        return out

    def keep_components(self, min_voxels: int = 1, largest: bool = False,
                        connectivity: int = 6) -> Tuple[int, int]:
        """arvx_components_keep: empties every component of fewer than min_voxels voxels and, with
        largest, every component but the largest (the least label among equals).
        -> (components kept, voxels removed)."""
        kept = C.c_int64()
        removed = C.c_int64()
        self._ck(self._lib.arvx_components_keep(self._h, int(connectivity), int(min_voxels),
                                                COMPONENTS_LARGEST if largest else 0,
                                                C.byref(kept), C.byref(removed)))
        return kept.value, removed.value

    def distance(self, border_occupied: bool = False) -> np.ndarray:
        """arvx_distance + arvx_distance_download: the signed squared Euclidean distance of every voxel
        to the nearest voxel of the other kind, int32 in flat index order: positive on occupied voxels
        (to the nearest empty site; the lattice points outside the grid count as empty unless
        border_occupied), negative on empty ones, +-DISTANCE_INF where there is no such site.  The
        state is unchanged."""
        self._ck(self._lib.arvx_distance(self._h, DISTANCE_BORDER_OCCUPIED if border_occupied else 0))
        out = np.empty(self.nvox, np.int32)
        self._ck(self._lib.arvx_distance_download(self._h, out.ctypes.data))
        return out

    def morph(self, op: int, radius_sq: int) -> Tuple[int, int]:
        """arvx_morph: erosion, dilation, opening or closing (MORPH_*) of the occupancy by the ball of
        the offsets o with |o|^2 <= radius_sq -> (voxels removed, voxels added)."""
        removed = C.c_int64()
        added = C.c_int64()
        self._ck(self._lib.arvx_morph(self._h, int(op), int(radius_sq), C.byref(removed), C.byref(added)))
        return removed.value, added.value

    def surface_visible(self) -> np.ndarray:
        """arvx_surface_visible_download: views each coloured voxel is visible in (surface()'s
        order; 0: the voxel took the plain vote)."""
        n = C.c_int64()
        self._ck(self._lib.arvx_surface_count(self._h, C.byref(n)))
        out = np.empty(n.value, np.int32)
        if n.value:
            self._ck(self._lib.arvx_surface_visible_download(
                self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def view_depth(self, view: int) -> np.ndarray:
        """arvx_view_depth_download: the depth buffer of one view, (H, W) float32."""
        out = np.empty((self.H, self.W), np.float32)
        self._ck(self._lib.arvx_view_depth_download(self._h, int(view), _fp(out)))
        return out

    SAMPLE_DTYPE = np.dtype([("r", np.uint8), ("g", np.uint8), ("b", np.uint8), ("valid", np.uint8),
                             ("depth", np.float32)])

    def color_samples(self, index) -> np.ndarray:
        """The colour lists behind the vote (Model::addColor / getColors of the reference):
        (n, V) records r, g, b, valid, depth for n voxels (flat indices over the owned planes)."""
        index = np.ascontiguousarray(index, dtype=np.int64)
        out = np.zeros((len(index), self.V), self.SAMPLE_DTYPE)
        self._lib.arvx_color_samples.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        self._ck(self._lib.arvx_color_samples(self._h, len(index), index.ctypes.data, out.shape[1],
                                              out.ctypes.data))
        return out

    def upload_colors(self, index, rgb) -> None:
        index = np.ascontiguousarray(index, dtype=np.int64)
        rgb = _f32(rgb).reshape(-1, 3)
        assert len(index) == len(rgb)
        self._ck(self._lib.arvx_colors_upload(self._h, len(index),
                                            index.ctypes.data_as(C.POINTER(C.c_int64)), _fp(rgb)))

    def closure(self, kernel_size: int = 3, apply_unseen: bool = True, download: bool = True):
        """applyClosure; returns (flat indices of the filled voxels, their RGBA) -- or, with
        download=False, only their number (the list stays on the device)."""
        self._ck(self._lib.arvx_closure(self._h, kernel_size, int(apply_unseen)))
        n = C.c_int64()
        self._ck(self._lib.arvx_closure_count(self._h, C.byref(n)))
        if not download:
            return int(n.value)
        idx = np.empty(n.value, np.int64)
        rgba = np.empty((n.value, 4), np.float32)
        if n.value:
            self._ck(self._lib.arvx_closure_download(
                self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), _fp(rgba)))
            i32 = np.empty(n.value, np.int32)  # the 32-bit form must say the same
            r32 = np.empty_like(rgba)
            self._lib.arvx_closure_download32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            self._ck(self._lib.arvx_closure_download32(self._h, i32.ctypes.data, r32.ctypes.data))
            assert np.array_equal(i32, idx) and np.array_equal(r32.view(np.uint32), rgba.view(np.uint32))
        return idx, rgba

    def closure_download(self):
        """The last closure's filled voxels (arvx_closure_count / _download): (flat indices, RGBA)."""
        n = C.c_int64()
        self._ck(self._lib.arvx_closure_count(self._h, C.byref(n)))
        idx = np.empty(n.value, np.int64)
        rgba = np.empty((n.value, 4), np.float32)
        if n.value:
            self._ck(self._lib.arvx_closure_download(
                self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), _fp(rgba)))
        return idx, rgba

    def mc_cells(self) -> np.ndarray:
        """(n, 4) int32 -- x, y, z, cube index of the cells marchingCubes would
        triangulate, in its visiting order (x outermost, z innermost)."""
        n = C.c_int64()
        self._ck(self._lib.arvx_mc_cells(self._h, C.byref(n)))
        cells = np.empty((n.value, 4), np.int32)
        if n.value:
            self._ck(self._lib.arvx_mc_cells_download(
                self._h, cells.ctypes.data_as(C.POINTER(C.c_int32))))
        return cells

    def mc_mesh(self, apply_unseen: bool = False):
        """(verts (3T, 3) float32 in voxel units, face_rgb (T, 3) uint32) of marchingCubes()."""
        n = C.c_int64()
        self._lib.arvx_mc_mesh.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        self._lib.arvx_mc_mesh_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._ck(self._lib.arvx_mc_mesh(self._h, int(apply_unseen), C.byref(n)))
        verts = np.empty((3 * n.value, 3), np.float32)
        rgb = np.empty((n.value, 3), np.uint32)
        if n.value:
            self._ck(self._lib.arvx_mc_mesh_download(self._h, verts.ctypes.data, rgb.ctypes.data))
            # the face-record form must say the same: (3t, 3t+1, 3t+2, r, g, b) per triangle
            v2 = np.empty_like(verts)
            faces = np.empty((n.value, 6), np.uint32)
            self._lib.arvx_mc_mesh_download_faces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            self._ck(self._lib.arvx_mc_mesh_download_faces(self._h, v2.ctypes.data,
                                                          faces.ctypes.data))
            t3 = 3 * np.arange(n.value, dtype=np.uint32)
            assert np.array_equal(v2, verts) and np.array_equal(faces[:, 3:], rgb)
            assert np.array_equal(faces[:, :3], t3[:, None] + np.arange(3, dtype=np.uint32))
        return verts, rgb

    def mc_mesh_welded(self, apply_unseen: bool = False, vertex_colors: bool = False):
        """The mesh of mc_mesh with shared vertices (arvx_mc_mesh_welded): (verts (V, 3) float32
        in voxel units, ascending (z, y, x), faces (T, 3) uint32 vertex indices, face_rgb (T, 3)
        uint32[, vertex_rgb (V, 3) float32 when vertex_colors])."""
        nv, nt = C.c_int64(), C.c_int64()
        self._lib.arvx_mc_mesh_welded.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64),
                                                  C.POINTER(C.c_int64)]
        self._lib.arvx_mc_mesh_welded_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p]
        self._ck(self._lib.arvx_mc_mesh_welded(self._h, int(apply_unseen), C.byref(nv),
                                               C.byref(nt)))
        self._weld_v = int(nv.value)  # (mc_mesh_smooth_download's V)
        verts = np.empty((nv.value, 3), np.float32)
        records = np.empty((nt.value, 6), np.uint32)  # i0, i1, i2, r, g, b
        vrgb = np.empty((nv.value, 3), np.float32) if vertex_colors else None
        self._ck(self._lib.arvx_mc_mesh_welded_download(
            self._h, verts.ctypes.data, records.ctypes.data,
            vrgb.ctypes.data if vrgb is not None else None))
        out = (verts, np.ascontiguousarray(records[:, :3]), np.ascontiguousarray(records[:, 3:]))
        return out + (vrgb,) if vertex_colors else out

    def mc_mesh_welded_count(self, apply_unseen: bool = False):
        """arvx_mc_mesh_welded without the download: (V, T); the mesh stays on the device."""
        nv, nt = C.c_int64(), C.c_int64()
        self._lib.arvx_mc_mesh_welded.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64),
                                                  C.POINTER(C.c_int64)]
        self._ck(self._lib.arvx_mc_mesh_welded(self._h, int(apply_unseen), C.byref(nv),
                                               C.byref(nt)))
        self._weld_v = int(nv.value)  # (mc_mesh_smooth_download's V)
        return int(nv.value), int(nt.value)

    def mc_mesh_smooth(self, iterations: int = 1, lam: float = 0.5, mu: float = -0.53,
                       download: bool = True):
        """Taubin smoothing and vertex normals of the mesh of the last mc_mesh_welded
        (arvx_mc_mesh_smooth): (verts (V, 3) float32, normals (V, 3) float32); the faces are
        mc_mesh_welded's.  download=False: the call only, the result stays on the device."""
        self._ck(self._lib.arvx_mc_mesh_smooth(self._h, int(iterations), float(lam), float(mu)))
        if not download:
            return None
        return self.mc_mesh_smooth_download()

    def mc_mesh_smooth_download(self, verts: bool = True, normals: bool = True):
        """arvx_mc_mesh_smooth_download: (verts, normals), each (V, 3) float32 or None."""
        nv = getattr(self, "_weld_v", 0)
        v = np.empty((nv, 3), np.float32) if verts else None
        n = np.empty((nv, 3), np.float32) if normals else None
        self._ck(self._lib.arvx_mc_mesh_smooth_download(
            self._h, v.ctypes.data if v is not None else None, n.ctypes.data if n is not None else None))
        return v, n

    def mc_mesh_decimate(self, cell: int, source: int = 0, download: bool = True):
        """Vertex clustering of the mesh of the last mc_mesh_welded (arvx_mc_mesh_decimate) with
        cubes of cell^3 voxels; source: DECIMATE_LATTICE or DECIMATE_SMOOTHED (the positions of
        the last mc_mesh_smooth).  Returns mc_mesh_decimate_download()'s tuple; download=False:
        (Vd, Td), the result stays on the device."""
        nv, nt = C.c_int64(), C.c_int64()
        self._ck(self._lib.arvx_mc_mesh_decimate(self._h, int(cell), int(source), C.byref(nv), C.byref(nt)))
        self._dec_vt = (int(nv.value), int(nt.value))
        if not download:
            return self._dec_vt
        return self.mc_mesh_decimate_download()

    def mc_mesh_decimate_download(self, verts: bool = True, faces: bool = True, vertex_rgb: bool = True,
                                  members: bool = True, vmap: bool = True):
        """arvx_mc_mesh_decimate_download: (verts (Vd, 3) float32, records (Td, 6) uint32 -- i0, i1,
        i2, r, g, b --, vertex_rgb (Vd, 3) float32, members (Vd,) int32, map (V,) int32), each None
        when not asked for."""
        nv, nt = getattr(self, "_dec_vt", (0, 0))
        V = getattr(self, "_weld_v", 0)
        out = [np.empty((nv, 3), np.float32) if verts else None,
               np.empty((nt, 6), np.uint32) if faces else None,
               np.empty((nv, 3), np.float32) if vertex_rgb else None,
               np.empty(nv, np.int32) if members else None,
               np.empty(V, np.int32) if vmap else None]
        self._ck(self._lib.arvx_mc_mesh_decimate_download(
            self._h, *[a.ctypes.data if a is not None else None for a in out]))
        return tuple(out)

    def mc_mesh_refined(self, bisections: int = 6, apply_unseen: bool = False, vertex_colors: bool = False,
                        details: bool = False):
        """Marching cubes with one vertex per cut edge, placed where the edge leaves the visual hull
        by `bisections` bisection steps against the views' masks (arvx_mc_mesh_refined; 0: plain
        midpoints): (verts (Vr, 3) float32 in voxel units, faces (T, 3) uint32, face_rgb (T, 3)
        uint32[, vertex_rgb (Vr, 3) float32 when vertex_colors][, edges (Vr, 4) int32 -- the occupied
        end and the direction to the empty one, + 8 where the edge is no silhouette edge --, cut (Vr,)
        int32, the position in units of 2^-(bisections+1), when details])."""
        nv, nt = self.mc_mesh_refined_count(bisections, apply_unseen)
        verts = np.empty((nv, 3), np.float32)
        records = np.empty((nt, 6), np.uint32)  # i0, i1, i2, r, g, b
        vrgb = np.empty((nv, 3), np.float32) if vertex_colors else None
        edges = np.empty((nv, 4), np.int32) if details else None
        cut = np.empty(nv, np.int32) if details else None
        self._ck(self._lib.arvx_mc_mesh_refined_download(
            self._h, verts.ctypes.data, records.ctypes.data,
            *[a.ctypes.data if a is not None else None for a in (vrgb, edges, cut)]))
        out = (verts, np.ascontiguousarray(records[:, :3]), np.ascontiguousarray(records[:, 3:]))
        if vertex_colors:
            out += (vrgb,)
        return out + (edges, cut) if details else out

    def mc_mesh_refined_count(self, bisections: int = 6, apply_unseen: bool = False):
        """arvx_mc_mesh_refined without the download: (Vr, T); the mesh stays on the device."""
        nv, nt = C.c_int64(), C.c_int64()
        self._ck(self._lib.arvx_mc_mesh_refined(self._h, int(apply_unseen), int(bisections), C.byref(nv),
                                                C.byref(nt)))
        return int(nv.value), int(nt.value)

    def render(self, M, W: int, H: int, background=None, download: bool = True):
        """arvx_render: the welded mesh's vertex voxels drawn into the camera M (3 x 4, world ->
        pixel) on a W x H image, over `background` ((H, W, 3) uint8 BGR, rows may be padded) or
        black: (bgr (H, W, 3) uint8, depth (H, W) float32, id (H, W) int32 -- the index into the
        welded vertex list, -1 where no voxel covers the pixel).  download=False: the call only."""
        M = _f32(M).reshape(12)
        bg, stride = None, 0
        if background is not None:
            bg = np.asarray(background)
            assert bg.dtype == np.uint8 and bg.shape == (H, W, 3) and bg.strides[1:] == (3, 1)
            stride = bg.strides[0]
        self._ck(self._lib.arvx_render(self._h, _fp(M), int(W), int(H),
                                       bg.ctypes.data if bg is not None else None, stride))
        self._render_wh = (int(W), int(H))
        return self.render_download() if download else None

    def render_view(self, view: int, download: bool = True):
        """arvx_render_view: render() with the camera and image size of the context's view `view`
        and no background."""
        self._ck(self._lib.arvx_render_view(self._h, int(view)))
        self._render_wh = (self.W, self.H)
        return self.render_download() if download else None

    def render_download(self, bgr: bool = True, depth: bool = True, id: bool = True):
        """arvx_render_download: (bgr, depth, id) of the last render, each an array or None."""
        W, H = getattr(self, "_render_wh", (0, 0))
        b = np.empty((H, W, 3), np.uint8) if bgr else None
        d = np.empty((H, W), np.float32) if depth else None
        i = np.empty((H, W), np.int32) if id else None
        self._ck(self._lib.arvx_render_download(self._h, *(a.ctypes.data if a is not None else None
                                                           for a in (b, d, i))))
        return b, d, i

    def render_agreement(self, view: int) -> Tuple[int, int, int]:
        """arvx_render_agreement: renders view `view` (it becomes the current render) and counts its
        pixels against the view's mask: (both: covered and foreground, model_only: covered and
        background, mask_only: uncovered and foreground)."""
        counts = (C.c_int64 * 3)()
        self._ck(self._lib.arvx_render_agreement(self._h, int(view), counts))
        self._render_wh = (self.W, self.H)
        return int(counts[0]), int(counts[1]), int(counts[2])

    @staticmethod
    def _background(background, W: int, H: int):
        if background is None:
            return None, 0
        bg = np.asarray(background)
        assert bg.dtype == np.uint8 and bg.shape == (H, W, 3) and bg.strides[1:] == (3, 1)
        return bg, bg.strides[0]

    def render_mesh(self, source: int, M, W: int, H: int, background=None, light=None, download: bool = True):
        """arvx_render_mesh: the triangles of the context's mesh `source` (MESH_WELDED, MESH_SMOOTHED,
        MESH_DECIMATED, MESH_REFINED) drawn with a depth buffer into the camera M (3 x 4, world -> pixel)
        on a W x H image, over `background` or black, flat-shaded by `light` (3 floats along the voxel
        axes, e.g. headlight(M); None: unshaded): (bgr, depth, id) as render() returns them, id the
        index into the source's face list.  download=False: the call only."""
        M = _f32(M).reshape(12)
        bg, stride = self._background(background, W, H)
        lt = None if light is None else _f32(light).reshape(3)
        self._ck(self._lib.arvx_render_mesh(self._h, int(source), _fp(M), int(W), int(H),
                                            bg.ctypes.data if bg is not None else None, stride,
                                            lt.ctypes.data if lt is not None else None))
        self._render_wh = (int(W), int(H))
        return self.render_download() if download else None

    def render_mesh_view(self, source: int, view: int, light=None, download: bool = True):
        """arvx_render_mesh_view: render_mesh() with the camera and image size of the context's view
        `view` and no background."""
        lt = None if light is None else _f32(light).reshape(3)
        self._ck(self._lib.arvx_render_mesh_view(self._h, int(source), int(view),
                                                 lt.ctypes.data if lt is not None else None))
        self._render_wh = (self.W, self.H)
        return self.render_download() if download else None

    def render_mesh_agreement(self, source: int, view: int) -> Tuple[int, int, int]:
        """arvx_render_mesh_agreement: render_agreement() of the mesh's triangles."""
        counts = (C.c_int64 * 3)()
        self._ck(self._lib.arvx_render_mesh_agreement(self._h, int(source), int(view), counts))
        self._render_wh = (self.W, self.H)
        return int(counts[0]), int(counts[1]), int(counts[2])

    def render_triangles(self, verts, vertex_rgb, faces, M, W: int, H: int, background=None, light=None,
                         download: bool = True):
        """arvx_render_triangles: render_mesh() of a caller's mesh -- verts (V, 3) float32 in voxel units,
        vertex_rgb (V, 3) float32, faces (T, 3) vertex indices or (T, 6) face records."""
        v, c = _f32(verts).reshape(-1, 3), _f32(vertex_rgb).reshape(-1, 3)
        assert len(v) == len(c)
        f = np.asarray(faces)
        rec = np.zeros((len(f), 6), np.uint32)
        if len(f):
            rec[:, :f.shape[1]] = f
        M = _f32(M).reshape(12)
        bg, stride = self._background(background, W, H)
        lt = None if light is None else _f32(light).reshape(3)
        self._ck(self._lib.arvx_render_triangles(self._h, len(v), v.ctypes.data, c.ctypes.data, len(rec),
                                                 rec.ctypes.data, _fp(M), int(W), int(H),
                                                 bg.ctypes.data if bg is not None else None, stride,
                                                 lt.ctypes.data if lt is not None else None))
        self._render_wh = (int(W), int(H))
        return self.render_download() if download else None

    def mesh_relax(self, source: int, iterations: int = 1, lam: float = 0.5, mu: float = -0.53,
                   download: bool = True):
        """arvx_mesh_relax: Taubin smoothing and vertex normals of the context's mesh `source` (MESH_WELDED,
        MESH_SMOOTHED, MESH_DECIMATED, MESH_REFINED) -- mc_mesh_smooth's definition on any of them.
        Returns mesh_relax_download()'s tuple; download=False: the call only, the product stays on the
        device.  MESH_RELAXED then names it as a source of render_mesh, mesh_color and mesh_texture."""
        self._ck(self._lib.arvx_mesh_relax(self._h, int(source), int(iterations), float(lam), float(mu)))
        return self.mesh_relax_download() if download else None

    def mesh_relax_info(self) -> Tuple[int, int, int]:
        """arvx_mesh_relax_info: (base source, V, T) of the relaxed mesh."""
        out = (C.c_int64 * 3)()
        self._ck(self._lib.arvx_mesh_relax_info(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def mesh_relax_download(self, verts: bool = True, normals: bool = True, degree: bool = True):
        """arvx_mesh_relax_download: (verts (V, 3) float32, normals (V, 3) float32, degree (V,) int32), each
        or None."""
        nv = self.mesh_relax_info()[1]
        v = np.empty((nv, 3), np.float32) if verts else None
        n = np.empty((nv, 3), np.float32) if normals else None
        d = np.empty(nv, np.int32) if degree else None
        self._ck(self._lib.arvx_mesh_relax_download(
            self._h, *(a.ctypes.data if a is not None else None for a in (v, n, d))))
        return v, n, d

    def mesh_relax_triangles(self, verts, faces, iterations: int = 1, lam: float = 0.5, mu: float = -0.53):
        """arvx_mesh_relax_triangles: mesh_relax() of a caller's mesh -- verts (V, 3) float32, faces (T, 3)
        vertex indices or (T, 6) face records.  Returns (verts, normals, degree); the context's own
        relaxed mesh stays as it was."""
        v = _f32(verts).reshape(-1, 3)
        f = np.asarray(faces)
        rec = np.zeros((len(f), 6), np.uint32)
        if len(f):
            rec[:, :f.shape[1]] = f
        q, n, d = np.empty_like(v), np.empty_like(v), np.empty(len(v), np.int32)
        self._ck(self._lib.arvx_mesh_relax_triangles(self._h, len(v), v.ctypes.data, len(rec), rec.ctypes.data,
                                                     int(iterations), float(lam), float(mu), q.ctypes.data,
                                                     n.ctypes.data, d.ctypes.data))
        return q, n, d

    def render_mesh_stats(self) -> Tuple[int, int, int, int]:
        """arvx_render_mesh_stats: (drawn, empty, flat, refused) triangles of the current triangle render."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.arvx_render_mesh_stats(self._h, out))
        return tuple(int(n) for n in out)

    def set_render_near(self, near: float) -> None:
        """arvx_ctx_set_render_near: the near plane of the triangle renders from the next one on -- faces
        that cross a2 = near are clipped against it.  0: none (the default)."""
        self._ck(self._lib.arvx_ctx_set_render_near(self._h, float(near)))

    def render_near(self) -> float:
        """arvx_ctx_render_near: the near plane as set (0: none)."""
        out = C.c_float()
        self._ck(self._lib.arvx_ctx_render_near(self._h, C.byref(out)))
        return float(out.value)

    def render_mesh_clip_stats(self) -> Tuple[int, int, int, int]:
        """arvx_render_mesh_clip_stats: (faces wholly behind the near plane, faces that straddle it,
        pieces made, pieces drawn) of the current triangle render; zeros for one made without a plane."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.arvx_render_mesh_clip_stats(self._h, out))
        return tuple(int(n) for n in out)

    def selftest_render_mesh_list(self, cap: int) -> None:
        """Room of the triangle render's list of large pixel boxes from the next render on (-1: default)."""
        self._ck(self._lib.arvx_selftest_render_mesh_list(self._h, int(cap)))

    def selftest_compute_units(self, n: int) -> None:
        """Compute units that size the context's launches from the next call on (0: the device's own
        count; never more than that)."""
        self._ck(self._lib.arvx_selftest_compute_units(self._h, int(n)))

    def mesh_color(self, source: int, mode: int, tolerance: float, flags: int = 0, download: bool = True):
        """arvx_mesh_color: the vertices of the context's mesh `source` coloured from the images -- per
        view the depth buffer of the mesh's own triangles, per vertex a vote (COLOR_CLOSEST or
        COLOR_AVERAGE) over the views that see it within `tolerance`, sampled bilinearly;
        MESH_COLOR_FOREGROUND drops the views whose mask has the vertex's pixel as background.
        -> (rgb (Vn, 3) float32, views (Vn,) int32: the views that see each vertex, coloured: the
        vertices some view sees).  render_mesh(source | MESH_IMAGE_COLORS, ...) draws them.
        download=False: the call only, -> coloured."""
        n = C.c_int64()
        self._ck(self._lib.arvx_mesh_color(self._h, int(source), int(mode), float(tolerance), int(flags),
                                           C.byref(n)))
        self._mesh_color_wh = (self.W, self.H)  # (the product keeps the image size of its call)
        if not download:
            return int(n.value)
        return self.mesh_color_download() + (int(n.value),)

    def mesh_color_download(self):
        """arvx_mesh_color_download: (rgb, views) of the product of the last mesh_color()."""
        nv = C.c_int64()
        self._ck(self._lib.arvx_mesh_color_count(self._h, C.byref(nv), None))
        rgb = np.empty((nv.value, 3), np.float32)
        views = np.empty(nv.value, np.int32)
        self._ck(self._lib.arvx_mesh_color_download(self._h, rgb.ctypes.data, views.ctypes.data))
        return rgb, views

    def mesh_color_depth(self, view: int) -> np.ndarray:
        """arvx_mesh_color_depth_download: the depth buffer of view `view` that mesh_color() voted with,
        (H, W) float32, +inf where no triangle covers the pixel."""
        self._ck(self._lib.arvx_mesh_color_count(self._h, None, None))  # (no product: refused before any buffer)
        W, H = self._mesh_color_wh
        d = np.empty((H, W), np.float32)
        self._ck(self._lib.arvx_mesh_color_depth_download(self._h, int(view), d.ctypes.data))
        return d

    def selftest_mesh_color_batch(self, views_per_batch: int) -> None:
        """Views per batch of mesh_color()'s depth pass from the next call on (0: the default bound)."""
        self._ck(self._lib.arvx_selftest_mesh_color_batch(self._h, int(views_per_batch)))

    def mesh_texture(self, source: int, resolution: int, atlas_width: int, tolerance: float = 0.0, flags: int = 0,
                     download: bool = True):
        """arvx_mesh_texture: a texture atlas of the context's mesh `source` with one triangle of texels
        per face (`resolution` texels along a leg, two faces per cell, `atlas_width` texels per atlas
        row), each face sampled from the view that sees its three corners within `tolerance` and shows
        it largest; MESH_TEXTURE_FOREGROUND as MESH_COLOR_FOREGROUND.
        -> (atlas (AH, AW, 3) uint8 BGR, face_view (T,) int32: the view or -1, face_uv (T, 3, 2)
        float32, counts (T, textured, AW, AH)).  render_mesh(source | MESH_TEXTURED, ...) draws it.
        download=False: the call only, -> counts."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.arvx_mesh_texture(self._h, int(source), int(resolution), int(atlas_width),
                                             float(tolerance), int(flags), out))
        counts = tuple(int(n) for n in out)
        if not download:
            return counts
        return self.mesh_texture_download() + (counts,)

    def mesh_texture_download(self):
        """arvx_mesh_texture_download: (atlas, face_view, face_uv) of the product of the last
        mesh_texture()."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.arvx_mesh_texture_info(self._h, out))
        T, _, AW, AH = (int(n) for n in out)
        atlas = np.empty((AH, AW, 3), np.uint8)
        view = np.empty(T, np.int32)
        uv = np.empty((T, 3, 2), np.float32)
        self._ck(self._lib.arvx_mesh_texture_download(self._h, atlas.ctypes.data, view.ctypes.data, uv.ctypes.data))
        return atlas, view, uv

    def mesh_texture_info(self) -> Tuple[int, int, int, int]:
        """arvx_mesh_texture_info: (T, textured, AW, AH) of the product."""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.arvx_mesh_texture_info(self._h, out))
        return tuple(int(n) for n in out)

    def mc_mesh_count(self, apply_unseen: bool = False) -> int:
        """arvx_mc_mesh without the download: the triangles stay on the device."""
        n = C.c_int64()
        self._lib.arvx_mc_mesh.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        self._ck(self._lib.arvx_mc_mesh(self._h, int(apply_unseen), C.byref(n)))
        return int(n.value)

    def export_model(self, apply_unseen: bool = False) -> np.ndarray:
        out = np.empty((self.nvox, 4), np.float32)
        self._ck(self._lib.arvx_export_model(self._h, _fp(out), int(apply_unseen)))
        return out

    def selftest_divide(self, a0, a1, b) -> np.ndarray:
        a0, a1, b = _f32(a0).reshape(-1), _f32(a1).reshape(-1), _f32(b).reshape(-1)
        out = np.empty((len(b), 4), np.float32)
        self._ck(self._lib.arvx_selftest_divide(self._h, len(b), _fp(a0), _fp(a1), _fp(b), _fp(out)))
        return out

    def selftest_round(self) -> int:
        """Mismatches between the kernels' pixel rounding and std::round (must be 0)."""
        n = C.c_int64(-1)
        self._ck(self._lib.arvx_selftest_round(self._h, C.byref(n)))
        return int(n.value)

    def set_rect_cache_limit(self, nbytes: int) -> None:
        """Bytes the context's table of cached rectangles may take (0: none).  Releases the table;
        it is built again, under the new limit, by the carves that follow."""
        self._ck(self._lib.arvx_ctx_set_rect_cache_limit(self._h, nbytes))

    def set_pixel_cache_limit(self, nbytes: int) -> None:
        """Bytes the context's table of cached pixels may take (0: none; default 6 GiB).  Releases
        the table; it is built again, under the new limit, with or right after the block table."""
        self._ck(self._lib.arvx_ctx_set_pixel_cache_limit(self._h, nbytes))

    def pixel_cache_views(self, V: int) -> Sequence[bool]:
        """Per view of the context: its pixels are read from the table of cached pixels (all False
        while the context holds no such table)."""
        nw = (V + 63) // 64
        words = (C.c_uint64 * nw)()
        self._ck(self._lib.arvx_pixel_cache_views(self._h, words, nw))
        return [bool((int(words[v // 64]) >> (v % 64)) & 1) for v in range(V)]

    def selftest_pixel_cache(self) -> int:
        """Bytes of the table of cached pixels that differ from a recomputation: must be 0
        (-1: the context holds no table)."""
        n = C.c_int64(-2)
        self._ck(self._lib.arvx_selftest_pixel_cache(self._h, C.byref(n)))
        return int(n.value)

    def set_view_window(self, on: bool) -> None:
        """Whether set_views writes only the part of each summed-area table that this context's
        grid projects into (default) or whole tables; from the next set_views on."""
        self._ck(self._lib.arvx_ctx_set_view_window(self._h, int(bool(on))))

    def view_window(self, view: int) -> Tuple[int, int, int, int]:
        """(first row, last row, first column, last column), inclusive, of view `view`'s table that
        the last set_views wrote."""
        rect = (C.c_int * 4)()
        self._ck(self._lib.arvx_view_window(self._h, view, rect))
        return tuple(int(r) for r in rect)

    def selftest_fill_view_tables(self, value: int) -> None:
        """Every byte of the table buffer <- value; the views count as not derived."""
        self._ck(self._lib.arvx_selftest_fill_view_tables(self._h, int(value)))

    def selftest_view_table_raw(self, view: int, H: int) -> np.ndarray:
        """View `view`'s table as it stands, (H + 1, ld) uint16, padding columns included; the
        entries outside the window are NOT written first (selftest_view_tables does that)."""
        ld = C.c_int()
        self._lib.arvx_selftest_view_tables.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                        C.POINTER(C.c_int)]
        self._ck(self._lib.arvx_selftest_view_tables(self._h, view, None, None, C.byref(ld)))
        table = np.zeros((H + 1, ld.value), np.uint16)
        self._ck(self._lib.arvx_selftest_view_table_raw(self._h, view, table.ctypes.data))
        return table

    def selftest_rect_cache(self) -> int:
        """Entries of the table of cached rectangles that differ from a recomputation: must be 0
        (-1: the context holds no table)."""
        n = C.c_int64(-2)
        self._ck(self._lib.arvx_selftest_rect_cache(self._h, C.byref(n)))
        return int(n.value)

    def stats(self) -> dict:
        s = Stats()
        self._ck(self._lib.arvx_get_stats(self._h, C.byref(s)))
        out = {k: int(getattr(s, k)) for k, _ in Stats._fields_ if k != "reserved"}
        out["slices_evaluated"] = int(s.reserved[0])  # 256-voxel slices projected exactly
        out["open_voxels_in_slices"] = int(s.reserved[1])  # of those voxels, not yet finished
        # (sub-tile, view) pairs that went to the exact kernel although every open voxel
        # got the same answer there: what a perfect classifier would have decided
        out["mixed_pairs_uniform"] = int(s.reserved[2])
        out["host_total_fallbacks"] = int(s.host_total_fallbacks)
        return out
