"""In-tree native builds: libarvx.so (hipcc, gfx950), the C++ host layer, and --
as test infrastructure only -- the CPU oracle (gcc)."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(directory: str, *targets: str) -> None:
    cmd = ["make", "-C", os.path.join(ROOT, directory), *targets]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{res.stdout}")


# the kernels of a bench step, the file that holds their launch geometry, and the compiler flags
STEP_KERNEL_SOURCES = ("arvx_device.h", "carve_kernels.h", "views_kernels.h", "arvx_ctx.h",
                       "arvx_capi.hip", "Makefile")


def source_stamp() -> str:
    """sha256 (16 hex digits) over the sources of the kernels of a bench step (view derivation +
    carve), their launch code (arvx_capi.hip, arvx_ctx.h) and the build's flags (the Makefile):
    what ties a PMC pass under profiles/ (tools/make_traffic.py) to the build bench.py is
    running."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "ar_voxel_project_amd", "csrc")
    for name in STEP_KERNEL_SOURCES:
        h.update(name.encode())
        h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def build_library() -> str:
    """hipcc --offload-arch=gfx950 -> ar_voxel_project_amd/lib/libarvx.so"""
    _make("ar_voxel_project_amd/csrc")
    return os.path.join(ROOT, "ar_voxel_project_amd", "lib", "libarvx.so")


def build_oracle() -> str:
    """gcc -> oracle/libarvx_oracle.so (checker for tests/smoke/cpu_baseline only)"""
    _make("oracle")
    return os.path.join(ROOT, "oracle", "libarvx_oracle.so")


def build_host_tests() -> str:
    """g++ -> tests/cpp/test_host: the C++ host layer (include/arvx/*.hpp) over libarvx.so"""
    build_library()
    _make("tests/cpp")
    _make("tools/cpp", "all")  # arvx_bench6 (the reference's -c=6 table), arvx_dropin_time
    build_weld_host_test()
    build_smooth_host_test()
    build_decimate_host_test()
    build_morph_host_test()
    build_refine_host_test()
    build_render_mesh_host_test()
    build_render_mesh_clip_host_test()
    build_mesh_color_host_test()
    build_mesh_texture_host_test()
    build_segment_host_test()
    build_mesh_relax_host_test()
    return os.path.join(ROOT, "tests", "cpp", "test_host")


def build_weld_host_test() -> str:
    """g++ -> tests/cpp/test_weld_host: arvx::weldMesh (include/arvx/marching_cubes.hpp) on a mesh
    from a file; the layer is header-only over libarvx.so, which is built first if missing."""
    return _build_host_test("test_weld_host")


def build_smooth_host_test() -> str:
    """g++ -> tests/cpp/test_smooth_host: arvx::smoothMesh (include/arvx/marching_cubes.hpp) on a
    welded mesh from a file, built as build_weld_host_test builds its test."""
    return _build_host_test("test_smooth_host")


def build_decimate_host_test() -> str:
    """g++ -> tests/cpp/test_decimate_host: arvx::decimateMesh (include/arvx/marching_cubes.hpp) on
    a welded mesh from a file, built as build_weld_host_test builds its test."""
    return _build_host_test("test_decimate_host")


def build_morph_host_test() -> str:
    """g++ -> tests/cpp/test_morph_host: arvx::signedDistance and arvx::morph
    (include/arvx/postprocessing.hpp) on a Model from a file, built as build_weld_host_test builds its
    test."""
    return _build_host_test("test_morph_host")


def build_refine_host_test() -> str:
    """g++ -> tests/cpp/test_refine_host: arvx::marchingCubesMeshRefined
    (include/arvx/marching_cubes.hpp) on a scene from a file, built as build_weld_host_test builds its
    test."""
    return _build_host_test("test_refine_host")


def build_render_mesh_host_test() -> str:
    """g++ -> tests/cpp/test_render_mesh_host: arvx::renderMesh (include/arvx/marching_cubes.hpp) on a
    scene from a file, built as build_weld_host_test builds its test."""
    return _build_host_test("test_render_mesh_host")


def build_render_mesh_clip_host_test() -> str:
    """g++ -> tests/cpp/test_render_mesh_clip_host: arvx::setRenderNear and arvx::renderMesh under a near
    plane (include/arvx/marching_cubes.hpp) on a scene from a file, built as build_weld_host_test
    builds its test."""
    return _build_host_test("test_render_mesh_clip_host")


def build_mesh_color_host_test() -> str:
    """g++ -> tests/cpp/test_mesh_color_host: arvx::colorMesh (include/arvx/marching_cubes.hpp) on a
    scene from a file, built as build_weld_host_test builds its test."""
    return _build_host_test("test_mesh_color_host")


def build_mesh_texture_host_test() -> str:
    """g++ -> tests/cpp/test_mesh_texture_host: the atlas layout and the OBJ writer
    (include/arvx/mesh_texture.hpp) on the host alone, and arvx::textureMesh
    (include/arvx/marching_cubes.hpp) on a scene from a file, built as build_weld_host_test builds its
    test."""
    return _build_host_test("test_mesh_texture_host")


def build_segment_host_test() -> str:
    """g++ -> tests/cpp/test_segment_host: arvx::segmentViews (include/arvx/segmentation.hpp) on a
    scene from a file, built as build_weld_host_test builds its test."""
    return _build_host_test("test_segment_host")


def build_mesh_relax_host_test() -> str:
    """g++ -> tests/cpp/test_mesh_relax_host: arvx::relaxMesh, both overloads
    (include/arvx/marching_cubes.hpp), on a scene from a file, built as build_weld_host_test builds its
    test."""
    return _build_host_test("test_mesh_relax_host")


def _build_host_test(name: str) -> str:
    lib_dir = os.path.join(ROOT, "ar_voxel_project_amd", "lib")
    if not os.path.exists(os.path.join(lib_dir, "libarvx.so")):
        build_library()
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    exe = os.path.join(ROOT, "tests", "cpp", name)
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
           "-I" + os.path.join(ROOT, "include"), "-pthread", "-o", exe, src, "-L" + lib_dir, "-larvx",
           "-Wl,-rpath," + lib_dir]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{res.stdout}")
    return exe


if __name__ == "__main__":
    print(build_library())
    print(build_oracle())
    print(build_host_tests())
