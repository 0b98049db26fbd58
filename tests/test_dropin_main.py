"""The drop-in headers (include/arvx/dropin/: Model.h, VoxelCarving.h, ColorReconstruction.h,
MarchingCubes.h, Postprocessing3d.h, Benchmark.h) type-check the way the reference's own caller
uses them ("keeping the Model/VoxelCarving C++ API surface so it drops in behind
main.cpp"): tests/cpp/dropin_typecheck.cpp exercises that surface against declarations-only
stand-ins for OpenCV and Eigen (tests/cpp/mock_opencv, tests/cpp/mock_eigen), with g++ and
ROCm's clang++ where it is installed.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
COMPILERS = ["g++"] + ([CLANG] if os.path.exists(CLANG) else [])


def _syntax_only(source, *include_dirs, extra=(), cxx="g++"):
    cmd = [cxx, "-std=c++17", "-fsyntax-only", *extra]
    for d in include_dirs:
        cmd.append("-I" + d)
    cmd.append(source)
    return subprocess.run(cmd, capture_output=True, text=True)


MOCKS = (os.path.join(ROOT, "tests", "cpp", "mock_opencv"),
         os.path.join(ROOT, "tests", "cpp", "mock_eigen"))


@pytest.mark.parametrize("cxx", COMPILERS)
@pytest.mark.parametrize("eigen", [False, True])
def test_dropin_surface_type_checks(eigen, cxx):
    """tests/cpp/dropin_typecheck.cpp: the five free functions and Model / SimpleMesh / Benchmark
    used the way the reference's replaced sources use them, with the stand-in vector types and
    with (mock) Eigen's; -Werror."""
    dirs = [os.path.join(ROOT, "include", "arvx", "dropin"), os.path.join(ROOT, "include"), MOCKS[0]]
    if eigen:
        dirs.append(MOCKS[1])
    r = _syntax_only(os.path.join(ROOT, "tests", "cpp", "dropin_typecheck.cpp"), *dirs,
                     extra=("-Wall", "-Wextra", "-Werror"), cxx=cxx)
    assert r.returncode == 0, r.stderr[-4000:]
