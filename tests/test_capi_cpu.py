"""CPU checks of the boundary: libarvx.so loads, exports every symbol the header
declares, its host-only helper is correct, the product never touches the oracle,
and without a GPU the library fails loudly instead of computing on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "arvx", "arvx.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(arvx_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_are_exported(arvx):
    lib = arvx.load_library()
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert getattr(lib, n) is not None, n
    assert sorted(arvx.SYMBOLS) == names, "capi.SYMBOLS out of sync with include/arvx/arvx.h"
    assert lib.arvx_version() == 100


def test_every_launch_goes_through_the_checked_helper():
    # the host convention ("One checked launch"): launch() is the only place of
    # arvx_capi.hip that launches a kernel, and it checks the launch itself
    text = open(os.path.join(ROOT, "ar_voxel_project_amd", "csrc", "arvx_capi.hip")).read()
    assert len(re.findall(r"\bhipLaunchKernelGGL\b", text)) == 1
    helper = text[text.index("static int launch("):]
    helper = helper[:helper.index("\n}\n")]
    assert "hipLaunchKernelGGL" in helper and "hipGetLastError()" in helper and "fail_hip" in helper
    stray = [n + 1 for n, line in enumerate(text.splitlines()) if line.strip() == "ARVX_HIP(hipGetLastError());"]
    assert not stray, f"hand-written launch checks at lines {stray}"


def test_no_torch_types_in_boundary():
    text = open(HEADER).read()
    assert "torch" not in text and "at::" not in text and "#include <hip" not in text


def test_compose_projection_host_helper(arvx, oracle):
    rng = np.random.default_rng(1)
    K = (rng.normal(size=(3, 3)) * 300).astype(np.float32)
    for _ in range(20):
        Rt = rng.normal(size=(3, 4)).astype(np.float32)
        assert np.array_equal(arvx.compose_projection(K, Rt), oracle.compose(K, Rt)[0])


def test_product_never_uses_the_oracle():
    bad = []
    for base in ("ar_voxel_project_amd", "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".h", ".hip", ".cpp", ".hpp", ".c")) or f == "Makefile":
                    txt = open(os.path.join(dp, f), errors="replace").read()
                    if re.search(r"pyoracle|arvx_oracle|from oracle|import oracle|oracle/", txt):
                        if not (f == "build.py"):  # build_oracle() only compiles the checker
                            bad.append(os.path.join(dp, f))
    assert not bad, f"product files reference the oracle: {bad}"


def test_fails_loudly_without_gpu(arvx):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(arvx.ArvxError) as ei:
        arvx.Context(8, 8, 8, 0.1)
    assert ei.value.code == 2  # ARVX_ERR_HIP: no silent CPU path


def test_argument_validation_needs_no_gpu(arvx):
    lib = arvx.load_library()
    assert lib.arvx_ctx_destroy(None) == 0
    assert lib.arvx_carve(None, 0) == 1  # ARVX_ERR_INVALID
    assert b"null" in lib.arvx_last_error()
    n = ctypes.c_int64()
    assert lib.arvx_ctx_voxels(None, ctypes.byref(n)) == 1
