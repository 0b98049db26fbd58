#!/usr/bin/env python3
"""Records what the reference program itself computes on the cases of tests/ref_program.py:
runs oracle/_ref/arvx_ref (the reference's own sources over functional stand-ins, built by
`make -C oracle` where the reference checkout is at hand) and writes, per case A, B, D, E, T, F3,
F5, tests/golden/ref_<case>.npz with the inputs (K, the pose the binary derived, masks, images,
the loaded model) and the model after every op, plus the OFF files marching cubes wrote.  Data
the reference's program wrote -- no source.  The GPU tests (tests/test_reference_gpu.py) read
these files only; tests/test_reference_cpu.py regenerates each and fails on a stale one.

    python tools/make_ref_fixtures.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import ref_program as rp  # noqa: E402

LIMIT = 220 * 1024  # today's largest single-scene fixture (noise24.npz)


def main():
    if not os.path.exists(rp.REF_BIN):
        sys.exit(f"{rp.REF_BIN} missing: run `make -C oracle` next to the reference checkout")
    for name, make in rp.FIXTURE_CASES.items():
        path = rp.fixture_path(name)
        np.savez_compressed(path, **rp.record(make()))
        size = os.path.getsize(path)
        print(f"{os.path.relpath(path, ROOT)}: {size} bytes")
        if size > LIMIT:
            sys.exit(f"{path} is larger than {LIMIT} bytes")


if __name__ == "__main__":
    main()
