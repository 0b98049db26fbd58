"""arvx::segmentViews (include/arvx/segmentation.hpp) through tests/cpp/test_segment_host, and
tools/cpp/arvx_cli -segment, against the restatement of the definition (tests/segment.py) and the same
pipeline given the masks."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import segment as S
from tests.test_cli_gpu import CLI, YML, write_inputs
from tests.test_cpp_host import write_scene

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def sphere():
    from ar_voxel_project_amd.synthetic import textured_sphere_scene
    return textured_sphere_scene(64, 5)  # 640 x 480, the data set's intrinsics; texture in [28, 228] on black


@pytest.mark.parametrize("rule,a,b,clean", [(0, 0, 20, (0, 0, 0, 0, 0)), (1, 20, 0, (0, 0, 0, 0, 0)),
                                            (1, 20, 0, (2, 3, 0, 0, 0))])
def test_cpp_segment_views_then_carve(arvx, sphere, tmp_path, rule, a, b, clean):
    from ar_voxel_project_amd import build
    exe = build.build_segment_host_test()
    sc = sphere
    X, Y, Z = 40, 36, 20
    s = F32(0.512 / 40)
    d = str(tmp_path)
    scene, out = os.path.join(d, "scene.bin"), os.path.join(d, "out.bin")
    # (the scene's own masks are zeroed: the run cannot have carved with them)
    write_scene(scene, X, Y, Z, s, sc.K, sc.Rt, np.zeros_like(sc.masks), sc.images, np.ones(X * Y * Z, np.uint8))
    r = subprocess.run([exe, scene, out, str(rule), str(a), str(b)] + [str(c) for c in clean], capture_output=True,
                       text=True, cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    p = S.params(open_radius=clean[0], close_radius=clean[1], min_area=clean[2], largest=bool(clean[3]),
                 max_hole=clean[4])
    if rule == 0:
        p.update(rule=S.RANGE, lo=(a,) * 3, hi=(b,) * 3)
        plates = None
    else:
        p.update(rule=S.PLATE, threshold=a)
        plates = np.full((sc.H, sc.W, 3), b, np.uint8)
    masks, counts = S.segment(sc.images, p, plates)
    if not any(clean):
        assert np.array_equal(masks != 0, sc.masks != 0)
    M = np.stack([arvx.compose_projection(sc.K, rt) for rt in sc.Rt])
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.set_views(M, masks)
        ctx.carve()
        want = ctx.download_state()
    raw = np.fromfile(out, np.uint8)
    n = masks.size
    assert len(raw) == n + 64 * sc.V + X * Y * Z
    assert raw[:n].tobytes() == masks.tobytes()
    assert np.array_equal(raw[n:n + 64 * sc.V].view(np.int64).reshape(sc.V, 8), counts)
    assert raw[n + 64 * sc.V:].tobytes() == want.tobytes() and 0 < (want & 1).sum() < want.size


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from ar_voxel_project_amd import build
        build.build_host_tests()
    return CLI


def read_pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n255\n", raw)
    W, H = int(m.group(1)), int(m.group(2))
    return np.frombuffer(raw[m.end():], np.uint8).reshape(H, W)


def test_cli_segment(cli, sphere, tmp_path):
    """arvx_cli -segment=plate on the scene's images, without -masks, writes the OFF the run with -masks
    writes; -segment=range with cleaning flags and -writeMasks writes the restatement's masks and logs its
    counts."""
    sc = sphere
    X, Y, Z = 40, 36, 20
    s = F32(0.512 / 40)
    d = str(tmp_path)
    write_inputs(d, sc)
    os.makedirs(os.path.join(d, "plates"))
    with open(os.path.join(d, "plates", "plate.ppm"), "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (sc.W, sc.H) + bytes(sc.W * sc.H * 3))
    common = [cli, "-c=5", f"-images={d}/images", f"-poses={d}/poses.txt", f"-calibration={YML}", f"-x={X}",
              f"-y={Y}", f"-z={Z}", f"-size={float(s)!r}", "-carve=1", "-color=2"]
    runs = {"masks": [f"-masks={d}/masks"],
            "plate": ["-segment=plate", f"-plates={d}/plates", "-segThreshold=20", f"-writeMasks={d}/plate_masks"],
            "range": ["-segment=range", "-segLo=0,0,0", "-segHi=100,100,100", "-segOpen=2", "-segClose=3",
                      "-segMinArea=5", "-segLargest=true", f"-writeMasks={d}/range_masks"]}
    outs = {}
    for name, flags in runs.items():
        r = subprocess.run(common + flags + [f"-outFile={d}/{name}.off"], capture_output=True, text=True, cwd=d)
        assert r.returncode == 0, r.stderr + r.stdout
        outs[name] = r.stdout
    off = open(os.path.join(d, "masks.off"), "rb").read()
    assert len(off) > 1000 and open(os.path.join(d, "plate.off"), "rb").read() == off
    for v in range(sc.V):
        assert np.array_equal(read_pgm(os.path.join(d, "plate_masks", f"mask{v:04d}.pgm")) != 0, sc.masks[v] != 0)
    p = S.params(lo=(0, 0, 0), hi=(100, 100, 100), open_radius=2, close_radius=3, min_area=5, largest=True)
    masks, counts = S.segment(sc.images, p)
    lines = re.findall(r"LOG - SEG: view (\d+) foreground (\d+) cleaned (\d+) specks (\d+) holes (\d+) "
                       r"\(specks removed (\d+), (\d+) px; holes filled (\d+), (\d+) px\)", outs["range"])
    assert len(lines) == sc.V
    for v in range(sc.V):
        assert np.array_equal(read_pgm(os.path.join(d, "range_masks", f"mask{v:04d}.pgm")), masks[v])
        assert [int(t) for t in lines[v]] == [v] + list(counts[v])
    # (pixels of the texture darker than 100 are background here: the opening and the closing have work to do)
    assert (counts[:, 0] != counts[:, 1]).all()
    assert "LOG - SEG" not in outs["masks"] and "LOG - SEG: masks segmented." in outs["plate"]
    # refusals of the flags' own
    bad = subprocess.run(common + ["-segment=hsv"], capture_output=True, text=True, cwd=d)
    assert bad.returncode == 1 and "segment" in bad.stderr
    bad = subprocess.run(common + ["-segment=plate"], capture_output=True, text=True, cwd=d)
    assert bad.returncode == 1 and "--plates" in bad.stderr
    bad = subprocess.run(common, capture_output=True, text=True, cwd=d)
    assert bad.returncode == 1 and "--masks" in bad.stderr  # (without -segment the masks are still required)
