"""arvx::colorMesh (include/arvx/marching_cubes.hpp) through tests/cpp/test_mesh_color_host and
tools/cpp/arvx_cli -meshColor against Context.mesh_color of the same pipeline: the colours, the view
counts and the renders drawn with them, byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import scenes
from tests.test_cli_gpu import CLI, YML, write_inputs
from tests.test_cpp_host import write_scene

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = 160, 120


@pytest.mark.parametrize("mode,flags", [(1, 0), (0, 1)])
def test_cpp_color_mesh_equals_the_c_abi(arvx, tmp_path, mode, flags):
    from ar_voxel_project_amd import build
    exe = build.build_mesh_color_host_test()
    X, Y, Z, B, view = 40, 36, 20, 4, 3
    s = F32(0.512 / 40)
    sc = scenes.syn.sphere_scene(64, 5, W=W, H=H, with_images=True)
    d = str(tmp_path)
    scene, out = os.path.join(d, "scene.bin"), os.path.join(d, "colours.bin")
    write_scene(scene, X, Y, Z, s, sc.K, sc.Rt, sc.masks, sc.images, np.ones(X * Y * Z, np.uint8))
    r = subprocess.run([exe, scene, out, str(B), str(view), str(mode), "1.5", str(flags)], capture_output=True,
                       text=True, cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    M = np.stack([arvx.compose_projection(sc.K, rt) for rt in sc.Rt])
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.set_views(M, sc.masks)
        ctx.set_images(sc.images)
        ctx.carve()
        verts, faces, _, vrgb = ctx.mc_mesh_refined(B, vertex_colors=True)
        rgb, views, coloured = ctx.mesh_color(arvx.MESH_REFINED, mode, float(F32(1.5) * s), flags)
        want = ctx.render_mesh(arvx.MESH_REFINED | arvx.MESH_IMAGE_COLORS, M[view], W, H,
                               background=sc.images[view], light=arvx.headlight(M[view]))
    Vn = len(verts)
    assert Vn > 500 and 0 < coloured and (views == 0).any() and (rgb[views > 0] != vrgb[views > 0]).any()
    raw = np.fromfile(out, np.uint8)
    npix = W * H
    assert len(raw) == 16 + 16 * Vn + 11 * npix
    assert tuple(raw[:16].view(np.int64)) == (Vn, coloured)
    assert raw[16:16 + 12 * Vn].tobytes() == rgb.tobytes()
    assert raw[16 + 12 * Vn:16 + 16 * Vn].tobytes() == views.tobytes()
    img = raw[16 + 16 * Vn:]
    got = (img[:3 * npix], img[3 * npix:7 * npix], img[7 * npix:])
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert (want[2] >= 0).any() and (want[2] < 0).any()


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from ar_voxel_project_amd import build
        build.build_host_tests()
    return CLI


def test_cli_mesh_color(cli, arvx, tmp_path):
    """arvx_cli -refine=4 -render=DIR -renderMesh=true -meshColor=average: every render%04d.ppm is the
    Python layer's render of the refined mesh with its image colours (tolerance: the default
    -visibleTol of 3 voxel edges) and a headlight over the input image."""
    X, Y, Z = 40, 36, 20
    s = F32(0.512 / 40)
    sc = scenes.syn.sphere_scene(64, 5, with_images=True)
    d = str(tmp_path)
    write_inputs(d, sc)
    cmd = [cli, "-c=5", f"-images={d}/images", f"-masks={d}/masks", f"-poses={d}/poses.txt",
           f"-calibration={YML}", f"-x={X}", f"-y={Y}", f"-z={Z}", f"-size={float(s)!r}",
           "-carve=1", "-color=0", "-postprocessing=false", "-refine=4", f"-render={d}/renders",
           "-renderMesh=true", "-meshColor=average", f"-outFile={d}/mesh.off"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    Hc, Wc = sc.masks[0].shape
    M = np.stack([arvx.compose_projection(sc.K, rt) for rt in sc.Rt])
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.set_views(M, sc.masks)
        ctx.set_images(sc.images)
        ctx.carve()
        assert ((ctx.download_state() & 2) != 0).all()  # (handleUnseen has nothing to paint)
        verts, _, _ = ctx.mc_mesh_refined(4)
        rgb, views, coloured = ctx.mesh_color(arvx.MESH_REFINED, arvx.COLOR_AVERAGE, float(F32(3) * s))
        line = re.search(r"LOG - MESH COLOR: (\d+) of (\d+) vertices", r.stdout)
        assert line and (int(line.group(1)), int(line.group(2))) == (coloured, len(verts)) and coloured > 0
        plain = 0
        for v in range(sc.V):
            bgr, _, ids = ctx.render_mesh(arvx.MESH_REFINED | arvx.MESH_IMAGE_COLORS, M[v], Wc, Hc,
                                          background=sc.images[v], light=arvx.headlight(M[v]))
            assert (ids >= 0).any()
            ppm = b"P6\n%d %d\n255\n" % (Wc, Hc) + np.ascontiguousarray(bgr[:, :, ::-1]).tobytes()
            assert open(os.path.join(d, "renders", f"render{v:04d}.ppm"), "rb").read() == ppm
            own = ctx.render_mesh(arvx.MESH_REFINED, M[v], Wc, Hc, background=sc.images[v],
                                  light=arvx.headlight(M[v]))[0]
            plain += int(not np.array_equal(own, bgr))
        assert plain == sc.V  # (the image colours are not the mesh's own)
    assert len(re.findall(r"LOG - RENDER MESH: view \d+ both", r.stdout)) == sc.V
    # refusals of the flag's own: a wrong value, and no -renderMesh
    bad = subprocess.run([c.replace("=average", "=nearest") for c in cmd], capture_output=True, text=True, cwd=d)
    assert bad.returncode == 1 and "-meshColor" in bad.stderr
    bad = subprocess.run([c for c in cmd if c != "-renderMesh=true"], capture_output=True, text=True, cwd=d)
    assert bad.returncode == 1 and "-renderMesh=true" in bad.stderr
