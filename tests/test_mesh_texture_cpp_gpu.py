"""arvx::textureMesh and arvx::writeOBJ (include/arvx/marching_cubes.hpp, include/arvx/mesh_texture.hpp)
through tests/cpp/test_mesh_texture_host and tools/cpp/arvx_cli -texture against Context.mesh_texture of
the same pipeline: the atlas, the views, the UVs and the renders drawn with them, byte for byte; the
three files of the textured mesh parsed back.  The layout and the writer alone run without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import scenes
from tests.conftest import ROOT
from tests.test_cli_gpu import CLI, YML, write_inputs
from tests.test_cpp_host import write_scene

F32 = np.float32
W, H = 160, 120


def test_layout_and_writer_on_the_host(tmp_path):
    """The host-only build of the test program: no library, no device."""
    exe = os.path.join(str(tmp_path), "tex_layout")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
           "-DARVX_MESH_TEXTURE_HOST_ONLY", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_mesh_texture_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "layout", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "layout ok\n", r.stderr + r.stdout


def read_obj(path):
    """-> (v (nv, 3) float32, vt (nvt, 2) float32, f (nt, 3, 2) int64 1-based, mtllib)."""
    v, vt, f, lib = [], [], [], None
    for line in open(path):
        tag, *rest = line.split()
        if tag == "v":
            v.append([float(x) for x in rest])
        elif tag == "vt":
            vt.append([float(x) for x in rest])
        elif tag == "f":
            f.append([[int(k) for k in corner.split("/")] for corner in rest])
        elif tag == "mtllib":
            lib = rest[0]
    return np.array(v, F32).reshape(-1, 3), np.array(vt, F32).reshape(-1, 2), np.array(f, np.int64).reshape(-1, 3, 2), lib


def check_files(obj, verts, faces, atlas, uv):
    """The OBJ at `obj` with its .mtl and .ppm against a mesh and a texture."""
    v, vt, f, lib = read_obj(obj)
    stem = os.path.splitext(obj)[0]
    T = len(faces)
    assert lib == os.path.basename(stem) + ".mtl" and (len(v), len(vt), len(f)) == (len(verts), 3 * T, T)
    assert np.array_equal(v, np.asarray(verts, F32))
    assert np.array_equal(f[:, :, 0], np.asarray(faces)[:, :3].astype(np.int64) + 1)
    assert np.array_equal(f[:, :, 1], 1 + np.arange(3 * T).reshape(T, 3))
    flat = uv.reshape(-1, 2)
    assert np.array_equal(vt[:, 0], flat[:, 0]) and np.array_equal(vt[:, 1], (F32(1) - flat[:, 1]).astype(F32))
    assert "map_Kd " + os.path.basename(stem) + ".ppm" in open(stem + ".mtl").read()
    AH, AW = atlas.shape[:2]
    assert open(stem + ".ppm", "rb").read() == b"P6\n%d %d\n255\n" % (AW, AH) + np.ascontiguousarray(atlas[:, :, ::-1]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("R,AW,flags", [(3, 512, 0), (1, 130, 1)])
def test_cpp_texture_mesh_equals_the_c_abi(arvx, tmp_path, R, AW, flags):
    from ar_voxel_project_amd import build
    exe = build.build_mesh_texture_host_test()
    X, Y, Z, B, view = 40, 36, 20, 4, 3
    s = F32(0.512 / 40)
    sc = scenes.syn.sphere_scene(64, 5, W=W, H=H, with_images=True)
    d = str(tmp_path)
    scene, out, obj = os.path.join(d, "scene.bin"), os.path.join(d, "texture.bin"), os.path.join(d, "mesh.obj")
    write_scene(scene, X, Y, Z, s, sc.K, sc.Rt, sc.masks, sc.images, np.ones(X * Y * Z, np.uint8))
    r = subprocess.run([exe, scene, out, obj, str(B), str(view), str(R), str(AW), "1.5", str(flags)], capture_output=True,
                       text=True, cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    M = np.stack([arvx.compose_projection(sc.K, rt) for rt in sc.Rt])
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.set_views(M, sc.masks)
        ctx.set_images(sc.images)
        ctx.carve()
        verts, faces, _ = ctx.mc_mesh_refined(B)
        atlas, fview, uv, counts = ctx.mesh_texture(arvx.MESH_REFINED, R, AW, float(F32(1.5) * s), flags)
        want = ctx.render_mesh(arvx.MESH_REFINED | arvx.MESH_TEXTURED, M[view], W, H,
                               background=sc.images[view], light=arvx.headlight(M[view]))
    T = len(faces)
    assert T > 1000 and 0 < counts[1] < T and counts[0] == T and atlas.any()
    raw = np.fromfile(out, np.uint8)
    npix = W * H
    assert len(raw) == 32 + atlas.size + 28 * T + 11 * npix
    assert tuple(raw[:32].view(np.int64)) == counts
    o = 32
    for a in (atlas, fview, uv):
        assert raw[o:o + a.nbytes].tobytes() == a.tobytes()
        o += a.nbytes
    img = raw[o:]
    got = (img[:3 * npix], img[3 * npix:7 * npix], img[7 * npix:])
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert (want[2] >= 0).any() and (want[2] < 0).any()
    # (WriteMesh's scaling: an fp32 product per coordinate)
    check_files(obj, (verts * s).astype(F32), faces, atlas, uv)


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from ar_voxel_project_amd import build
        build.build_host_tests()
    return CLI


def read_off(path):
    tok = open(path).read().split()
    assert tok[0] == "OFF"
    nv, nt = int(tok[1]), int(tok[2])
    v = np.array(tok[4:4 + 3 * nv], np.float64).astype(F32).reshape(nv, 3)
    f = np.array(tok[4 + 3 * nv:], np.int64).reshape(nt, 7)
    return v, f[:, 1:4]


@pytest.mark.gpu
def test_cli_texture(cli, arvx, tmp_path):
    """arvx_cli -refine=4 -texture=4 -atlasWidth=700 -render=DIR -renderMesh=true: mesh.obj / .mtl / .ppm
    beside mesh.off hold the OFF file's mesh and the Python layer's texture (tolerance: the default
    -visibleTol of 3 voxel edges), and every render%04d.ppm is the Python layer's textured render with a
    headlight over the input image."""
    X, Y, Z = 40, 36, 20
    s = F32(0.512 / 40)
    sc = scenes.syn.sphere_scene(64, 5, with_images=True)
    d = str(tmp_path)
    write_inputs(d, sc)
    cmd = [cli, "-c=5", f"-images={d}/images", f"-masks={d}/masks", f"-poses={d}/poses.txt",
           f"-calibration={YML}", f"-x={X}", f"-y={Y}", f"-z={Z}", f"-size={float(s)!r}",
           "-carve=1", "-color=0", "-postprocessing=false", "-refine=4", f"-render={d}/renders",
           "-renderMesh=true", "-texture=4", "-atlasWidth=700", f"-outFile={d}/mesh.off"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    Hc, Wc = sc.masks[0].shape
    M = np.stack([arvx.compose_projection(sc.K, rt) for rt in sc.Rt])
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.set_views(M, sc.masks)
        ctx.set_images(sc.images)
        ctx.carve()
        verts, faces, _ = ctx.mc_mesh_refined(4)
        atlas, fview, uv, counts = ctx.mesh_texture(arvx.MESH_REFINED, 4, 700, float(F32(3) * s))
        line = re.search(r"LOG - MESH TEXTURE: (\d+) of (\d+) faces textured from the images, atlas (\d+) x (\d+)", r.stdout)
        assert line and tuple(int(g) for g in line.groups()) == (counts[1], counts[0], counts[2], counts[3])
        assert 0 < counts[1] < counts[0] == len(faces)
        off_v, off_f = read_off(os.path.join(d, "mesh.off"))
        assert np.array_equal(off_f, faces[:, :3])
        check_files(os.path.join(d, "mesh.obj"), off_v, off_f, atlas, uv)
        plain = 0
        for v in range(sc.V):
            bgr, _, ids = ctx.render_mesh(arvx.MESH_REFINED | arvx.MESH_TEXTURED, M[v], Wc, Hc,
                                          background=sc.images[v], light=arvx.headlight(M[v]))
            assert (ids >= 0).any()
            ppm = b"P6\n%d %d\n255\n" % (Wc, Hc) + np.ascontiguousarray(bgr[:, :, ::-1]).tobytes()
            assert open(os.path.join(d, "renders", f"render{v:04d}.ppm"), "rb").read() == ppm
            own = ctx.render_mesh(arvx.MESH_REFINED, M[v], Wc, Hc, background=sc.images[v],
                                  light=arvx.headlight(M[v]))[0]
            plain += int(not np.array_equal(own, bgr))
        assert plain == sc.V  # (the texture is not the mesh's own colours)
    # refusals of the flag's own: no mesh with shared vertices, -meshColor as well, a resolution out of range
    bad = subprocess.run([c for c in cmd if c != "-refine=4"], capture_output=True, text=True, cwd=d)
    assert bad.returncode == 1 and "-texture" in bad.stderr
    bad = subprocess.run(cmd + ["-meshColor=average"], capture_output=True, text=True, cwd=d)
    assert bad.returncode == 1 and "-meshColor" in bad.stderr
    bad = subprocess.run([c.replace("-texture=4", "-texture=254") for c in cmd], capture_output=True, text=True, cwd=d)
    assert bad.returncode == 3
