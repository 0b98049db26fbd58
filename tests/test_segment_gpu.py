"""arvx_segment_views on the device against the restatement of its definition (tests/segment.py), bit
for bit: the final masks, the eight counts, and the views' tables against those of a context given
the restatement's masks through set_views.

Shapes: 70 x 37 (rows straddle words of the flat plane, two words per work row), 33 x 5 (less than a
word), 64 x 64 (whole words), 130 x 3 (three words, the last nearly empty) and 1 x 1, with one view and
with five.  Radii 0, 1, 2 (one launch per pass), 9, 12, 16 (doubled windows) and max(W, H) and more."""
import ctypes as C

import numpy as np
import pytest

from tests import scenes
from tests import segment as S

pytestmark = pytest.mark.gpu
E = 0.512
SHAPES = [(70, 37), (33, 5), (64, 64), (130, 3), (1, 1)]


@pytest.fixture(scope="module")
def pair(arvx):
    """(the context under test, the context that is given the restatement's masks)"""
    with arvx.Context(16, 16, 16, E / 16) as ctx, arvx.Context(16, 16, 16, E / 16) as ref:
        yield ctx, ref


def cameras(V, W, H, seed=0):
    return scenes.random_cameras(V, E, seed=seed, W=W, H=H)[2]


def check(pair, images, p, plates=None, what="", device=False, M=None):
    ctx, ref = pair
    images = np.ascontiguousarray(images)
    V, H, W, _ = images.shape
    M = cameras(V, W, H) if M is None else M
    want, want_counts = S.segment(images, p, plates)
    if device:
        import torch
        # one byte into a fresh allocation: the views start at every alignment
        buf = torch.zeros(images.size + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.from_numpy(images.reshape(-1))
        pbuf, n_plates = None, 0
        if plates is not None:
            pl = np.ascontiguousarray(plates).reshape(-1, H, W, 3)
            n_plates = len(pl)
            pbuf = torch.zeros(pl.size + 3, dtype=torch.uint8, device="cuda")
            pbuf[3:] = torch.from_numpy(pl.reshape(-1))
        torch.cuda.synchronize()
        ctx.segment_views_device(M, buf.data_ptr() + 1, W, H, dev_plates_ptr=pbuf.data_ptr() + 3 if n_plates else 0,
                                 plate_count=n_plates, **p)
        ctx._lib.arvx_ctx_synchronize(ctx._h)
    else:
        ctx.segment_views(M, images, plates=plates, **p)
    ref.set_views(M, want)
    for v in range(V):
        got = ctx.segment_mask(v)
        assert np.array_equal(got, want[v]), f"{what}: mask of view {v}: {np.argwhere(got != want[v])[:5]}"
        assert list(ctx.segment_counts(v)) == list(want_counts[v]), f"{what}: counts of view {v}"
        bg, table = ctx.selftest_view_tables(v, W, H)
        rbg, rtable = ref.selftest_view_tables(v, W, H)
        assert np.array_equal(bg, want[v] == 0) and np.array_equal(bg, rbg), f"{what}: bit plane of view {v}"
        assert np.array_equal(table, rtable), f"{what}: table of view {v}"
    return want


def cleaning_configs(W, H):
    big = max(W, H)
    return [dict(), dict(open_radius=1), dict(open_radius=2), dict(open_radius=big), dict(close_radius=1),
            dict(close_radius=2), dict(close_radius=big + 3), dict(min_area=3), dict(largest=True),
            dict(min_area=3, largest=True), dict(max_hole=2), dict(max_hole=-1),
            dict(open_radius=1, close_radius=1, min_area=3, max_hole=2),
            dict(open_radius=1, close_radius=2, min_area=3, largest=True, max_hole=-1)]


@pytest.mark.parametrize("V", [1, 5])
@pytest.mark.parametrize("W,H", SHAPES)
def test_noise_under_every_step(pair, W, H, V):
    for d, density in enumerate((0.3, 0.55)):
        masks = S.noise_masks(V, H, W, density, seed=7 * W + H + d)
        images = S.image_of(masks)
        for k, kw in enumerate(cleaning_configs(W, H)):
            for r in (S.RANGE, S.PLATE):
                per_view = (k + d) % 3 == 0 and V > 1
                plates = S.plate_of(H, W, V if per_view else 1) if r == S.PLATE else None
                p = S.params(rule=r, threshold=20, **kw)
                check(pair, images, p, plates, f"{W}x{H} V={V} density {density} {kw} rule {r}")


@pytest.mark.parametrize("W,H", [(70, 37), (130, 3), (64, 64)])
def test_large_radii_double_their_windows(pair, W, H):
    masks = S.blocks_masks(2, H, W, seed=W)
    images = S.image_of(masks)
    for r in (9, 12, 16):
        w1 = check(pair, images, S.params(open_radius=r), None, f"open {r}")
        w2 = check(pair, images, S.params(close_radius=r), None, f"close {r}")
        check(pair, images, S.params(open_radius=r, close_radius=r + 1, min_area=4, max_hole=-1), None, f"both {r}")
        if (W, H, r) == (70, 37, 9):  # (the case is not a trivial one: neither all nor nothing, and not the input)
            for w in (w1, w2):
                assert 0 < (w != 0).sum() < w.size and not np.array_equal(w != 0, masks)


def test_rule_edges(pair):
    W, H, V = 70, 37, 2
    rng = np.random.default_rng(3)
    edge = rng.choice(np.array([0, 119, 120, 121, 254, 255], np.uint8), (V, H, W, 3))
    check(pair, edge, S.params(), None, "the reference's range on its edges")
    check(pair, edge, S.params(lo=(119, 120, 121), hi=(120, 254, 255)), None, "a range per channel")
    check(pair, edge, S.params(lo=(0, 0, 0), hi=(255, 255, 255)), None, "everything is background")
    check(pair, edge, S.params(lo=(255, 255, 255), hi=(255, 255, 255)), None, "a single value")
    any_byte, plate = S.noise_images(V, H, W, seed=4), S.noise_images(V, H, W, seed=5)
    plate[0, :, :35] = any_byte[0, :, :35]  # (differences of exactly 0)
    plate[1, :5], any_byte[1, :5] = 0, 255  # (and of exactly 255)
    for t in (0, 1, 119, 120, 254, 255):
        check(pair, any_byte, S.params(rule=S.PLATE, threshold=t), plate, f"threshold {t}, a plate per view")
        check(pair, any_byte, S.params(rule=S.PLATE, threshold=t), plate[1], f"threshold {t}, one plate")


@pytest.mark.parametrize("name", sorted(S.HAND_SCENES))
def test_hand_built_scenes(pair, name):
    build, kw = S.HAND_SCENES[name]
    m = build()
    # the scene beside its mirror images: the labels' order differs in each
    for views in ([m], [m, m[::-1], m[:, ::-1], m[::-1, ::-1], m]):
        check(pair, S.image_of(np.stack(views)), S.params(**kw), None, name)
        check(pair, S.image_of(np.stack(views)), S.params(rule=S.PLATE, threshold=100, **kw),
              S.plate_of(*m.shape), name + " plate")


def test_batches_never_change_the_result(pair):
    ctx, _ = pair
    W, H, V = 70, 37, 5
    images = S.image_of(S.noise_masks(V, H, W, 0.5, seed=11))
    p = S.params(open_radius=1, close_radius=1, min_area=3, largest=True, max_hole=-1)
    whole = check(pair, images, p, None, "one batch")
    try:
        for n in (2, 1, 4, 7):  # (2: batches of 2, 2 and 1 views)
            ctx.selftest_segment_batch(n)
            assert np.array_equal(check(pair, images, p, None, f"batches of {n}"), whole)
    finally:
        ctx.selftest_segment_batch(0)


@pytest.mark.parametrize("W,H", [(70, 37), (33, 5), (64, 64), (1, 1)])
def test_device_form(pair, W, H):
    V = 3
    images = S.image_of(S.noise_masks(V, H, W, 0.5, seed=W))
    p = dict(open_radius=1, close_radius=1, min_area=3, max_hole=-1)
    check(pair, images, S.params(**p), None, "device, range", device=True)
    check(pair, images, S.params(rule=S.PLATE, threshold=20, **p), S.plate_of(H, W, 1), "device, one plate", device=True)
    check(pair, images, S.params(rule=S.PLATE, threshold=20, **p), S.plate_of(H, W, V), "device, V plates", device=True)


# ---- end to end ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sphere():
    from ar_voxel_project_amd.synthetic import textured_sphere_scene
    return textured_sphere_scene(32, 8, W=128, H=96)


DARK = dict(lo=(0, 0, 0), hi=(20, 20, 20))  # the sphere's photographs: texture in [28, 228] on black


def carved(ctx):
    ctx.reset()
    ctx.carve()
    return ctx.download_state()


def test_segment_then_carve_and_color(arvx, sphere):
    sc = sphere
    with arvx.Context(sc.X, sc.Y, sc.Z, sc.voxel_size) as ctx, arvx.Context(sc.X, sc.Y, sc.Z, sc.voxel_size) as ref:
        ref.set_views(sc.M, sc.masks, sc.campos)
        want = carved(ref)
        ref.set_images(sc.images)
        ref.color(arvx.COLOR_AVERAGE)
        want_idx, want_rgb = ref.surface()
        for plates, p in ((None, S.params(**DARK)),
                          (np.zeros((sc.H, sc.W, 3), np.uint8), S.params(rule=S.PLATE, threshold=20))):
            ctx.segment_views(sc.M, sc.images, sc.campos, plates=plates, **p)
            assert np.array_equal(carved(ctx), want) and 0 < (want & 1).sum() < want.size
            ctx.color(arvx.COLOR_AVERAGE)  # (the images are resident from the one call)
            idx, rgb = ctx.surface()
            assert len(idx) and np.array_equal(idx, want_idx) and np.array_equal(rgb, want_rgb)
            # a second derivation drops the colours as set_views does
            ctx.segment_views(sc.M, sc.images, sc.campos, plates=plates, **p)
            with pytest.raises(arvx.ArvxError) as ei:
                ctx.surface()
            assert ei.value.code == 3
            ref.set_views(sc.M, sc.masks, sc.campos)
            with pytest.raises(arvx.ArvxError) as ei:
                ref.surface()
            assert ei.value.code == 3
            ref.set_images(sc.images)
            ref.color(arvx.COLOR_AVERAGE)


def test_cleaning_repairs_a_speck_and_a_hole(arvx, sphere):
    sc = sphere
    clean = np.where(sc.masks != 0, 255, 0).astype(np.uint8)
    images = sc.images.copy()
    cy, cx = np.argwhere(clean[2]).mean(axis=0).astype(int)
    assert clean[1, 2:5, 2:5].max() == 0 and clean[2, cy - 1:cy + 2, cx - 1:cx + 2].min() == 255
    images[1, 2:5, 2:5] = 100                      # a 3 x 3 speck in a corner of view 1
    images[2, cy - 1:cy + 2, cx - 1:cx + 2] = 0    # a 3 x 3 hole in the middle of view 2's silhouette
    with arvx.Context(sc.X, sc.Y, sc.Z, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, clean, sc.campos)
        want = carved(ctx)
        ctx.segment_views(sc.M, images, sc.campos, **S.params(**DARK))
        assert ctx.segment_counts(1)[0] == (clean[1] != 0).sum() + 9
        assert ctx.segment_counts(2)[0] == (clean[2] != 0).sum() - 9
        assert not np.array_equal(carved(ctx), want)  # (the hole drills through the model)
        ctx.segment_views(sc.M, images, sc.campos, **S.params(min_area=10, max_hole=9, **DARK))
        for v in range(sc.V):
            assert np.array_equal(ctx.segment_mask(v), clean[v])
        assert list(ctx.segment_counts(1)[4:]) == [1, 9, 0, 0] and list(ctx.segment_counts(2)[4:]) == [0, 0, 1, 9]
        assert np.array_equal(carved(ctx), want)


# ---- refusals -----------------------------------------------------------------------------------

def test_refusals(arvx):
    W, H, V = 33, 5, 3
    images = S.image_of(S.noise_masks(V, H, W, 0.5, seed=1))
    plates = S.plate_of(H, W, V)
    M = np.ascontiguousarray(cameras(V, W, H), np.float32).reshape(-1, 12)
    ptrs = (C.c_void_p * V)(*[images[i].ctypes.data for i in range(V)])
    pptrs = (C.c_void_p * V)(*[plates[i].ctypes.data for i in range(V)])
    fp = M.ctypes.data_as(C.POINTER(C.c_float))

    def sp(**kw):
        d = dict(S.DEFAULTS)
        d.update(kw)
        return arvx.Context._segment_params(**d)

    with arvx.Context(16, 16, 16, E / 16) as ctx:
        lib, h = ctx._lib, ctx._h

        def host(V=V, M=fp, images=ptrs, W=W, H=H, stride=W * 3, plates=None, plate_count=0, params=sp()):
            return lib.arvx_segment_views(h, V, M, None, images, W, H, stride, plates, plate_count,
                                          C.byref(params) if params is not None else None)

        def refused(rc, code=1):
            assert rc == code, (rc, lib.arvx_last_error())
            # ... and nothing changed: the views of the good call below are still there
            assert list(ctx.segment_counts(0)) == list(good_counts)

        with pytest.raises(arvx.ArvxError) as ei:  # before the first call
            ctx.segment_counts(0)
        assert ei.value.code == 3
        with pytest.raises(arvx.ArvxError) as ei:
            ctx.segment_mask(0)
        assert ei.value.code == 3
        assert host() == 0
        good_counts = ctx.segment_counts(0)
        refused(host(images=None))
        refused(host(M=None))
        refused(host(params=None))
        refused(host(images=(C.c_void_p * V)(ptrs[0], None, ptrs[2])))
        refused(host(params=sp(rule=S.PLATE)))  # no plates
        refused(host(params=sp(rule=S.PLATE), plates=(C.c_void_p * V)(pptrs[0], None, pptrs[2]), plate_count=V))
        for bad_v in (0, -1, 4097):
            refused(host(V=bad_v))
        for bad in (0, -3, 16385):
            refused(host(W=bad))
            refused(host(H=bad))
        refused(host(stride=W * 3 - 1))
        refused(host(params=sp(rule=2)))
        refused(host(params=sp(rule=-1)))
        refused(host(params=sp(lo=(0, 121, 0), hi=(255, 120, 255))))
        for t in (-1, 256):
            refused(host(params=sp(rule=S.PLATE, threshold=t), plates=pptrs, plate_count=V))
            refused(host(params=sp(threshold=t)))
        refused(host(params=sp(open_radius=-1)))
        refused(host(params=sp(close_radius=-1)))
        refused(host(params=sp(min_area=-1)))
        for n in (0, 2, V + 1):
            refused(host(params=sp(rule=S.PLATE), plates=pptrs, plate_count=n))
        flagged = sp()
        flagged.flags = 2
        refused(host(params=flagged))
        # the device form refuses the same (nothing is read through a pointer before)
        dev = lambda **kw: lib.arvx_segment_views_device(  # noqa: E731
            h, kw.get("V", V), fp, None, kw.get("images", C.c_void_p(256)), kw.get("W", W), H, kw.get("plates"),
            kw.get("plate_count", 0), C.byref(kw.get("params", sp())))
        refused(dev(images=None))
        refused(dev(V=0))
        refused(dev(W=16385))
        refused(dev(params=sp(rule=3)))
        refused(dev(params=sp(rule=S.PLATE)))
        refused(dev(params=sp(rule=S.PLATE), plates=C.c_void_p(256), plate_count=2))
        refused(dev(params=sp(open_radius=-2)))
        # the downloads: a view outside [0, V), a null pointer; then views of another origin
        assert lib.arvx_segment_download(h, V, images.ctypes.data) == 1
        assert lib.arvx_segment_download(h, -1, images.ctypes.data) == 1
        assert lib.arvx_segment_download(h, 0, None) == 1
        assert lib.arvx_segment_counts(h, 0, None) == 1
        assert lib.arvx_selftest_segment_batch(h, -1) == 1
        ctx.set_views(M, S.segment(images, S.params())[0])
        out = (C.c_int64 * 8)()
        assert lib.arvx_segment_counts(h, 0, out) == 3 and lib.arvx_segment_download(h, 0, images.ctypes.data) == 3
        assert host(params=sp(rule=S.PLATE), plates=pptrs, plate_count=V) == 0
        assert lib.arvx_segment_counts(h, 0, out) == 0
