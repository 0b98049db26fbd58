"""The restatement of arvx_segment_views' definition (tests/segment.py) and the reach of the scenes
the GPU tests replay, checked without a GPU."""
import numpy as np

from tests import segment as S


def test_random_cases_reach_every_decision():
    removed = kept_at_min = filled = left_border = left_size = 0
    for _, masks, p in S.random_cases():
        for m in masks:
            _, info = S.components(m, 8)
            removed += sum(a < p["min_area"] for a, _ in info.values())
            kept_at_min += sum(a == p["min_area"] for a, _ in info.values())
            m4, _, _ = S.specks(m, p["min_area"], p["largest"])
            _, binfo = S.components(~m4, 4)
            filled += sum(not b and a <= p["max_hole"] for a, b in binfo.values())
            left_border += sum(b and a <= p["max_hole"] for a, b in binfo.values())
            left_size += sum(not b and a > p["max_hole"] for a, b in binfo.values())
            out, c = S.segment_view(S.image_of(m), p)
            assert c[4] == sum(a < p["min_area"] for a, _ in info.values())
            assert c[6] == sum(not b and a <= p["max_hole"] for a, b in binfo.values())
            assert c[3] == out.sum() == c[2] + c[7] and c[2] == c[1] - c[5]
    assert min(removed, kept_at_min, filled, left_border, left_size) >= 1, (
        removed, kept_at_min, filled, left_border, left_size)


def test_largest_tie_has_two_largest_components():
    m = S.tie_scene()
    lab, info = S.components(m, 8)
    areas = sorted((a for a, _ in info.values()), reverse=True)
    assert areas[0] == areas[1] > areas[2]
    out, c = S.segment_view(S.image_of(m), S.params(largest=True))
    first = min(k for k, (a, _) in info.items() if a == areas[0])
    assert np.array_equal(out, lab == first)  # ties go to the smaller label
    assert list(c[4:6]) == [2, areas[1] + areas[2]]


def test_diagonal_gap_pocket_is_a_hole_under_4_only():
    m = S.diagonal_gap_scene()
    _, info4 = S.components(~m, 4)
    _, info8 = S.components(~m, 8)
    assert sorted(b for _, b in info4.values()) == [False, True]  # the pocket and the outside
    assert [b for _, b in info8.values()] == [True]               # one background through the gap
    out, c = S.segment_view(S.image_of(m), S.params(max_hole=-1))
    assert list(c[6:8]) == [1, 6] and out[2:4, 2:5].all()


def test_speck_removal_merges_background_before_the_holes():
    m = S.speck_merge_scene()
    p = S.params(**S.HAND_SCENES["speck_merge"][1])
    right, c = S.segment_view(S.image_of(m), p)
    wrong, _ = S.segment_view(S.image_of(m), p, holes_see_step4=False)
    assert not np.array_equal(right, wrong)
    assert list(c[4:8]) == [1, 1, 0, 0]  # the speck goes, and the 9-pixel hole it leaves is above max_hole
    assert wrong[2:5, 2:5].sum() == 8     # the 8-pixel ring of background around the speck would have been filled


def test_opening_is_anti_extensive_and_closing_extensive():
    for density in (0.3, 0.6):
        m = S.noise_masks(1, 37, 70, density, seed=5)[0]
        for r in (1, 2, 80):
            opened = S.dilate(S.erode(m, r), r)
            closed = S.erode(S.dilate(m, r), r)
            assert not (opened & ~m).any() and not (m & ~closed).any()
            assert np.array_equal(S.dilate(S.erode(opened, r), r), opened)  # idempotent
    # a radius of max(W, H) and more: the window is the image
    m = np.zeros((5, 9), bool)
    m[2, 3] = True
    assert S.dilate(m, 9).all() and not S.erode(~m, 9).any() and S.erode(np.ones((5, 9), bool), 9).all()


def test_hole_exactly_max_hole_against_one_more():
    a, ca = S.segment_view(S.image_of(S.hole_scene(6)), S.params(max_hole=6))
    b, cb = S.segment_view(S.image_of(S.hole_scene(7)), S.params(max_hole=6))
    assert list(ca[6:8]) == [1, 6] and list(cb[6:8]) == [0, 0]


def test_reference_rule_on_the_textured_sphere():
    from ar_voxel_project_amd.synthetic import textured_sphere_scene
    sc = textured_sphere_scene(32, 8, W=128, H=96)
    fg = sc.masks != 0
    # texture_rgb lies in [28, 228] on a black background: every foreground byte is above 20
    assert sc.images[fg].min() >= 28 and sc.images[fg].max() <= 228 and sc.images[~fg].max() == 0
    want = np.where(fg, 255, 0).astype(np.uint8)
    got, _ = S.segment(sc.images, S.params(rule=S.RANGE, lo=(0, 0, 0), hi=(20, 20, 20)))
    assert np.array_equal(got, want)
    got, _ = S.segment(sc.images, S.params(rule=S.PLATE, threshold=20), plates=np.zeros((96, 128, 3), np.uint8))
    assert np.array_equal(got, want)
    # the reference's own constants (src/Segmentation.h:10-11): background 120..255 in every channel
    img = np.array([[[119, 200, 200], [120, 120, 120], [255, 255, 255], [120, 255, 119]]], np.uint8)
    assert list(S.rule(img, S.params())[0]) == [True, False, False, True]
