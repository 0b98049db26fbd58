"""The definition of arvx_segment_views (include/arvx/arvx.h) restated in numpy and plain loops, and the
scenes the segmentation tests share.  Nothing here is taken from the kernels: windows are counted with
cumulative sums, components are flood-filled in flat index order (so the first pixel met is the label).
"""
import numpy as np

RANGE, PLATE = 0, 1

DEFAULTS = dict(rule=RANGE, lo=(120, 120, 120), hi=(255, 255, 255), threshold=0, open_radius=0,
                close_radius=0, min_area=0, largest=False, max_hole=0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---- the five steps ---------------------------------------------------------------------------

def rule(img, p, plate=None):
    """Step 1: (H, W) bool foreground of one BGR image."""
    if p["rule"] == RANGE:
        lo, hi = np.array(p["lo"]), np.array(p["hi"])
        return ~np.all((img >= lo) & (img <= hi), axis=-1)
    d = np.abs(img.astype(np.int64) - plate.astype(np.int64)).max(axis=-1)
    return d > p["threshold"]


def _window_count(m, r, axis):
    """Per pixel the number of set pixels within r along `axis` (outside the image: none)."""
    n = m.shape[axis]
    c = np.concatenate([np.zeros_like(np.take(m, [0], axis), np.int64), np.cumsum(m, axis=axis, dtype=np.int64)],
                       axis=axis)
    i = np.arange(n)
    hi = np.minimum(i + r + 1, n)
    lo = np.maximum(i - r, 0)
    return np.take(c, hi, axis) - np.take(c, lo, axis)


def dilate(m, r):
    """Box dilation: pixels outside the image are background."""
    for axis in (1, 0):
        m = _window_count(m, r, axis) > 0
    return m


def erode(m, r):
    """Box erosion: pixels outside the image are foreground."""
    return ~dilate(~m, r)


def components(m, conn):
    """The components of the set pixels of m under 4- or 8-connectivity.
    -> (labels (H, W) int64, -1 where m is clear; {label: (area, touches the border)})."""
    H, W = m.shape
    lab = np.full((H, W), -1, np.int64)
    info = {}
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if conn == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    for y0 in range(H):
        for x0 in range(W):
            if not m[y0, x0] or lab[y0, x0] >= 0:
                continue
            label = y0 * W + x0
            lab[y0, x0] = label
            stack = [(y0, x0)]
            area, border = 0, False
            while stack:
                y, x = stack.pop()
                area += 1
                border = border or y == 0 or x == 0 or y == H - 1 or x == W - 1
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and m[yy, xx] and lab[yy, xx] < 0:
                        lab[yy, xx] = label
                        stack.append((yy, xx))
            info[label] = (area, border)
    return lab, info


def specks(m, min_area, largest):
    """Step 4 -> (mask, components removed, pixels removed)."""
    if min_area <= 0 and not largest:
        return m, 0, 0
    lab, info = components(m, 8)
    keep = {k for k, (a, _) in info.items() if a >= min_area}
    if largest and keep:
        best = max(keep, key=lambda k: (info[k][0], -k))
        keep = {best}
    out = m & np.isin(lab, sorted(keep))
    gone = [k for k in info if k not in keep]
    return out, len(gone), sum(info[k][0] for k in gone)


def holes(m, max_hole):
    """Step 5 -> (mask, holes filled, pixels filled)."""
    if max_hole == 0:
        return m, 0, 0
    lab, info = components(~m, 4)
    fill = [k for k, (a, b) in info.items() if not b and (max_hole < 0 or a <= max_hole)]
    return m | np.isin(lab, fill), len(fill), sum(info[k][0] for k in fill)


def segment_view(img, p, plate=None, holes_see_step4=True):
    """One view -> (final mask (H, W) bool, the eight counts of arvx_segment_counts).
    holes_see_step4=False: step 5 decides on step 3's result instead (what the definition rules out)."""
    m1 = rule(img, p, plate)
    m = m1
    if p["open_radius"] > 0:
        m = dilate(erode(m, p["open_radius"]), p["open_radius"])
    if p["close_radius"] > 0:
        m = erode(dilate(m, p["close_radius"]), p["close_radius"])
    m3 = m
    m4, sc, sp = specks(m3, p["min_area"], p["largest"])
    base = m4 if holes_see_step4 else m3
    filled, hc, hp = holes(base, p["max_hole"])
    m5 = m4 | (filled & ~base)
    return m5, np.array([m1.sum(), m3.sum(), m4.sum(), m5.sum(), sc, sp, hc, hp], np.int64)


def segment(images, p, plates=None):
    """All views -> (masks (V, H, W) uint8, 255 foreground; counts (V, 8))."""
    masks, counts = [], []
    for v, img in enumerate(images):
        plate = None
        if plates is not None:
            pl = np.asarray(plates).reshape(-1, *img.shape)
            plate = pl[0] if len(pl) == 1 else pl[v]
        m, c = segment_view(img, p, plate)
        masks.append(np.where(m, 255, 0).astype(np.uint8))
        counts.append(c)
    return np.stack(masks), np.stack(counts)


# ---- scenes -----------------------------------------------------------------------------------

FG, BG = 50, 200  # under the reference's range rule (background 120..255) and against a plate of BG


def image_of(mask):
    """(..., H, W) bool -> BGR images whose foreground under the default rule is `mask`."""
    return np.repeat(np.where(mask, FG, BG).astype(np.uint8)[..., None], 3, axis=-1)


def plate_of(H, W, n=1):
    return np.full((n, H, W, 3), BG, np.uint8)


def noise_masks(V, H, W, density, seed):
    return np.random.default_rng(seed).random((V, H, W)) < density


def blocks_masks(V, H, W, seed, n=5):
    """One large rectangle clear of the border, random smaller ones and 2 % of salt: what box openings
    and closings of large radii (9 and more) neither wipe out nor leave alone."""
    rng = np.random.default_rng(seed)
    m = rng.random((V, H, W)) < 0.02
    m[:, 1:max(2, H - 1), 2:max(3, 3 * W // 4)] = True
    for v in range(V):
        for _ in range(n):
            h, w = rng.integers(1, max(2, H // 2 + 1)), rng.integers(1, max(2, W // 2 + 1))
            y, x = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
            m[v, y:y + h, x:x + w] = True
    return m


def noise_images(V, H, W, seed):
    """Photographs with every byte value: for the rules' edges."""
    return np.random.default_rng(seed).integers(0, 256, (V, H, W, 3), dtype=np.uint8)


def rows(*text):
    """A mask from rows of '#' (foreground) and '.'."""
    return np.array([[c == "#" for c in row] for row in text])


def tie_scene():
    """Two largest components of 6 pixels each and a smaller one: LARGEST keeps the first."""
    return rows("..........",
                ".###..###.",
                ".###..###.",
                "..........",
                ".##.......",
                "..........")


def diagonal_gap_scene():
    """A ring whose only opening is a diagonal gap between two foreground pixels: the pocket is closed
    under 4-connectivity of the background, open under 8."""
    return rows(".......",
                ".####..",
                ".#...#.",
                ".#...#.",
                ".#####.",
                ".......")


def speck_merge_scene():
    """A ring with a one-pixel speck inside: once step 4 has removed the speck (and only then) the
    ring's inside is ONE hole of 9 pixels, above max_hole = 8 -- before, it is a hole of 8."""
    return rows(".......",
                ".#####.",
                ".#...#.",
                ".#.#.#.",
                ".#...#.",
                ".#####.",
                ".......")


def spiral_scene(H=16, W=64):
    """A one-pixel-wide rectangular spiral with one-pixel gaps: one long component (and one long
    background channel) whose equivalences chain round and round, across word boundaries."""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def free(yy, xx):
        return not (0 <= yy < H and 0 <= xx < W) or not m[yy, xx]

    while True:
        for _ in range(2):  # straight on, or one turn to the right
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = ny, nx
        m[y, x] = True


def comb_scene(H=16, W=64):
    """A comb: a spine along the bottom row, a tooth in every other column -- every tooth's label is
    replaced when the spine joins it to the first tooth."""
    m = np.zeros((H, W), bool)
    m[:, ::2] = True
    m[H - 1, :] = True
    return m


def hole_scene(area):
    """A frame around a hole of exactly `area` pixels (a 1 x area slot)."""
    m = np.ones((5, area + 4), bool)
    m[0, :] = m[-1, :] = False
    m[:, 0] = m[:, -1] = False
    m[2, 2:2 + area] = False
    return m


HAND_SCENES = {
    "tie": (tie_scene, dict(largest=True)),
    "diagonal_gap": (diagonal_gap_scene, dict(max_hole=-1)),
    "speck_merge": (speck_merge_scene, dict(min_area=2, max_hole=8)),
    "spiral": (spiral_scene, dict(min_area=5, max_hole=-1)),
    "spiral_130": (lambda: spiral_scene(9, 130), dict(largest=True, max_hole=-1)),
    "comb": (comb_scene, dict(largest=True, max_hole=-1)),
    "all_foreground": (lambda: np.ones((7, 70), bool), dict(min_area=3, largest=True, max_hole=-1, open_radius=1)),
    "all_background": (lambda: np.zeros((7, 70), bool), dict(min_area=3, largest=True, max_hole=-1, close_radius=1)),
    "hole_at_max": (lambda: hole_scene(6), dict(max_hole=6)),
    "hole_above_max": (lambda: hole_scene(7), dict(max_hole=6)),
}

RANDOM_MIN_AREA, RANDOM_MAX_HOLE = 3, 2


def random_cases():
    """(name, masks (V, H, W) bool, params): noise at two densities under the cleaning steps' sizes."""
    out = []
    for density in (0.3, 0.55):
        for (W, H) in ((70, 37), (33, 5)):
            m = noise_masks(2, H, W, density, seed=int(density * 100) + W)
            out.append((f"noise{density}_{W}x{H}", m, params(min_area=RANDOM_MIN_AREA, max_hole=RANDOM_MAX_HOLE)))
    return out
