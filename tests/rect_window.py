"""numpy restatement of the pixel rectangle of rect_prepare (csrc/carve_kernels.h) for many boxes
at once, in fp32 and in the kernel's order of operations, and the boxes the carve kernels form.

Two instructions have no numpy counterpart: the fused multiply-adds of the base corner are formed
here as an exact fp64 product plus an fp64 sum rounded to fp32 (a second rounding, at most one unit
in the last place away), and v_rcp_f32 (one unit) is 1 / x.  Both are far inside the whole pixel of
slack that the window (arvx.h, arvx_view_window_host) adds for exactly this kind of difference."""
import numpy as np

f32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def rectangles(M, boxes, s, W, H):
    """M: (3, 4) float32.  boxes: (n, 6) ints x0, x1, y0, y1, z0, z1 (voxel indices, inclusive, global
    z).  Returns (reads, pxlo, pxhi, pylo, pyhi): reads[i] = rect_prepare answers code < 0 for box
    i, i.e. the four entries (pylo, pxlo) .. (pyhi + 1, pxhi + 1) of the table are read."""
    M = np.asarray(M, f32).reshape(3, 4)
    b = np.asarray(boxes, np.int64)
    s = f32(s)
    n = len(b)
    with np.errstate(all="ignore"):
        wx0, wx1 = b[:, 0].astype(f32) * s, b[:, 1].astype(f32) * s
        wy0, wy1 = b[:, 2].astype(f32) * s, b[:, 3].astype(f32) * s
        wz0, wz1 = (-b[:, 4]).astype(f32) * s, (-b[:, 5]).astype(f32) * s
        dy, dx, dz = wy1 - wy0, wx1 - wx0, wz1 - wz0
        ay = np.maximum(np.abs(wy0), np.abs(wy1))
        ax = np.maximum(np.abs(wx0), np.abs(wx1))
        az = np.maximum(np.abs(wz0), np.abs(wz1))
        a = np.empty((3, 8, n), f32)
        E = np.empty((3, n), f32)
        for r in range(3):
            m0, m1, m2, m3 = (np.full(n, M[r, k], f32) for k in range(4))
            E[r] = ((np.abs(m0) * ay + np.abs(m1) * ax) + np.abs(m2) * az) + np.abs(m3)
            base = _fma(m0, wy0, _fma(m1, wx0, _fma(m2, wz0, m3)))
            ey, ex, ez = m0 * dy, m1 * dx, m2 * dz
            a[r, 0] = base
            a[r, 1] = base + ey
            a[r, 2] = base + ex
            a[r, 3] = a[r, 1] + ex
            for c in range(4):
                a[r, 4 + c] = a[r, c] + ez
        rc = f32(1.0) / a[2]
        fu, fv = a[0] * rc, a[1] * rc
        umin, umax = fu.min(axis=0), fu.max(axis=0)
        vmin, vmax = fv.min(axis=0), fv.max(axis=0)
        bad = np.isnan(fu).any(axis=0) | np.isnan(fv).any(axis=0)
        cmin, cmax = a[2].min(axis=0), a[2].max(axis=0)
        k19, k20, k12 = f32(2.0 ** -19), f32(2.0 ** -20), f32(2.0 ** -12)
        eps0, eps1, eps2 = E[0] * k19, E[1] * k19, E[2] * k19
        cabs = np.where(cmin > 0, cmin, np.where(cmax < 0, -cmax, f32(0))).astype(f32)
        ok = cabs > f32(8.0) * eps2 + f32(1e-30)
        Ua = np.maximum(np.abs(umin), np.abs(umax))
        Va = np.maximum(np.abs(vmin), np.abs(vmax))
        ok &= (Ua < f32(1.0e6)) & (Va < f32(1.0e6)) & ~bad
        rden = f32(1.0001) / (cabs - eps2)
        mu = (eps0 + Ua * eps2) * rden + Ua * k20 + k12
        mv = (eps1 + Va * eps2) * rden + Va * k20 + k12
        big = np.float64(1 << 30)

        def to_int(x):
            return np.clip(np.nan_to_num(x.astype(np.float64), nan=big, posinf=big, neginf=-big), -big, big).astype(np.int64)

        pxlo = to_int(np.ceil(umin - mu - f32(0.5)))
        pxhi = to_int(np.floor(umax + mu + f32(0.5)))
        pylo = to_int(np.ceil(vmin - mv - f32(0.5)))
        pyhi = to_int(np.floor(vmax + mv + f32(0.5)))
    inside = (pxlo >= 0) & (pxhi < W) & (pylo >= 0) & (pyhi < H)
    small = (pxhi + 1 - pxlo) * (pyhi + 1 - pylo) < 65536
    return ok & inside & small, pxlo, pxhi, pylo, pyhi


def grid_boxes(X, Y, Z, size):
    """Every box of size = (bx, by, bz) voxels of the raster from the origin, clipped to the grid:
    (n, 6) x0, x1, y0, y1, z0, z1."""
    bx, by, bz = size
    x0, y0, z0 = np.meshgrid(np.arange(0, X, bx), np.arange(0, Y, by), np.arange(0, Z, bz), indexing="ij")
    x0, y0, z0 = x0.ravel(), y0.ravel(), z0.ravel()
    return np.stack([x0, np.minimum(x0 + bx - 1, X - 1), y0, np.minimum(y0 + by - 1, Y - 1),
                     z0, np.minimum(z0 + bz - 1, Z - 1)], axis=1)


# what the carve kernels test: coarse tiles (contiguous slabs; striped slabs), sub-tiles, blocks
BOX_SIZES = {"coarse": (64, 32, 32), "coarse, striped": (64, 64, 8), "sub-tile": (16, 8, 8), "block": (4, 4, 4)}
