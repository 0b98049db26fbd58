"""Numpy restatement of the triangle render with a near plane (arvx_ctx_set_render_near; the
definition is in include/arvx/arvx.h, in the triangle render's block), built on render_mesh and
np_restate: every face becomes a list of PIECES -- itself with the identity for B when all its corners
are in front, one or two clipped triangles when it straddles the plane, none when it is behind --, the
pieces are rasterised as render_mesh rasterises triangles, and the resolve finds the winner's least
piece.  Faces are clipped one at a time in plain loops; nothing here calls the device or is derived
from it."""
from collections import namedtuple

import numpy as np

from tests import np_restate as npr
from tests import render_mesh as rm
from tests.render import EMPTY, Rendered, channel

F32, F64, I64 = np.float32, np.float64, np.int64
DRAWN, EMPTY_CLASS, FLAT, REFUSED = range(4)

# image, counts, classes as render_mesh.Result; clip = (behind, straddling, pieces made, pieces drawn);
# pieces: per piece its face, index k, class and shape (corners in front: 3 for an unclipped face);
# weights = (pix, t, (w0, w1, w2), S) of the covered pixels; qmax: the largest |qu|, |qv| of a clipped
# vertex
Result = namedtuple("Result", "image counts classes clip pieces weights qmax")
Pieces = namedtuple("Pieces", "face k cls front")


def clipped_vertex(a, lo, hi, n):
    """The clipped vertex of the edge (lo, hi), lo < hi vertex indices, from the fp32 rows a (3, V):
    -> (fx, fy, valid, t, (qu, qv))."""
    assert lo < hi
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (F64(n) - F64(a[2][lo])) / (F64(a[2][hi]) - F64(a[2][lo]))
        c0 = F32(F64(a[0][lo]) + t * (F64(a[0][hi]) - F64(a[0][lo])))
        c1 = F32(F64(a[1][lo]) + t * (F64(a[1][hi]) - F64(a[1][lo])))
        qu, qv = F32(c0 / F32(n)), F32(c1 / F32(n))
        valid = bool(np.isfinite(qu) and np.isfinite(qv) and abs(qu) <= 32768 and abs(qv) <= 32768)
    fx = int(npr.round_half_away(F32(qu * F32(16.0)))) if valid else 0
    fy = int(npr.round_half_away(F32(qv * F32(16.0)))) if valid else 0
    return fx, fy, valid, t, (qu, qv)


def clip_face(face, a, pr, n):
    """One face (3 vertex indices) against the plane: -> (front corners, polygon), the polygon a list of
    (fx, fy, valid, a2, B) with B the three fp32 weights towards the face's corners."""
    front = [bool(a[2][i] >= n) for i in face]  # (a NaN compares false: behind)
    nf = sum(front)
    if nf == 0 or nf == 3:
        return nf, None

    def corner(j):
        i = face[j]
        B = [F32(0)] * 3
        B[j] = F32(1)
        return int(pr.fx[i]), int(pr.fy[i]), bool(pr.valid[i]), F32(a[2][i]), B

    def cut(j, k):  # C(j, k): the clipped vertex of the edge between corners j and k
        lo, hi = (j, k) if face[j] < face[k] else (k, j)
        fx, fy, valid, t, quv = clipped_vertex(a, int(face[lo]), int(face[hi]), n)
        qs.append(quv)
        B = [F32(0)] * 3
        with np.errstate(invalid="ignore"):
            B[hi] = F32(t)
            B[lo] = F32(F64(1.0) - t)
        return fx, fy, valid, F32(n), B

    qs = []
    if nf == 1:
        r = front.index(True)
        poly = [corner(r), cut(r, (r + 1) % 3), cut((r + 2) % 3, r)]
    else:
        r = (front.index(False) + 1) % 3
        poly = [corner(r), corner((r + 1) % 3), cut((r + 1) % 3, (r + 2) % 3), cut((r + 2) % 3, r)]
    return nf, (poly, qs)


def render(M, s, verts, vertex_rgb, faces, W, H, near=0.0, background=None, light=None, assoc_left=True):
    """-> Result; with near == 0 render_mesh.render's images, counts and classes and zeros for the rest."""
    if near == 0:
        res = rm.render(M, s, verts, vertex_rgb, faces, W, H, background, light, assoc_left)
        return Result(res.image, res.counts, res.classes, (0, 0, 0, 0), None, None, 0.0)
    n = F32(near)
    assert np.isfinite(n) and n >= rm.FLT_MIN
    verts = np.asarray(verts, F32).reshape(-1, 3)
    col = np.asarray(vertex_rgb, F32).reshape(-1, 3)
    faces = np.asarray(faces)
    faces = faces.reshape(-1, faces.shape[-1] if faces.ndim == 2 else 3)[:, :3].astype(I64)
    T = len(faces)
    pr = rm.project(M, s, verts, assoc_left)
    a, _, _ = npr.project_raw(M, s, verts[:, 0], verts[:, 1], verts[:, 2], assoc_left)
    assert np.array_equal(a[2].view(np.uint32), pr.a2.view(np.uint32))

    # ---- the pieces ----
    p_face, p_k, p_front, p_ok, px, py, pa2, pB = [], [], [], [], [], [], [], []
    behind = straddle = 0
    qmax = 0.0
    for t in range(T):
        nf, out = clip_face(faces[t], a, pr, n)
        if nf == 0:
            behind += 1
            continue
        if nf == 3:
            f = faces[t]
            polys = [[(int(pr.fx[f[j]]), int(pr.fy[f[j]]), bool(pr.valid[f[j]]), F32(a[2][f[j]]),
                       [F32(j == i) for i in range(3)]) for j in range(3)]]
        else:
            straddle += 1
            poly, qs = out
            qmax = max([qmax] + [float(abs(q)) for uv in qs for q in uv if np.isfinite(q)])
            polys = [[poly[0], poly[1], poly[2]]] + ([[poly[0], poly[2], poly[3]]] if nf == 2 else [])
        for k, tri in enumerate(polys):
            p_face.append(t), p_k.append(k), p_front.append(nf)
            p_ok.append(all(c[2] for c in tri))
            px.append([c[0] for c in tri]), py.append([c[1] for c in tri])
            pa2.append([c[3] for c in tri]), pB.append([c[4] for c in tri])
    P = len(p_face)
    p_face, p_k, p_front = np.array(p_face, I64), np.array(p_k, I64), np.array(p_front, I64)
    key = np.full(H * W, EMPTY, np.uint64)
    p_cls = np.full(P, REFUSED, I64)
    if P:
        ok = np.array(p_ok, bool)
        x = np.array(px, I64).reshape(P, 3).T  # (3, P)
        y = np.array(py, I64).reshape(P, 3).T
        B = np.array(pB, F32).reshape(P, 3, 3)  # [piece, piece corner, face corner]
        with np.errstate(divide="ignore"):
            iz = F64(1.0) / np.array(pa2, F32).reshape(P, 3).T.astype(F64)
        A = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        p_cls[ok & (A == 0)] = FLAT
        live = ok & (A != 0)
        neg, absA = A < 0, np.abs(A)
        c0 = np.maximum(-((-x.min(axis=0)) // 16), 0)
        c1 = np.minimum(x.max(axis=0) // 16, W - 1)
        r0 = np.maximum(-((-y.min(axis=0)) // 16), 0)
        r1 = np.minimum(y.max(axis=0) // 16, H - 1)
        wc, hr = np.maximum(c1 - c0 + 1, 0), np.maximum(r1 - r0 + 1, 0)
        box = np.where(live, wc * hr, 0)
        p_cls[live] = EMPTY_CLASS

        def at(k, c, r):
            """pieces k at pixels (c, r): covered, the fp64 weights t_0..t_2, S and the depth's bits"""
            e = rm._edges(x[:, k], y[:, k], 16 * c, 16 * r, neg[k])
            cov = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                tw, S = rm._weights(e, iz[:, k])
                depth = (absA[k].astype(F64) / S).astype(F32)
            return cov, tw, S, depth

        todo = np.flatnonzero(box)
        start = 0
        while start < len(todo):
            end = start + max(1, int(np.searchsorted(np.cumsum(box[todo[start:]]), rm.PAIRS, side="right")))
            k = todo[start:end]
            start = end
            rep = np.repeat(k, box[k])
            first = np.cumsum(box[k]) - box[k]
            j = np.arange(len(rep)) - np.repeat(first, box[k])
            c = c0[rep] + j % wc[rep]
            r = r0[rep] + j // wc[rep]
            cov, _, _, depth = at(rep, c, r)
            rep, c, r, depth = rep[cov], c[cov], r[cov], depth[cov]
            if not len(rep):
                continue
            assert (depth > 0).all()
            word = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | p_face[rep].astype(np.uint64)
            np.minimum.at(key, r * W + c, word)
            p_cls[np.unique(rep)] = DRAWN
    # ---- classes: a face takes the best of its pieces; one behind the plane is REFUSED ----
    classes = np.full(T, REFUSED, I64)
    if P:
        np.minimum.at(classes, p_face, p_cls)
    # ---- resolve ----
    empty = key == EMPTY
    ids = np.where(empty, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    dbits = np.where(empty, np.uint32(0x7F800000), (key >> np.uint64(32)).astype(np.uint32)).astype(np.uint32)
    bgr = np.zeros((H * W, 3), np.uint8) if background is None else \
        np.array(background, np.uint8).reshape(H * W, 3)
    pix = np.flatnonzero(~empty)
    weights = None
    if len(pix):
        t = ids[pix].astype(I64)
        piece_of = np.full((T, 2), -1, I64)
        piece_of[p_face, p_k] = np.arange(P)
        w = np.zeros((3, len(pix)), F64)
        S = np.zeros(len(pix), F64)
        found = np.zeros(len(pix), bool)
        for k in range(2):  # the least piece of the face that covers the pixel with exactly that depth
            pk = piece_of[t, k]
            sel = np.flatnonzero(~found & (pk >= 0) & (p_cls[np.maximum(pk, 0)] == DRAWN))
            if not len(sel):
                continue
            q = pk[sel]
            cov, tw, Sk, depth = at(q, pix[sel] % W, pix[sel] // W)
            hit = cov & (depth.view(np.uint32) == dbits[pix[sel]])
            sel, q = sel[hit], q[hit]
            for j in range(3):
                w[j, sel] = (tw[0][hit] * B[q, 0, j].astype(F64) + tw[1][hit] * B[q, 1, j].astype(F64)) + \
                    tw[2][hit] * B[q, 2, j].astype(F64)
            S[sel] = Sk[hit]
            found[sel] = True
        assert found.all()
        f = rm.shade(verts, faces, light)[t] if light is not None else None
        out = np.empty((len(pix), 3), F32)
        for ch in range(3):
            cc = [col[faces[t, j], ch].astype(F64) for j in range(3)]
            num = (w[0] * cc[0] + w[1] * cc[1]) + w[2] * cc[2]
            v = (num / S).astype(F32)
            out[:, ch] = v if f is None else (f * v).astype(F32)
        bgr[pix] = channel(out)[:, ::-1]
        weights = (pix, t, w, S)
    counts = tuple(int(np.count_nonzero(classes == k)) for k in range(4))
    clipped = p_front < 3
    clip = (behind, straddle, int(np.count_nonzero(clipped)), int(np.count_nonzero(clipped & (p_cls == DRAWN))))
    image = Rendered(bgr.reshape(H, W, 3), dbits.view(F32).reshape(H, W), ids.reshape(H, W))
    return Result(image, counts, classes, clip, Pieces(p_face, p_k, p_cls, p_front), weights, qmax)


def draw_textured(res, tex, verts, faces, background=None, light=None):
    """`res` drawn with source | ARVX_MESH_TEXTURED: mesh_texture.draw's lookup fed w in place of t."""
    from tests import mesh_texture as mt
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces)
    faces = faces.reshape(-1, faces.shape[-1] if faces.ndim == 2 else 3)[:, :3].astype(I64)
    Hh, Ww = res.image.id.shape
    bgr = np.zeros((Hh * Ww, 3), np.uint8) if background is None else \
        np.array(background, np.uint8).reshape(Hh * Ww, 3)
    if res.weights is not None:
        pix, t, w, S = res.weights
        i, j = mt.drawn_texel(w[1], w[2], S, tex.layout.R)
        tx, ty = mt.texel_xy(tex.layout, t, i, j)
        v = tex.atlas[ty, tx][:, ::-1].astype(F32)
        if light is not None:
            v = (rm.shade(verts, faces, light)[t][:, None] * v).astype(F32)
        bgr[pix] = channel(v)[:, ::-1]
    return Rendered(bgr.reshape(Hh, Ww, 3), res.image.depth, res.image.id)
