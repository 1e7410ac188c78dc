"""NumPy restatement of the exact multi-view visibility ("Dropping what no camera sees"), written from the
definition, not from the kernels.  The key image of a view is raster_ref's (the z-buffer of the whole mesh at cull = 0); all
floating point after it is one IEEE double addition and one comparison per (vertex, view); the rest is integer.  The device
results must equal run() byte for byte.
"""
from __future__ import annotations

import numpy as np

import raster_ref as R
import raycast_ref as RR
import sdist_ref as DR

DEFAULTS = dict(min_views=1, cull=1, fill=0)  # z_min and depth_tol have no default
COUNTS = ("faces_seen", "faces_back_only", "faces_unseen", "faces_kept", "verts_kept", "pairs_visible", "pairs_occluded", "pairs_off")
ARRAYS = ("verts", "faces", "vert_src", "face_src", "face_views", "face_back_views", "vert_views")


def check_params(z_min=0.0, depth_tol=-1.0, min_views=1, cull=1, fill=0):
    return bool(np.isfinite(z_min) and z_min > 0 and np.isfinite(depth_tol) and depth_tol >= 0 and min_views >= 0 and cull in (0, 1)
                and 0 <= fill <= 255)


def key_image(verts, F, cam, z_min, brute=False):
    """(pr, keys uint64 [h][w]) of one view: raster_ref's projection and contest of every face, nothing culled"""
    w, h = int(cam["w"]), int(cam["h"])
    assert 1 <= w <= R.W_MAX and h >= 1 and w * h <= R.WH_MAX
    pr = R.project(verts, cam, z_min)
    _, idx = R._classify(F, len(pr[0]), pr, 0)
    keys = (R._contest_brute if brute else R._contest_boxes)(F, idx, pr, w, h)[0]
    return pr, keys


def view_visibility(verts, F, cam, z_min, depth_tol, brute=False):
    """of one view: visible, off (bool [n]; occluded is neither), x, y (int64 [n], the vertex's pixel where visible), p = X - c
    ([3] of f64 [n]), A (int64 [m], the integer area of every face from the snapped corners, 0 where a corner is not inband)"""
    X = np.asarray(verts, np.float64).reshape(-1, 3)
    w, h = int(cam["w"]), int(cam["h"])
    (near, inband, U, V, r), keys = key_image(X, F, cam, z_min, brute)
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    Rm = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        p = [X[:, a] - c[a] for a in range(3)]
        q2 = (Rm[2, 0] * p[0] + Rm[2, 1] * p[1]) + Rm[2, 2] * p[2]
    x, y = (U + 128) >> 8, (V + 128) >> 8
    inside = inband & (x >= 0) & (x < w) & (y >= 0) & (y < h)
    xs, ys = np.where(inside, x, 0), np.where(inside, y, 0)
    k = keys[ys, xs]
    D = (k >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        passes = q2 <= D + float(depth_tol)
    visible = inside & ((k == R.EMPTY) | passes)
    Uf, Vf = U[F], V[F]
    A = (Uf[:, 1] - Uf[:, 0]) * (Vf[:, 2] - Vf[:, 0]) - (Vf[:, 1] - Vf[:, 0]) * (Uf[:, 2] - Uf[:, 0])
    return visible, ~inside, xs, ys, p, A


def run(verts, faces, cams, z_min, depth_tol, normals=None, images=None, min_views=1, cull=1, fill=0, brute=False):
    """dict(the ARRAYS, normals with normals, grey u8 [n] and grey_views int32 [n] with images, the COUNTS); ValueError for a face
    index outside [0, n).  cams: dicts with w and h; images: None or one uint8 [h][w] per view."""
    assert check_params(z_min, depth_tol, min_views, cull, fill)
    X = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    F32 = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    F = F32.astype(np.int64)
    n, m = len(X), len(F)
    assert n < R.N_MAX and m < R.M_MAX
    if ((F < 0) | (F >= n)).any():
        raise ValueError("a face index outside [0, n)")
    assert images is None or len(images) == len(cams)
    N = None if normals is None else np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    assert not (images is not None and cull == 1 and N is None and n > 0)
    fv, fb, vv = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(n, np.int32)
    acc, cnt = np.zeros(n, np.int64), np.zeros(n, np.int32)
    pairs = [0, 0, 0]
    for k, cam in enumerate(cams):
        vis, off, x, y, p, A = view_visibility(X, F, cam, z_min, depth_tol, brute)
        vv += vis
        pairs[0] += int(vis.sum())
        pairs[2] += int(off.sum())
        pairs[1] += int((~vis & ~off).sum())
        all3 = vis[F].all(1) if m else np.zeros(0, bool)
        fv += all3 & (A < 0)
        fb += all3 & (A > 0)
        if images is not None:
            use = vis.copy()
            if cull == 1 and n:
                with np.errstate(all="ignore"):
                    use &= ((N[:, 0] * p[0] + N[:, 1] * p[1]) + N[:, 2] * p[2]) < 0.0
            img = np.asarray(images[k], np.uint8)
            assert img.shape == (int(cam["h"]), int(cam["w"]))
            acc += np.where(use, img[y, x].astype(np.int64), 0)
            cnt += use
    keep = fv >= int(min_views)
    vkeep = np.zeros(n, bool)
    vkeep[F[keep].ravel()] = True
    vsrc = np.nonzero(vkeep)[0].astype(np.int32)
    fsrc = np.nonzero(keep)[0].astype(np.int32)
    renum = np.cumsum(vkeep) - 1
    out = dict(verts=X[vsrc].copy(), faces=renum[F[keep]].astype(np.int32).reshape(-1, 3), vert_src=vsrc, face_src=fsrc, face_views=fv,
               face_back_views=fb, vert_views=vv, faces_seen=int((fv >= 1).sum()), faces_back_only=int(((fv == 0) & (fb >= 1)).sum()),
               faces_unseen=int(((fv == 0) & (fb == 0)).sum()), faces_kept=int(keep.sum()), verts_kept=int(vkeep.sum()),
               pairs_visible=pairs[0], pairs_occluded=pairs[1], pairs_off=pairs[2])
    if N is not None:
        out["normals"] = N[vsrc].copy()
    if images is not None:
        c64 = cnt.astype(np.int64)
        out["grey"] = np.where(cnt > 0, (2 * acc + c64) // np.maximum(2 * c64, 1), int(fill)).astype(np.uint8)
        out["grey_views"] = cnt
    return out


def counts(ref):
    return {k: int(ref[k]) for k in COUNTS}


def same(a, b, what=""):
    """byte equality of two results: the counts, the arrays, normals and grey when either has them"""
    assert counts(a) == counts(b), (what, counts(a), counts(b))
    keys = ARRAYS
    for opt in ("normals", "grey", "grey_views"):
        assert (opt in a) == (opt in b), (what, opt)
        if opt in a:
            keys = keys + (opt,)
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.tobytes() != y.tobytes():
            xv = x.view(np.uint64) if x.dtype == np.float64 else x
            yv = y.view(np.uint64) if y.dtype == np.float64 else y
            bad = np.argwhere(xv != yv)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} elements, first {bad[0].tolist()}: {x[tuple(bad[0])]!r} != {y[tuple(bad[0])]!r}")


# ---- test scenes -------------------------------------------------------------------------------------------------------------
Z_MIN = 0.05


def six_cameras(f=300.0, w=160, h=160, dist=0.5):
    """on +-x, +-y, +-z at `dist` from the origin, looking at it"""
    out = []
    for a in range(3):
        for sg in (1.0, -1.0):
            c = np.zeros(3)
            c[a] = sg * dist
            out.append(RR.camera(c, (0.0, 0.0, 0.0), f, w, h))
    return out


def nested_spheres():
    """(verts, faces, normals, n_outer, m_outer): icosphere(3, 0.1) around icosphere(2, 0.05), both outward; the normal of a vertex
    is its direction from the centre"""
    vo, fo = DR.icosphere(3, 0.1)
    vi, fi = DR.icosphere(2, 0.05)
    v = np.concatenate([vo, vi])
    f = np.concatenate([fo, fi + len(vo)]).astype(np.int32)
    return v, f, v / np.linalg.norm(v, axis=1)[:, None], len(vo), len(fo)


def flipped_patch(count=40):
    """the outer sphere alone with its first `count` faces wound the other way: (verts, faces, normals)"""
    v, f = DR.icosphere(3, 0.1)
    f = f.astype(np.int32).copy()
    f[:count] = f[:count, ::-1]
    return v, f, v / np.linalg.norm(v, axis=1)[:, None]


def inside_camera(f=300.0, w=160, h=160):
    """at the centre of the spheres, looking along +z"""
    return RR.axis_camera((0.0, 0.0, 0.0), f, w, h, (w - 1) / 2.0, (h - 1) / 2.0)


def images_for(cams, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (int(c["h"]), int(c["w"]))).astype(np.uint8) for c in cams]


def _quad(z, lo=1.0, hi=6.0):
    """two faces, front-facing (A < 0) for the pixel camera, at depth z"""
    return R.at_pixels([(lo, lo), (lo, hi), (hi, hi), (hi, lo)], z), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def hand_cases():
    """name -> dict(verts, faces, cams, z_min, depth_tol): pixel_camera scenes (f = 256, cx = cy = 0, R = I at the origin), so a
    vertex built by at_pixels at depth z has q2 = z exactly and, at a power-of-two depth, snaps to 256 times its pixel position"""
    out = {}

    def add(name, verts, faces, cams=None, z_min=0.5, depth_tol=0.25):
        out[name] = dict(verts=np.ascontiguousarray(verts, np.float64), faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3),
                         cams=cams if cams is not None else [R.pixel_camera(8, 8)], z_min=z_min, depth_tol=depth_tol)

    # two parallel quads: the far one's vertices lie behind the near one; gap below, at and one ulp above depth_tol = 0.25.  The
    # near quad is at depth 1 (exact in float), the far one larger in the image so that its corners project inside the near one
    for name, far in (("gap-below", np.nextafter(1.25, 0.0)), ("gap-at", 1.25), ("gap-ulp-above", np.nextafter(1.25, 2.0))):
        vn, fn = _quad(1.0, 0.0, 7.0)
        vf, ff = _quad(far, 2.0, 5.0)
        add(name, np.concatenate([vn, vf]), np.concatenate([fn, ff + 4]))
    # snapped position exactly between two pixel centres: U = 256 x + 128 goes to x + 1 ((U + 128) >> 8), in x and in y.  The
    # plane in front has 1 / depth = 1 / 2 - (x + y) / 56, i.e. depth 3 where x + y = 9 1/3: a vertex at depth 3 on (4.5, 5) is
    # visible at pixel (5, 5) and would be occluded at (4, 5); likewise (5, 4.5).  (-0.5, 3) is pixel (0, 3), (7.5, 7.5) is off
    vq = R.at_pixels([(0, 0), (0, 7), (7, 7), (7, 0)], [2.0, 8.0 / 3.0, 4.0, 8.0 / 3.0])
    vh = R.at_pixels([(4.5, 5.0), (5.0, 4.5), (6.5, 6.5)], 3.0)
    vo = R.at_pixels([(-0.5, 3.0), (3.0, -0.5), (7.5, 7.5)], 1.0)
    add("half-pixel", np.concatenate([vq, vh, vo]), [[0, 1, 2], [0, 2, 3], [5, 4, 6]], depth_tol=0.0)  # the last three: no face
    # vertices over empty pixels: a face that does not cover the pixels its own corners snap to, in both windings
    add("empty-pixel", R.at_pixels([(1.2, 1.2), (1.4, 6.3), (6.2, 1.3)], 1.0), [[0, 2, 1], [0, 1, 2]])
    # off each border (not in the image though inband), at z_min and one ulp below, NaN and infinite
    v = R.at_pixels([(3, 3), (3, 5), (5, 5), (-0.51, 3), (3, -0.51), (7.5, 3), (3, 7.5), (7.49, 7.49), (-0.5, -0.5)], 1.0)
    f = [[0, 1, 2], [3, 0, 1], [4, 0, 1], [5, 1, 2], [6, 1, 2], [7, 1, 2], [8, 0, 1]]
    add("off-borders", v, f)
    v = R.at_pixels([(1, 1), (1, 6), (6, 6)] * 2, [0.5, 1.0, 1.0, np.nextafter(0.5, 0.0), 1.0, 1.0])
    add("z-min", v, [[0, 1, 2], [3, 4, 5]])
    v = R.at_pixels([(1, 1), (1, 6), (6, 6)] * 4, 1.0)
    v[3, 0], v[7, 1], v[11, 2] = np.nan, np.inf, -np.inf
    add("non-finite", v, np.arange(12).reshape(4, 3))
    # sub-pixel faces that own no pixel centre: their vertices see empty pixels (or a face far behind) and the faces are seen
    vb, fb_ = _quad(2.0, 0.0, 7.0)
    vs = R.at_pixels([(2.2, 2.2), (2.4, 2.9), (2.8, 2.3), (9.2, 9.2), (9.4, 9.9), (9.8, 9.3)], 1.0)
    add("no-centre", np.concatenate([vb, vs]), np.concatenate([fb_, [[4, 5, 6], [7, 8, 9]]]), cams=[R.pixel_camera(12, 12)])
    # collinear after snapping: A = 0, neither seen nor seen from behind, though all three corners are visible
    add("collinear", R.at_pixels([(1, 1), (2, 2), (3, 3), (2.001, 2.0005), (5, 1), (5, 1)], 1.0), [[0, 1, 2], [0, 3, 2], [0, 4, 5], [0, 1, 1]])
    # a back face at depth 1 in front of a front face at depth 2: the back face occludes it
    add("back-before-front", R.at_pixels([(0, 0), (7, 0), (0, 7), (2, 2), (2, 4), (4, 2)], [1.0] * 3 + [2.0] * 3), [[0, 1, 2], [3, 4, 5]])
    # nothing at all, vertices without faces
    add("no-faces", R.at_pixels([(1, 1), (2, 2), (30, 2)], 1.0), np.zeros((0, 3), np.int32))
    add("no-verts", np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    # two views of different sizes, the second sees the quads from the back (it looks along -z from beyond them)
    vn, fn = _quad(1.0, 1.0, 6.0)
    behind = dict(R_rw=np.diag([-1.0, 1.0, -1.0]), c_left=np.array([0.0, 0.0, 3.0]), f=256.0, cx=4.0, cy=0.0, B=0.0, w=5, h=9)
    add("two-views", vn, fn, cams=[R.pixel_camera(8, 8), behind])
    return out


def mixed_views():
    """cameras of sizes around the 8 x 8 and 16 x 16 tiles, 1 x 1 and 4096 x 1 among them, all pixel cameras over one scene"""
    return [R.pixel_camera(w, h) for w, h in ((1, 1), (7, 9), (8, 8), (17, 16), (64, 4), (4096, 1), (16, 16), (3, 33))]


def soup(count=300, seed=5, w=24, h=20):
    """a random soup over (and past) a w x h image: (verts, faces, normals)"""
    v, f, nrm, _ = R.random_scene(w, h, count, seed)
    return v, f, nrm


BAD_PARAMS = (dict(z_min=0.0, depth_tol=0.1), dict(z_min=-1.0, depth_tol=0.1), dict(z_min=float("nan"), depth_tol=0.1),
              dict(z_min=float("inf"), depth_tol=0.1), dict(z_min=1.0, depth_tol=-1e-300), dict(z_min=1.0, depth_tol=float("nan")),
              dict(z_min=1.0, depth_tol=float("inf")), dict(z_min=1.0, depth_tol=0.1, min_views=-1), dict(z_min=1.0, depth_tol=0.1, cull=2),
              dict(z_min=1.0, depth_tol=0.1, cull=-1), dict(z_min=1.0, depth_tol=0.1, fill=256), dict(z_min=1.0, depth_tol=0.1, fill=-1))
GOOD_PARAMS = (dict(z_min=1.0, depth_tol=0.0), dict(z_min=5e-324, depth_tol=1.7e308), dict(z_min=0.5, depth_tol=0.1, min_views=0),
               dict(z_min=0.5, depth_tol=0.1, min_views=1 << 30, cull=0, fill=255))
