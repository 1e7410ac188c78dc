"""NumPy restatement of the best-view per-face texture atlas ("Texturing the surface"), written from the
definition, not from the kernels.  Which view sees a face is visib_ref.view_visibility's answer (the z-buffer of the whole mesh,
the per-vertex depth test, the integer area A); the best view, the ranks and the layout are integers; a texel is IEEE double in
the definition's expression order and one rounding.  The device results must equal run() byte for byte.
"""
from __future__ import annotations

import numpy as np

import raster_ref as R
import visib_ref as VR

DEFAULTS = dict(patch=8, cells_per_row=0, fill=0)  # z_min and depth_tol have no default
COUNTS = ("faces_textured", "faces_untextured", "cells", "W", "H", "cells_per_row")
ARRAYS = ("atlas", "face_view", "face_area", "uv_half", "view_faces")
PATCH_MIN, PATCH_MAX, W_MAX, TEXELS_MAX = 3, 64, 16384, 1 << 28


def check_params(z_min=0.0, depth_tol=-1.0, patch=8, cells_per_row=0, fill=0):
    return bool(np.isfinite(z_min) and z_min > 0 and np.isfinite(depth_tol) and depth_tol >= 0 and PATCH_MIN <= patch <= PATCH_MAX
                and cells_per_row >= 0 and 0 <= fill <= 255)


def half_texels(S):
    """(i, j) int64 [k] of the texels a half owns: i, j >= 0, i + j <= S - 1"""
    i, j = np.meshgrid(np.arange(S, dtype=np.int64), np.arange(S, dtype=np.int64), indexing="ij")
    own = i + j <= S - 1
    return i[own], j[own]


def half_local(S, half, i, j):
    """the local texel (x, y) in the (S + 1) x S cell of texel (i, j) of a half"""
    return (i, j) if half == 0 else (S - i, S - 1 - j)


def gutter(S, i, j):
    """(i', j'): the barycentric steps a texel samples at; the texels with i + j = S - 1 repeat the hypotenuse"""
    L = S - 2
    i2 = np.minimum(i, L)
    return i2, np.minimum(j, L - i2)


def corners_half(S, half):
    """int64 [3][2]: the corners a, b, c of a half in half-texels relative to the cell"""
    c = np.array([[1, 1], [2 * S - 3, 1], [1, 2 * S - 3]], np.int64)
    return c if half == 0 else np.array([2 * (S + 1), 2 * S], np.int64) - c


def best_views(verts, F, cams, z_min, depth_tol, brute=False):
    """face_view int32 [m] (-1: no view sees the face), face_area int64 [m]"""
    m = len(F)
    fv, fa = np.full(m, -1, np.int32), np.zeros(m, np.int64)
    for k, cam in enumerate(cams):
        vis, _, _, _, _, A = VR.view_visibility(verts, F, cam, z_min, depth_tol, brute)
        seen = (vis[F].all(1) if m else np.zeros(0, bool)) & (A < 0)
        better = seen & (-A > fa)
        fv[better] = k
        fa[better] = -A[better]
    return fv, fa


def layout(n_tex, n_un, patch=8, cells_per_row=0):
    """dict(cells, cells_per_row, W, H); ValueError when the atlas would be wider than 16 384 or larger than 2^28 texels"""
    S = int(patch)
    cells = (n_tex + 1) // 2 + (1 if n_un > 0 else 0)
    C = int(cells_per_row)
    if C == 0:
        C = 1
        while C * C < cells:
            C += 1
        C = max(1, min(C, W_MAX // (S + 1)))
    if cells == 0:
        return dict(cells=0, cells_per_row=C, W=0, H=0)
    W, H = C * (S + 1), -(-cells // C) * S
    if W > W_MAX or W * H > TEXELS_MAX:
        raise ValueError("the atlas is too large")
    return dict(cells=cells, cells_per_row=C, W=W, H=H)


def uv_half(face_view, lay, patch):
    """int32 [m][3][2]: the corners of every face in half-texels of the atlas"""
    S, C = int(patch), lay["cells_per_row"]
    tex = face_view >= 0
    rank = np.cumsum(tex) - 1
    m = len(face_view)
    out = np.zeros((m, 3, 2), np.int64)
    cell = np.where(tex, rank >> 1, lay["cells"] - 1)
    x0, y0 = (cell % C) * (S + 1), (cell // C) * S
    for half in (0, 1):
        sel = tex & ((rank & 1) == half)
        out[sel] = corners_half(S, half)[None]
    out[~tex] = np.array([S + 1, S], np.int64)[None, None]
    out[:, :, 0] += 2 * x0[:, None]
    out[:, :, 1] += 2 * y0[:, None]
    return out.astype(np.int32)


def texel_map(face_view, lay, patch):
    """per atlas texel, flat [H W]: face int64 (-1: a fill texel), i, j int64 (the texel inside its half)"""
    S, C, W, H, cells = int(patch), lay["cells_per_row"], lay["W"], lay["H"], lay["cells"]
    tex_list = np.nonzero(face_view >= 0)[0]
    n_tex, n_un = len(tex_list), len(face_view) - len(tex_list)
    y, x = np.divmod(np.arange(W * H, dtype=np.int64), max(W, 1))
    cc, lx = np.divmod(x, S + 1)
    cr, ly = np.divmod(y, S)
    c = cr * C + cc
    half = (lx + ly >= S).astype(np.int64)
    i = np.where(half == 1, S - lx, lx)
    j = np.where(half == 1, S - 1 - ly, ly)
    r = 2 * c + half
    valid = (c < cells) & ~((n_un > 0) & (c == cells - 1)) & (r < n_tex)
    face = np.where(valid, tex_list[np.where(valid, r, 0)] if n_tex else -1, -1)
    return face, i, j


def texel_points(verts, F, face, i, j, patch):
    """[3] of f64 [k]: the surface point of texel (i, j) of face `face`"""
    L = int(patch) - 2
    i2, j2 = gutter(int(patch), i, j)
    a, b, c = F[face, 0], F[face, 1], F[face, 2]
    wa, wb, wc = (L - i2 - j2).astype(np.float64), i2.astype(np.float64), j2.astype(np.float64)
    with np.errstate(all="ignore"):
        return [((wa * verts[a, r] + wb * verts[b, r]) + wc * verts[c, r]) / float(L) for r in range(3)]


def sample(X, cam, img, fill):
    """u8 [k]: the bilinear sample of img at the projection of the points X ([3] of f64 [k])"""
    Rm = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    f, cx, cy = float(cam["f"]), float(cam["cx"]), float(cam["cy"])
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    I = img.astype(np.float64)
    with np.errstate(all="ignore"):
        p = [X[a] - c[a] for a in range(3)]
        q = [(Rm[r, 0] * p[0] + Rm[r, 1] * p[1]) + Rm[r, 2] * p[2] for r in range(3)]
        u = (f * q[0]) / q[2] + cx
        v = (f * q[1]) / q[2] + cy
        ok = (q[2] > 0) & np.isfinite(u) & np.isfinite(v)
        u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        uc = np.minimum(np.maximum(u, -1.0), float(w))
        vc = np.minimum(np.maximum(v, -1.0), float(h))
        x0, y0 = np.floor(uc), np.floor(vc)
        ax, ay = uc - x0, vc - y0
        xi0 = np.clip(x0.astype(np.int64), 0, w - 1)
        xi1 = np.clip(x0.astype(np.int64) + 1, 0, w - 1)
        yi0 = np.clip(y0.astype(np.int64), 0, h - 1)
        yi1 = np.clip(y0.astype(np.int64) + 1, 0, h - 1)
        top = (1.0 - ax) * I[yi0, xi0] + ax * I[yi0, xi1]
        bot = (1.0 - ax) * I[yi1, xi0] + ax * I[yi1, xi1]
        g = (1.0 - ay) * top + ay * bot
        t = np.minimum(255.0, np.floor(g + 0.5))
    return np.where(ok, t, float(fill)).astype(np.uint8)


def bake(verts, F, cams, images, face_view, lay, patch, fill):
    """atlas u8 [H][W]"""
    W, H = lay["W"], lay["H"]
    face, i, j = texel_map(face_view, lay, patch)
    atlas = np.full(W * H, int(fill), np.uint8)
    view = np.where(face >= 0, face_view[np.maximum(face, 0)], -1)
    for k in np.unique(view[view >= 0]):
        sel = np.nonzero(view == k)[0]
        X = texel_points(verts, F, face[sel], i[sel], j[sel], patch)
        atlas[sel] = sample(X, cams[k], images[k], fill)
    return atlas.reshape(H, W)


def run(verts, faces, cams, images, z_min, depth_tol, patch=8, cells_per_row=0, fill=0, brute=False, best=None):
    """dict(atlas u8 [H][W], face_view int32 [m], face_area int64 [m], uv_half int32 [m][3][2], view_faces int32 [V], the COUNTS);
    ValueError for a face index outside [0, n), no views, a view without an image, parameters outside their range and an atlas
    that is too large.  best: (face_view, face_area) of an earlier run on the same mesh, views, z_min and depth_tol"""
    if not check_params(z_min, depth_tol, patch, cells_per_row, fill):
        raise ValueError("parameters")
    X = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    n, m = len(X), len(F)
    assert n < R.N_MAX and m < R.M_MAX
    if len(cams) < 1 or images is None or len(images) != len(cams) or any(im is None for im in images):
        raise ValueError("every view needs an image, and there is at least one view")
    for cam, im in zip(cams, images):
        assert np.asarray(im).shape == (int(cam["h"]), int(cam["w"]))
    if ((F < 0) | (F >= n)).any():
        raise ValueError("a face index outside [0, n)")
    fv, fa = best_views(X, F, cams, z_min, depth_tol, brute) if best is None else best
    n_tex = int((fv >= 0).sum())
    lay = layout(n_tex, m - n_tex, patch, cells_per_row)
    return dict(atlas=bake(X, F, cams, images, fv, lay, patch, fill), face_view=fv, face_area=fa, uv_half=uv_half(fv, lay, patch),
                view_faces=np.bincount(fv[fv >= 0], minlength=len(cams)).astype(np.int32), faces_textured=n_tex,
                faces_untextured=m - n_tex, **lay)


def uv(uvh, W, H):
    """f64 [m][3][2]: u = hx / (2 W), v = 1 - hy / (2 H)"""
    uvh = np.asarray(uvh, np.float64)
    out = np.zeros(uvh.shape)
    if W and H:
        out[..., 0] = uvh[..., 0] / (2.0 * W)
        out[..., 1] = 1.0 - uvh[..., 1] / (2.0 * H)
    return out


def counts(ref):
    return {k: int(ref[k]) for k in COUNTS}


def same(a, b, what=""):
    """byte equality of two results: the counts and the arrays"""
    assert counts(a) == counts(b), (what, counts(a), counts(b))
    for k in ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.tobytes() != y.tobytes():
            bad = np.argwhere(x != y)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} elements, first {bad[0].tolist()}: {x[tuple(bad[0])]!r} != {y[tuple(bad[0])]!r}")


BAD_PARAMS = (dict(z_min=0.0, depth_tol=0.1), dict(z_min=float("nan"), depth_tol=0.1), dict(z_min=1.0, depth_tol=-1e-300),
              dict(z_min=1.0, depth_tol=float("inf")), dict(z_min=1.0, depth_tol=0.1, patch=2), dict(z_min=1.0, depth_tol=0.1, patch=65),
              dict(z_min=1.0, depth_tol=0.1, cells_per_row=-1), dict(z_min=1.0, depth_tol=0.1, fill=256), dict(z_min=1.0, depth_tol=0.1, fill=-1))
GOOD_PARAMS = (dict(z_min=1.0, depth_tol=0.0), dict(z_min=5e-324, depth_tol=1.7e308, patch=3), dict(z_min=0.5, depth_tol=0.1, patch=64, fill=255),
               dict(z_min=0.5, depth_tol=0.1, cells_per_row=1 << 30))


# ---- fidelity on the textured sphere of DESIGN.md 14 ---------------------------------------------------------------------------
FIDELITY = dict(level=4, radius=0.1, z_min=0.05, depth_tol=0.002, patch=8)


def fidelity_scene():
    """(verts, faces, cams, images): a level-4 icosphere of radius 0.1 under appearance_ref.textured_sphere_views' 26 cameras"""
    import appearance_ref as AR
    import sdist_ref as DR
    v, f = DR.icosphere(FIDELITY["level"], FIDELITY["radius"])
    views = AR.textured_sphere_views(FIDELITY["radius"])
    cams = [dict(cam, w=img.shape[1], h=img.shape[0]) for cam, _, img in views]
    return v, f.astype(np.int32), cams, [img for _, _, img in views]


def fidelity(verts, faces, res, patch, vertex_grey=None):
    """over the textured non-gutter texels of a result: (mean, 99th percentile) of |texel - T(the texel's point)| with T
    appearance_ref.texture, and, with vertex_grey u8 [n], the mean of |the vertex grey interpolated to the point - T|"""
    import appearance_ref as AR
    S, L = int(patch), int(patch) - 2
    X = np.asarray(verts, np.float64).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    lay = {k: int(res[k]) for k in ("cells", "cells_per_row", "W", "H")}
    face, i, j = texel_map(np.asarray(res["face_view"]), lay, S)
    sel = np.nonzero((face >= 0) & (i + j <= L))[0]
    P = np.stack(texel_points(X, F, face[sel], i[sel], j[sel], S), 1)
    T = AR.texture(P)
    err = np.abs(np.asarray(res["atlas"]).ravel()[sel].astype(np.float64) - T)
    out = (float(err.mean()), float(np.percentile(err, 99)))
    if vertex_grey is not None:
        G = np.asarray(vertex_grey, np.float64)[F[face[sel]]]
        wgt = np.stack([L - i[sel] - j[sel], i[sel], j[sel]], 1) / float(L)
        out += (float(np.abs((G * wgt).sum(1) - T).mean()),)
    return out
