"""NumPy restatement of the photometric re-rendering of a textured mesh ("Looking at the result"), written from
the definition, not from the kernels.  The key image of a view is raster_ref's (the contest of every face of the whole mesh at
cull = 0); the layout a rendered pixel reads from is texture_ref's.  A pixel is IEEE double in the definition's expression order
and one rounding; every count, sum and histogram bin is an integer.  The device results must equal run() byte for byte.

The batching model: the views are taken in batches of `batch` (0: all at once); the hit pixels of a batch are resolved as one flat
array and added to the per-view sums with np.add.at.  Nothing may depend on it.

run() also asserts, on every case it is given, the containment property: every atlas texel a rendered pixel reads with a weight
above 2^-40 is an own or gutter texel of the winning face's half cell (texture_ref.texel_map gives the owner of every texel).
"""
from __future__ import annotations

import math

import numpy as np

import raster_ref as R
import texture_ref as TR

DEFAULTS = dict(background=0)  # z_min has no default
CLASSES = ("empty", "back", "untextured", "own", "cross")
ARRAYS = ("rendered", "cls", "face", "classes", "stats", "hist")
PIXELS_MAX = 1 << 28
CONTAIN_W = 2.0 ** -40


def check_params(z_min=0.0, background=0):
    return bool(np.isfinite(z_min) and z_min > 0 and 0 <= background <= 255)


def key_image(X, F, cam, z_min, brute=False):
    """(projection, keys uint64 [h][w]) of the whole mesh at cull = 0"""
    w, h = int(cam["w"]), int(cam["h"])
    pr = R.project(X, cam, z_min)
    _, idx = R._classify(F, len(X), pr, 0)
    keys, _, _ = (R._contest_brute if brute else R._contest_boxes)(F, idx, pr, w, h)
    return pr, keys


def _winners(F, pr, keys, w):
    """per hit pixel of a view: its flat index, the winning face, back, t [3], s"""
    keys = keys.ravel()
    px = np.nonzero(keys != R.EMPTY)[0]
    fw = (keys[px] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    x, y = px % w, px // w
    dx, dy, Uj, Vj, _, _, rr = R._edges(F, fw, pr)
    ef = [(dx[:, i] * (R.SUB * y - Vj[:, i]) - dy[:, i] * (R.SUB * x - Uj[:, i])).astype(np.float64) for i in range(3)]
    _, _, U, V, _ = pr
    Uf, Vf = U[F[fw]], V[F[fw]]
    back = (Uf[:, 1] - Uf[:, 0]) * (Vf[:, 2] - Vf[:, 0]) - (Vf[:, 1] - Vf[:, 0]) * (Uf[:, 2] - Uf[:, 0]) > 0
    with np.errstate(all="ignore"):
        s = (ef[0] * rr[:, 0] + ef[1] * rr[:, 1]) + ef[2] * rr[:, 2]
        t = [ef[i] * rr[:, i] for i in range(3)]
    return px, fw, back, t, s


def lookup(t, s, uvh, atlas):
    """the rendered byte of pixels with barycentric products t [3] and s on faces whose corners in half-texels are uvh [k][3][2];
    also the four taps: (flat texel index int64 [k][4], weight f64 [k][4])"""
    A = np.asarray(atlas, np.uint8)
    H, W = A.shape
    Af = A.astype(np.float64)
    h = np.asarray(uvh, np.int32).astype(np.float64)
    hx = ((t[0] * h[:, 0, 0] + t[1] * h[:, 1, 0]) + t[2] * h[:, 2, 0]) / s
    hy = ((t[0] * h[:, 0, 1] + t[1] * h[:, 1, 1]) + t[2] * h[:, 2, 1]) / s
    a, b = hx * 0.5 - 0.5, hy * 0.5 - 0.5
    ac, bc = np.minimum(np.maximum(a, 0.0), float(W - 1)), np.minimum(np.maximum(b, 0.0), float(H - 1))
    x0, y0 = np.floor(ac), np.floor(bc)
    fx, fy = ac - x0, bc - y0
    xi0, yi0 = x0.astype(np.int64), y0.astype(np.int64)
    xi1, yi1 = np.minimum(xi0 + 1, W - 1), np.minimum(yi0 + 1, H - 1)
    top = (1.0 - fx) * Af[yi0, xi0] + fx * Af[yi0, xi1]
    bot = (1.0 - fx) * Af[yi1, xi0] + fx * Af[yi1, xi1]
    g = (1.0 - fy) * top + fy * bot
    out = np.minimum(255.0, np.floor(g + 0.5)).astype(np.uint8)
    taps = np.stack([yi0 * W + xi0, yi0 * W + xi1, yi1 * W + xi0, yi1 * W + xi1], 1)
    wts = np.stack([(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy], 1)
    return out, taps, wts


def foreign_weight(owner, fw, taps, wts):
    """the largest weight with which a pixel reads a texel that its winning face (fw [k]) does not own; 0.0 without one"""
    foreign = owner[taps] != fw[:, None]
    return float(np.where(foreign, wts, 0.0).max()) if len(fw) else 0.0


def run(verts, faces, cams, images, tex_views, tex, z_min, patch=8, fill=0, atlas=None, background=0, batch=0, brute=False, contain=True):
    """cams: the views; images: per view u8 [h][w] or None; tex_views: per view its index in the texture's view list or -1; tex:
    a texture result (texture_ref.run's dict or the device's: face_view, uv_half, W, H, cells, cells_per_row, view_faces) on this
    mesh, made with `patch` and `fill`; atlas: the levelled atlas, or None for tex's.
    dict(rendered u8 / cls u8 / face int32 [sum w h], classes int64 [Q][5], stats int64 [Q][2][3], hist int64 [Q][2][256],
    offsets int64 [Q + 1], foreign_weight); ValueError for every refusal of sfmx_photo_run."""
    if not check_params(z_min, background):
        raise ValueError("parameters")
    if tex is None:
        raise ValueError("the texture needs a successful run")
    X = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    n, m = len(X), len(F)
    fview, uvh = np.asarray(tex["face_view"]), np.asarray(tex["uv_half"])
    W, H = int(tex["W"]), int(tex["H"])
    if len(fview) != m or ("n" in tex and int(tex["n"]) != n):
        raise ValueError("the mesh of the texture's run")
    A = np.asarray(tex["atlas"] if atlas is None else atlas, np.uint8)
    if A.shape != (H, W):
        raise ValueError("the levelled atlas has another size")
    V = len(tex["view_faces"])
    Q = len(cams)
    assert len(images) == Q and len(tex_views) == Q
    if any(not -1 <= int(k) < V for k in tex_views):
        raise ValueError("tex_view outside [-1, V)")
    sizes = [int(c["w"]) * int(c["h"]) for c in cams]
    off = np.zeros(Q + 1, np.int64)
    off[1:] = np.cumsum(sizes, dtype=np.int64)
    if int(off[-1]) > PIXELS_MAX:
        raise ValueError("more than 2^28 pixels")
    if ((F < 0) | (F >= n)).any():
        raise ValueError("a face index outside [0, n)")
    total = int(off[-1])
    rendered, cls, face = np.full(total, int(background), np.uint8), np.zeros(total, np.uint8), np.full(total, -1, np.int32)
    classes, stats, hist = np.zeros((Q, 5), np.int64), np.zeros((Q, 2, 3), np.int64), np.zeros((Q, 2, 256), np.int64)
    owner = None
    if contain and m and W:
        lay = {k: int(tex[k]) for k in ("cells", "cells_per_row", "W", "H")}
        owner = TR.texel_map(fview, lay, patch)[0]
    worst = 0.0
    step = int(batch) if batch else max(Q, 1)
    for lo in range(0, Q, step):
        part = []
        for q in range(lo, min(lo + step, Q)):
            pr, keys = key_image(X, F, cams[q], z_min, brute)
            px, fw, back, t, s = _winners(F, pr, keys, int(cams[q]["w"]))
            part.append((np.full(len(px), q, np.int64), off[q] + px, fw, back, t, s))
        vq = np.concatenate([p[0] for p in part])
        at = np.concatenate([p[1] for p in part])
        fw = np.concatenate([p[2] for p in part])
        back = np.concatenate([p[3] for p in part])
        t = [np.concatenate([p[4][i] for p in part]) for i in range(3)]
        s = np.concatenate([p[5] for p in part])
        k = fview[fw] if m else np.zeros(0, np.int32)
        c = np.where(back, 1, np.where(k < 0, 2, np.where(k == np.asarray(tex_views, np.int64)[vq], 3, 4))).astype(np.uint8)
        out = np.where(c == 2, int(fill), int(background)).astype(np.uint8)
        sel = np.nonzero(c >= 3)[0]
        if len(sel):
            with np.errstate(all="ignore"):
                out[sel], taps, wts = lookup([ti[sel] for ti in t], s[sel], uvh[fw[sel]], A)
            if owner is not None:
                worst = max(worst, foreign_weight(owner, fw[sel], taps, wts))
        rendered[at], cls[at], face[at] = out, c, fw
        for q in range(lo, min(lo + step, Q)):
            mine = vq == q
            classes[q] = np.bincount(c[mine], minlength=5)
            classes[q, 0] += sizes[q] - int(mine.sum())
        has = np.array([images[q] is not None for q in range(Q)])
        sc = np.nonzero((c >= 3) & has[vq])[0]
        if len(sc):
            I = np.zeros(total, np.uint8)
            for q in range(lo, min(lo + step, Q)):
                if has[q]:
                    im = np.asarray(images[q], np.uint8)
                    assert im.shape == (int(cams[q]["h"]), int(cams[q]["w"]))
                    I[off[q]:off[q + 1]] = im.ravel()
            d = np.abs(out[sc].astype(np.int64) - I[at[sc]].astype(np.int64))
            o = (c[sc] - 3).astype(np.int64)
            np.add.at(stats, (vq[sc], o, 0), 1)
            np.add.at(stats, (vq[sc], o, 1), d)
            np.add.at(stats, (vq[sc], o, 2), d * d)
            np.add.at(hist, (vq[sc], o, d), 1)
    if contain:
        assert worst <= CONTAIN_W, f"a pixel reads a texel of another face with weight {worst!r} > 2^-40"
    return dict(rendered=rendered, cls=cls, face=face, classes=classes, stats=stats, hist=hist, offsets=off, foreign_weight=worst)


def view_image(res, cams, q, key="rendered"):
    return res[key][int(res["offsets"][q]):int(res["offsets"][q + 1])].reshape(int(cams[q]["h"]), int(cams[q]["w"]))


def same(a, b, what=""):
    """byte equality of two results"""
    for k in ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.tobytes() != y.tobytes():
            bad = np.argwhere(x != y)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} elements, first {bad[0].tolist()}: {x[tuple(bad[0])]!r} != {y[tuple(bad[0])]!r}")


def measures(stats3, hist256):
    """count, MAE, RMSE, PSNR and the 90th percentile (the smallest d with 10 cum(d) >= 9 count) from the integers"""
    cnt, sd, sd2 = (int(v) for v in stats3)
    if cnt == 0:
        return dict(count=0, mae=None, rmse=None, psnr=None, p90=None)
    cum = np.cumsum(np.asarray(hist256, np.int64))
    return dict(count=cnt, mae=sd / cnt, rmse=math.sqrt(sd2 / cnt), psnr=float("inf") if sd2 == 0 else 10.0 * math.log10(65025.0 * cnt / sd2),
                p90=int(np.nonzero(10 * cum >= 9 * cnt)[0][0]))


def pooled(res, views, o):
    """measures of own (o = 0) or cross (o = 1) pooled over the listed views"""
    views = list(views)
    return measures(res["stats"][views, o].sum(0), res["hist"][views, o].sum(0))


def pgm(img):
    """the bytes of a binary PGM of u8 [h][w]"""
    img = np.ascontiguousarray(img, np.uint8)
    return b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes()


BAD_PARAMS = (dict(z_min=0.0), dict(z_min=-1.0), dict(z_min=float("nan")), dict(z_min=float("inf")), dict(z_min=-0.0))
GOOD_PARAMS = (dict(z_min=1.0), dict(z_min=5e-324), dict(z_min=1.7e308), dict(z_min=0.5, background=255))


# ---- test scenes -------------------------------------------------------------------------------------------------------------
def aligned_face(S, x0=1, y0=1, w=None, h=None, seed=3):
    """(verts, faces, cam, image): one front-facing face under raster_ref.pixel_camera whose corners lie on the pixel centres
    (x0, y0), (x0, y0 + L), (x0 + L, y0) at depth 1, L = S - 2: pixel (x0 + i, y0 + j) is the centre of texel (j, i) of the
    face's half, so a render from that camera reads single texels"""
    L = S - 2
    w, h = w or x0 + L + 2, h or y0 + L + 2
    v = R.at_pixels([(x0, y0), (x0, y0 + L), (x0 + L, y0)])
    img = np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)
    return v, np.array([[0, 1, 2]], np.int32), R.pixel_camera(w, h), img


def five_classes(S=4):
    """(verts, faces, tex_cams, tex_images, photo_cams, photo_images, tex_views): face 0 in front of the texture camera (8 x 8),
    face 1 outside its image and inside the photo cameras' (24 x 8), face 2 back-facing; the first photo view is the texture
    camera widened (own), the second the same camera held out (cross)"""
    v = R.at_pixels([(1, 1), (1, 6), (6, 1), (10, 1), (10, 6), (15, 1), (17, 1), (22, 1), (17, 6)])
    f = np.arange(9, dtype=np.int32).reshape(3, 3)
    rng = np.random.default_rng(5)
    tcam, pcam = R.pixel_camera(8, 8), R.pixel_camera(24, 8)
    timg = rng.integers(0, 256, (8, 8)).astype(np.uint8)
    pimg = rng.integers(0, 256, (8, 24)).astype(np.uint8)
    return v, f, [tcam], [timg], [pcam, pcam], [pimg, pimg], [0, -1]


def quilt(nx, ny, size=5.0, seed=0):
    """(verts, faces): nx x ny disjoint front-facing quads of two faces each, one per size x size cell of pixels, their corners
    jittered off the pixel centres, every quad at its own depth: every face is seen whole and none occludes another"""
    rng = np.random.default_rng(seed)
    q = np.arange(nx * ny)
    org = np.stack([(q % nx) * size, (q // nx) * size], 1)[:, None, :]
    lo, hi = rng.uniform(0.1, 0.9, (nx * ny, 4, 2)), rng.uniform(size - 1.9, size - 1.1, (nx * ny, 4, 2))
    pick = np.array([[0, 0], [0, 1], [1, 1], [1, 0]])[None]  # down the left side first: front-facing
    c = org + np.where(pick == 0, lo, hi)
    v = R.at_pixels(c.reshape(-1, 2), np.repeat(rng.uniform(1.0, 2.0, nx * ny), 4))
    b = 4 * q
    f = np.stack([np.stack([b, b + 1, b + 2], 1), np.stack([b, b + 2, b + 3], 1)], 1).reshape(-1, 3)
    return v, np.ascontiguousarray(f, np.int32)


def strips(m, w=64, seed=9):
    """m faces, two to a quad around a pixel centre (its corners snap into that pixel, so every face is seen), row after row of a
    w-wide image, at random depths per quad: (verts, faces, h)"""
    quads = (m + 1) // 2
    h = (quads + w - 1) // w
    q = np.arange(quads)
    x, y = (q % w).astype(np.float64), (q // w).astype(np.float64)
    o = 0.375
    c = np.stack([np.stack([x - o, y - o], 1), np.stack([x - o, y + o], 1), np.stack([x + o, y + o], 1), np.stack([x + o, y - o], 1)], 1)
    z = np.repeat(np.random.default_rng(seed).uniform(1.0, 2.0, quads), 4)
    v = R.at_pixels(c.reshape(-1, 2), z)
    b = 4 * q
    f = np.stack([np.stack([b, b + 1, b + 2], 1), np.stack([b, b + 2, b + 3], 1)], 1).reshape(-1, 3)[:m]
    return v, np.ascontiguousarray(f, np.int32), h
