"""NumPy restatement of the exact z-buffer ("Rendering the surface"), written from the definition, not from the
kernels.

Two forms of the same definition:
 * brute()   tests every face against every pixel of the image (in slabs of faces) and keeps the smallest key per pixel;
 * render()  walks each face's box of pixel centres, all (face, pixel) candidates of a batch of faces as one flat array.
They share the projection and the per-pixel resolve (a function of the winning face alone) and differ in everything that decides
which fragments exist and which one wins.  All floating point is IEEE double in the definition's expression order, except the one
rounding to float that forms the key.  The device results must equal brute() byte for byte.
"""
from __future__ import annotations

import numpy as np

import raycast_ref as RR

COUNTS = ("faces_behind", "faces_outside", "faces_degenerate", "faces_back", "faces_culled", "faces_drawn", "hits", "back_pixels")
ARRAYS = ("depth", "face", "points", "normals", "shaded")
DEFAULTS = dict(cull=0, background=0)  # z_min has no default
BAND = 16384.0
SUB = 256
W_MAX, WH_MAX, N_MAX, M_MAX = 4096, 1 << 24, 1 << 24, 1 << 30
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def check_params(z_min=0.0, cull=0, background=0):
    return bool(np.isfinite(z_min) and z_min > 0 and cull in (0, 1, 2) and 0 <= background <= 255)


def project(verts, cam, z_min):
    """near, inband (bool [n]), U, V (int64 [n], 0 where not inband), r (f64 [n], 0 where not inband)"""
    X = np.asarray(verts, np.float64).reshape(-1, 3)
    R = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    f, cx, cy = float(cam["f"]), float(cam["cx"]), float(cam["cy"])
    with np.errstate(all="ignore"):
        p = [X[:, a] - c[a] for a in range(3)]
        q = [(R[r, 0] * p[0] + R[r, 1] * p[1]) + R[r, 2] * p[2] for r in range(3)]
        near = q[2] >= float(z_min)
        u = (f * q[0]) / q[2] + cx
        v = (f * q[1]) / q[2] + cy
        inband = near & (np.abs(u) <= BAND) & (np.abs(v) <= BAND)
        U = np.where(inband, np.floor(np.where(inband, u, 0.0) * 256.0 + 0.5), 0.0).astype(np.int64)
        V = np.where(inband, np.floor(np.where(inband, v, 0.0) * 256.0 + 0.5), 0.0).astype(np.int64)
        r = np.where(inband, 1.0 / np.where(inband, q[2], 1.0), 0.0)
    return near, inband, U, V, r


def _classify(faces, n, pr, cull):
    """the counts of the face classes and, for the faces that are rasterised: their indices and oriented edge functions"""
    near, inband, U, V, r = pr
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    if ((F < 0) | (F >= n)).any():
        raise ValueError("a face index outside [0, n)")
    nf = near[F].all(1)
    ib = inband[F].all(1)
    behind = ~nf
    outside = nf & ~ib
    ok = nf & ib
    Uf, Vf = U[F], V[F]
    A = (Uf[:, 1] - Uf[:, 0]) * (Vf[:, 2] - Vf[:, 0]) - (Vf[:, 1] - Vf[:, 0]) * (Uf[:, 2] - Uf[:, 0])
    degenerate = ok & (A == 0)
    ok &= A != 0
    back = ok & (A > 0)
    culled = ok & ((back & (cull == 1)) | (~back & (cull == 2)))
    counts = dict(faces_behind=int(behind.sum()), faces_outside=int(outside.sum()), faces_degenerate=int(degenerate.sum()),
                  faces_back=int(back.sum()), faces_culled=int(culled.sum()))
    idx = np.nonzero(ok & ~culled)[0]
    return counts, idx


def _edges(F, idx, pr):
    """per rasterised face: dx, dy, Uj, Vj int64 [k][3], own bool [k][3], absA int64 [k], r f64 [k][3]"""
    _, _, U, V, r = pr
    Fi = F[idx]
    Uf, Vf = U[Fi], V[Fi]
    A = (Uf[:, 1] - Uf[:, 0]) * (Vf[:, 2] - Vf[:, 0]) - (Vf[:, 1] - Vf[:, 0]) * (Uf[:, 2] - Uf[:, 0])
    sg = np.sign(A)
    j, k = [1, 2, 0], [2, 0, 1]
    dx = sg[:, None] * (Uf[:, k] - Uf[:, j])
    dy = sg[:, None] * (Vf[:, k] - Vf[:, j])
    own = (dy < 0) | ((dy == 0) & (dx > 0))
    return dx, dy, Uf[:, j], Vf[:, j], own, np.abs(A), r[Fi]


def _keys(depth, face):
    """(bits((float)depth) << 32) | face"""
    with np.errstate(over="ignore"):
        bits = depth.astype(np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | face.astype(np.uint64)


def _contest_brute(F, idx, pr, w, h, slab=None):
    """keys uint64 [h][w], fragments, faces_drawn: every face against every pixel"""
    dx, dy, Uj, Vj, own, absA, r = _edges(F, idx, pr)
    keys = np.full((h, w), EMPTY, np.uint64)
    X = (SUB * np.arange(w, dtype=np.int64))[None, None, :]
    Y = (SUB * np.arange(h, dtype=np.int64))[None, :, None]
    fragments = drawn = 0
    slab = slab or max(1, (1 << 21) // (w * h))
    for lo in range(0, len(idx), slab):
        s_ = slice(lo, lo + slab)
        cov = np.ones((len(idx[s_]), h, w), bool)
        e = []
        for i in range(3):
            ei = dx[s_, i, None, None] * (Y - Vj[s_, i, None, None]) - dy[s_, i, None, None] * (X - Uj[s_, i, None, None])
            cov &= (ei > 0) | ((ei == 0) & own[s_, i, None, None])
            e.append(ei.astype(np.float64))
        with np.errstate(all="ignore"):
            s = (e[0] * r[s_, 0, None, None] + e[1] * r[s_, 1, None, None]) + e[2] * r[s_, 2, None, None]
            depth = absA[s_, None, None].astype(np.float64) / s
        k = np.where(cov, _keys(depth, np.broadcast_to(idx[s_, None, None], depth.shape)), EMPTY)
        keys = np.minimum(keys, k.min(0))
        fragments += int(cov.sum())
        drawn += int(cov.any((1, 2)).sum())
    return keys, fragments, drawn


def boxes(F, idx, pr, w, h):
    """x0, y0, x1, y1 int64 [k] of the rasterised faces: the pixel centres inside the snapped bounding box and the image (empty
    when x1 < x0 or y1 < y0)"""
    _, _, U, V, _ = pr
    Uf, Vf = U[F[idx]], V[F[idx]]
    x0 = np.maximum(-((-Uf.min(1)) // SUB), 0)
    y0 = np.maximum(-((-Vf.min(1)) // SUB), 0)
    x1 = np.minimum(Uf.max(1) // SUB, w - 1)
    y1 = np.minimum(Vf.max(1) // SUB, h - 1)
    return x0, y0, x1, y1


def _contest_boxes(F, idx, pr, w, h, batch=1 << 22):
    """the same from each face's box of pixel centres"""
    dx, dy, Uj, Vj, own, absA, r = _edges(F, idx, pr)
    x0, y0, x1, y1 = boxes(F, idx, pr, w, h)
    bw, bh = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    cnt = bw * bh
    keys = np.full(w * h, EMPTY, np.uint64)
    fragments = drawn = 0
    live = np.nonzero(cnt > 0)[0]
    cum = np.cumsum(cnt[live])
    lo = 0
    while lo < len(live):
        base = cum[lo - 1] if lo else 0
        hi = max(lo + 1, int(np.searchsorted(cum, base + batch, "right")))
        sel = live[lo:hi]
        c = cnt[sel]
        k = np.repeat(np.arange(len(sel)), c)        # candidate -> position in sel
        local = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        g = sel[k]
        x = x0[g] + local % bw[g]
        y = y0[g] + local // bw[g]
        cov = np.ones(len(g), bool)
        e = []
        for i in range(3):
            ei = dx[g, i] * (SUB * y - Vj[g, i]) - dy[g, i] * (SUB * x - Uj[g, i])
            cov &= (ei > 0) | ((ei == 0) & own[g, i])
            e.append(ei.astype(np.float64))
        with np.errstate(all="ignore"):
            s = (e[0] * r[g, 0] + e[1] * r[g, 1]) + e[2] * r[g, 2]
            depth = absA[g].astype(np.float64) / s
        kk = _keys(depth[cov], idx[g[cov]])
        np.minimum.at(keys, (y[cov] * w + x[cov]), kk)
        fragments += int(cov.sum())
        drawn += len(np.unique(g[cov]))
        lo = hi
    return keys.reshape(h, w), fragments, drawn


def _resolve(verts, F, normals, grey, cam, pr, keys, w, h, background):
    X = np.asarray(verts, np.float64).reshape(-1, 3)
    _, _, U, V, r = pr
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    n = w * h
    keys = keys.ravel()
    hit = keys != EMPTY
    px = np.nonzero(hit)[0]
    fw = (keys[px] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    x, y = px % w, px // w
    dx, dy, Uj, Vj, _, absA, rr = _edges(F, fw, pr)
    e = [dx[:, i] * (SUB * y - Vj[:, i]) - dy[:, i] * (SUB * x - Uj[:, i]) for i in range(3)]
    ef = [v.astype(np.float64) for v in e]
    Fi = F[fw]
    Uf, Vf = U[Fi], V[Fi]
    back = (Uf[:, 1] - Uf[:, 0]) * (Vf[:, 2] - Vf[:, 0]) - (Vf[:, 1] - Vf[:, 0]) * (Uf[:, 2] - Uf[:, 0]) > 0
    with np.errstate(all="ignore"):
        s = (ef[0] * rr[:, 0] + ef[1] * rr[:, 1]) + ef[2] * rr[:, 2]
        d = absA.astype(np.float64) / s
        dw = [v.ravel()[px] for v in RR.rays(cam, w, h)]
        P = [c[a] + d * dw[a] for a in range(3)]
        t = [ef[i] * rr[:, i] for i in range(3)]
        if normals is None:
            A_ = [X[Fi[:, 1], a] - X[Fi[:, 0], a] for a in range(3)]
            B_ = [X[Fi[:, 2], a] - X[Fi[:, 0], a] for a in range(3)]
            N = [A_[1] * B_[2] - A_[2] * B_[1], A_[2] * B_[0] - A_[0] * B_[2], A_[0] * B_[1] - A_[1] * B_[0]]
        else:
            Nv = np.asarray(normals, np.float64).reshape(-1, 3)
            N = [(t[0] * Nv[Fi[:, 0], a] + t[1] * Nv[Fi[:, 1], a]) + t[2] * Nv[Fi[:, 2], a] for a in range(3)]
        ln = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
        nr = [np.where(ln > 0, N[a] / ln, 0.0) for a in range(3)]
        L = np.sqrt((dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2])
        lam = -(((nr[0] * dw[0] + nr[1] * dw[1]) + nr[2] * dw[2]) / L)
        sh = np.where(lam > 0, np.minimum(255.0, np.floor(lam * 255.0 + 0.5)), 0.0).astype(np.uint8)
    depth, face = np.zeros(n), np.full(n, -1, np.int32)
    points, nrm, shaded = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, int(background), np.uint8)
    depth[px], face[px], shaded[px] = d, fw, sh
    for a in range(3):
        points[px, a] = P[a]
        nrm[px, a] = nr[a]
    out = dict(depth=depth.reshape(h, w), face=face.reshape(h, w), points=points.reshape(h, w, 3), normals=nrm.reshape(h, w, 3),
               shaded=shaded.reshape(h, w), hits=len(px), back_pixels=int(back.sum()))
    if grey is not None:
        G = np.asarray(grey, np.uint8).astype(np.float64)
        with np.errstate(all="ignore"):
            g = ((t[0] * G[Fi[:, 0]] + t[1] * G[Fi[:, 1]]) + t[2] * G[Fi[:, 2]]) / s
            gv = np.minimum(255.0, np.floor(g + 0.5)).astype(np.uint8)
        go = np.full(n, int(background), np.uint8)
        go[px] = gv
        out["grey"] = go.reshape(h, w)
    return out


def _run(contest, verts, faces, cam, z_min, normals, grey, w, h, cull, background):
    w, h = int(cam["w"] if w is None else w), int(cam["h"] if h is None else h)
    n = len(np.asarray(verts).reshape(-1, 3))
    assert check_params(z_min, cull, background) and 1 <= w <= W_MAX and h >= 1 and w * h <= WH_MAX and n < N_MAX
    pr = project(verts, cam, z_min)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    counts, idx = _classify(F, n, pr, cull)
    keys, fragments, drawn = contest(F, idx, pr, w, h)
    out = _resolve(verts, F, normals, grey, cam, pr, keys, w, h, background)
    out.update(counts, fragments=fragments, faces_drawn=drawn, keys=keys)
    return out


def brute(verts, faces, cam, z_min, normals=None, grey=None, w=None, h=None, cull=0, background=0):
    """every face against every pixel.  dict(depth [h][w], face int32 [h][w], points / normals [h][w][3], shaded u8 [h][w], grey
    u8 [h][w] with grey, the COUNTS, fragments, keys uint64 [h][w]); ValueError for a face index outside [0, n)"""
    return _run(_contest_brute, verts, faces, cam, z_min, normals, grey, w, h, cull, background)


def render(verts, faces, cam, z_min, normals=None, grey=None, w=None, h=None, cull=0, background=0):
    """brute()'s result from the faces' boxes"""
    return _run(_contest_boxes, verts, faces, cam, z_min, normals, grey, w, h, cull, background)


def counts(ref):
    return {k: int(ref[k]) for k in COUNTS + ("fragments",)}


def same(a, b, what=""):
    """byte equality of two results (arrays, grey when either has it, counts)"""
    assert counts(a) == counts(b), (what, counts(a), counts(b))
    assert ("grey" in a) == ("grey" in b), what
    for k in ARRAYS + (("grey",) if "grey" in a else ()):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.tobytes() != y.tobytes():
            bad = np.argwhere(x.view(np.uint64 if x.dtype == np.float64 else x.dtype) != y.view(np.uint64 if y.dtype == np.float64 else y.dtype))
            raise AssertionError(f"{what}: {k} differs at {len(bad)} elements, first {bad[0].tolist()}: {x[tuple(bad[0])]!r} != {y[tuple(bad[0])]!r}")


def fragments_per_pixel(verts, faces, cam, z_min, w=None, h=None, cull=0):
    """int [h][w]: the fragments at every pixel (brute form)"""
    w, h = int(cam["w"] if w is None else w), int(cam["h"] if h is None else h)
    pr = project(verts, cam, z_min)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    _, idx = _classify(F, len(pr[0]), pr, cull)
    dx, dy, Uj, Vj, own, _, _ = _edges(F, idx, pr)
    X = (SUB * np.arange(w, dtype=np.int64))[None, None, :]
    Y = (SUB * np.arange(h, dtype=np.int64))[None, :, None]
    out = np.zeros((h, w), np.int64)
    slab = max(1, (1 << 21) // (w * h))
    for lo in range(0, len(idx), slab):
        s_ = slice(lo, lo + slab)
        cov = np.ones((len(idx[s_]), h, w), bool)
        for i in range(3):
            ei = dx[s_, i, None, None] * (Y - Vj[s_, i, None, None]) - dy[s_, i, None, None] * (X - Uj[s_, i, None, None])
            cov &= (ei > 0) | ((ei == 0) & own[s_, i, None, None])
        out += cov.sum(0)
    return out


# ---- test scenes -------------------------------------------------------------------------------------------------------------
# the calibration of DESIGN.md 23: a level-4 icosphere of radius 0.1 (2 562 v / 5 120 f, faces outward), f 300, 160 x 160
CALIB_Z_MIN = 0.05
CALIB = {
    "axis": dict(cam=lambda: RR.axis_camera((0.0, 0.0, -0.5), 300.0, 160, 160, 80.0, 80.0), hits=11769, faces_back=3086),
    "oblique": dict(cam=lambda: RR.camera((0.31, 0.22, -0.33), (0.0, 0.0, 0.0), 300.0, 160, 160), hits=11605, faces_back=3074),
}


def permute_faces(faces, seed):
    """(faces in another order, perm): new face i is old face perm[i]"""
    perm = np.random.default_rng(seed).permutation(len(faces))
    return np.ascontiguousarray(np.asarray(faces)[perm]), perm


def rotate_corners(faces, seed):
    """every face starting at another (random) corner, never reflected"""
    f = np.asarray(faces)
    rot = np.random.default_rng(seed).integers(0, 3, len(f))
    return np.ascontiguousarray(np.stack([f[np.arange(len(f)), (rot + j) % 3] for j in range(3)], 1))


def pixel_camera(w, h, f=256.0, cx=0.0, cy=0.0):
    """R = I at the origin: the point (x, y, 1) f / f ... a vertex (u / f, v / f, 1) lands on image position (u, v) when cx = cy =
    0, so with f a power of two snapped coordinates are known by construction"""
    return RR.axis_camera((0.0, 0.0, 0.0), f, w, h, cx, cy)


def at_pixels(uv, z=1.0, f=256.0):
    """world vertices (R = I, c = 0, cx = cy = 0) whose image positions are uv [n][2] at depth z (scalar or [n])"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(uv),))
    return np.stack([uv[:, 0] * z / f, uv[:, 1] * z / f, z], 1)


def tiny_faces(count, w, h, size=0.75, seed=21, f=256.0):
    """`count` disjoint faces, each inside its own pixel-sized cell of a w x h image (cells reused row by row when count exceeds
    w * h: then faces overlap in the image at different depths): sub-pixel and few-pixel faces, random orientation and depth"""
    rng = np.random.default_rng(seed)
    cell = np.arange(count) % (w * h)
    cxy = np.stack([cell % w, cell // w], 1).astype(np.float64)
    tri = cxy[:, None, :] + rng.uniform(-size, size, (count, 3, 2))
    z = np.repeat(rng.uniform(1.0, 2.0, count), 3)
    v = at_pixels(tri.reshape(-1, 2), z, f)
    return v, np.arange(3 * count, dtype=np.int32).reshape(count, 3)


def _tri(uv, z=1.0):
    return at_pixels(uv, z), np.arange(len(uv), dtype=np.int32).reshape(-1, 3)


def hand_cases():
    """name -> dict(verts, faces, w, h, z_min): pixel_camera scenes (f = 256, cx = cy = 0, so a vertex built by at_pixels at
    depth 1 snaps to exactly 256 times its pixel coordinates)"""
    out = {}

    def add(name, verts, faces, w=8, h=8, z_min=0.5):
        out[name] = dict(verts=np.ascontiguousarray(verts, np.float64), faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3), w=w, h=h,
                         z_min=z_min)

    # the worked check and its mirror images: top and left edges own their centres, right, bottom and slanted-down ones do not;
    # both windings cover the same pixels
    add("top-left", *_tri([(2, 2), (6, 2), (2, 6)]))
    add("top-left-reversed", *_tri([(2, 2), (2, 6), (6, 2)]))
    add("bottom-right", *_tri([(6, 6), (2, 6), (6, 2)]))
    add("bottom-right-reversed", *_tri([(6, 6), (6, 2), (2, 6)]))
    # a quad split along a diagonal through pixel centres, and the other diagonal
    q = [(1, 1), (7, 1), (7, 7), (1, 7)]
    add("shared-diagonal", at_pixels(q), [[0, 1, 2], [0, 2, 3]])
    add("shared-antidiagonal", at_pixels(q), [[0, 1, 3], [1, 2, 3]])
    add("shared-diagonal-mixed-winding", at_pixels(q), [[0, 1, 2], [0, 3, 2]])
    # six faces around a vertex on the centre (4, 4), rim vertices on and off centres
    rim = [(7, 4), (6, 7), (2, 7), (1, 4), (2.5, 1), (6, 1.25)]
    add("fan", at_pixels([(4, 4)] + rim), [[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)])
    add("no-centre", *_tri([(2.2, 2.2), (2.8, 2.3), (2.4, 2.9)]))
    add("degenerate", at_pixels([(1, 1), (2, 2), (3, 3), (2.001, 2.0005), (5, 1), (5, 1)]),
        [[0, 1, 2], [0, 3, 2], [0, 1, 1], [0, 4, 5], [4, 0, 2]])
    # z_min = 0.5: a vertex exactly there is near, one just below is not
    v, f = _tri([(1, 1), (6, 1), (1, 6), (1, 1), (6, 1), (1, 6)], z=[0.5, 1.0, 1.0, np.nextafter(0.5, 0.0), 1.0, 1.0])
    add("z-min", v, f)
    # |u| = 16384 exactly is inband (and the face covers the whole image from the tiled path), one ulp past it is not
    big = np.array([(-16384.0, -16384.0), (16384.0, -16384.0), (0.0, 16384.0)])
    v = at_pixels(np.concatenate([big, big]), z=[1.0, 1.0, 1.0, 2.0, 2.0, 2.0])
    v[4, 0] = np.nextafter(v[4, 0], np.inf)
    add("band", v, [[0, 1, 2], [3, 4, 5]], w=12, h=10)
    v, f = _tri([(1, 1), (6, 1), (1, 6)] * 4)
    v[3, 0], v[7, 1], v[11, 2] = np.nan, np.inf, -np.inf
    add("non-finite", v, f)
    add("coplanar-copies", *_tri([(1, 1), (1, 7), (7, 1)] * 2))
    # depths 1 + 2^-30 and 1 round to one float: face 0, the farther, wins; 1 + 2^-22 and 1 do not: face 1, the nearer, wins
    t = [(1, 1), (1, 7), (7, 1)]
    add("same-float", *_tri(t * 2, z=[1.0 + 2.0 ** -30] * 3 + [1.0] * 3))
    add("neighbouring-floats", *_tri(t * 2, z=[1.0 + 2.0 ** -22] * 3 + [1.0] * 3))
    # a back face (A > 0) at depth 1 in front of a front face at depth 2
    add("back-before-front", *_tri([(2, 2), (6, 2), (2, 6), (0, 0), (0, 7.5), (7.5, 0)], z=[1.0] * 3 + [2.0] * 3))
    add("no-faces", np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    add("no-faces-some-verts", at_pixels([(1, 1), (2, 2)]), np.zeros((0, 3), np.int32))
    # boxes of SMALL - 1, SMALL and SMALL + 1 = 63, 64, 65 pixel centres
    for name, (bw, bh) in (("box-63", (7, 9)), ("box-64", (8, 8)), ("box-65", (5, 13))):
        add(name, *_tri([(3, 2), (3 + bw - 1, 2), (3, 2 + bh - 1)]), w=20, h=20)
    # tiled faces partly off each border, and one over all of them
    add("off-borders", *_tri([(-9, 5), (12, 3), (4, 22), (30, -7), (47, 12), (25, 14), (10, 20), (33, 41), (-4, 36), (-30, -30), (90, 4), (3, 80)],
                             z=[1.0] * 9 + [1.5] * 3), w=40, h=30)
    return out


def hand_camera(case):
    return pixel_camera(case["w"], case["h"])


def random_scene(w, h, count=40, seed=0):
    """triangles of every size over (and past) a w x h image, each vertex at its own depth: (verts, faces, normals, grey)"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    m = 6.0
    big = rng.uniform((-m, -m), (w + m, h + m), (count, 3, 2))
    c = rng.uniform((0, 0), (w, h), (count, 1, 2))
    small = c + rng.uniform(-1.5, 1.5, (count, 3, 2))
    uv = np.concatenate([big, small]).reshape(-1, 2)
    v = at_pixels(uv, rng.uniform(1.0, 2.0, len(uv)))
    f = np.arange(len(uv), dtype=np.int32).reshape(-1, 3)
    return v, f, rng.standard_normal(v.shape), rng.integers(0, 256, len(v)).astype(np.uint8)


def hot_pixel(m=65536, seed=31):
    """m faces that all cover the centre (3, 3) of an 8 x 8 image, at random depths"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi, m)[:, None] + np.array([0.0, 2.1, 4.2])[None, :] + rng.uniform(-0.3, 0.3, (m, 3))
    rad = rng.uniform(0.6, 2.5, (m, 3))
    uv = np.stack([3.0 + rad * np.cos(a), 3.0 + rad * np.sin(a)], -1).reshape(-1, 2)
    v = at_pixels(uv, np.repeat(rng.uniform(1.0, 2.0, m), 3))
    return v, np.arange(3 * m, dtype=np.int32).reshape(m, 3)


BAD_PARAMS = (dict(z_min=0.0), dict(z_min=-1.0), dict(z_min=float("nan")), dict(z_min=float("inf")), dict(z_min=-0.0),
              dict(z_min=1.0, cull=3), dict(z_min=1.0, cull=-1))
GOOD_PARAMS = (dict(z_min=1.0), dict(z_min=5e-324), dict(z_min=1.7e308), dict(z_min=0.5, cull=1), dict(z_min=0.5, cull=2, background=255))
