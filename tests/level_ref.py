"""NumPy restatement of the seam levelling of a texture atlas ("Levelling the seams"), written from the definition,
not from the kernels, on top of texture_ref (the best views, the layout, the texel map and the texel points).  Nodes, views of a
vertex and neighbours are sets; a node sample and a texel are IEEE double in the definition's expression order; every sum is an
integer and every integer division a floor division.  The device results must equal run() byte for byte.
"""
from __future__ import annotations

import numpy as np

import texture_ref as TR

DEFAULTS = dict(iterations=64)
ITER_MAX = 65536
COUNTS = ("nodes", "seam_vertices", "pinned_nodes", "free_nodes", "node_edges", "iterations")
ARRAYS = ("atlas", "corner_adj", "corner_sample", "vertex_views")
G_MAX = 65280  # |g| <= 255 * 256

BAD_PARAMS = (dict(iterations=-1), dict(iterations=ITER_MAX + 1), dict(iterations=-2 ** 31))
GOOD_PARAMS = (dict(iterations=0), dict(iterations=1), dict(iterations=64), dict(iterations=ITER_MAX))


def check_params(iterations=64):
    return bool(0 <= iterations <= ITER_MAX)


def graw(X, cam, img):
    """(g f64 [k], ok bool [k]): texture_ref.sample's sequence up to g, not rounded"""
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
    return g, ok


def graph(F, face_view, V):
    """the nodes and their edges: dict(node_v, node_k int64 [N], corner_node int64 [m][3] (-1 on an untextured face), lo, hi int64 [E])"""
    tex = np.nonzero(face_view >= 0)[0]
    key = (F[tex] * int(V) + face_view[tex].astype(np.int64)[:, None]).ravel()
    uniq, inv = np.unique(key, return_inverse=True)
    corner_node = np.full((len(F), 3), -1, np.int64)
    corner_node[tex] = inv.reshape(-1, 3)
    N = len(uniq)
    cn = corner_node[tex]
    a = np.concatenate([cn[:, 0], cn[:, 1], cn[:, 2]])
    b = np.concatenate([cn[:, 1], cn[:, 2], cn[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    e = np.unique(lo[lo != hi] * max(N, 1) + hi[lo != hi])
    return dict(node_v=uniq // int(V), node_k=uniq % int(V), corner_node=corner_node, lo=e // max(N, 1), hi=e % max(N, 1))


def sweep(g, free, lo, hi, deg):
    """one Jacobi sweep, int64 [N]: every free node gets (2 sum + deg) // (2 deg) over its neighbours' g"""
    n = len(g)  # the float64 sums are exact: |g| <= 65 280 and far fewer than 2^36 terms
    s = (np.bincount(lo, g[hi].astype(np.float64), n) + np.bincount(hi, g[lo].astype(np.float64), n)).astype(np.int64)
    d = np.maximum(deg, 1)
    move = free & (deg > 0)
    return np.where(move, (2 * s + d) // (2 * d), g)


def solve(fx, node_v, n, lo, hi, iterations, history=False):
    """(g int64 [N] after the sweeps, pinned bool [N], vertex_views int64 [n], target int64 [n]); with history the list of all g^t"""
    vv = np.bincount(node_v, minlength=n).astype(np.int64)
    sums = np.zeros(n, np.int64)
    np.add.at(sums, node_v, fx)
    seam = vv >= 2
    c = np.maximum(vv, 1)
    target = np.where(seam, (2 * sums + c) // (2 * c), 0)
    pinned = seam[node_v] if len(node_v) else np.zeros(0, bool)
    g = np.where(pinned, target[node_v] - fx, 0).astype(np.int64)
    deg = np.bincount(np.concatenate([lo, hi]), minlength=len(fx)).astype(np.int64)
    hist = [g]
    for _ in range(int(iterations)):
        g = sweep(g, ~pinned, lo, hi, deg)
        if history:
            hist.append(g)
    return (hist if history else g), pinned, vv, target


def run(verts, faces, cams, images, tex, iterations=64, patch=8, fill=0):
    """tex: texture_ref.run's result on this mesh with this patch and fill.  dict(atlas u8 [H][W], corner_adj int32 [m][3],
    corner_sample int32 [m][3], vertex_views int32 [n], the COUNTS); ValueError for parameters outside their range"""
    if not check_params(iterations):
        raise ValueError("parameters")
    X = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    n, m, V = len(X), len(F), len(cams)
    fv = np.asarray(tex["face_view"], np.int32)
    assert len(fv) == m
    S, L = int(patch), int(patch) - 2
    lay = {k: int(tex[k]) for k in ("cells", "cells_per_row", "W", "H")}
    G = graph(F, fv, V)
    node_v, node_k = G["node_v"], G["node_k"]
    N = len(node_v)
    fx = np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        for k in np.unique(node_k):
            sel = np.nonzero(node_k == k)[0]
            P = [(float(L) * X[node_v[sel], r]) / float(L) for r in range(3)]
            g, ok = graw(P, cams[k], images[k])
            fx[sel] = np.where(ok, np.floor(np.where(ok, g, 0.0) * 256.0 + 0.5), 256.0 * fill).astype(np.int64)
    g, pinned, vv, _ = solve(fx, node_v, n, G["lo"], G["hi"], iterations)
    cn = G["corner_node"]
    texd = cn[:, 0] >= 0 if m else np.zeros(0, bool)
    cadj, csamp = np.zeros((m, 3), np.int64), np.zeros((m, 3), np.int64)
    cadj[texd] = g[cn[texd]]
    csamp[texd] = fx[cn[texd]]
    # the atlas: texture_ref.bake with the blend of the corner offsets added before the rounding
    W, H = lay["W"], lay["H"]
    face, i, j = TR.texel_map(fv, lay, S)
    atlas = np.full(W * H, int(fill), np.uint8)
    view = np.where(face >= 0, fv[np.maximum(face, 0)], -1)
    for k in np.unique(view[view >= 0]):
        sel = np.nonzero(view == k)[0]
        P = TR.texel_points(X, F, face[sel], i[sel], j[sel], S)
        gr, ok = graw(P, cams[k], images[k])
        i2, j2 = TR.gutter(S, i[sel], j[sel])
        A = cadj[face[sel]]
        Nn = (L - i2 - j2) * A[:, 0] + i2 * A[:, 1] + j2 * A[:, 2]
        with np.errstate(all="ignore"):
            t = np.minimum(255.0, np.maximum(0.0, np.floor((np.where(ok, gr, 0.0) + Nn.astype(np.float64) / float(256 * L)) + 0.5)))
        atlas[sel] = np.where(ok, t, float(fill)).astype(np.uint8)
    return dict(atlas=atlas.reshape(H, W), corner_adj=cadj.astype(np.int32), corner_sample=csamp.astype(np.int32),
                vertex_views=vv.astype(np.int32), nodes=N, seam_vertices=int((vv >= 2).sum()), pinned_nodes=int(pinned.sum()),
                free_nodes=int(N - pinned.sum()), node_edges=len(G["lo"]), iterations=int(iterations))


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


# ---- the seam step ---------------------------------------------------------------------------------------------------------------
def texel_xy(face_view, lay, patch, f, i, j):
    """the atlas position (x, y) of texel (i, j) of the textured face f"""
    S, C = int(patch), lay["cells_per_row"]
    rank = int((np.asarray(face_view)[:f] >= 0).sum())
    cell, half = rank >> 1, rank & 1
    lx, ly = TR.half_local(S, half, i, j)
    return (cell % C) * (S + 1) + lx, (cell // C) * S + ly


def seam_edges(faces, face_view):
    """[(lower vertex, higher vertex, face, face)] of the edges shared by exactly two textured faces of different views"""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    users = {}
    for f in np.nonzero(np.asarray(face_view) >= 0)[0]:
        for e in range(3):
            a, b = int(F[f, e]), int(F[f, (e + 1) % 3])
            users.setdefault((min(a, b), max(a, b)), []).append(int(f))
    return [(lo, hi, u[0], u[1]) for (lo, hi), u in sorted(users.items()) if len(u) == 2 and face_view[u[0]] != face_view[u[1]]]


def edge_texels(F, f, lo, hi, L):
    """(i, j) int64 [L + 1] of face f's texels at the points s / L, s = 0 .. L, from vertex lo towards vertex hi"""
    a, b, c = (int(x) for x in F[f])
    s = np.arange(L + 1, dtype=np.int64)
    if {lo, hi} == {a, b}:
        t = s if lo == a else L - s  # ab -> (s, 0) from a
        return t, np.zeros_like(t)
    if {lo, hi} == {b, c}:
        t = s if lo == b else L - s  # bc from b -> (L - s, s)
        return L - t, t
    t = s if lo == c else L - s  # ca from c -> (0, L - s)
    return np.zeros_like(t), L - t


def seam_step(faces, face_view, atlas, lay, patch):
    """(the mean of |difference| between the two faces' own texels along the seam edges, the number of seam edges)"""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    L = int(patch) - 2
    A = np.asarray(atlas).astype(np.int64)
    diffs = []
    for lo, hi, f0, f1 in seam_edges(F, face_view):
        vals = []
        for f in (f0, f1):
            i, j = edge_texels(F, f, lo, hi, L)
            xy = [texel_xy(face_view, lay, patch, f, int(ii), int(jj)) for ii, jj in zip(i, j)]
            vals.append(np.array([A[y, x] for x, y in xy], np.int64))
        diffs.append(np.abs(vals[0] - vals[1]))
    n = len(diffs)
    return (float(np.concatenate(diffs).mean()) if n else 0.0), n


# ---- the disturbed fidelity scene ------------------------------------------------------------------------------------------------
CALIBRATION = dict(patch=8, iterations=64)


def disturb(images):
    """image k as clip(floor(a_k I + b_k + 0.5), 0, 255), a_k = 0.85 + 0.3 ((7 k) mod 26) / 25, b_k = ((11 k) mod 26) - 13"""
    out = []
    for k, img in enumerate(images):
        a, b = 0.85 + 0.3 * ((7 * k) % 26) / 25, ((11 * k) % 26) - 13
        out.append(np.clip(np.floor(a * np.asarray(img, np.float64) + b + 0.5), 0, 255).astype(np.uint8))
    return out


def layout_of(tex):
    return {k: int(tex[k]) for k in ("cells", "cells_per_row", "W", "H")}


# ---- hand scenes: pixel cameras (raster_ref.pixel_camera) whose image windows decide which view sees which face -------------------
def _window(x0, y0, w, h, f=256.0):
    """a pixel camera that sees the pixel positions [x0, x0 + w) x [y0, y0 + h) of the f = 256 camera at the origin"""
    import raster_ref as R
    s = f / 256.0
    return R.pixel_camera(int(w * s), int(h * s), f=f, cx=-x0 * s, cy=-y0 * s)


def roof(v0=100, v1=140):
    """(verts, faces, cams, images): two faces over the diagonal 0 - 2 of a quad; view 0 (a constant image v0) sees face 0 alone,
    view 1 (v1) face 1 alone"""
    import raster_ref as R
    verts = R.at_pixels([(3.0, 1.0), (1.0, 4.0), (5.0, 5.0), (7.0, 2.0)], 1.0)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    cams = [_window(0, 0, 6, 7), _window(2, 0, 6, 7)]
    return verts, faces, cams, [np.full((7, 6), v0, np.uint8), np.full((7, 6), v1, np.uint8)]


def apex3(seed=1):
    """three faces about one apex, each seen by its own view"""
    import raster_ref as R
    import visib_ref as VR
    verts = R.at_pixels([(6.0, 6.0), (6.0, 1.0), (1.0, 9.0), (11.0, 9.0)], 1.0)
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1]], np.int32)
    cams = [_window(0, 0, 8, 11), _window(0, 5, 13, 6), _window(5, 0, 8, 11)]
    return verts, faces, cams, VR.images_for(cams, seed)


def strip(m, seed=2, binary=False, unseen=False):
    """m faces in a strip under two views that overlap in the middle (a tie goes to view 0): the left part takes view 0, the right
    part view 1 (from m = 4 on; with fewer faces both views see all of them and view 0 takes them).  binary: images of 0 and 255 alone.  unseen: one more face, wound the other way, on the strip's vertices"""
    import raster_ref as R
    cols = m // 2 + 2
    span = 60.0 if m < 1000 else 4000.0
    x = 1.0 + span * np.arange(cols) / (cols - 1)
    top = np.stack([x, np.full(cols, 1.0)], 1)
    bot = np.stack([x + 0.25 * span / (cols - 1), np.full(cols, 4.0)], 1)
    verts = R.at_pixels(np.concatenate([top, bot]), 1.0)
    q = np.arange(m) // 2
    even = np.stack([q, cols + q, cols + q + 1], 1)
    odd = np.stack([q, cols + q + 1, q + 1], 1)
    faces = np.where((np.arange(m) % 2 == 0)[:, None], even, odd).astype(np.int32)
    if unseen:
        faces = np.concatenate([faces, faces[:1, ::-1]]).astype(np.int32)
    w = int(0.75 * span) + 3 if m >= 4 else int(1.25 * span) + 4
    cams = [_window(0, 0, w, 6), _window(int(span) + 3 - w, 0, w, 6)]
    rng = np.random.default_rng(seed)
    if binary:
        images = [(255 * rng.integers(0, 2, (6, w))).astype(np.uint8) for _ in cams]
    else:
        images = [rng.integers(40 + 60 * k, 140 + 60 * k, (6, w)).astype(np.uint8) for k in range(2)]
    return verts, faces, cams, images


def fan(count=4096, seed=3):
    """a fan of `count` faces about one apex with a ring of `count` faces around it.  View 0 sees everything; view 1 has twice the
    focal length and a window right of the apex, so it takes the ring faces it sees and no fan face: the apex is a free node of
    view 0 with `count` neighbours"""
    import raster_ref as R
    a = 2.0 * np.pi * np.arange(count) / count
    c = np.array([32.0, 32.0])
    rim = c[None] + 20.0 * np.stack([np.cos(a), -np.sin(a)], 1)  # y grows downwards: front-facing as (apex, rim i, rim i + 1)
    out = c[None] + 26.0 * np.stack([np.cos(a + np.pi / count), -np.sin(a + np.pi / count)], 1)
    verts = R.at_pixels(np.concatenate([c[None], rim, out]), 1.0)
    i = np.arange(count)
    j = (i + 1) % count
    faces = np.concatenate([np.stack([np.zeros(count, np.int64), 1 + i, 1 + j], 1), np.stack([1 + i, 1 + count + i, 1 + j], 1)]).astype(np.int32)
    cams = [R.pixel_camera(64, 64), _window(36, 0, 28, 64, f=512.0)]
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 120, (64, 64)).astype(np.uint8), rng.integers(100, 256, (128, 56)).astype(np.uint8)]
    return verts, faces, cams, images


def raw_range(verts, faces, cams, images, tex, res, patch):
    """(min, max) over the valid texels of floor((g + N / (256 L)) + 0.5) before the clamps, from a result's corner_adj"""
    X = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    S, L = int(patch), int(patch) - 2
    fv = np.asarray(tex["face_view"], np.int32)
    face, i, j = TR.texel_map(fv, layout_of(tex), S)
    lo, hi = np.inf, -np.inf
    for k in np.unique(fv[fv >= 0]):
        sel = np.nonzero((face >= 0) & (fv[np.maximum(face, 0)] == k))[0]
        g, ok = graw(TR.texel_points(X, F, face[sel], i[sel], j[sel], S), cams[k], images[k])
        i2, j2 = TR.gutter(S, i[sel], j[sel])
        A = np.asarray(res["corner_adj"], np.int64)[face[sel]]
        t = np.floor((g + ((L - i2 - j2) * A[:, 0] + i2 * A[:, 1] + j2 * A[:, 2]).astype(np.float64) / float(256 * L)) + 0.5)[ok]
        lo, hi = min(lo, t.min()), max(hi, t.max())
    return float(lo), float(hi)
