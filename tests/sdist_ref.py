"""NumPy restatement of the point-to-mesh distance stage and of the surface evaluation (TEST INFRASTRUCTURE).

Every distance is the device's sequence of IEEE double operations, one NumPy operation each (NumPy never contracts a
multiplication and an addition), so `brute` is compared with the device bit for bit.  `pruned` computes the same minimum over
a superset of the faces that can count for each query (a KD-tree on face centroids if scipy imports, else its own grid): a
minimum with the smallest-index tie rule does not depend on the candidates that lose.
"""
from __future__ import annotations

import math

import numpy as np

GROW = 1.0009765625  # 1 + 2^-10: a face counts for a query inside its bounding box grown by d_max * GROW
COORD_LIMIT = 2.0 ** 40  # |coordinate| <= COORD_LIMIT * d_max


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1],
                     x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def seg(p, a, b):
    """squared distance from p to the segment a b (broadcasting [..., 3] arrays)"""
    ab, ap = b - a, p - a
    ab, ap = np.broadcast_arrays(ab, ap)
    den, num = dot(ab, ab), dot(ap, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = num / den
    t = np.where(~(num > 0.0), 0.0, np.where(num >= den, 1.0, q))
    e = p - (a + t[..., None] * ab)
    return dot(e, e)


def tri(p, a, b, c):
    """squared distance from p to the triangle a b c (broadcasting [..., 3] arrays)"""
    n = cross(b - a, c - a)
    nn = dot(n, n)
    s1 = dot(cross(b - a, p - a), n)
    s2 = dot(cross(c - b, p - b), n)
    s3 = dot(cross(a - c, p - c), n)
    h = dot(p - a, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        plane = (h * h) / nn
    edges = np.minimum(np.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a))
    return np.where((nn > 0.0) & (s1 >= 0.0) & (s2 >= 0.0) & (s3 >= 0.0), plane, edges)


def _mesh(V, F):
    V = np.ascontiguousarray(V, np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(F, np.int32).reshape(-1, 3)
    if len(F):
        assert F.min() >= 0 and F.max() < len(V), "face index out of range"
        assert np.isfinite(V[np.unique(F)]).all(), "non-finite used vertex"
    return V, F


def boxes(V, F, d_max):
    """the grown bounding box of every face: (lo [m][3], hi [m][3])"""
    g = d_max * GROW
    T = V[F]
    return T.min(axis=1) - g, T.max(axis=1) + g


def _clip(d2min, fmin, d_max):
    dm2 = d_max * d_max
    hit = d2min < dm2
    return np.where(hit, d2min, dm2), np.where(hit, fmin, -1).astype(np.int32)


def brute(P, V, F, d_max, chunk=256, box=True):
    """(d2 f64 [n], face i32 [n]) by testing every face for every query.  box=False drops the grown-box rule (the plain minimum
    over all faces): on well-shaped meshes both give the same bits, which the CPU suite checks."""
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
    V, F = _mesh(V, F)
    assert np.isfinite(P).all(), "non-finite query"
    n, m = len(P), len(F)
    d2 = np.full(n, np.inf)
    fm = np.full(n, -1, np.int64)
    if m:
        a, b, c = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
        lo, hi = boxes(V, F, d_max)
        for s in range(0, n, chunk):
            p = P[s:s + chunk, None, :]
            D = tri(p, a, b, c)
            if box:
                D = np.where(((p >= lo[None]) & (p <= hi[None])).all(axis=-1), D, np.inf)
            k = D.argmin(axis=1)  # the first, so the smallest index, among equals
            d2[s:s + chunk] = D[np.arange(len(k)), k]
            fm[s:s + chunk] = k
    return _clip(d2, fm, d_max)


def _candidates(P, V, F, d_max):
    """(query index, face index) pairs that hold, for every query, each face that can attain its minimum.  A face counts only
    if its grown box holds the query, so its centroid is within sqrt(3) grow + (its radius) of it; and once one face is known at
    squared distance u, only faces whose centroid is within sqrt(u) + (their radius) can be as near.  The slack of 1e-6 is far
    above the rounding of the distances of any face that is not degenerate to working precision."""
    T = V[F]
    cen = T.mean(axis=1)
    rad = float(np.sqrt(((T - cen[:, None]) ** 2).sum(axis=2)).max()) * (1.0 + 1e-6) + 1e-300
    full = np.sqrt(3.0) * d_max * GROW * (1.0 + 1e-6) + rad
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if cKDTree is not None:
        tree = cKDTree(cen)
        j0 = tree.query(P)[1]
        lo, hi = boxes(V, F, d_max)
        u = np.where(((P >= lo[j0]) & (P <= hi[j0])).all(axis=-1), tri(P, T[j0, 0], T[j0, 1], T[j0, 2]), np.inf)
        r = np.minimum(np.sqrt(u) * (1.0 + 1e-6) + rad, full)
        lists = tree.query_ball_point(P, r)
        cnt = np.fromiter((len(x) for x in lists), np.int64, len(lists))
        fi = np.fromiter((j for x in lists for j in x), np.int64, int(cnt.sum()))
        return np.repeat(np.arange(len(P)), cnt), fi
    # own grid of edge `full` over the centroids: a face within `full` of the query is in one of the 27 cells around it
    org = cen.min(axis=0) - full
    key = lambda x: np.floor((x - org) / full).astype(np.int64)
    cells = {}
    for j, k in enumerate(map(tuple, key(cen))):
        cells.setdefault(k, []).append(j)
    qi, fi = [], []
    for i, k in enumerate(map(tuple, key(P))):
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    js = cells.get((k[0] + dx, k[1] + dy, k[2] + dz), ())
                    qi.extend([i] * len(js))
                    fi.extend(js)
    return np.asarray(qi, np.int64), np.asarray(fi, np.int64)


def pruned(P, V, F, d_max, chunk=20000):
    """brute()'s result from candidate lists; for the sizes brute force cannot reach"""
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
    V, F = _mesh(V, F)
    assert np.isfinite(P).all(), "non-finite query"
    n = len(P)
    d2 = np.full(n, np.inf)
    fm = np.full(n, -1, np.int64)
    if len(F):
        lo, hi = boxes(V, F, d_max)
        for s in range(0, n, chunk):
            qi, fi = _candidates(P[s:s + chunk], V, F, d_max)
            p = P[s:s + chunk][qi]
            ok = ((p >= lo[fi]) & (p <= hi[fi])).all(axis=-1)
            qi, fi, p = qi[ok], fi[ok], p[ok]
            D = tri(p, V[F[fi, 0]], V[F[fi, 1]], V[F[fi, 2]])
            o = np.lexsort((fi, D, qi))  # by query, then distance, then face index
            qi, fi, D = qi[o], fi[o], D[o]
            first = np.ones(len(qi), bool)
            first[1:] = qi[1:] != qi[:-1]
            d2[s + qi[first]] = D[first]
            fm[s + qi[first]] = fi[first]
    return _clip(d2, fm, d_max)


def used_vertices(V, F):
    """the vertices a face uses, in index order"""
    V, F = _mesh(V, F)
    mask = np.zeros(len(V), bool)
    mask[F.ravel()] = True
    return V[mask]


def nearest_rank(sorted_vals, percentile):
    n = len(sorted_vals)
    k = min(max(int(math.ceil(percentile / 100.0 * n)), 1), n)
    return float(sorted_vals[k - 1])


def evaluate(Rv, Rf, Gv, Gf, d_max, tau, percentile=90.0, dist=pruned):
    """accuracy / completeness of the reconstruction (Rv, Rf) against the ground truth (Gv, Gf), sampled at used vertices"""
    assert tau <= d_max
    nan = float("nan")
    q = used_vertices(Rv, Rf)
    d = np.sqrt(dist(q, Gv, Gf, d_max)[0])
    out = dict(n_rec=len(q), acc_within=int((d <= tau).sum()))
    if len(q):
        out.update(accuracy=nearest_rank(np.sort(d), percentile), acc_mean=float(np.cumsum(d)[-1] / len(q)), acc_max=float(d.max()))
    else:
        out.update(accuracy=nan, acc_mean=nan, acc_max=nan)
    g = used_vertices(Gv, Gf)
    dg = np.sqrt(dist(g, Rv, Rf, d_max)[0])
    out.update(n_gt=len(g), comp_within=int((dg <= tau).sum()))
    out["completeness"] = out["comp_within"] / len(g) if len(g) else nan
    return out


def icosphere(level, radius=1.0):
    """(verts f64 [n][3], faces i32 [m][3]): an icosahedron subdivided `level` times, outward faces, vertices on the sphere"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                w = v[i] + v[j]
                v.append(w / np.linalg.norm(w))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius, np.asarray(f, np.int32)
