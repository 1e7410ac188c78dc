"""NumPy restatement of the exact Taubin lambda|mu filter of DESIGN.md 21 (sfmx_smooth_*), and the inputs its tests share.

The fixed-point positions are one sequence of IEEE double operations per vertex, the edges come from np.unique on lo n + hi, the
neighbour sums are int64 (np.add.at), and every step is one fixed expression per vertex: nothing depends on an order of
additions, so the device result is compared byte for byte."""
import numpy as np

from simplify_ref import outward_share, permute_vertices, radius_error  # noqa: F401  (reused by the tests)

DEFAULTS = dict(origin=(0.0, 0.0, 0.0), lam=0.5, mu=-0.53, iters=10, pin=1)  # unit has no default
SCALE = float(2 ** 20)   # the fixed-point scale
MAX_Q = float(2 ** 18)   # the largest |q| of an input coordinate
MAX_FIXED = 2 ** 38      # the largest |Q| after a step
MAX_ITERS = 64
COUNTS = ("edges", "boundary_edges", "irregular_edges", "pinned", "isolated")
PINNED, ISOLATED = 1, 2


def check_params(unit=0.0, origin=(0.0, 0.0, 0.0), lam=0.5, mu=-0.53, iters=10, pin=1):
    unit, origin, lam, mu = np.float64(unit), np.asarray(origin, np.float64), np.float64(lam), np.float64(mu)
    return bool(np.isfinite(unit) and unit > 0 and origin.shape == (3,) and np.isfinite(origin).all() and 0 < lam <= 1
                and -1 <= mu <= 0 and int(iters) == iters and 1 <= iters <= MAX_ITERS and pin in (0, 1))


def quantise(verts, unit, origin=(0.0, 0.0, 0.0)):
    """Q int64 [n][3]; ValueError for a coordinate that is not finite or with |q| > 2^18"""
    verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = (verts - np.asarray(origin, np.float64)[None, :]) / np.float64(unit)
        if not (np.abs(q) <= MAX_Q).all():  # NaN and infinities included
            raise ValueError("a coordinate is not finite or exceeds 2^18 units")
        return np.floor(q * SCALE + 0.5).astype(np.int64)


def edge_table(faces, n):
    """(lo, hi, fwd, bwd) of every edge in ascending lo n + hi; ValueError for a face index outside [0, n)"""
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    if len(f) and (f.min() < 0 or f.max() >= n):
        raise ValueError("face index out of range")
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    lo, hi = np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1])
    keys, inv = np.unique(lo * max(n, 1) + hi, return_inverse=True)
    inv = inv.reshape(-1)
    up = e[:, 0] < e[:, 1]
    fwd = np.bincount(inv[up], minlength=len(keys)).astype(np.int64)
    bwd = np.bincount(inv[~up], minlength=len(keys)).astype(np.int64)
    return keys // max(n, 1), keys % max(n, 1), fwd, bwd


def smooth(verts, faces, unit=0.0, origin=(0.0, 0.0, 0.0), lam=0.5, mu=-0.53, iters=10, pin=1):
    """dict(verts f64 [n][3], flags u8 [n], edges, boundary_edges, irregular_edges, pinned, isolated); every condition the library
    answers with SFMX_ERR_INVALID raises ValueError"""
    if not check_params(unit, origin, lam, mu, iters, pin):
        raise ValueError("refused parameters")
    verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    n = len(verts)
    assert n < 2 ** 24
    origin, unit = np.asarray(origin, np.float64), np.float64(unit)
    Q = quantise(verts, unit, origin)
    lo, hi, fwd, bwd = edge_table(faces, n)
    regular = (fwd == 1) & (bwd == 1)
    boundary = fwd + bwd == 1
    cnt = np.bincount(lo, minlength=n) + np.bincount(hi, minlength=n)
    cnt = cnt[:n].astype(np.int64)
    isolated = cnt == 0
    pinned = np.zeros(n, bool)
    if pin:
        pinned[lo[~regular]] = True
        pinned[hi[~regular]] = True
    moves = ~isolated & ~pinned
    cntf = cnt[moves].astype(np.float64)[:, None]
    for step in range(2 * int(iters)):
        f = np.float64(lam if step % 2 == 0 else mu)
        S = np.zeros((n, 3), np.int64)
        np.add.at(S, lo, Q[hi])
        np.add.at(S, hi, Q[lo])
        mean = S[moves].astype(np.float64) / cntf
        d = mean - Q[moves].astype(np.float64)
        Qn = Q.copy()
        Qn[moves] = Q[moves] + np.floor(f * d + 0.5).astype(np.int64)
        if len(Qn) and np.abs(Qn).max() > MAX_FIXED:
            raise ValueError("diverged: a fixed-point coordinate exceeds 2^38")
        Q = Qn
    out = verts.copy()
    out[moves] = origin[None, :] + (Q[moves].astype(np.float64) * (1.0 / SCALE)) * unit
    flags = (pinned * PINNED + isolated * ISOLATED).astype(np.uint8)
    return dict(verts=out, flags=flags, edges=len(lo), boundary_edges=int(boundary.sum()),
                irregular_edges=int((~regular & ~boundary).sum()), pinned=int(pinned.sum()), isolated=int(isolated.sum()))


def counts(ref):
    return {k: ref[k] for k in COUNTS}


# ---- quality figures ----------------------------------------------------------------------------------------
def roughness(verts, faces):
    """RMS angle (degrees) between the unit normals of the two faces on each regular edge; faces of zero area are skipped"""
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    n = len(verts)
    p = verts[f]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(nrm, axis=1)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    owner = np.tile(np.arange(len(f)), 3)
    ok = e[:, 0] != e[:, 1]
    e, owner = e[ok], owner[ok]
    up = e[:, 0] < e[:, 1]
    key = np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1])
    keys, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    fwd, bwd = np.bincount(inv[up], minlength=len(keys)), np.bincount(inv[~up], minlength=len(keys))
    regular = (fwd == 1) & (bwd == 1)
    fa, fb = np.zeros(len(keys), np.int64), np.zeros(len(keys), np.int64)
    fa[inv[up]] = owner[up]
    fb[inv[~up]] = owner[~up]
    sel = regular & (ln[fa] > 0) & (ln[fb] > 0)
    if not sel.any():
        return 0.0
    a, b = nrm[fa[sel]] / ln[fa[sel]][:, None], nrm[fb[sel]] / ln[fb[sel]][:, None]
    ang = np.degrees(np.arccos(np.clip((a * b).sum(1), -1.0, 1.0)))
    return float(np.sqrt((ang * ang).mean()))


def max_move(before, after, unit):
    return float(np.linalg.norm(after - before, axis=1).max() / unit) if len(before) else 0.0


# ---- inputs ----------------------------------------------------------------------------------------------------------------
F0 = np.zeros((0, 3), np.int32)


def disjoint_triangles(m, n=None, seed=1):
    """m triangles over 3 m vertices of their own (every edge a boundary edge), padded with unused vertices up to n"""
    n = 3 * m if n is None else n
    assert n >= 3 * m
    verts = np.random.default_rng(seed + n).random((n, 3)) * 8.0 - 4.0
    return verts, np.arange(3 * m, dtype=np.int32).reshape(m, 3)


def closed_strip(m, seed=2):
    """a closed band of m (even) faces over m vertices, two rims of m / 2: every vertex has 4 neighbours, the rim edges are
    boundary edges and the rungs and diagonals regular"""
    assert m % 2 == 0 and m >= 6
    k = m // 2
    i = np.arange(k, dtype=np.int64)
    j = (i + 1) % k
    faces = np.concatenate([np.stack([i, j, k + i], 1), np.stack([j, k + j, k + i], 1)])
    t = 2 * np.pi * i / k
    ring = np.stack([np.cos(t), np.sin(t), np.zeros(k)], 1) * 3.0
    verts = np.concatenate([ring, ring + (0.0, 0.0, 0.5)]) + np.random.default_rng(seed + m).random((m, 3)) * 0.05
    return verts, faces.astype(np.int32)


def closed_tube(k, rings, seed=3):
    """a torus of rings x k vertices, 2 k rings faces: closed, every edge regular, every vertex 6 neighbours"""
    r, c = np.meshgrid(np.arange(rings, dtype=np.int64), np.arange(k, dtype=np.int64), indexing="ij")
    a, b = r * k + c, r * k + (c + 1) % k
    d, e = ((r + 1) % rings) * k + c, ((r + 1) % rings) * k + (c + 1) % k
    faces = np.concatenate([np.stack([a, b, d], -1).reshape(-1, 3), np.stack([b, e, d], -1).reshape(-1, 3)])
    u, v = 2 * np.pi * r / rings, 2 * np.pi * c / k
    verts = np.stack([(3 + np.cos(v)) * np.cos(u), (3 + np.cos(v)) * np.sin(u), np.sin(v)], -1).reshape(-1, 3)
    return verts + np.random.default_rng(seed + k).random(verts.shape) * 0.02, faces.astype(np.int32)


def double_cone(rim=32768, seed=4):
    """two hubs over a rim: closed, every edge regular, each hub has `rim` neighbours"""
    i = np.arange(rim, dtype=np.int64)
    j = (i + 1) % rim
    top, bot = rim, rim + 1
    faces = np.concatenate([np.stack([i, j, np.full(rim, top)], 1), np.stack([j, i, np.full(rim, bot)], 1)])
    t = 2 * np.pi * i / rim
    rng = np.random.default_rng(seed)
    ring = np.stack([np.cos(t), np.sin(t), rng.random(rim) * 0.1], 1) * 100.0
    verts = np.concatenate([ring, [[0.3, -0.2, 70.0], [0.1, 0.4, -60.0]]])
    return verts, faces.astype(np.int32)


def open_fan(rim=32768, seed=5):
    """half of the double cone: one hub, the rim edges are boundary edges"""
    v, f = double_cone(rim, seed)
    return v[:rim + 1].copy(), f[:rim].copy()


def hot_edge(m=65536):
    """m faces over the same three vertices in all three rotations: three irregular edges that take every counter update"""
    rot = np.random.default_rng(6).integers(0, 3, m)
    base = np.array([0, 1, 2], np.int32)
    faces = np.stack([base[(rot + j) % 3] for j in range(3)], 1)
    return np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]]), faces.astype(np.int32)


UNIT_TRIANGLE = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]], np.int32))
DIVERGING = dict(unit=1.0, lam=1.0, mu=-1.0, pin=0)  # grows by 1.25 per pair about the centroid


def hand_cases():
    """name -> dict(verts, faces, unit[, origin, lam, mu, iters, pin]): the rare branches, small enough to check by eye"""
    quad = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [1.0, 1.0, 0.0], [0.0, 1.0, -0.25]])
    tet = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.125, 0.25, 1.0]])
    tet_f = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]
    edge = 2.0 ** 18
    return {
        "empty": dict(verts=np.zeros((0, 3)), faces=F0, unit=1.0),
        "only-isolated": dict(verts=np.arange(15.0).reshape(5, 3) / 7.0, faces=F0, unit=0.01),
        "triangle-pinned": dict(verts=quad[:3], faces=[[0, 1, 2]], unit=0.5, pin=1),
        "triangle-free": dict(verts=quad[:3], faces=[[0, 1, 2]], unit=0.5, pin=0),
        "shared-edge-opposite": dict(verts=quad, faces=[[0, 1, 2], [0, 2, 3]], unit=0.25, pin=0),  # edge 0-2 regular
        "shared-edge-same": dict(verts=quad, faces=[[0, 1, 2], [0, 2, 3][::-1]], unit=0.25, pin=0),  # edge 0-2 used twice as 2->0
        "shared-edge-same-pinned": dict(verts=quad, faces=[[0, 1, 2], [3, 2, 0]], unit=0.25, pin=1),
        "tetrahedron": dict(verts=tet, faces=tet_f, unit=0.125),  # closed: nothing pinned
        "edge-used-three-times": dict(verts=np.concatenate([tet, [[0.5, 0.5, -1.0]]]), faces=tet_f + [[0, 1, 4]], unit=0.125),
        "face-a-a-b": dict(verts=tet, faces=tet_f + [[3, 3, 1]], unit=0.125),  # only 3->1 counts: edge 1-3 becomes irregular
        "face-a-a-a": dict(verts=tet, faces=tet_f + [[2, 2, 2]], unit=0.125),  # no edge at all
        "unused-vertex": dict(verts=np.concatenate([tet, [[9.0, 9.0, 9.0]]]), faces=tet_f, unit=0.125),
        "minus-zero": dict(verts=[[-0.0, 0.0, -0.0], [1.0, -0.0, 0.0], [-0.0, 1.0, 0.0], [0.0, -0.0, 1.0], [-0.0, -0.0, -0.0]],
                           faces=tet_f, unit=1.0),
        "at-the-limit": dict(verts=[[edge, 0.0, 0.0], [0.0, -edge, 0.0], [0.0, 0.0, edge], [-edge, edge, -edge]], faces=tet_f, unit=1.0),
        "at-the-limit-origin": dict(verts=[[edge * 0.5 + 3.0, 3.0, 3.0], [3.0, 3.0 - edge * 0.5, 3.0], [3.0, 3.0, 3.0], [4.0, 4.0, 5.0]],
                                    faces=tet_f, unit=0.5, origin=(3.0, 3.0, 3.0)),
        "mu-zero": dict(verts=tet, faces=tet_f, unit=0.125, mu=0.0, iters=3),
        "lambda-one": dict(verts=tet, faces=tet_f, unit=0.125, lam=1.0, iters=2),
        "half-way-rounding": dict(verts=[[0.0, 0.0, 0.0], [2.0 ** -20, 0.0, 0.0], [0.0, 3 * 2.0 ** -20, 0.0], [0.0, 0.0, 5 * 2.0 ** -20]],
                                  faces=tet_f, unit=1.0, lam=0.5, mu=-0.5, iters=4),
    }


def run_case(case):
    c = dict(case)
    return smooth(c.pop("verts"), c.pop("faces"), **c)


def invalid_inputs():
    """(name, dict(verts, faces, unit)) for every condition the device answers with SFMX_ERR_INVALID, parameters and divergence
    excluded: each differs from a valid mesh in one value"""
    base_v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 1.5], [7.0, 7.0, 7.0]])  # vertex 4 is unused
    base_f = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    out = []
    for name, bad in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("one ulp beyond 2^18", np.nextafter(MAX_Q, np.inf)),
                      ("one ulp beyond -2^18", -np.nextafter(MAX_Q, np.inf))):
        for k in range(3):
            for vtx in (3, 4):  # also when no face uses the vertex
                v = base_v.copy()
                v[vtx, k] = bad
                out.append((f"coordinate {name} in component {k} of vertex {vtx}", dict(verts=v, faces=base_f, unit=1.0)))
    for bad in (5, -1, 2 ** 31 - 1, -2 ** 31):
        for pos in range(3):
            f = base_f.copy()
            f[1, pos] = bad
            out.append((f"face index {bad} in corner {pos}", dict(verts=base_v, faces=f, unit=1.0)))
    out.append(("a face and no vertex", dict(verts=np.zeros((0, 3)), faces=[[0, 0, 0]], unit=1.0)))
    return out, dict(verts=base_v, faces=base_f, unit=1.0)


BAD_PARAMS = (dict(unit=0.0), dict(unit=-1.0), dict(unit=float("nan")), dict(unit=float("inf")), dict(unit=-0.0),
              dict(unit=1.0, origin=(0.0, float("nan"), 0.0)), dict(unit=1.0, origin=(float("inf"), 0.0, 0.0)),
              dict(unit=1.0, lam=0.0), dict(unit=1.0, lam=-0.5), dict(unit=1.0, lam=1.0000001), dict(unit=1.0, lam=float("nan")),
              dict(unit=1.0, mu=0.0000001), dict(unit=1.0, mu=-1.0000001), dict(unit=1.0, mu=float("nan")),
              dict(unit=1.0, iters=0), dict(unit=1.0, iters=65), dict(unit=1.0, iters=-1), dict(unit=1.0, pin=2), dict(unit=1.0, pin=-1))
GOOD_PARAMS = (dict(unit=1.0), dict(unit=5e-324), dict(unit=1.7e308), dict(unit=0.01, origin=(-1.5, 2.0, 1e300)),
               dict(unit=1.0, lam=1.0, mu=-1.0, iters=64, pin=0), dict(unit=1.0, lam=5e-324, mu=-0.0, iters=1))
