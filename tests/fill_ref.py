"""NumPy restatement of the exact hole filling of DESIGN.md 22 (sfmx_fill_*), and the inputs its tests share.

The fixed-point positions and the edge table are smooth_ref's.  The gap half-edges, the simple vertices and next
follow from integer counts; a loop is walked from its smallest vertex; its centroid is an int64 sum and a true floor, its normal
a sequential double sum from +0.0 in traversal order: nothing depends on a schedule, so the device result is compared byte for
byte."""
import numpy as np

import smooth_ref as MR
from simplify_ref import edge_share, outward_share, permute_vertices  # noqa: F401  (reused by the tests)

DEFAULTS = dict(origin=(0.0, 0.0, 0.0), max_edges=32)  # unit has no default
MAX_EDGES = 1024
MAX_VERTS, MAX_FACES = 2 ** 24, 2 ** 30
COUNTS = ("edges", "boundary_edges", "irregular_edges", "complex_vertices", "filled_loops", "filled_edges", "new_verts", "new_faces")
F0 = MR.F0


def check_params(unit=0.0, origin=(0.0, 0.0, 0.0), max_edges=32):
    unit, origin = np.float64(unit), np.asarray(origin, np.float64)
    return bool(np.isfinite(unit) and unit > 0 and origin.shape == (3,) and np.isfinite(origin).all()
                and int(max_edges) == max_edges and 3 <= max_edges <= MAX_EDGES)


def gaps(faces, n):
    """dict(next int64 [n] (-1 where the vertex is not simple), complex bool [n], edges, boundary_edges, irregular_edges)"""
    lo, hi, fwd, bwd = MR.edge_table(faces, n)
    regular = (fwd == 1) & (bwd == 1)
    boundary = fwd + bwd == 1
    irregular = ~regular & ~boundary
    # a boundary edge used as lo -> hi has the gap half-edge hi -> lo, and the other way round
    tail = np.where(fwd[boundary] == 1, hi[boundary], lo[boundary])
    head = np.where(fwd[boundary] == 1, lo[boundary], hi[boundary])
    out, inn = np.bincount(tail, minlength=n)[:n], np.bincount(head, minlength=n)[:n]
    irr = np.zeros(n, bool)
    irr[lo[irregular]] = True
    irr[hi[irregular]] = True
    simple = (out == 1) & (inn == 1) & ~irr
    nxt = np.full(n, -1, np.int64)
    nxt[tail] = head  # where out > 1 one of the heads: overwritten below
    nxt[~simple] = -1
    return dict(next=nxt, complex=((out + inn) > 0) & ~simple, edges=len(lo), boundary_edges=int(boundary.sum()),
                irregular_edges=int(irregular.sum()))


def leaders(nxt, max_edges):
    """(leader, L) of every loop of at most max_edges vertices, in ascending leader order"""
    start = np.nonzero(nxt >= 0)[0]
    cur = nxt[start]
    found_v, found_l = [], []
    for step in range(1, int(max_edges) + 1):
        if not len(start):
            break
        back = cur == start
        found_v.append(start[back])
        found_l.append(np.full(int(back.sum()), step, np.int64))
        go = cur > start  # a smaller vertex: not the leader
        start, cur = start[go], nxt[cur[go]]
        go = cur >= 0     # a vertex that is not simple: a chain
        start, cur = start[go], cur[go]
    v = np.concatenate(found_v) if found_v else np.zeros(0, np.int64)
    ln = np.concatenate(found_l) if found_l else np.zeros(0, np.int64)
    order = np.argsort(v, kind="stable")
    return v[order], ln[order]


def fill(verts, faces, normals=None, unit=0.0, origin=(0.0, 0.0, 0.0), max_edges=32):
    """dict(verts f64 [n + K][3], faces i32 [m + F][3], normals f64 [n + K][3] or None, leaders, lengths, and the eight counts);
    every condition the library answers with SFMX_ERR_INVALID raises ValueError"""
    if not check_params(unit, origin, max_edges):
        raise ValueError("refused parameters")
    verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    normals = None if normals is None else np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    n, m = len(verts), len(faces)
    assert n < MAX_VERTS and m < MAX_FACES and (normals is None or len(normals) == n)
    origin, unit = np.asarray(origin, np.float64), np.float64(unit)
    Q = MR.quantise(verts, unit, origin)
    g = gaps(faces, n)
    nxt = g["next"]
    lead, L = leaders(nxt, max_edges)
    kv = (L > 3).astype(np.int64)
    kf = np.where(L == 3, 1, L)
    K, F = int(kv.sum()), int(kf.sum())
    if n + K >= MAX_VERTS or m + F >= MAX_FACES:
        raise ValueError("the filled mesh exceeds 2^24 vertices or 2^30 faces")
    voff, foff = np.cumsum(kv) - kv, np.cumsum(kf) - kf
    out_v = np.concatenate([verts, np.zeros((K, 3))])
    out_f = np.concatenate([faces, np.zeros((F, 3), np.int32)])
    out_n = None if normals is None else np.concatenate([normals, np.zeros((K, 3))])
    for ln in np.unique(L):
        sel = L == ln
        ln = int(ln)
        loop = np.empty((int(sel.sum()), ln), np.int64)
        loop[:, 0] = lead[sel]
        for i in range(1, ln):
            loop[:, i] = nxt[loop[:, i - 1]]
        assert (nxt[loop[:, -1]] == loop[:, 0]).all() and (loop[:, 1:] > loop[:, :1]).all()
        rows = (m + foff[sel])[:, None] + np.arange(1 if ln == 3 else ln)[None, :]
        if ln == 3:
            out_f[rows[:, 0]] = loop
            continue
        c = n + voff[sel]
        out_f[rows] = np.stack([loop, np.roll(loop, -1, axis=1), np.broadcast_to(c[:, None], loop.shape)], -1)
        S = Q[loop].sum(1)  # int64 [k][3]
        Qc = (2 * S + ln) // (2 * ln)  # // on int64 is a true floor
        out_v[c] = origin[None, :] + (Qc.astype(np.float64) * (1.0 / MR.SCALE)) * unit
        if normals is not None:
            with np.errstate(all="ignore"):
                s = np.zeros((len(loop), 3))
                for i in range(ln):
                    s = s + normals[loop[:, i]]
                lnn = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
                ok = lnn > 0
                out_n[c] = np.where(ok[:, None], s / np.where(ok, lnn, 1.0)[:, None], 0.0)
    return dict(verts=out_v, faces=out_f, normals=out_n, leaders=lead, lengths=L, edges=g["edges"],
                boundary_edges=g["boundary_edges"], irregular_edges=g["irregular_edges"], complex_vertices=int(g["complex"].sum()),
                filled_loops=len(lead), filled_edges=int(L.sum()), new_verts=K, new_faces=F)


def counts(ref):
    return {k: ref[k] for k in COUNTS}


def same(a, b):
    """two results (restatement or device) agree in every byte and count"""
    assert a["verts"].tobytes() == b["verts"].tobytes() and a["faces"].tobytes() == b["faces"].tobytes()
    assert (a.get("normals") is None) == (b.get("normals") is None)
    assert a.get("normals") is None or a["normals"].tobytes() == b["normals"].tobytes()
    assert counts(a) == counts(b)


def all_loops(faces, n):
    """lengths of all loops, whatever their length (the calibration's histogram)"""
    return leaders(gaps(faces, n)["next"], n)[1]


def euler(n, faces):
    """V - E + F of a mesh that uses all its n vertices"""
    return n - len(MR.edge_table(faces, n)[0]) + len(faces)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def open_tube(k, rings=2, seed=3):
    """rings x k vertices, 2 k (rings - 1) faces: an open tube whose two rims are loops of k edges (k >= 3); every vertex is used"""
    r, c = np.meshgrid(np.arange(rings - 1, dtype=np.int64), np.arange(k, dtype=np.int64), indexing="ij")
    a, b = r * k + c, r * k + (c + 1) % k
    d, e = (r + 1) * k + c, (r + 1) * k + (c + 1) % k
    faces = np.concatenate([np.stack([a, b, d], -1).reshape(-1, 3), np.stack([b, e, d], -1).reshape(-1, 3)])
    rr, cc = np.meshgrid(np.arange(rings, dtype=np.float64), np.arange(k, dtype=np.float64), indexing="ij")
    t = 2 * np.pi * cc / k
    verts = np.stack([np.cos(t) * 2.0, np.sin(t) * 2.0, rr * 0.5 - 1.0], -1).reshape(-1, 3)
    rng = np.random.default_rng(seed + k)
    verts = verts + rng.random(verts.shape) * 0.02
    return verts, faces.astype(np.int32), rng.standard_normal(verts.shape)


def lone_triangles(count, seed=11):
    """disjoint triangles: each is a loop of three (its back face closes it): K = 0, F = 1 each"""
    rng = np.random.default_rng(seed + count)
    verts = rng.random((3 * count, 3)) * 16.0 - 8.0
    return verts, np.arange(3 * count, dtype=np.int32).reshape(count, 3), rng.standard_normal((3 * count, 3))


def open_quads(count, seed=12):
    """disjoint quads of two faces (0 1 2)(0 2 3): each rim is a loop of four: K = 1, F = 4 each"""
    rng = np.random.default_rng(seed + count)
    verts = rng.random((4 * count, 3)) * 16.0 - 8.0
    b = 4 * np.arange(count, dtype=np.int64)[:, None]
    faces = np.concatenate([b + np.array([[0, 1, 2]]), b + np.array([[0, 2, 3]])], 1).reshape(-1, 3)
    return verts, faces.astype(np.int32), rng.standard_normal((4 * count, 3))


TET = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.125, 0.25, 1.0]])
TET_F = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]
CUBE = np.array([[x, y, z] for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)]) + 0.25
# outward faces of the cube, two triangles per side; the last two are the top (z = 1)
CUBE_F = [[0, 2, 3], [0, 3, 1], [0, 1, 5], [0, 5, 4], [1, 3, 7], [1, 7, 5], [3, 2, 6], [3, 6, 7], [2, 0, 4], [2, 4, 6], [4, 5, 7], [4, 7, 6]]


def hand_cases():
    """name -> dict(verts, faces, unit[, origin, normals]): the rare branches, small enough to check by eye"""
    quad = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [1.0, 1.0, 0.0], [0.0, 1.0, -0.25]])
    edge = 2.0 ** 18
    nq = np.array([[0.0, 0.0, 1.0], [0.0, 0.6, 0.8], [0.6, 0.0, 0.8], [0.0, 0.0, 1.0]])
    # two open quads that share vertex 0: out(0) = in(0) = 2
    bow_v = np.concatenate([quad, quad[1:] * -1.0 + (0.0, 0.0, 3.0)])
    bow_f = [[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6]]
    # the cube without its top, and a two-sided fin on the side edge {0, 4}: that edge is used twice in each direction, so it is
    # irregular and the rim vertex 4 is not simple although out(4) == in(4) == 1
    fin_v = np.concatenate([CUBE, [[-1.0, -1.0, 0.5]]])
    fin_f = CUBE_F[:10] + [[0, 4, 8], [4, 0, 8]]
    half = 2.0 ** -21  # half a fixed-point step at unit 1
    return {
        "empty": dict(verts=np.zeros((0, 3)), faces=F0, unit=1.0),
        "no-faces": dict(verts=np.arange(15.0).reshape(5, 3) / 7.0, faces=F0, unit=0.01, normals=np.ones((5, 3))),
        "lone-triangle": dict(verts=quad[:3], faces=[[0, 1, 2]], unit=0.5, normals=nq[:3]),  # gets its back face
        "tetrahedron-closed": dict(verts=TET, faces=TET_F, unit=0.125, normals=nq),
        "tetrahedron-open": dict(verts=TET, faces=TET_F[:3], unit=0.125, normals=nq),  # L = 3: the missing face, no vertex
        "cube-open": dict(verts=CUBE, faces=CUBE_F[:10], unit=0.25, normals=np.tile(nq, (2, 1))),  # L = 4 around the top
        "open-quad": dict(verts=quad, faces=[[0, 1, 2], [0, 2, 3]], unit=0.25, origin=(0.5, -0.5, 0.125), normals=nq),
        "open-quad-relabelled": dict(verts=quad[[2, 3, 0, 1]], faces=[[2, 3, 0], [2, 0, 1]], unit=0.25, normals=nq[[2, 3, 0, 1]]),
        "two-holes-share-a-vertex": dict(verts=bow_v, faces=bow_f, unit=0.25),  # vertex 0 is complex: neither is filled
        "irregular-edge-at-the-rim": dict(verts=fin_v, faces=fin_f, unit=0.25),
        "face-a-a-b": dict(verts=TET, faces=TET_F[:3] + [[3, 3, 1]], unit=0.125),  # 3->1 a second time: edge {1, 3} irregular
        "face-a-a-a": dict(verts=TET, faces=TET_F[:3] + [[2, 2, 2]], unit=0.125),  # no edge at all: filled as the open one
        "unused-vertex": dict(verts=np.concatenate([CUBE, [[9.0, 9.0, 9.0]]]), faces=CUBE_F[:10], unit=0.25),
        "minus-zero": dict(verts=[[-0.0, 0.0, -0.0], [1.0, -0.0, 0.0], [1.0, 1.0, -0.0], [-0.0, 1.0, 0.0]], faces=[[0, 1, 2], [0, 2, 3]],
                           unit=1.0, normals=[[-0.0, -0.0, -0.0]] * 4),
        "at-the-limit": dict(verts=[[edge, 0.0, 0.0], [0.0, -edge, 0.0], [edge, edge, edge], [-edge, edge, -edge]],
                             faces=[[0, 1, 2], [0, 2, 3]], unit=1.0),
        # S = 2 per component of x: the centroid 2 / 4 lies on a half and rounds up to 1; with -2 it rounds up to 0
        "half-positive": dict(verts=[[2 * half, 0.0, 0.0], [2 * half, 4 * half, 0.0], [0.0, 0.0, 0.0], [0.0, 2 * half, 0.0]],
                              faces=[[0, 1, 2], [0, 2, 3]], unit=1.0),
        "half-negative": dict(verts=[[-2 * half, 0.0, 0.0], [-2 * half, -12 * half, 0.0], [0.0, 0.0, 0.0], [0.0, -2 * half, 0.0]],
                              faces=[[0, 1, 2], [0, 2, 3]], unit=1.0),
        "normals-sum-to-zero": dict(verts=quad, faces=[[0, 1, 2], [0, 2, 3]], unit=0.25,
                                    normals=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]),
        "nan-normals": dict(verts=quad, faces=[[0, 1, 2], [0, 2, 3]], unit=0.25,
                            normals=[[1.0, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]),
    }


def run_case(case, **over):
    c = dict(case, **over)
    return fill(c.pop("verts"), c.pop("faces"), **c)


def invalid_inputs():
    """(name, dict(verts, faces, unit)) for every condition the device answers with SFMX_ERR_INVALID, parameters excluded: each
    differs from a valid mesh in one value"""
    out, good = MR.invalid_inputs()
    return out, good


BAD_PARAMS = (dict(unit=0.0), dict(unit=-1.0), dict(unit=float("nan")), dict(unit=float("inf")), dict(unit=-0.0),
              dict(unit=1.0, origin=(0.0, float("nan"), 0.0)), dict(unit=1.0, origin=(float("inf"), 0.0, 0.0)),
              dict(unit=1.0, max_edges=2), dict(unit=1.0, max_edges=0), dict(unit=1.0, max_edges=-1), dict(unit=1.0, max_edges=1025),
              dict(unit=1.0, max_edges=2 ** 31 - 1))
GOOD_PARAMS = (dict(unit=1.0), dict(unit=5e-324), dict(unit=1.7e308), dict(unit=0.01, origin=(-1.5, 2.0, 1e300)),
               dict(unit=1.0, max_edges=3), dict(unit=1.0, max_edges=1024))
