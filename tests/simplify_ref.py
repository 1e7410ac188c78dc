"""NumPy restatement of the exact vertex clustering of DESIGN.md 20 (sfmx_simplify_*), and the inputs its tests share.

Cells and fixed-point offsets are one sequence of IEEE double operations, the cluster sums are int64 (np.add.at), clusters and
duplicate triples come from np.unique: everything downstream of the doubles is an integer, so the device result is compared
byte for byte."""
import numpy as np

DEFAULTS = dict(origin=(0.0, 0.0, 0.0))  # cell has no default
ONE = float(2 ** 30)  # the fixed-point scale, and the largest cell index
MAX_CELLS = 2 ** 27
MAX_NORMAL = 4.0
ARRAYS = ("verts", "faces", "vert_dst", "face_src", "members")
COUNTS = ("clusters", "degenerate", "duplicates", "n_verts", "n_faces")


def check_params(cell=0.0, origin=(0.0, 0.0, 0.0)):
    cell, origin = np.float64(cell), np.asarray(origin, np.float64)
    return bool(np.isfinite(cell) and cell > 0 and origin.shape == (3,) and np.isfinite(origin).all())


def cells(verts, cell, origin=(0.0, 0.0, 0.0)):
    """(c int64 [n][3], Q int64 [n][3]) of every vertex; ValueError for a coordinate that is not finite or a cell index beyond 2^30"""
    verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = (verts - np.asarray(origin, np.float64)[None, :]) / np.float64(cell)
        c = np.floor(q)
        if not (np.abs(c) <= ONE).all():  # NaN and infinities included
            raise ValueError("a coordinate is not finite or its cell index exceeds 2^30")
        t = q - c
        Q = np.floor(t * ONE + 0.5).astype(np.int64)
    return c.astype(np.int64), Q


def simplify(verts, faces, normals=None, cell=0.0, origin=(0.0, 0.0, 0.0)):
    """dict(verts, faces, vert_dst, face_src, members, clusters, degenerate, duplicates, n_verts, n_faces[, normals]); every
    condition the library answers with SFMX_ERR_INVALID raises ValueError"""
    if not check_params(cell, origin):
        raise ValueError("cell must be finite and > 0, origin finite")
    verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    origin = np.asarray(origin, np.float64)
    cell = np.float64(cell)
    n, m = len(verts), len(faces)
    if normals is not None:
        normals = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
        assert len(normals) == n
    out = {}
    if n:
        c, Q = cells(verts, cell, origin)
        if normals is not None and not (np.abs(normals) <= MAX_NORMAL).all():
            raise ValueError("a normal component is not finite or exceeds 4")
        cmin = c.min(0)
        dims = c.max(0) - cmin + 1
        if int(dims[0]) * int(dims[1]) * int(dims[2]) > MAX_CELLS:
            raise ValueError("the box of the occupied cells has more than 2^27 cells")
        lin = (c[:, 0] - cmin[0]) + dims[0] * ((c[:, 1] - cmin[1]) + dims[1] * (c[:, 2] - cmin[2]))
        occupied, vclu = np.unique(lin, return_inverse=True)  # ascending linear index
        vclu = vclu.reshape(-1)
        ncl = len(occupied)
    else:
        vclu, ncl = np.zeros(0, np.int64), 0
    if m and (faces.min() < 0 or faces.max() >= n):
        raise ValueError("face index out of range")
    if n:
        S = np.zeros((ncl, 3), np.int64)
        np.add.at(S, vclu, Q)
        cnt = np.bincount(vclu, minlength=ncl).astype(np.int32)
        cc = np.zeros((ncl, 3), np.int64)
        cc[vclu] = c
        pos = origin[None, :] + (cc.astype(np.float64) + (S.astype(np.float64) / cnt.astype(np.float64)[:, None]) / ONE) * cell
        if normals is not None:
            Sn = np.zeros((ncl, 3), np.int64)
            np.add.at(Sn, vclu, np.floor(normals * ONE + 0.5).astype(np.int64))
            s = Sn.astype(np.float64)
            ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
            with np.errstate(all="ignore"):
                nrm = np.where(ln[:, None] == 0.0, 0.0, s / ln[:, None])
    else:
        pos, cnt, nrm = np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 3))
    # faces
    tri = vclu[faces.astype(np.int64)].reshape(-1, 3) if m else np.zeros((0, 3), np.int64)
    deg = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    k = np.argmin(tri, axis=1)  # the smallest is unique in a non-degenerate triple
    rows = np.arange(m)
    canon = np.stack([tri[rows, k], tri[rows, (k + 1) % 3], tri[rows, (k + 2) % 3]], 1)
    idx = np.nonzero(~deg)[0]
    keep = np.zeros(m, bool)
    if len(idx):
        _, first = np.unique(canon[idx], axis=0, return_index=True)  # the first occurrence = the smallest input index
        keep[idx[first]] = True
    face_src = np.nonzero(keep)[0].astype(np.int32)
    used = np.zeros(ncl, bool)
    used[canon[face_src].ravel()] = True
    remap = np.where(used, np.cumsum(used) - 1, -1)
    out.update(verts=np.ascontiguousarray(pos[used]), faces=remap[canon[face_src]].astype(np.int32).reshape(-1, 3),
               vert_dst=remap[vclu].astype(np.int32), face_src=face_src, members=cnt[used].astype(np.int32),
               clusters=ncl, degenerate=int(deg.sum()), duplicates=int(m - deg.sum() - keep.sum()), n_verts=int(used.sum()),
               n_faces=int(keep.sum()))
    if normals is not None:
        out["normals"] = np.ascontiguousarray(nrm[used])
    return out


def counts(ref):
    return {k: ref[k] for k in COUNTS}


def max_members(ref):
    return int(ref["members"].max()) if len(ref["members"]) else 0


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def permute_vertices(verts, faces, normals, seed):
    """the same mesh with its vertices in another order: new vertex j is old vertex perm[j]"""
    perm = np.random.default_rng(seed).permutation(len(verts))
    inv = np.empty(len(verts), np.int64)
    inv[perm] = np.arange(len(verts))
    return verts[perm], inv[faces].astype(np.int32), (None if normals is None else normals[perm]), perm


def face_set(ref):
    """the output mesh as a set that does not depend on the face order: each face as the bytes of its three corner positions"""
    v = ref["verts"][ref["faces"]]
    return sorted(v[i].tobytes() for i in range(len(v)))


def grid_triangles(dims, m, cell=1.0, stride=1):
    """m disjoint triangles; triangle i has its three corners in the cells i * stride + (0, 1, 2) (linear index) of a grid with
    the given dims, whose box is pinned by two extra vertices in its first and last cell: 3 m + 2 vertices"""
    dims = np.asarray(dims, np.int64)
    total = int(dims.prod())
    assert (m - 1) * stride + 2 < total
    lin = (np.arange(m, dtype=np.int64) * stride)[:, None] + np.arange(3)[None, :]
    lin = np.concatenate([lin.ravel(), [0, total - 1]])
    c = np.stack([lin % dims[0], (lin // dims[0]) % dims[1], lin // (dims[0] * dims[1])], 1)
    frac = np.random.default_rng(m).random((len(lin), 3)) * 0.9 + 0.05
    verts = (c + frac) * cell
    faces = np.arange(3 * m, dtype=np.int32).reshape(m, 3)
    return verts, faces


def hot_vertex(n=65536, cell=1.0, seed=3):
    """n vertices in one cell and three more in three other cells, with faces from the crowd to the three"""
    rng = np.random.default_rng(seed)
    crowd = rng.random((n, 3)) * cell
    far = np.array([[1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5]]) * cell
    verts = np.concatenate([crowd, far])
    a = rng.integers(0, n, 300)
    faces = np.stack([a, np.full(300, n), np.full(300, n + 1)], 1)
    faces = np.concatenate([faces, np.stack([a, np.full(300, n + 1), np.full(300, n + 2)], 1), [[n, n + 1, n + 2]]])
    return verts, faces.astype(np.int32), np.clip(rng.standard_normal((n + 3, 3)), -MAX_NORMAL, MAX_NORMAL)


def line_of_cells(k, cell=1.0):
    """k vertices in k cells in a row (the box has exactly k cells, all occupied) and floor(k / 3) faces over them"""
    verts = np.random.default_rng(k).random((k, 3)) * 0.9 + 0.05
    verts[:, 0] += np.arange(k)
    faces = np.arange(3 * (k // 3), dtype=np.int32).reshape(-1, 3)
    return verts * cell, faces


def unit(normals):
    return normals / np.linalg.norm(normals, axis=1)[:, None]


def hot_triple(m=65536, cell=1.0, seed=4):
    """m faces over 3 m vertices that all collapse to one canonical triple, in all three rotations"""
    rng = np.random.default_rng(seed)
    base = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) * cell
    verts = (base[None, :, :] + rng.random((m, 3, 3)) * cell).reshape(-1, 3)
    faces = np.arange(3 * m, dtype=np.int64).reshape(m, 3)
    rot = rng.integers(0, 3, m)
    faces = np.stack([faces[np.arange(m), (rot + j) % 3] for j in range(3)], 1)
    return verts, faces.astype(np.int32)


F0 = np.zeros((0, 3), np.int32)


def hand_cases():
    """name -> dict(verts, faces[, normals], cell[, origin]): the rare branches, small enough to check by eye"""
    tri3 = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]])  # one corner in each of three cells (cell 1)
    two = np.concatenate([tri3, tri3 + 0.25])
    return {
        "empty": dict(verts=np.zeros((0, 3)), faces=F0, cell=1.0),
        "vertices-no-face": dict(verts=np.arange(15.0).reshape(5, 3), faces=F0, cell=2.0),
        "one-face": dict(verts=tri3, faces=[[2, 0, 1]], normals=np.eye(3), cell=1.0),
        # x = origin + k cell for k < 0, = 0, > 0, and -0.0: the vertex belongs to cell k with offset 0
        "on-cell-faces": dict(verts=[[-0.5, 0.0, 0.75], [0.0, -0.0, 0.25], [0.25, 0.5, -0.25], [-0.0, 0.25, 0.0]],
                              faces=[[0, 1, 2], [1, 2, 3], [3, 0, 2]], cell=0.25),
        "on-cell-faces-origin": dict(verts=[[0.625, 1.125, 2.375], [1.125, 1.125, 1.875], [1.375, 1.625, 1.375]], faces=[[0, 1, 2]],
                                     cell=0.25, origin=(1.125, 1.125, 1.875)),
        # t = q - floor(q) rounds to 1, so Q = 2^30: the vertex sits on the upper face of the cell it belongs to
        "t-rounds-to-one": dict(verts=[[-1e-20, 0.5, 0.5], [1.5, -1e-300, 0.5], [0.5, 1.5, -2.0 ** -60]], faces=[[0, 1, 2]], cell=1.0),
        "same-orientation": dict(verts=two, faces=[[4, 5, 3], [0, 1, 2], [1, 2, 0]], cell=1.0),  # one kept: the smallest index
        "opposite-orientation": dict(verts=two, faces=[[0, 1, 2], [3, 5, 4]], cell=1.0),  # both kept
        "two-corners-in-one-cell": dict(verts=two, faces=[[0, 3, 1], [0, 1, 2]], cell=1.0),
        "inside-one-cell": dict(verts=tri3 / 4.0, faces=[[0, 1, 2], [2, 1, 0]], normals=np.eye(3), cell=1.0),
        # vertex 3 is used by no face and still moves the mean of the cell it shares with vertex 0
        "unused-vertex": dict(verts=np.concatenate([tri3, [[0.25, 0.125, 0.75]]]), faces=[[0, 1, 2]], cell=1.0),
        "zero-normal-sum": dict(verts=two, faces=[[0, 1, 2]], cell=1.0,
                                normals=[[1, 0, 0], [0, 0.5, 0], [0, 0, -4.0], [-1, 0, 0], [0, 0.25, 0.25], [0, 0, 4.0]]),
    }


def run_case(case):
    return simplify(case["verts"], case["faces"], case.get("normals"), case["cell"], case.get("origin", (0.0, 0.0, 0.0)))


def invalid_inputs():
    """(name, dict(verts, faces, normals or None, cell, origin)) for every condition the device answers with SFMX_ERR_INVALID,
    parameters excluded: each differs from a valid mesh in one value"""
    base_v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 1.5]])
    base_f = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    base_n = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0.5, 0.5, 0.5]])
    out = []
    for name, bad in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for k in range(3):
            v = base_v.copy()
            v[3, k] = bad  # vertex 3: also when no face used it
            out.append((f"coordinate {name} in component {k}", dict(verts=v, faces=base_f, normals=None, cell=1.0)))
    for bad in (4, -1, 2 ** 31 - 1, -2 ** 31):
        for pos in range(3):
            f = base_f.copy()
            f[1, pos] = bad
            out.append((f"face index {bad} in corner {pos}", dict(verts=base_v, faces=f, normals=None, cell=1.0)))
    for k in range(3):
        for sign in (1.0, -1.0):
            v = base_v.copy()
            v[1, k] = sign * (2.0 ** 30 + 1.0)  # cell 1, origin 0: the cell index is the coordinate
            out.append((f"cell index beyond 2^30 in component {k}", dict(verts=v, faces=base_f, normals=None, cell=1.0)))
    v = base_v.copy()
    v[3] = (600.0, 600.0, 600.0)  # 601^3 > 2^27 cells between the two ends
    out.append(("a box of more than 2^27 cells", dict(verts=v, faces=base_f, normals=None, cell=1.0)))
    for bad in (4.000001, -4.000001, np.nan, np.inf):
        for k in range(3):
            nr = base_n.copy()
            nr[2, k] = bad
            out.append((f"normal component {bad} in component {k}", dict(verts=base_v, faces=base_f, normals=nr, cell=1.0)))
    return out, dict(verts=base_v, faces=base_f, normals=base_n, cell=1.0)


BAD_PARAMS = (dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(cell=-0.0),
              dict(cell=1.0, origin=(0.0, float("nan"), 0.0)), dict(cell=1.0, origin=(float("inf"), 0.0, 0.0)))


# ---- quality figures ----------------------------------------------------------------------------------------
def edge_share(faces):
    """the share of undirected edges that are used exactly once in each direction"""
    f = np.asarray(faces, np.int64)
    if not len(f):
        return 1.0
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    und = np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1])
    keys, inv = np.unique(und, return_inverse=True)
    inv = inv.reshape(-1)
    lo_first = (e[:, 0] < e[:, 1])
    a = np.bincount(inv, weights=lo_first, minlength=len(keys))
    b = np.bincount(inv, weights=~lo_first, minlength=len(keys))
    return float(((a == 1) & (b == 1)).sum() / len(keys))


def outward_share(verts, faces, centre=(0.0, 0.0, 0.0)):
    """the share of faces whose normal points away from the centre"""
    p = verts[faces] - np.asarray(centre)[None, None, :]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return float(((nrm * p.mean(1)).sum(1) > 0).mean()) if len(faces) else 1.0


def radius_error(verts, faces, voxel, radius=0.1):
    """(RMS, max) of |r - radius| / voxel over the vertices a face uses"""
    used = np.zeros(len(verts), bool)
    used[np.asarray(faces).ravel()] = True
    e = np.abs(np.linalg.norm(verts[used], axis=1) - radius) / voxel
    return float(np.sqrt((e * e).mean())), float(e.max())
