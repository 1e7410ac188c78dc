"""NumPy restatement of the small-component removal of DESIGN.md 16 (sfmx_clean_*), and the meshes its tests share.

Components come from scipy when it is importable, else from the union-find fallback (tests/stereo_ref._components); their
labels are turned into smallest-index labels here.  Everything else is NumPy on integers, so the device result is compared
byte for byte."""
import numpy as np

import stereo_ref as SR

DEFAULTS = dict(min_faces=0, min_permille=10)


def labels(n, faces):
    """int32 [n]: the smallest vertex index of every vertex's component"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if n == 0:
        return np.zeros(0, np.int32)
    a = np.concatenate([faces[:, 0], faces[:, 0]])
    b = np.concatenate([faces[:, 1], faces[:, 2]])
    comp = np.asarray(SR._components(n, a, b), np.int64) if len(a) else np.arange(n)
    first = np.full(int(comp.max()) + 1, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp].astype(np.int32)


def clean(verts, faces, normals=None, min_faces=0, min_permille=10):
    """dict(verts, faces, vert_src, face_src, label, comp_faces, n_verts, n_faces, components, largest[, normals]); a face
    index outside [0, n) raises ValueError"""
    verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    n, m = len(verts), len(faces)
    if m and (faces.min() < 0 or faces.max() >= n):
        raise ValueError("face index out of range")
    lab = labels(n, faces)
    cnt = np.bincount(lab[faces[:, 0]], minlength=n).astype(np.int64) if m else np.zeros(n, np.int64)
    largest = int(cnt.max()) if n and m else 0
    keep_c = (cnt >= 1) & (cnt >= min_faces) & (cnt * 1000 >= largest * int(min_permille))
    fkeep = keep_c[lab[faces[:, 0]]] if m else np.zeros(0, bool)
    vkeep = np.zeros(n, bool)
    vkeep[faces[fkeep].ravel()] = True
    vert_src = np.nonzero(vkeep)[0].astype(np.int32)
    face_src = np.nonzero(fkeep)[0].astype(np.int32)
    remap = np.cumsum(vkeep) - 1
    out = dict(verts=verts[vert_src].copy(), faces=remap[faces[face_src]].astype(np.int32).reshape(-1, 3), vert_src=vert_src,
               face_src=face_src, label=lab, comp_faces=cnt[lab].astype(np.int32), n_verts=len(vert_src), n_faces=len(face_src),
               components=int((cnt > 0).sum()), largest=largest)
    if normals is not None:
        out["normals"] = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)[vert_src].copy()
    return out


def counts(ref):
    return {k: ref[k] for k in ("n_verts", "n_faces", "components", "largest")}


def kept_labels(ref):
    """the labels of the kept components"""
    return set(np.unique(ref["label"][ref["vert_src"]]).tolist())


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def _verts(n, seed=0):
    """distinct, reproducible vertex bytes (a NaN and an infinity among them: they are copied, never computed with)"""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    if n > 2:
        v[1, 0], v[2, 1] = np.nan, -np.inf
    return v


def disjoint_triangles(m, k):
    """m triangles on 3 m vertices; every k-th one shares its first vertex's component with the next (face 3 i + 2 -> the next
    triangle's first vertex), so components of 1 and of 2 faces mix"""
    f = np.arange(3 * m, dtype=np.int32).reshape(m, 3)
    assert k >= 2  # never chains of three
    j = np.arange(0, m - 1, k)
    f[j, 2] = f[j + 1, 0]  # vertex 3 j + 2 is now unused
    return _verts(3 * m, m), f


def strip(m, order, seed=5):
    """an m-face triangle strip over m + 2 vertices, their indices ascending, descending or permuted"""
    i = np.arange(m, dtype=np.int64)
    f = np.stack([i, i + 1, i + 2], 1)
    n = m + 2
    if order == "descending":
        f = n - 1 - f
    elif order == "permuted":
        f = np.random.default_rng(seed).permutation(n)[f]
    return _verts(n, 1), f.astype(np.int32)


def soup(n=20000, m=15000, seed=7):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    f = rng.integers(0, n, (m, 3)).astype(np.int32)
    return v, f, rng.standard_normal((n, 3))


# ---- calibration surfaces -----------------------------------------------------------------------------------
RING_SHELL = (0.065, 0.105)


def ring_off_shell(verts):
    r = np.linalg.norm(verts, axis=1)
    return (r < RING_SHELL[0]) | (r > RING_SHELL[1])


def sphere_off_shell(verts, voxel, radius=0.1):
    return np.abs((np.linalg.norm(verts, axis=1) - radius) / voxel) > 1.0


def figures(verts, faces, off, **params):
    """one row of DESIGN.md 16's table: dict(components, faces, largest, second, off_before, off_after, on_dropped, faces_after)"""
    r = clean(verts, faces, **params)
    sizes = np.sort(np.bincount(r["label"][faces[:, 0]], minlength=len(verts)))[::-1]
    kept = np.zeros(len(verts), bool)
    kept[r["vert_src"]] = True
    return dict(components=r["components"], faces=len(faces), largest=r["largest"], second=int(sizes[1]) if len(sizes) > 1 else 0,
                off_before=int(off.sum()), off_after=int((off & kept).sum()), on_dropped=int((~off & ~kept).sum()),
                faces_after=r["n_faces"], ref=r)
