"""NumPy restatement of multi-pair depth fusion (TSDF integration) and marching-tetrahedra surface extraction, written from
the definition (DESIGN.md "Multi-pair depth fusion"), not from the kernels.

Integration is IEEE double in one fixed expression order per view; extraction derives its triangle table from the rule
itself (no copied table).  The device results must equal these bit for bit.
"""
from __future__ import annotations

import itertools

import numpy as np

DEFAULTS = dict(trunc=0.0, disp_min=1.0, min_weight=1, max_views=64)
# the 7 positive edge directions of a cell, slot 0..6
D7 = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)], np.int64)
# corner index b = bx + 2 by + 4 bz  ->  slot of the direction b (b != 0)
_SLOT_OF_MASK = {int(d[0] + 2 * d[1] + 4 * d[2]): s for s, d in enumerate(D7)}


def corner_xyz(b):
    return np.array([b & 1, (b >> 1) & 1, (b >> 2) & 1], np.int64)


def tets():
    """the six Kuhn tetrahedra of a cell as corner chains (0, e_a, e_a + e_b, 7), permutations in lexicographic order"""
    out = []
    for perm in itertools.permutations(range(3)):
        a, b = perm[0], perm[1]
        out.append((0, 1 << a, (1 << a) | (1 << b), 7))
    return out


def make_table():
    """ntri [6][16] and tri [6][16][2][3] (each entry (lower corner, slot) of a tet edge; -1 where unused).
    case bit q = chain corner q is inside."""
    ntri = np.zeros((6, 16), np.int64)
    tri = -np.ones((6, 16, 2, 3, 2), np.int64)
    for t, chain in enumerate(tets()):
        P = [corner_xyz(c) for c in chain]
        for case in range(16):
            ins = [q for q in range(4) if (case >> q) & 1]
            out = [q for q in range(4) if not (case >> q) & 1]
            if len(ins) in (0, 4):
                continue
            if len(ins) == 2:
                a, b = ins
                c, d = out
                tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
            else:
                lone = ins[0] if len(ins) == 1 else out[0]
                others = [q for q in range(4) if q != lone]
                tris = [[(lone, o) for o in others]]
            # orientation: cross(p1 - p0, p2 - p0) . (centroid(out) - centroid(in)) > 0, vertices at edge midpoints
            # (all coordinates x2 and the centroids x |in| |out|, so everything is an integer)
            dirv = sum(P[q] for q in out) * len(ins) - sum(P[q] for q in ins) * len(out)
            for k, tr in enumerate(tris):
                m = [P[e[0]] + P[e[1]] for e in tr]
                s = int(np.dot(np.cross(m[1] - m[0], m[2] - m[0]), dirv))
                assert s != 0
                if s < 0:
                    tr = [tr[0], tr[2], tr[1]]
                for v, (q0, q1) in enumerate(tr):
                    lo, hi = sorted((chain[q0], chain[q1]))
                    tri[t, case, k, v] = (lo, _SLOT_OF_MASK[hi ^ lo])
            ntri[t, case] = len(tris)
    return ntri, tri


NTRI, TRI = make_table()


def resolve(voxel, trunc=0.0, **_):
    return 4.0 * voxel if trunc == 0.0 else trunc


def grid_x(origin, voxel, dims):
    """per-axis world coordinates of the grid points: ox + (double)i * vs"""
    return [float(origin[a]) + np.arange(dims[a], dtype=np.float64) * float(voxel) for a in range(3)]


def integrate(origin, voxel, dims, views, trunc=0.0, disp_min=1.0, sum_=None, count=None):
    """views: list of (cam, disp16) with cam = dict(R_rw, c_left, f, cx, cy, B); returns (sum, count) [nz][ny][nx]"""
    nx, ny, nz = dims
    trunc = resolve(voxel, trunc)
    sum_ = np.zeros((nz, ny, nx)) if sum_ is None else sum_.copy()
    count = np.zeros((nz, ny, nx), np.int32) if count is None else count.copy()
    gx, gy, gz = grid_x(origin, voxel, dims)
    X0 = np.broadcast_to(gx[None, None, :], (nz, ny, nx)).ravel()
    X1 = np.broadcast_to(gy[None, :, None], (nz, ny, nx)).ravel()
    X2 = np.broadcast_to(gz[:, None, None], (nz, ny, nx)).ravel()
    s, c = sum_.ravel(), count.ravel()
    for cam, d16 in views:
        R = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
        cl = np.asarray(cam["c_left"], np.float64).reshape(3)
        f, cx, cy, B = float(cam["f"]), float(cam["cx"]), float(cam["cy"]), float(cam["B"])
        d16 = np.asarray(d16, np.int16)
        h, w = d16.shape
        p0, p1, p2 = X0 - cl[0], X1 - cl[1], X2 - cl[2]
        q = [(R[r, 0] * p0 + R[r, 1] * p1) + R[r, 2] * p2 for r in range(3)]
        ok = q[2] > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u = (f * q[0]) / q[2] + cx
            v = (f * q[1]) / q[2] + cy
            x = np.floor(u + 0.5)
            y = np.floor(v + 0.5)
        ok &= (x >= 0) & (x < w) & (y >= 0) & (y < h)
        idx = np.nonzero(ok)[0]
        d = d16[y[idx].astype(np.int64), x[idx].astype(np.int64)]
        dd = d.astype(np.float64) / 16.0
        good = (d != -16) & (dd >= disp_min)
        idx, dd = idx[good], dd[good]
        Z = (f * B) / dd
        sdf = Z - q[2][idx]
        keep = ~(sdf < -trunc)
        idx, sdf = idx[keep], sdf[keep]
        t = np.where(sdf >= trunc, 1.0, sdf / trunc)
        s[idx] += t
        c[idx] += 1
    return s.reshape(nz, ny, nx), c.reshape(nz, ny, nx)


def values(sum_, count, min_weight=1):
    """s(g) = sum / count where count >= min_weight, NaN (undefined) elsewhere"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count >= min_weight, sum_ / count.astype(np.float64), np.nan)


def extract(sum_, count, origin, voxel, min_weight=1):
    """marching tetrahedra on the Kuhn split: (verts [n][3] f64, faces [m][3] i32)"""
    nz, ny, nx = sum_.shape
    S = values(sum_, count, min_weight)
    k, j, i = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    k, j, i = k.ravel(), j.ravel(), i.ravel()
    L = i + nx * (j + ny * k)
    corner = np.stack([S[k + ((b >> 2) & 1), j + ((b >> 1) & 1), i + (b & 1)] for b in range(8)], 1)
    ok = ~np.isnan(corner).any(1)
    L, corner = L[ok], corner[ok]
    inside = corner < 0
    keys, edges = [], []
    for t, chain in enumerate(tets()):
        case = sum(inside[:, chain[q]].astype(np.int64) << q for q in range(4))
        n = NTRI[t, case]
        for tr in range(2):
            sel = np.nonzero(n > tr)[0]
            if len(sel) == 0:
                continue
            e = TRI[t, case[sel], tr]  # [m][3][2]: (lower corner, slot)
            lo = e[..., 0]
            Lg = L[sel][:, None] + (lo & 1) + nx * (((lo >> 1) & 1) + ny * ((lo >> 2) & 1))
            edges.append(7 * Lg + e[..., 1])
            keys.append((L[sel] * 6 + t) * 2 + tr)
    if not keys:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    keys = np.concatenate(keys)
    edges = np.concatenate(edges)
    order = np.argsort(keys, kind="stable")
    edges = edges[order]
    uniq = np.unique(edges)
    faces = np.searchsorted(uniq, edges).astype(np.int32)
    Lg, slot = uniq // 7, uniq % 7
    gi, gj, gk = Lg % nx, (Lg // nx) % ny, Lg // (nx * ny)
    d = D7[slot]
    sg = S[gk, gj, gi]
    sq = S[gk + d[:, 2], gj + d[:, 1], gi + d[:, 0]]
    t = sg / (sg - sq)
    verts = np.zeros((len(uniq), 3))
    for a, (g, dd) in enumerate(((gi, d[:, 0]), (gj, d[:, 1]), (gk, d[:, 2]))):
        Xg = float(origin[a]) + g.astype(np.float64) * float(voxel)
        Xq = float(origin[a]) + (g + dd).astype(np.float64) * float(voxel)
        verts[:, a] = Xg + t * (Xq - Xg)
    return verts, faces


def fuse(origin, voxel, dims, views, trunc=0.0, disp_min=1.0, min_weight=1):
    s, c = integrate(origin, voxel, dims, views, trunc, disp_min)
    v, f = extract(s, c, origin, voxel, min_weight)
    return dict(sum=s, count=c, verts=v, faces=f)


# ---- test geometry ---------------------------------------------------------------------------------------------------
def look_at_cam(centre, target, f, w, h, B=0.05):
    """a rectified left camera at `centre` looking at `target` (rows of R_rw: camera axes in world coordinates)"""
    centre = np.asarray(centre, np.float64)
    z = np.asarray(target, np.float64) - centre
    z /= np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return dict(R_rw=np.stack([x, y, z]), c_left=centre, f=float(f), cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, B=float(B))


def sphere_disp16(cam, w, h, radius, centre=(0.0, 0.0, 0.0)):
    """analytic disparity map of a sphere seen by a rectified camera: rint(16 f B / Z), Z the ray's depth; -16 on a miss"""
    R = np.asarray(cam["R_rw"], np.float64)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    dc = np.stack([(x - cam["cx"]) / cam["f"], (y - cam["cy"]) / cam["f"], np.ones_like(x)], -1)  # depth-1 ray, camera frame
    dw = dc @ R  # world direction (R_rw^T dc)
    oc = np.asarray(cam["c_left"], np.float64) - np.asarray(centre, np.float64)
    a = (dw * dw).sum(-1)
    b = 2.0 * (dw @ oc)
    c = oc @ oc - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    Z = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), np.inf)
    d = np.rint(16.0 * cam["f"] * cam["B"] / Z)
    return np.where(hit & (Z > 0), d, -16).astype(np.int16)


def fibonacci_dirs(n):
    k = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * k / n)
    th = np.pi * (1 + 5 ** 0.5) * k
    return np.stack([np.cos(th) * np.sin(phi), np.cos(phi), np.sin(th) * np.sin(phi)], 1)
