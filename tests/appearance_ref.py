"""NumPy restatement of the appearance stages of the fused surface -- vertex normals from the volume's gradient and vertex
intensity from the views that see the vertex -- written from the definition ("Appearance of the fused surface"),
not from the kernels.  The volume, its values s(g) and the triangle table come from fusion_ref.

Everything up to the depth test is IEEE double in the definition's expression order; everything after it is int32.  The device
results must equal these bit for bit.
"""
from __future__ import annotations

import numpy as np

import fusion_ref as FR


# ---- which edges carry a vertex ----------------------------------------------------------------------------------------------
def surface_edges(S):
    """ascending ids 7 L(g) + slot of the edges the extraction's triangles use (S = fusion_ref.values: NaN = undefined).
    The same cells, cases and table as fusion_ref.extract; only the ids are kept."""
    nz, ny, nx = S.shape
    k, j, i = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    k, j, i = k.ravel(), j.ravel(), i.ravel()
    L = i + nx * (j + ny * k)
    corner = np.stack([S[k + ((b >> 2) & 1), j + ((b >> 1) & 1), i + (b & 1)] for b in range(8)], 1)
    ok = ~np.isnan(corner).any(1)
    L, inside = L[ok], corner[ok] < 0
    ids = []
    for t, chain in enumerate(FR.tets()):
        case = sum(inside[:, chain[q]].astype(np.int64) << q for q in range(4))
        n = FR.NTRI[t, case]
        for tr in range(2):
            sel = np.nonzero(n > tr)[0]
            if len(sel):
                e = FR.TRI[t, case[sel], tr]
                lo = e[..., 0]
                Lg = L[sel][:, None] + (lo & 1) + nx * (((lo >> 1) & 1) + ny * ((lo >> 2) & 1))
                ids.append((7 * Lg + e[..., 1]).ravel())
    return np.unique(np.concatenate(ids)) if ids else np.zeros(0, np.int64)


# ---- normals -----------------------------------------------------------------------------------------------------------------
def gradient(S):
    """G [3][nz][ny][nx] (axis 0 = x) and the branch taken per axis and grid point: 0 neither, 1 only g - e, 2 only g + e,
    3 both (central).  Values at undefined grid points are meaningless and never used."""
    P = np.pad(S, 1, constant_values=np.nan)
    core = (slice(1, -1),) * 3
    G, branch = [], []
    for axis in (2, 1, 0):  # x is the last array axis
        hi = [slice(1, -1)] * 3
        lo = [slice(1, -1)] * 3
        hi[axis] = slice(2, None)
        lo[axis] = slice(0, -2)
        sp, sm, s = P[tuple(hi)], P[tuple(lo)], P[core]
        dp, dm = ~np.isnan(sp), ~np.isnan(sm)
        with np.errstate(invalid="ignore"):
            central = (sp - sm) * 0.5
            fwd = sp - s
            bwd = s - sm
        G.append(np.where(dp & dm, central, np.where(dp, fwd, np.where(dm, bwd, 0.0))))
        branch.append(dp.astype(np.int8) * 2 + dm.astype(np.int8))
    return np.stack(G), np.stack(branch)


def normals(sum_, count, min_weight=1, with_branches=False):
    """normals [n][3] f64 of fusion_ref.extract's vertices, in its vertex order (ascending 7 L + slot)"""
    nz, ny, nx = sum_.shape
    S = FR.values(sum_, count, min_weight)
    ids = surface_edges(S)
    if len(ids) == 0:
        return (np.zeros((0, 3)), np.zeros((0, 2, 3), np.int8)) if with_branches else np.zeros((0, 3))
    G, branch = gradient(S)
    Lg, slot = ids // 7, ids % 7
    gi, gj, gk = Lg % nx, (Lg // nx) % ny, Lg // (nx * ny)
    d = FR.D7[slot]
    qi, qj, qk = gi + d[:, 0], gj + d[:, 1], gk + d[:, 2]
    sg, sq = S[gk, gj, gi], S[qk, qj, qi]
    t = sg / (sg - sq)
    N = [G[a][gk, gj, gi] + t * (G[a][qk, qj, qi] - G[a][gk, gj, gi]) for a in range(3)]
    ln = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.stack([np.where(ln > 0, N[a] / ln, 0.0) for a in range(3)], 1)
    if with_branches:
        br = np.stack([branch[:, gk, gj, gi].T, branch[:, qk, qj, qi].T], 1)  # [n][endpoint][axis]
        return out, br
    return out


# ---- intensity ---------------------------------------------------------------------------------------------------------------
def shade_accumulate(verts, nrm, views, depth_tol, disp_min=1.0, cull=1, acc=None, cnt=None):
    """adds `views` (list of (cam, disp16, image)) to the int32 running sums acc / cnt of every vertex"""
    n = len(verts)
    acc = np.zeros(n, np.int32) if acc is None else acc.copy()
    cnt = np.zeros(n, np.int32) if cnt is None else cnt.copy()
    X = np.asarray(verts, np.float64).reshape(n, 3)
    for cam, d16, img in views:
        R = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
        cl = np.asarray(cam["c_left"], np.float64).reshape(3)
        f, cx, cy, B = float(cam["f"]), float(cam["cx"]), float(cam["cy"]), float(cam["B"])
        d16 = np.asarray(d16, np.int16)
        img = np.asarray(img, np.uint8)
        h, w = d16.shape
        assert img.shape == (h, w)
        p0, p1, p2 = X[:, 0] - cl[0], X[:, 1] - cl[1], X[:, 2] - cl[2]
        q = [(R[r, 0] * p0 + R[r, 1] * p1) + R[r, 2] * p2 for r in range(3)]
        ok = q[2] > 0
        if cull:
            ok &= ((nrm[:, 0] * p0 + nrm[:, 1] * p1) + nrm[:, 2] * p2) < 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u = (f * q[0]) / q[2] + cx
            v = (f * q[1]) / q[2] + cy
            x = np.floor(u + 0.5)
            y = np.floor(v + 0.5)
        ok &= (x >= 0) & (x < w) & (y >= 0) & (y < h)
        idx = np.nonzero(ok)[0]
        yy, xx = y[idx].astype(np.int64), x[idx].astype(np.int64)
        d = d16[yy, xx]
        dd = d.astype(np.float64) / 16.0
        good = (d != -16) & (dd >= disp_min)
        idx, yy, xx, dd = idx[good], yy[good], xx[good], dd[good]
        with np.errstate(divide="ignore"):  # a disparity of 0 under disp_min <= 0: Z = +inf, never within a finite tolerance
            Z = (f * B) / dd
        near = np.abs(Z - q[2][idx]) <= depth_tol
        idx, yy, xx = idx[near], yy[near], xx[near]
        acc[idx] += img[yy, xx].astype(np.int32)
        cnt[idx] += 1
    return acc, cnt


def shade(verts, nrm, views, depth_tol, disp_min=1.0, cull=1, fill=0, chunk=None):
    """(grey u8 [n], views i32 [n]); chunk: views per accumulate call (the result cannot depend on it)"""
    views = list(views)
    if nrm is None:
        assert not cull
        nrm = np.zeros((len(verts), 3))
    step = len(views) if not chunk else int(chunk)
    acc = cnt = None
    for a in range(0, len(views), max(step, 1)):
        acc, cnt = shade_accumulate(verts, nrm, views[a:a + step], depth_tol, disp_min, cull, acc, cnt)
    if acc is None:
        acc, cnt = np.zeros(len(verts), np.int32), np.zeros(len(verts), np.int32)
    grey = np.where(cnt > 0, (2 * acc + cnt) // np.maximum(2 * cnt, 1), int(fill)).astype(np.uint8)
    return grey, cnt


def fuse(origin, voxel, dims, views, depth_tol=None, trunc=0.0, disp_min=1.0, min_weight=1, cull=1, fill=0):
    """fusion_ref.fuse on (cam, disp16, image) views plus normals, grey, vertex_views; depth_tol None = the resolved trunc"""
    r = FR.fuse(origin, voxel, dims, [(c, d) for c, d, _ in views], trunc, disp_min, min_weight)
    r["normals"] = normals(r["sum"], r["count"], min_weight)
    assert len(r["normals"]) == len(r["verts"])
    tol = FR.resolve(voxel, trunc) if depth_tol is None else depth_tol
    r["grey"], r["vertex_views"] = shade(r["verts"], r["normals"], views, tol, disp_min, cull, fill)
    return r


# ---- test scenes -------------------------------------------------------------------------------------------------------------
def texture(X):
    """T(X) = 128 + 60 sin(25 x) cos(25 y) + 40 sin(30 z): a smooth pattern in [28, 228]"""
    X = np.asarray(X, np.float64)
    return 128.0 + 60.0 * np.sin(25.0 * X[..., 0]) * np.cos(25.0 * X[..., 1]) + 40.0 * np.sin(30.0 * X[..., 2])


def sphere_hits(cam, w, h, radius, centre=(0.0, 0.0, 0.0)):
    """(hit [h][w] bool, P [h][w][3] world hit point of each pixel's ray on the sphere): fusion_ref.sphere_disp16's rays"""
    R = np.asarray(cam["R_rw"], np.float64)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    dc = np.stack([(x - cam["cx"]) / cam["f"], (y - cam["cy"]) / cam["f"], np.ones_like(x)], -1)
    dw = dc @ R
    c0 = np.asarray(cam["c_left"], np.float64)
    oc = c0 - np.asarray(centre, np.float64)
    a = (dw * dw).sum(-1)
    b = 2.0 * (dw @ oc)
    c = oc @ oc - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    Z = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), 0.0)
    hit &= Z > 0
    return hit, c0 + Z[..., None] * dw


def textured_sphere_views(radius=0.1, w=320, h=320, f=600.0, n_views=26):
    """test_fusion_cpu's sphere views with an image each: rint(T(hit point)), 0 on a miss"""
    out = []
    for d in FR.fibonacci_dirs(n_views):
        cam = FR.look_at_cam(0.5 * d, (0.0, 0.0, 0.0), f, w, h)
        hit, P = sphere_hits(cam, w, h, radius)
        img = np.where(hit, np.rint(texture(P)), 0.0).astype(np.uint8)
        out.append((cam, FR.sphere_disp16(cam, w, h, radius), img))
    return out


TWO = dict(A=dict(radius=0.08, centre=(0.0, 0.0, 0.0), grey=80), B=dict(radius=0.03, centre=(0.15, 0.0, 0.0), grey=200))
TWO_VOL = dict(origin=(-0.2, -0.2, -0.2), voxel=0.004, dims=(101, 101, 101))


def two_sphere_views(w=320, h=320, f=600.0, n_views=26):
    """a large and a small sphere that hide each other from some cameras: per pixel the nearer one's (larger) disparity and
    that sphere's constant grey, 0 on a miss"""
    out = []
    for d in FR.fibonacci_dirs(n_views):
        cam = FR.look_at_cam(0.5 * d, (0.0, 0.0, 0.0), f, w, h)
        dA = FR.sphere_disp16(cam, w, h, TWO["A"]["radius"], TWO["A"]["centre"])
        dB = FR.sphere_disp16(cam, w, h, TWO["B"]["radius"], TWO["B"]["centre"])
        d16 = np.maximum(dA, dB)
        img = np.where(d16 == -16, 0, np.where(dA >= dB, TWO["A"]["grey"], TWO["B"]["grey"])).astype(np.uint8)
        out.append((cam, d16, img))
    return out


def two_sphere_labels(verts, tol=0.006):
    """(on A, on B): vertices within tol of each sphere's surface"""
    on = []
    for s in (TWO["A"], TWO["B"]):
        r = np.linalg.norm(verts - np.asarray(s["centre"], np.float64), axis=1)
        on.append(np.abs(r - s["radius"]) < tol)
    return on[0], on[1]
