"""NumPy restatement of shape from silhouette (DESIGN.md "Carving with silhouettes"): the signed squared distance map of a
silhouette, the visual hull of a set of views on the fusion grid, and carving / overwriting a fusion volume with it.  Written from
the definition, not from the kernels.

The distance map is integer; the hull is IEEE double in one fixed expression order per view and a max over the views.  The device
results must equal these byte for byte.  Views are (cam, sd2) with cam = dict(R_rw, c_left, f, cx, cy) as in tests/fusion_ref.py
(B is not used).
"""
from __future__ import annotations

import numpy as np

import appearance_ref as AR
import consist_ref as CR
import fusion_ref as FR

DEFAULTS = dict(cap=16, min_views=1, margin=0.5, mode="intersect", trunc=0.0)
MODES = ("intersect", "clear")
ROW_TILE = 256  # pixels of a row one block of the device's row pass takes (the shapes of the GPU suite straddle it)


def check_params(cap=16, min_views=1, margin=0.5, mode="intersect", trunc=0.0) -> bool:
    if not (isinstance(cap, (int, np.integer)) and 1 <= cap <= 64 and min_views >= 1):
        return False
    if not (np.isfinite(margin) and 0.0 <= margin < 1.0):
        return False
    if mode not in MODES and mode not in (0, 1):
        return False
    return bool(np.isfinite(trunc) and trunc >= 0.0)


# ---- the signed squared distance map ------------------------------------------------------------------------------------------
def sd2_brute(image, threshold=1, cap=16):
    """the definition as a search: every pixel against every pixel of the other class"""
    I = np.asarray(image, np.uint8)
    h, w = I.shape
    m = I >= threshold
    y, x = np.mgrid[0:h, 0:w]
    D2 = np.full((h, w), cap * cap, np.int64)
    for cls in (False, True):
        oy, ox = np.nonzero(m != cls)  # the other class's pixels
        sy, sx = y[m == cls], x[m == cls]
        if len(oy) == 0 or len(sy) == 0:
            continue
        best = np.full(len(sy), cap * cap, np.int64)
        for s in range(0, len(oy), 4096):
            d = (sx[:, None] - ox[None, s:s + 4096]) ** 2 + (sy[:, None] - oy[None, s:s + 4096]) ** 2
            best = np.minimum(best, d.min(1))
        D2[m == cls] = best
    return np.where(m, -D2, D2).astype(np.int16)


def sd2_map(image, threshold=1, cap=16):
    """the same map by two separable passes: the vertical distance to the other class in each column (window +- cap), then
    min(dx^2 + g^2) over |dx| <= cap along the row"""
    I = np.asarray(image, np.uint8)
    h, w = I.shape
    m = I >= threshold
    BIG = 1 << 20
    g = np.full((h, w), BIG, np.int64)  # vertical distance to the nearest pixel of the other class in the column
    for d in range(cap, 0, -1):
        up = np.zeros((h, w), bool)
        dn = np.zeros((h, w), bool)
        if d < h:
            up[d:] = m[d:] != m[:-d]
            dn[:-d] = m[:-d] != m[d:]
        g[up | dn] = d
    g2 = np.where(g < BIG, g * g, BIG)
    D2 = np.minimum(g2, cap * cap)
    for dx in range(1, cap + 1):
        if dx >= w:
            break
        for sgn in (-1, 1):
            src = slice(dx, w) if sgn > 0 else slice(0, w - dx)  # the neighbour's column
            dst = slice(0, w - dx) if sgn > 0 else slice(dx, w)  # the pixel's
            cand = np.where(m[:, src] != m[:, dst], dx * dx, dx * dx + g2[:, src])
            D2[:, dst] = np.minimum(D2[:, dst], cand)
    return np.where(m, -D2, D2).astype(np.int16)


# ---- the hull ------------------------------------------------------------------------------------------------------------------
def table(cap):
    return np.sqrt(np.arange(cap * cap + 1, dtype=np.float64)) - 0.5


def hull(origin, voxel, dims, views, cap=16, min_views=1, trunc=0.0, counter=None):
    """views: list of (cam, sd2 int16 [h][w]).  Returns (hull f64, views i32) [nz][ny][nx]; a point is defined where views >=
    min_views.  counter (a dict) collects how many (point, view) tests ended behind the camera / outside the image / clamped."""
    nx, ny, nz = dims
    trunc = FR.resolve(voxel, trunc)
    tab = table(cap)
    gx, gy, gz = FR.grid_x(origin, voxel, dims)
    X0 = np.broadcast_to(gx[None, None, :], (nz, ny, nx)).ravel()
    X1 = np.broadcast_to(gy[None, :, None], (nz, ny, nx)).ravel()
    X2 = np.broadcast_to(gz[:, None, None], (nz, ny, nx)).ravel()
    H = np.full(nx * ny * nz, -1.0)
    n = np.zeros(nx * ny * nz, np.int32)
    for cam, sd2 in views:
        R = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
        cl = np.asarray(cam["c_left"], np.float64).reshape(3)
        f, cx, cy = float(cam["f"]), float(cam["cx"]), float(cam["cy"])
        sd2 = np.asarray(sd2, np.int16)
        assert int(np.abs(sd2.astype(np.int64)).max()) <= cap * cap and (sd2 != 0).all(), "a map of another cap"
        h, w = sd2.shape
        ft = f * trunc
        p0, p1, p2 = X0 - cl[0], X1 - cl[1], X2 - cl[2]
        q = [(R[r, 0] * p0 + R[r, 1] * p1) + R[r, 2] * p2 for r in range(3)]
        front = q[2] > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u = (f * q[0]) / q[2] + cx
            v = (f * q[1]) / q[2] + cy
            x = np.floor(u + 0.5)
            y = np.floor(v + 0.5)
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        idx = np.nonzero(front & inside)[0]
        k = sd2[y[idx].astype(np.int64), x[idx].astype(np.int64)].astype(np.int64)
        d = np.where(k < 0, -tab[np.abs(k)], tab[np.abs(k)])
        t = (d * q[2][idx]) / ft
        if counter is not None:
            for name, c in (("behind", (~front).sum()), ("outside", (front & ~inside).sum()), ("clamp_hi", (t >= 1.0).sum()),
                            ("clamp_lo", (t <= -1.0).sum())):
                counter[name] = counter.get(name, 0) + int(c)
        t = np.where(t >= 1.0, 1.0, np.where(t <= -1.0, -1.0, t))
        H[idx] = np.where(t > H[idx], t, H[idx])
        n[idx] += 1
    return H.reshape(nz, ny, nx), n.reshape(nz, ny, nx)


# ---- into a fusion volume -----------------------------------------------------------------------------------------------------
def store(hull_, views_, min_views=1, min_weight=1):
    """(sum, count) that hold the hull: count W and sum hull * W where defined, zeros elsewhere; W = max(1, min_weight)"""
    W = max(1, int(min_weight))
    defined = views_ >= min_views
    return np.where(defined, hull_ * float(W), 0.0), np.where(defined, W, 0).astype(np.int32)


def apply(sum_, count, hull_, views_, min_views=1, margin=0.5, mode="intersect", min_weight=1):
    """the carved (sum, count) and dict(defined, outside, changed); changed counts the points whose sum or count bits differ"""
    W = max(1, int(min_weight))
    s1, c1 = np.array(sum_, np.float64), np.array(count, np.int32)
    defined = views_ >= min_views
    out = defined & (hull_ > margin)
    hm = hull_ - margin
    if mode in ("clear", 1):
        c1[out] = 0
        s1[out] = 0.0
    else:
        was = count >= min_weight
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(was, sum_ / count.astype(np.float64), 0.0)
        v = np.where(was, np.where(s > hm, s, hm), hm)
        write = out & (~was | (hm > s))
        c1[write] = W
        s1[write] = (v * float(W))[write]
    changed = (c1 != count) | (s1.view(np.int64) != np.asarray(sum_, np.float64).view(np.int64))
    return s1, c1, dict(defined=int(defined.sum()), outside=int(out.sum()), changed=int(changed.sum()))


# ---- fixtures --------------------------------------------------------------------------------------------------------------
_cache = {}


def sphere_silhouettes(cap=16):
    """DESIGN.md 13's sphere-26 fixture with its pictures (appearance_ref): [(cam, sd2)], the pictures and the disparity maps"""
    if ("sil", cap) not in _cache:
        tv = AR.textured_sphere_views()
        _cache["sil", cap] = ([(cam, sd2_map(img, 1, cap)) for cam, _, img in tv], [img for _, _, img in tv], [d for _, d, _ in tv])
    return _cache["sil", cap]


def sphere_hull(n_views=26):
    """(hull, views) of the first n_views sphere silhouettes on the sphere-26 volume, defaults"""
    if ("hull", n_views) not in _cache:
        V = CR.SPHERE26_VOL
        _cache["hull", n_views] = hull(V["origin"], V["voxel"], V["dims"], sphere_silhouettes()[0][:n_views])
    return _cache["hull", n_views]


def sphere_volume(noisy):
    """the integrated sphere-26 volume (sum, count), clean or with 5 % outliers"""
    if ("vol", noisy) not in _cache:
        V = CR.SPHERE26_VOL
        views, _ = CR.sphere26(noisy)
        _cache["vol", noisy] = FR.integrate(V["origin"], V["voxel"], V["dims"], views)
    return _cache["vol", noisy]


def radius_error(verts, voxel=CR.SPHERE26_VOL["voxel"]):
    """(RMS, min, max, vertices more than a voxel outside, more than a voxel inside) of the radius error in voxels"""
    e = (np.linalg.norm(verts, axis=1) - CR.RADIUS) / voxel
    return float(np.sqrt((e ** 2).mean())), float(e.min()), float(e.max()), int((e > 1.0).sum()), int((e < -1.0).sum())


def closed_euler(faces, n_verts):
    """(every directed edge appears once and its reverse once, V - E + F)"""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * n_verts + e[:, 1]
    rev = e[:, 1] * n_verts + e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    closed = bool((cnt == 1).all() and np.isin(rev, uniq).all())
    return closed, int(n_verts - len(uniq) // 2 + len(faces))
