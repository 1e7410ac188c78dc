"""NumPy restatement of the keyframe-pair stereo stages (rectify, census, cost, 4-path SGM, select, speckle) and of the
grid mesh, written from the algorithm's definition (DESIGN.md "Keyframe-pair stereo mesh"), not from the kernels.

Every stage is integer arithmetic or IEEE double with a fixed expression order, so the device results must equal these
bit for bit.  Poses are camera->world (R, centre c), as the pipeline keeps them.
"""
from __future__ import annotations

import math

import numpy as np

DEFAULTS = dict(num_disparities=128, census=5, p1=8, p2=96, uniqueness=10, lr_max_diff=1, speckle_window=100,
                speckle_range=2)
MESH_DEFAULTS = dict(step=4, disp_min=1.0, disp_jump=3.0, z_max_percentile=98.0)
INVALID_BIT = np.uint64(1) << np.uint64(63)


# ---- host geometry --------------------------------------------------------------------------------------------------
def rectify(K, Ra, ca, Rb, cb):
    """dict(R_rw, c_left, c_right, f, cx, cy, B, swapped, H_l, H_r); H_* map a rectified pixel to a source pixel."""
    K = np.asarray(K, np.float64)
    Ra, Rb = np.asarray(Ra, np.float64), np.asarray(Rb, np.float64)
    ca, cb = np.asarray(ca, np.float64), np.asarray(cb, np.float64)
    base = cb - ca
    if np.linalg.norm(base) == 0.0:
        raise ValueError("zero baseline")
    x = base / np.linalg.norm(base)
    swapped = float(x @ Ra[:, 0]) < 0.0
    if swapped:
        Ra, Rb, ca, cb = Rb, Ra, cb, ca
        x = (cb - ca) / np.linalg.norm(cb - ca)
    y = np.cross(Ra[:, 2] + Rb[:, 2], x)
    y /= np.linalg.norm(y)
    z = np.cross(x, y)
    R_rw = np.stack([x, y, z])
    f = (K[0, 0] + K[1, 1]) / 2.0
    Kr = np.array([[f, 0.0, K[0, 2]], [0.0, f, K[1, 2]], [0.0, 0.0, 1.0]])
    Kr_inv = np.linalg.inv(Kr)
    H_l = K @ Ra.T @ R_rw.T @ Kr_inv
    H_r = K @ Rb.T @ R_rw.T @ Kr_inv
    return dict(R_rw=R_rw, c_left=ca, c_right=cb, f=f, cx=float(K[0, 2]), cy=float(K[1, 2]), B=float(np.linalg.norm(cb - ca)),
                swapped=swapped, H_l=H_l, H_r=H_r)


# ---- device stages --------------------------------------------------------------------------------------------------
def remap(img, H):
    """stage 1: (rectified u8 [h][w], valid bool [h][w])"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    H = np.asarray(H, np.float64).reshape(9)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    den = H[6] * x + H[7] * y + H[8]
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = (H[0] * x + H[1] * y + H[2]) / den
        sy = (H[3] * x + H[4] * y + H[5]) / den
    valid = (sx >= 0.0) & (sx <= w - 1) & (sy >= 0.0) & (sy <= h - 1)
    sxv, syv = np.where(valid, sx, 0.0), np.where(valid, sy, 0.0)
    x0 = np.floor(sxv).astype(np.int64)
    y0 = np.floor(syv).astype(np.int64)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.minimum(y0 + 1, h - 1)
    ax = sxv - x0
    ay = syv - y0
    I = img.astype(np.float64)
    i00, i01, i10, i11 = I[y0, x0], I[y0, x1], I[y1, x0], I[y1, x1]
    v = (1.0 - ay) * ((1.0 - ax) * i00 + ax * i01) + ay * ((1.0 - ax) * i10 + ax * i11)
    out = np.where(valid, np.floor(v + 0.5), 0.0).astype(np.uint8)
    return out, valid


def census(img, valid, win):
    """stage 2: u64 [h][w]; bit k = (neighbour k < centre), neighbours row-major without the centre; bit 63 = invalid"""
    h, w = img.shape
    r = win // 2
    I = img.astype(np.int32)
    code = np.zeros((h, w), np.uint64)
    bad = ~valid.copy()
    bad[:r, :] = True
    bad[h - r:, :] = True
    bad[:, :r] = True
    bad[:, w - r:] = True
    Ip = np.pad(I, r)
    Vp = np.pad(valid, r, constant_values=False)
    bit = 0
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            nb = Ip[r + dy:r + dy + h, r + dx:r + dx + w]
            bad |= ~Vp[r + dy:r + dy + h, r + dx:r + dx + w]
            if dy == 0 and dx == 0:
                continue
            code |= (nb < I).astype(np.uint64) << np.uint64(bit)
            bit += 1
    code[bad] = INVALID_BIT
    return code


def cost_volume(cl, cr, D, nbits):
    """stage 3: u8 [h][w][D]"""
    h, w = cl.shape
    C = np.full((h, w, D), nbits, np.uint8)
    lbad = (cl & INVALID_BIT) != 0
    for d in range(min(D, w)):
        a, b = cl[:, d:], cr[:, :w - d]
        c = np.bitwise_count(a ^ b).astype(np.uint8)
        bad = lbad[:, d:] | ((b & INVALID_BIT) != 0)
        C[:, d:, d] = np.where(bad, nbits, c)
    return C


def _path(C, p1, p2, axis, reverse):
    """L_r of one path direction as int32, same shape as C"""
    Cm = np.moveaxis(C, axis, 0).astype(np.int32)  # [steps][lines][D]
    if reverse:
        Cm = Cm[::-1]
    L = np.empty_like(Cm)
    L[0] = Cm[0]
    big = np.int32(1 << 20)
    for i in range(1, Cm.shape[0]):
        q = L[i - 1]
        m = q.min(axis=1, keepdims=True)
        lo = np.concatenate([np.full((q.shape[0], 1), big, np.int32), q[:, :-1]], axis=1)
        hi = np.concatenate([q[:, 1:], np.full((q.shape[0], 1), big, np.int32)], axis=1)
        best = np.minimum(np.minimum(q, np.minimum(lo, hi) + p1), m + p2)
        L[i] = Cm[i] + best - m
    if reverse:
        L = L[::-1]
    return np.moveaxis(L, 0, axis)


def aggregate(C, p1, p2):
    """stage 4: S u16 [h][w][D] = L_lr + L_rl + L_tb + L_bt"""
    S = _path(C, p1, p2, 1, False)
    S += _path(C, p1, p2, 1, True)
    S += _path(C, p1, p2, 0, False)
    S += _path(C, p1, p2, 0, True)
    assert S.max() < 65536
    return S.astype(np.uint16)


def select(S, cl, uniqueness, lr_max_diff):
    """stage 5: disp16 int16 [h][w] (-16 = invalid)"""
    h, w, D = S.shape
    S32 = S.astype(np.int32)
    dstar = S32.argmin(axis=2)  # first minimum = smallest d
    smin = np.take_along_axis(S32, dstar[..., None], 2)[..., 0]
    valid = (cl & INVALID_BIT) == 0
    if uniqueness > 0:
        dd = np.arange(D)[None, None, :]
        far = np.abs(dd - dstar[..., None]) > 1
        valid &= ~(far & (S32 * (100 - uniqueness) < smin[..., None] * 100)).any(axis=2)
    d16 = 16 * dstar
    inner = (dstar > 0) & (dstar < D - 1)
    sm = np.take_along_axis(S32, np.clip(dstar - 1, 0, D - 1)[..., None], 2)[..., 0]
    sp = np.take_along_axis(S32, np.clip(dstar + 1, 0, D - 1)[..., None], 2)[..., 0]
    den2 = np.maximum(sm + sp - 2 * smin, 1)
    num = (sm - sp) * 16 + den2
    q = np.abs(num) // (den2 * 2) * np.sign(num)  # C division: truncation toward zero
    d16 = np.where(inner, d16 + q, d16)
    if lr_max_diff >= 0:
        dr = right_disparity(S)
        ys, xs = np.mgrid[0:h, 0:w]
        xr = xs - dstar
        ok = xr >= 0
        drv = dr[ys, np.clip(xr, 0, w - 1)]
        valid &= ~(ok & (np.abs(drv - dstar) > lr_max_diff))
    return np.where(valid, d16, -16).astype(np.int16)


def right_disparity(S):
    """argmin_d S(xr + d, y, d) over xr + d < w, smallest d on ties"""
    h, w, D = S.shape
    big = np.int64(1 << 40)
    best = np.full((h, w), big)
    arg = np.zeros((h, w), np.int64)
    for d in range(min(D, w)):
        v = np.full((h, w), big)
        v[:, :w - d] = S[:, d:, d]
        better = v < best
        best = np.where(better, v, best)
        arg = np.where(better, d, arg)
    return arg


def _components(n, a, b):
    """label of every node's connected component under the edges (a[i], b[i])"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        return connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(n, n)), directed=False)[1]
    except ImportError:
        parent = np.arange(n)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for i, j in zip(a.tolist(), b.tolist()):
            ri, rj = find(i), find(j)
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)
        return np.array([find(i) for i in range(n)])


def speckle(d16, window, rng):
    """stage 6: components (4-connected, |d16 step| <= 16*rng) of fewer than `window` pixels become -16"""
    d16 = d16.copy()
    if window <= 0:
        return d16
    h, w = d16.shape
    flat = d16.ravel().astype(np.int64)
    valid = flat != -16
    lim = 16 * rng
    idx = np.arange(h * w)
    right = valid[:-1] & valid[1:] & (np.abs(flat[:-1] - flat[1:]) <= lim) & (idx[:-1] % w != w - 1)
    down = valid[:-w] & valid[w:] & (np.abs(flat[:-w] - flat[w:]) <= lim)
    a = np.concatenate([np.nonzero(right)[0], np.nonzero(down)[0]])
    b = np.concatenate([np.nonzero(right)[0] + 1, np.nonzero(down)[0] + w])
    roots = _components(h * w, a, b)
    sizes = np.bincount(roots[valid], minlength=h * w)
    small = valid & (sizes[roots] < window)
    flat = d16.ravel()
    flat[small] = -16
    return flat.reshape(h, w)


def disparity(img_l, img_r, H_l, H_r, p=None, want=False):
    """stages 1-6: disp16, or dict(disp16, rect, S) with want=True"""
    p = {**DEFAULTS, **(p or {})}
    rl, vl = remap(img_l, H_l)
    rr, vr = remap(img_r, H_r)
    cl, cr = census(rl, vl, p["census"]), census(rr, vr, p["census"])
    C = cost_volume(cl, cr, p["num_disparities"], p["census"] ** 2 - 1)
    S = aggregate(C, p["p1"], p["p2"])
    d16 = select(S, cl, p["uniqueness"], p["lr_max_diff"])
    d16 = speckle(d16, p["speckle_window"], p["speckle_range"])
    if want:
        return dict(disp16=d16, rect=np.stack([rl, rr]), S=S)
    return d16


# ---- host mesh ------------------------------------------------------------------------------------------------------
def grid_mesh(d16, rect, step=4, disp_min=1.0, disp_jump=3.0, z_max_percentile=98.0):
    """(verts [n][3] f64, faces [m][3] i32, warn): warn is None or the reason the export is skipped"""
    h, w = d16.shape
    f, cx, cy, B = rect["f"], rect["cx"], rect["cy"], rect["B"]
    R, c = np.asarray(rect["R_rw"], np.float64), np.asarray(rect["c_left"], np.float64)
    empty = (np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    d = d16.astype(np.float64) / 16.0
    ok = (d16 != -16) & (d >= disp_min)
    with np.errstate(divide="ignore"):
        Z = (f * B) / d
    if not ok.any():
        return (*empty, "no valid disparity/depth")
    zs = np.sort(Z[ok])
    k = min(max(int(math.ceil(z_max_percentile / 100.0 * len(zs))), 1), len(zs))
    ok &= Z <= zs[k - 1]
    ys, xs = list(range(0, h, step)), list(range(0, w, step))
    vid = -np.ones((len(ys), len(xs)), np.int64)
    verts = []
    for yi, y in enumerate(ys):
        for xi, x in enumerate(xs):
            if not ok[y, x]:
                continue
            z = Z[y, x]
            X = ((x - cx) * z) / f
            Y = ((y - cy) * z) / f
            P = [R[0, i] * X + R[1, i] * Y + R[2, i] * z + c[i] for i in range(3)]
            vid[yi, xi] = len(verts)
            verts.append(P)
    if len(verts) < 3:
        return (*empty, "insufficient valid vertices")
    faces = []
    for yi in range(len(ys) - 1):
        for xi in range(len(xs) - 1):
            v00, v01, v10, v11 = vid[yi, xi], vid[yi, xi + 1], vid[yi + 1, xi], vid[yi + 1, xi + 1]
            if min(v00, v01, v10, v11) < 0:
                continue
            y0, y1, x0, x1 = ys[yi], ys[yi + 1], xs[xi], xs[xi + 1]
            d00, d01, d10, d11 = d[y0, x0], d[y0, x1], d[y1, x0], d[y1, x1]
            if abs(d00 - d01) > disp_jump or abs(d00 - d10) > disp_jump or abs(d11 - d01) > disp_jump or abs(d11 - d10) > disp_jump:
                continue
            faces.append([v00, v01, v11])
            faces.append([v00, v11, v10])
    if not faces:
        return (*empty, "no faces survived filtering")
    return np.array(verts, np.float64), np.array(faces, np.int32), None
