"""NumPy restatement of the multi-view consistency filter of disparity maps (DESIGN.md "Multi-view consistency filtering"),
written from the definition, not from the kernel, and the fixtures its tests share.

Every test is IEEE double in one fixed expression order up to its comparison; the support is an integer count.  The device
results must equal these byte for byte.  Views are (cam, disp16) with cam = dict(R_rw, c_left, f, cx, cy, B), as in
tests/fusion_ref.py.
"""
from __future__ import annotations

import numpy as np

import fusion_ref as FR

DEFAULTS = dict(rel_tol=0.01, reproj_px=1.0, disp_min=1.0, min_support=2)
# what can happen to one (pixel, other view) test, in the order the definition tries them
OUTCOMES = ("behind", "outside", "invalid", "depth", "back_behind", "reproj", "ok")


class _Cam:
    def __init__(self, cam, d16):
        self.R = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
        self.c = np.asarray(cam["c_left"], np.float64).reshape(3)
        self.f, self.cx, self.cy = float(cam["f"]), float(cam["cx"]), float(cam["cy"])
        self.fB = self.f * float(cam["B"])
        self.d16 = np.ascontiguousarray(d16, np.int16)
        self.h, self.w = self.d16.shape

    def lift(self, x, y, dd):
        """the 3-D point of pixel (x, y) (doubles) with disparity dd"""
        Z = self.fB / dd
        q0 = ((x - self.cx) * Z) / self.f
        q1 = ((y - self.cy) * Z) / self.f
        R, c = self.R, self.c
        return [c[a] + ((R[0, a] * q0 + R[1, a] * q1) + R[2, a] * Z) for a in range(3)]

    def camera(self, X):
        """q: the point in camera coordinates"""
        R, c = self.R, self.c
        p = [X[a] - c[a] for a in range(3)]
        return [(R[r, 0] * p[0] + R[r, 1] * p[1]) + R[r, 2] * p[2] for r in range(3)]

    def pixel(self, q):
        return (self.f * q[0]) / q[2] + self.cx, (self.f * q[1]) / q[2] + self.cy


def _take(arrs, keep):
    return [a[keep] for a in arrs]


def _support(Vi, Vj, X, x, y, rel_tol, reproj_px, disp_min, counter):
    """1 where view j supports the pixels (x, y) of view i whose points are X, else 0"""
    n = len(x)
    idx = np.arange(n)

    def drop(name, keep):
        nonlocal idx
        if counter is not None:
            counter[name] = counter.get(name, 0) + int((~keep).sum())
        idx = idx[keep]
        return keep

    q = Vj.camera(X)
    k = drop("behind", q[2] > 0)  # a NaN skips
    q, X, x, y = _take(q, k), _take(X, k), x[k], y[k]
    u, v = Vj.pixel(q)
    xr, yr = np.floor(u + 0.5), np.floor(v + 0.5)
    k = drop("outside", (xr >= 0) & (xr < Vj.w) & (yr >= 0) & (yr < Vj.h))
    q, x, y, xr, yr = _take(q, k), x[k], y[k], xr[k], yr[k]
    d2 = Vj.d16[yr.astype(np.int64), xr.astype(np.int64)]
    dd2 = d2.astype(np.float64) / 16.0
    k = drop("invalid", (d2 != -16) & (dd2 >= disp_min))
    q, x, y, xr, yr, dd2 = _take(q, k), x[k], y[k], xr[k], yr[k], dd2[k]
    Z2 = Vj.fB / dd2
    k = drop("depth", np.abs(Z2 - q[2]) <= rel_tol * q[2])
    x, y, xr, yr, dd2 = x[k], y[k], xr[k], yr[k], dd2[k]
    Y = Vj.lift(xr, yr, dd2)
    t = Vi.camera(Y)
    k = drop("back_behind", t[2] > 0)
    t, x, y = _take(t, k), x[k], y[k]
    uu, vv = Vi.pixel(t)
    e0, e1 = uu - x, vv - y
    drop("reproj", (e0 * e0 + e1 * e1) <= reproj_px * reproj_px)
    if counter is not None:
        counter["ok"] = counter.get("ok", 0) + len(idx)
    out = np.zeros(n, np.int64)
    out[idx] = 1
    return out


def filter_views(views, rel_tol=0.01, reproj_px=1.0, disp_min=1.0, min_support=2, counter=None, only=None):
    """views: [(cam, disp16)].  Returns dict(disp16=[int16 [h][w]], support=[u8 [h][w]], valid=int32 [n], kept=int32 [n]).
    counter (optional dict): gains the number of (pixel, other view) tests that ended in each of OUTCOMES.
    only (optional): the reference views to filter (against all the others); the lists then hold those, in that order."""
    V = [_Cam(cam, d16) for cam, d16 in views]
    outs, sups, valid_n, kept_n = [], [], [], []
    if counter is not None:
        for name in OUTCOMES:
            counter.setdefault(name, 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in (range(len(V)) if only is None else only):
            Vi = V[i]
            d = Vi.d16.ravel()
            dd = d.astype(np.float64) / 16.0
            valid = (d != -16) & (dd >= disp_min)
            idx = np.nonzero(valid)[0]
            x, y = (idx % Vi.w).astype(np.float64), (idx // Vi.w).astype(np.float64)
            X = Vi.lift(x, y, dd[idx])
            s = np.zeros(len(idx), np.int64)
            for j, Vj in enumerate(V):
                if j != i:
                    s += _support(Vi, Vj, X, x, y, rel_tol, reproj_px, disp_min, counter)
            support = np.zeros(d.shape, np.int64)
            support[idx] = s
            out = np.where(valid & (support >= min_support), d, -16).astype(np.int16)
            outs.append(out.reshape(Vi.h, Vi.w))
            sups.append(np.minimum(support, 255).astype(np.uint8).reshape(Vi.h, Vi.w))
            valid_n.append(int(valid.sum()))
            kept_n.append(int((out != -16).sum()))
    return dict(disp16=outs, support=sups, valid=np.array(valid_n, np.int32), kept=np.array(kept_n, np.int32))


def filtered_views(views, res):
    return [(cam, f) for (cam, _), f in zip(views, res["disp16"])]


# ---- fixtures --------------------------------------------------------------------------------------------------------------
def sphere_views(n_views, w, h, f, radius=0.1, dist=0.5, B=0.05):
    """Fibonacci directions around a sphere at the origin, analytic disp16 (tests/fusion_ref.py)"""
    out = []
    for d in FR.fibonacci_dirs(n_views):
        cam = FR.look_at_cam(dist * d, (0.0, 0.0, 0.0), f, w, h, B=B)
        out.append((cam, FR.sphere_disp16(cam, w, h, radius)))
    return out


def add_outliers(views, seed, lo, hi, frac=0.05):
    """replace `frac` of ALL pixels (misses included) by a uniform random disp16 in [lo, hi): one generator, the views in
    order, per view first the mask, then the values.  Returns (noisy views, masks)."""
    rng = np.random.default_rng(seed)
    out, masks = [], []
    for cam, d16 in views:
        m = rng.random(d16.shape) < frac
        d = d16.copy()
        d[m] = rng.integers(lo, hi, int(m.sum()))
        out.append((cam, d))
        masks.append(m)
    return out, masks


SPHERE26 = dict(n_views=26, w=320, h=320, f=600.0)  # DESIGN.md 13's fixture
SPHERE26_VOL = dict(origin=(-0.15, -0.15, -0.15), voxel=0.005, dims=(61, 61, 61))
RADIUS = 0.1


def sphere26(noisy):
    views = sphere_views(**SPHERE26)
    if not noisy:
        return views, None
    return add_outliers(views, 1, 16 * 20, 16 * 120)


def off_shell(verts, voxel=SPHERE26_VOL["voxel"]):
    """(vertices more than one voxel off the sphere, RMS of the radius error in voxels)"""
    e = (np.linalg.norm(verts, axis=1) - RADIUS) / voxel
    return int((np.abs(e) > 1.0).sum()), float(np.sqrt((e ** 2).mean())) if len(e) else 0.0


def centre_view(w=64, h=64, f=40.0):
    """a camera at the sphere's centre looking out, with a hand-set map: the other cameras' points are all around it, many
    of them behind it"""
    cam = FR.look_at_cam((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), f, w, h)
    d16 = np.full((h, w), -16, np.int16)
    d16[8:56, 8:56] = int(round(16 * f * 0.05 / 0.1))  # Z = 0.1 in the middle
    d16[::7, ::5] = 16 * 3
    # what disp_min <= 0 lets through: 0 (Z = +inf), negative disparities, both ends of int16
    d16[1::9, 2::6] = 0
    d16[2::9, 3::6] = -7
    d16[3, 3], d16[60, 60], d16[3, 60] = 32767, -32768, -1
    return cam, d16


def sphere8():
    """eight 64 x 64 views with 5 % outliers, and the ninth camera at the centre"""
    views, _ = add_outliers(sphere_views(8, 64, 64, 120.0), 3, 32, 480)
    return views + [centre_view()]


EDGE_SHAPES = ((1, 1), (1, 300), (300, 1), (63, 4), (64, 4), (65, 5), (4096, 2))  # (w, h) around the 64 x 4 tile


def edge_shape_views(f=300.0):
    """views of EDGE_SHAPES, all looking at the sphere's centre from nearby positions with one focal length: crops of about the
    same image around its middle, so the flat ones overlap along the middle rows and can support each other"""
    out = []
    for k, (w, h) in enumerate(EDGE_SHAPES):
        a = np.radians(2.0 * (k - 3))  # an arc in the x-z plane: the rows of all the views line up
        cam = FR.look_at_cam((0.5 * np.sin(a), 0.0, -0.5 * np.cos(a)), (0.0, 0.0, 0.0), f, w, h)
        out.append((cam, FR.sphere_disp16(cam, w, h, RADIUS)))
    return out


def identical_views(n=300, w=8, h=8):
    cam = FR.look_at_cam((0.0, 0.0, -0.5), (0.0, 0.0, 0.0), 30.0, w, h)
    d16 = FR.sphere_disp16(cam, w, h, RADIUS)
    return [(cam, d16)] * n


RING6_ANGLES = [(10.0 * k, 10.0 * k + 3.0) for k in range(6)]
RING6_VOL = dict(origin=(-0.13, -0.13, -0.13), voxel=0.004, dims=(66, 66, 66))


def ring_frames(synth, angles_ab, w, h):
    """frames at the given (a, b) ring angles: (images [2m][h][w], K, poses [2m] camera->world (R, c), pairs [(2k, 2k+1)])"""
    angles = [a for ab in angles_ab for a in ab]
    seq = synth.make_sequence(len(angles), w, h, angles=angles)
    poses = [(seq["R"][i].T, -seq["R"][i].T @ seq["t"][i]) for i in range(len(angles))]
    return seq["images"], seq["K"], poses, [(2 * k, 2 * k + 1) for k in range(len(angles_ab))]


def mesh_quality(verts, faces):
    """(share of faces whose normal points away from the origin, share of vertices with radius in 0.065..0.105, vertices)"""
    n = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    outward = float(((n * verts[faces].mean(1)).sum(1) > 0).mean())
    r = np.linalg.norm(verts, axis=1)
    return outward, float(((r >= 0.065) & (r <= 0.105)).mean()), len(verts)
