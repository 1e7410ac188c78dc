"""NumPy restatement of direct TSDF pose alignment ("Registering a view to the volume"), written from the
definition, not from the kernel.  The volume, s(g) and "defined" come from fusion_ref, the gradient G from appearance_ref, the
trilinear interpolation from raycast_ref.Volume.

system() is one evaluation (the 28 ordered sums and n), solve() the 6 x 6 Cholesky solve and update() the Cayley pose update in
Python floats (IEEE double, one operation at a time, nothing contracted), align() the Gauss-Newton loop.  All arithmetic is IEEE
double in the definition's expression order; the only library function is sqrt.  The device results must equal these bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

import raycast_ref as RR

DEFAULTS = dict(max_iters=10, stride=1, disp_min=1.0, min_weight=0, min_pixels=64, damping=0.0, eps_rot=1e-6, eps_trans=1e-4)
CONVERGED, MAX_ITERS, TOO_FEW, DEGENERATE = range(4)
TERMS = 28
# the pairs (m, n), m <= n, of A in the order of the sums: row by row
PAIRS = [(m, n) for m in range(6) for n in range(m, 6)]


def pivot(origin, voxel, dims):
    """the box centre: origin + 0.5 * ((double)(n - 1) * voxel)"""
    return [float(origin[a]) + 0.5 * (float(dims[a] - 1) * float(voxel)) for a in range(3)]


def sample_grid(w, h, stride):
    """(nsx, nsy): the samples are the pixels (stride i, stride j) with stride i < w and stride j < h"""
    return (w + stride - 1) // stride, (h + stride - 1) // stride


def rows(vol, cam, disp16, stride=1, disp_min=1.0):
    """(used bool [nsy][nsx], J [6] of [nsy][nsx], s [nsy][nsx], reasons): the row of every sample; J and s are 0 where the
    sample is not used.  reasons counts the samples each test of the definition removed, in the order they are applied."""
    d16 = np.asarray(disp16, np.int16)
    h, w = d16.shape
    R = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    f, cx, cy, B = float(cam["f"]), float(cam["cx"]), float(cam["cy"]), float(cam["B"])
    nsx, nsy = sample_grid(w, h, stride)
    y, x = np.meshgrid(np.arange(nsy, dtype=np.int64) * stride, np.arange(nsx, dtype=np.int64) * stride, indexing="ij")
    d = d16[y, x].astype(np.int64).ravel()
    xs, ys = x.ravel().astype(np.float64), y.ravel().astype(np.float64)
    dd = d.astype(np.float64) / 16.0
    valid = (d != -16) & (dd >= float(disp_min))
    fB = f * B
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Z = fB / dd
        l0, l1 = ((xs - cx) * Z) / f, ((ys - cy) * Z) / f
        X = [c[a] + ((R[0, a] * l0 + R[1, a] * l1) + R[2, a] * Z) for a in range(3)]
        g = vol.grid(X)
        # Volume.inside is false for NaN, as the device's comparisons are
        ok, (s, G0, G1, G2) = vol.interp([vol.S, vol.G[0], vol.G[1], vol.G[2]], [np.where(valid, v, np.nan) for v in g])
        inside = vol.inside([np.where(valid, v, np.nan) for v in g])
    near = np.abs(s) < 1.0
    used = valid & ok & near
    reasons = dict(invalid=int((~valid).sum()), outside=int((valid & ~inside).sum()), undefined=int((valid & inside & ~ok).sum()),
                   far=int((valid & ok & ~near).sum()), used=int(used.sum()))
    p = pivot(vol.origin, vol.voxel, vol.n)
    with np.errstate(invalid="ignore", over="ignore"):
        gw = [G * vol.inv for G in (G0, G1, G2)]
        q = [X[a] - p[a] for a in range(3)]
        J = [q[1] * gw[2] - q[2] * gw[1], q[2] * gw[0] - q[0] * gw[2], q[0] * gw[1] - q[1] * gw[0], gw[0], gw[1], gw[2]]
    J = [np.where(used, v, 0.0).reshape(nsy, nsx) for v in J]
    s = np.where(used, s, 0.0).reshape(nsy, nsx)
    return used.reshape(nsy, nsx), J, s, reasons


def terms(used, J, s):
    """[28][nsy][nsx]: A_mn (m <= n, row by row), b_m, e; +0.0 where the sample is not used"""
    out = [J[m] * J[n] for m, n in PAIRS] + [J[m] * s for m in range(6)] + [s * s]
    return np.stack([np.where(used, v, 0.0) for v in out])


def tree256(a):
    """the halving tree over the last axis (length 256): offsets 128, 64, ..., 1"""
    off = 128
    while off >= 1:
        a = a[..., :off] + a[..., off:2 * off]
        off //= 2
    return a[..., 0]


def block_layout(T):
    """T [28][nsy][nsx] -> [28][blocks][256]: 16 x 16 tiles of samples, blocks row by row, padded with +0.0; inside a tile the
    sample (i, j) sits at the tree index t = 4 lane + wave, wave = 2 (j / 8) + (i / 8), lane = 8 (j % 8) + (i % 8)"""
    k, nsy, nsx = T.shape
    nby, nbx = (nsy + 15) // 16, (nsx + 15) // 16
    P = np.zeros((k, nby * 16, nbx * 16))
    P[:, :nsy, :nsx] = T
    # [k][by][wy][ly][bx][wx][lx] -> [k][by][bx][ly][lx][wy][wx]: t = ((ly * 8 + lx) * 2 + wy) * 2 + wx
    P = P.reshape(k, nby, 2, 8, nbx, 2, 8).transpose(0, 1, 4, 3, 6, 2, 5)
    return P.reshape(k, nby * nbx, 256)


def ordered_sum(T):
    """the 28 sums of T [28][nsy][nsx] in the definition's order"""
    r = tree256(block_layout(T))  # [28][blocks]
    while r.shape[1] > 1:
        groups = (r.shape[1] + 255) // 256
        P = np.zeros((r.shape[0], groups * 256))
        P[:, :r.shape[1]] = r
        r = tree256(P.reshape(r.shape[0], groups, 256))
    return r[:, 0].copy()


def volume(sum_, count, origin, voxel, min_weight=1):
    return RR.Volume(sum_, count, origin, voxel, max(int(min_weight), 1))


def system(vol, cam, disp16, stride=1, disp_min=1.0):
    """(sums f64 [28], n) of one evaluation at cam's pose; vol: volume(...)"""
    used, J, s, _ = rows(vol, cam, disp16, stride, disp_min)
    return ordered_sum(terms(used, J, s)), int(used.sum())


def solve(sums, damping=0.0):
    """delta [6] of (A + damping I) delta = -b by Cholesky in the definition's order, or None when a pivot is <= 0 or not finite"""
    v = [float(x) for x in sums]
    M = [[0.0] * 6 for _ in range(6)]
    for t, (m, n) in enumerate(PAIRS):
        M[m][n] = M[n][m] = v[t]
    for m in range(6):
        M[m][m] = M[m][m] + float(damping)
    b = v[21:27]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = M[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not (d > 0.0) or not math.isfinite(d):
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            x = M[i][j]
            for k in range(j):
                x = x - L[i][k] * L[j][k]
            L[i][j] = x / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        x = -b[i]
        for k in range(i):
            x = x - L[i][k] * y[k]
        y[i] = x / L[i][i]
    delta = [0.0] * 6
    for i in range(5, -1, -1):
        x = y[i]
        for k in range(i + 1, 6):
            x = x - L[k][i] * delta[k]
        delta[i] = x / L[i][i]
    return delta


def cayley(omega):
    """dR [3][3] = I + k ([a]x + [a]x^2), a = omega / 2, k = 2 / (1 + |a|^2), element by element"""
    a0, a1, a2 = 0.5 * omega[0], 0.5 * omega[1], 0.5 * omega[2]
    k = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2))
    return [[1.0 - k * (a1 * a1 + a2 * a2), k * (a0 * a1 - a2), k * (a0 * a2 + a1)],
            [k * (a0 * a1 + a2), 1.0 - k * (a0 * a0 + a2 * a2), k * (a1 * a2 - a0)],
            [k * (a0 * a2 - a1), k * (a1 * a2 + a0), 1.0 - k * (a0 * a0 + a1 * a1)]]


def update(cam, p, delta):
    """the camera after the step delta = (omega, v) about the pivot p: a new dict, everything but R_rw and c_left unchanged"""
    D = cayley(delta[0:3])
    R = [[float(x) for x in row] for row in np.asarray(cam["R_rw"], np.float64).reshape(3, 3)]
    c = [float(x) for x in np.asarray(cam["c_left"], np.float64).reshape(3)]
    Rn = [[(D[a][0] * row[0] + D[a][1] * row[1]) + D[a][2] * row[2] for a in range(3)] for row in R]
    u = [c[a] - p[a] for a in range(3)]
    cn = [(p[a] + ((D[a][0] * u[0] + D[a][1] * u[1]) + D[a][2] * u[2])) + delta[3 + a] for a in range(3)]
    out = dict(cam)
    out.update(R_rw=np.array(Rn), c_left=np.array(cn))
    return out


def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def align(vol, cam, disp16, max_iters=10, stride=1, disp_min=1.0, min_pixels=64, damping=0.0, eps_rot=1e-6, eps_trans=1e-4):
    """the loop: dict(view, status, iterations, trace=[(n, e, |omega|, |v|), ...])"""
    p = pivot(vol.origin, vol.voxel, vol.n)
    cur, good = dict(cam), dict(cam)
    status, trace = MAX_ITERS, []
    for _ in range(int(max_iters)):
        sums, n = system(vol, cur, disp16, stride, disp_min)
        e = float(sums[27])
        if n < min_pixels:
            trace.append((n, e, 0.0, 0.0))
            status, cur = TOO_FEW, good
            break
        delta = solve(sums, damping)
        if delta is None:
            trace.append((n, e, 0.0, 0.0))
            status, cur = DEGENERATE, good
            break
        good = cur
        cur = update(cur, p, delta)
        rot, tr = norm3(delta[0:3]), norm3(delta[3:6])
        trace.append((n, e, rot, tr))
        if rot <= eps_rot and tr <= eps_trans * vol.voxel:
            status = CONVERGED
            break
    return dict(view=cur, status=status, iterations=len(trace), trace=trace)


def same_result(a, b):
    """bit equality of two loop results (view, status, iterations, trace)"""
    def bits(x):
        return np.asarray(x, np.float64).tobytes()
    if a["status"] != b["status"] or a["iterations"] != b["iterations"]:
        return False
    if bits(a["view"]["R_rw"]) != bits(b["view"]["R_rw"]) or bits(a["view"]["c_left"]) != bits(b["view"]["c_left"]):
        return False
    return all(x[0] == y[0] and bits(x[1:]) == bits(y[1:]) for x, y in zip(a["trace"], b["trace"]))


# ---- test scenes -------------------------------------------------------------------------------------------------------------
# four spheres (centre, radius): no rotation about any axis leaves the scene unchanged
SPHERES = (((0.05, 0.04, 0.03), 0.05), ((-0.06, 0.03, -0.04), 0.045), ((0.0, -0.07, 0.04), 0.04), ((0.03, -0.02, -0.07), 0.035))
SCENE = dict(n_views=26, dist=0.5, f=300.0, w=160, h=160, B=0.05)
VOL = dict(origin=(-0.15, -0.15, -0.15), voxel=0.005, dims=(61, 61, 61))
NOVEL = ((0.31, 0.22, -0.33), (0.0, 0.1, -0.5))
STARTS = ((0.0, 0.0), (2.0, 2.0), (4.0, 3.0))  # (degrees about the pivot, voxels)


def scene_disp16(cam, w, h):
    """the disparity map of the four spheres: the pixel-wise maximum (the nearest surface) of the single spheres' maps"""
    import fusion_ref as FR
    out = None
    for centre, radius in SPHERES:
        d = FR.sphere_disp16(cam, w, h, radius, centre)
        out = d if out is None else np.maximum(out, d)
    return out


def scene_views():
    import fusion_ref as FR
    views = []
    for d in FR.fibonacci_dirs(SCENE["n_views"]):
        cam = FR.look_at_cam(SCENE["dist"] * d, (0.0, 0.0, 0.0), SCENE["f"], SCENE["w"], SCENE["h"], SCENE["B"])
        views.append((cam, scene_disp16(cam, SCENE["w"], SCENE["h"])))
    return views


_scene = {}


def scene_volume():
    """(sum, count, vol) of the four-sphere fixture, integrated once"""
    if not _scene:
        import fusion_ref as FR
        s, c = FR.integrate(VOL["origin"], VOL["voxel"], VOL["dims"], scene_views())
        s.setflags(write=False)
        c.setflags(write=False)
        _scene.update(sum=s, count=c, vol=VOL, volume=volume(s, c, VOL["origin"], VOL["voxel"]))
    return _scene


def novel_view(pos):
    """(cam, disp16) of a novel camera at pos looking at the origin, at the true pose"""
    import fusion_ref as FR
    cam = FR.look_at_cam(pos, (0.0, 0.0, 0.0), SCENE["f"], SCENE["w"], SCENE["h"], SCENE["B"])
    return cam, scene_disp16(cam, SCENE["w"], SCENE["h"])


def perturb(cam, p, degrees, voxels, voxel, rng):
    """cam rotated by `degrees` about a random axis through p and moved by `voxels` voxels in a random direction (test geometry,
    not part of the definition: plain NumPy with sin / cos)"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    dirn = rng.normal(size=3)
    dirn /= np.linalg.norm(dirn)
    th = np.radians(degrees)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    D = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    R = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    p = np.asarray(p, np.float64)
    out = dict(cam)
    out.update(R_rw=R @ D.T, c_left=p + D @ (c - p) + voxels * voxel * dirn)
    return out


def pose_error(cam, true, voxel):
    """(rotation in degrees, centre distance in voxels) between two cameras"""
    Ra, Rb = np.asarray(cam["R_rw"], np.float64).reshape(3, 3), np.asarray(true["R_rw"], np.float64).reshape(3, 3)
    cos = np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0)
    dc = np.asarray(cam["c_left"], np.float64) - np.asarray(true["c_left"], np.float64)
    return float(np.degrees(np.arccos(cos))), float(np.linalg.norm(dc) / voxel)
