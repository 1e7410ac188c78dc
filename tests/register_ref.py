"""NumPy restatement of the surface registration stage ("Registering a surface to a reference mesh"), written from
the definition, not from the kernel.  The correspondences are sdist_ref's (d2, face); cross, dot and the face normal are its
expressions.

apply() moves points by a transform, pivot() is the target's box centre, system() one evaluation (the 37 ordered sums and
n_used), solve() the Cholesky solve at dimension 7 or 6 and update() the Cayley step in Python floats (IEEE double, one operation
at a time, nothing contracted), register() the Gauss-Newton loop.  The only library function is sqrt.  The device results must
equal these bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

import sdist_ref as SR

DEFAULTS = dict(cell=0.0, max_iters=20, stride=1, min_points=16, with_scale=1, damping=0.0, eps_rot=1e-4, eps_scale=1e-4, eps_trans=1e-3)
CONVERGED, MAX_ITERS, TOO_FEW, DEGENERATE = range(4)
TERMS = 37
ITERS_CAP = 64
# the pairs (m, n), m <= n, of A in the order of the sums: row by row
PAIRS = [(m, n) for m in range(7) for n in range(m, 7)]


def check_params(d_max, **kw):
    """the library's sfmx_register_check_params, field by field"""
    d = {**DEFAULTS, **kw}
    if not (d_max >= 2.0 ** -500) or not (d_max <= 2.0 ** 60):
        return False
    if not (d["cell"] >= 0.0) or not math.isfinite(d["cell"]):
        return False
    if d["max_iters"] < 1 or d["max_iters"] > ITERS_CAP or d["stride"] < 1 or d["min_points"] < 7:
        return False
    for k in ("damping", "eps_rot", "eps_scale", "eps_trans"):
        if not (d[k] >= 0.0) or not math.isfinite(d[k]):
            return False
    return True


def identity():
    return dict(s=1.0, R=np.eye(3), t=np.zeros(3))


def transform_ok(T):
    return bool(math.isfinite(T["s"]) and T["s"] > 0.0 and np.isfinite(T["R"]).all() and np.isfinite(T["t"]).all())


def apply(T, X):
    """y_a = s*((R_a0*x0 + R_a1*x1) + R_a2*x2) + t_a for X [n][3]"""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    s, R, t = float(T["s"]), np.asarray(T["R"], np.float64).reshape(3, 3), np.asarray(T["t"], np.float64).reshape(3)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([s * ((R[a, 0] * X[:, 0] + R[a, 1] * X[:, 1]) + R[a, 2] * X[:, 2]) + t[a] for a in range(3)], axis=1)


def _key(x):
    """the order of the finite doubles as unsigned integers, -0.0 below +0.0"""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def pivot(V, F):
    """p_a = 0.5*(min_a + max_a) over the vertices a face uses; 0 for a target without faces"""
    V = np.ascontiguousarray(V, np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(F, np.int32).reshape(-1, 3)
    if len(F) == 0:
        return [0.0, 0.0, 0.0]
    U = V[np.unique(F)]
    out = []
    for a in range(3):
        k = _key(U[:, a])
        out.append(0.5 * (float(U[k.argmin(), a]) + float(U[k.argmax(), a])))
    return out


def rows(T, X, V, F, d_max, stride=1, dist=SR.brute):
    """(used bool [ns], J [7] of [ns], h, w, d2, reasons): the row of every sample.  reasons counts the samples by the branch
    they took: clipped (sdist gave no face), collinear (nn == 0), used."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    V = np.ascontiguousarray(V, np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(F, np.int32).reshape(-1, 3)
    Y = apply(T, X[::stride])
    if not (np.isfinite(X[::stride]).all() and np.isfinite(Y).all()):
        raise ValueError("a sampled source coordinate, or its transform, is not finite")
    ns = len(Y)
    if ns == 0 or len(F) == 0:
        z = np.zeros(ns)
        return np.zeros(ns, bool), [z] * 7, z, z, np.full(ns, d_max * d_max), dict(clipped=ns, collinear=0, used=0)
    d2, f = dist(Y, V, F, d_max)
    hit = f >= 0
    fi = np.where(hit, f, 0)
    a, b, c = V[F[fi, 0]], V[F[fi, 1]], V[F[fi, 2]]
    n = SR.cross(b - a, c - a)
    nn = SR.dot(n, n)
    used = hit & (nn > 0.0)
    p = np.array(pivot(V, F))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        h = SR.dot(Y - a, n)
        q = Y - p
        w = 1.0 / nn
        J = [q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2], q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0],
             n[:, 0], n[:, 1], n[:, 2], SR.dot(q, n)]
    reasons = dict(clipped=int((~hit).sum()), collinear=int((hit & ~(nn > 0.0)).sum()), used=int(used.sum()))
    return used, J, h, w, d2, reasons


def terms(used, J, h, w, d2):
    """[37][ns]: A_mn (m <= n, row by row), b_m, e, c; +0.0 where the sample is not used"""
    with np.errstate(invalid="ignore", over="ignore"):
        out = [(J[m] * J[n]) * w for m, n in PAIRS] + [(J[m] * h) * w for m in range(7)] + [(h * h) * w, d2]
    return np.stack([np.where(used, v, 0.0) for v in out]) if len(used) else np.zeros((TERMS, 0))


def tree256(a):
    """the halving tree over the last axis (length 256): offsets 128, 64, ..., 1"""
    off = 128
    while off >= 1:
        a = a[..., :off] + a[..., off:2 * off]
        off //= 2
    return a[..., 0]


def block_layout(T):
    """T [k][ns] -> [k][blocks][256]: sample j of a block (j = k % 256) sits at the tree index 4 (j % 64) + j / 64"""
    k, ns = T.shape
    nb = (ns + 255) // 256
    P = np.zeros((k, nb * 256))
    P[:, :ns] = T
    # [k][block][wave][lane] -> [k][block][lane][wave]
    return P.reshape(k, nb, 4, 64).transpose(0, 1, 3, 2).reshape(k, nb, 256)


def ordered_sum(T):
    """the sums of T [k][ns] in the definition's order; ns = 0 gives +0.0"""
    if T.shape[1] == 0:
        return np.zeros(T.shape[0])
    r = tree256(block_layout(T))  # [k][blocks]
    while r.shape[1] > 1:
        groups = (r.shape[1] + 255) // 256
        P = np.zeros((r.shape[0], groups * 256))
        P[:, :r.shape[1]] = r
        r = tree256(P.reshape(r.shape[0], groups, 256))
    return r[:, 0].copy()


def system(T, X, V, F, d_max, stride=1, dist=SR.brute):
    """(sums f64 [37], n_used) of one evaluation at T"""
    used, J, h, w, d2, _ = rows(T, X, V, F, d_max, stride, dist)
    return ordered_sum(terms(used, J, h, w, d2)), int(used.sum())


def solve(sums, damping=0.0, dim=7):
    """delta [7] of (A + damping I) delta = -b by Cholesky at dimension dim in the definition's order (delta[6] = 0.0 at
    dimension 6), or None when a pivot is <= 0 or not finite"""
    v = [float(x) for x in sums]
    M = [[0.0] * 7 for _ in range(7)]
    for t, (m, n) in enumerate(PAIRS):
        M[m][n] = M[n][m] = v[t]
    for m in range(dim):
        M[m][m] = M[m][m] + float(damping)
    b = v[28:35]
    L = [[0.0] * 7 for _ in range(7)]
    for j in range(dim):
        d = M[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not (d > 0.0) or not math.isfinite(d):
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, dim):
            x = M[i][j]
            for k in range(j):
                x = x - L[i][k] * L[j][k]
            L[i][j] = x / L[j][j]
    y = [0.0] * 7
    for i in range(dim):
        x = -b[i]
        for k in range(i):
            x = x - L[i][k] * y[k]
        y[i] = x / L[i][i]
    delta = [0.0] * 7
    for i in range(dim - 1, -1, -1):
        x = y[i]
        for k in range(i + 1, dim):
            x = x - L[k][i] * delta[k]
        delta[i] = x / L[i][i]
    return delta


def cayley(omega):
    """D [3][3] = I + k ([a]x + [a]x^2), a = omega / 2, k = 2 / (1 + |a|^2), element by element"""
    a0, a1, a2 = 0.5 * omega[0], 0.5 * omega[1], 0.5 * omega[2]
    k = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2))
    return [[1.0 - k * (a1 * a1 + a2 * a2), k * (a0 * a1 - a2), k * (a0 * a2 + a1)],
            [k * (a0 * a1 + a2), 1.0 - k * (a0 * a0 + a2 * a2), k * (a1 * a2 - a0)],
            [k * (a0 * a2 - a1), k * (a1 * a2 + a0), 1.0 - k * (a0 * a0 + a1 * a1)]]


def update(T, p, delta):
    """the transform after the step delta = (omega, v, sigma) about the pivot p"""
    D = cayley(delta[0:3])
    g = 1.0 + delta[6]
    s = float(T["s"])
    R = [[float(x) for x in row] for row in np.asarray(T["R"], np.float64).reshape(3, 3)]
    t = [float(x) for x in np.asarray(T["t"], np.float64).reshape(3)]
    Rn = [[(D[a][0] * R[0][b] + D[a][1] * R[1][b]) + D[a][2] * R[2][b] for b in range(3)] for a in range(3)]
    u = [t[a] - p[a] for a in range(3)]
    tn = [(p[a] + g * ((D[a][0] * u[0] + D[a][1] * u[1]) + D[a][2] * u[2])) + delta[3 + a] for a in range(3)]
    return dict(s=g * s, R=np.array(Rn), t=np.array(tn))


def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def register(X, V, F, d_max, init=None, dist=SR.brute, iterates=None, **kw):
    """the loop: dict(T, status, iterations, trace=[(n_used, e, c, |omega|, |v|, sigma), ...]); iterates (a list) receives the
    transform every evaluation was made at"""
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown register parameters {sorted(unknown)}")
    P = {**DEFAULTS, **kw}
    assert check_params(d_max, **kw)
    cur = identity() if init is None else dict(s=float(init["s"]), R=np.array(init["R"], np.float64).reshape(3, 3), t=np.array(init["t"], np.float64).reshape(3))
    assert transform_ok(cur)
    good = cur
    p = pivot(V, F)
    dim = 7 if P["with_scale"] else 6
    status, trace = MAX_ITERS, []
    for _ in range(int(P["max_iters"])):
        if iterates is not None:
            iterates.append(cur)
        sums, n = system(cur, X, V, F, d_max, P["stride"], dist)
        e, c = float(sums[35]), float(sums[36])
        if n < P["min_points"]:
            trace.append((n, e, c, 0.0, 0.0, 0.0))
            status, cur = TOO_FEW, good
            break
        delta = solve(sums, P["damping"], dim)
        nxt = None
        if delta is not None and 1.0 + delta[6] > 0.0:
            with np.errstate(over="ignore", invalid="ignore"):
                nxt = update(cur, p, delta)
            if not transform_ok(nxt):
                nxt = None
        if nxt is None:
            trace.append((n, e, c, 0.0, 0.0, 0.0))
            status, cur = DEGENERATE, good
            break
        good, cur = cur, nxt
        rot, tr = norm3(delta[0:3]), norm3(delta[3:6])
        trace.append((n, e, c, rot, tr, delta[6]))
        if rot <= P["eps_rot"] and abs(delta[6]) <= P["eps_scale"] and tr <= P["eps_trans"] * d_max:
            status = CONVERGED
            break
    return dict(T=cur, status=status, iterations=len(trace), trace=trace)


def bits(x):
    return np.asarray(x, np.float64).tobytes()


def same_transform(a, b):
    return bits(a["s"]) == bits(b["s"]) and bits(a["R"]) == bits(b["R"]) and bits(a["t"]) == bits(b["t"])


def same_result(a, b):
    """bit equality of two loop results (transform, status, iterations, trace)"""
    if a["status"] != b["status"] or a["iterations"] != b["iterations"] or not same_transform(a["T"], b["T"]):
        return False
    return len(a["trace"]) == len(b["trace"]) and all(x[0] == y[0] and bits(x[1:]) == bits(y[1:]) for x, y in zip(a["trace"], b["trace"]))


def rms(result):
    """(rms_plane, rms_point, n) of the last evaluation of a loop result"""
    n, e, c = result["trace"][-1][:3]
    return (math.sqrt(e / n), math.sqrt(c / n), n) if n > 0 else (float("nan"), float("nan"), 0)


# ---- test scenes -------------------------------------------------------------------------------------------------------------
# DESIGN.md 19's four spheres (centre, radius): no rotation about any axis leaves the scene unchanged
SPHERES = (((0.05, 0.04, 0.03), 0.05), ((-0.06, 0.03, -0.04), 0.045), ((0.0, -0.07, 0.04), 0.04), ((0.03, -0.02, -0.07), 0.035))
D_MAX = 0.01
# (degrees about the pivot, scale factor, translation): the true frame, a moderate and a larger disturbance
STARTS = ((0.0, 1.0, 0.0), (2.0, 1.02, 0.005), (4.0, 1.04, 0.011))


def rotation(axis, degrees):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    th = np.radians(degrees)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def spheres_mesh(level=3, spheres=SPHERES):
    """(V, F): one icosphere per sphere, concatenated"""
    Vs, Fs, off = [], [], 0
    for centre, radius in spheres:
        v, f = SR.icosphere(level, radius)
        Vs.append(v + np.asarray(centre))
        Fs.append(f + off)
        off += len(v)
    return np.concatenate(Vs), np.concatenate(Fs).astype(np.int32)


def spheres_source(level=3, spheres=SPHERES, cover=0.2, noise=0.0005, outliers=0.05, seed=7):
    """source points in the target's frame: icosphere vertices rotated per sphere (so that none coincides with a target
    vertex), kept where they lie on the side dot(direction, pole) > -cover of a random pole (about 60 % of the sphere at
    cover = 0.2), with radial noise, and a share moved far off the surface; one seeded generator"""
    rng = np.random.default_rng(seed)
    out = []
    for centre, radius in spheres:
        v, _ = SR.icosphere(level, 1.0)
        v = v @ rotation(rng.normal(size=3), 17.0 + 10.0 * rng.random()).T
        pole = rng.normal(size=3)
        pole /= np.linalg.norm(pole)
        v = v[v @ pole > -cover]
        r = radius + noise * rng.normal(size=len(v))
        gross = rng.random(len(v)) < outliers
        r = np.where(gross, radius * (1.0 + rng.uniform(0.3, 1.0, len(v)) * rng.choice([-1.0, 1.0], len(v))), r)
        out.append(np.asarray(centre) + v * r[:, None])
    return np.concatenate(out)


def disturb(p, degrees, scale, shift, rng):
    """a Sim(3) (as a transform dict) that rotates by `degrees` about a random axis through p, scales by `scale` about p and
    moves by `shift` in a random direction (test geometry, not part of the definition: plain NumPy with sin / cos)"""
    D = rotation(rng.normal(size=3), degrees)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    p = np.asarray(p, np.float64)
    return dict(s=float(scale), R=D, t=p - scale * (D @ p) + shift * d)


def inverse(T):
    """the inverse similarity (test geometry)"""
    R = np.asarray(T["R"], np.float64).reshape(3, 3)
    return dict(s=1.0 / T["s"], R=R.T, t=-(R.T @ np.asarray(T["t"], np.float64)) / T["s"])


def compose(A, B):
    """A after B (test geometry)"""
    RA, RB = np.asarray(A["R"], np.float64).reshape(3, 3), np.asarray(B["R"], np.float64).reshape(3, 3)
    return dict(s=A["s"] * B["s"], R=RA @ RB, t=A["s"] * (RA @ np.asarray(B["t"], np.float64)) + np.asarray(A["t"], np.float64))


def transform_error(T, true, p):
    """(rotation in degrees, |scale ratio - 1|, distance of the two images of the point p) between two transforms"""
    E = compose(T, inverse(true))
    R = np.asarray(E["R"], np.float64)
    cos = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(cos))), abs(float(E["s"]) - 1.0), float(np.linalg.norm(apply(T, p)[0] - apply(true, p)[0]))
