"""Deterministic inputs for the range suite of the RANSAC kernels (tests/test_gpu_ransac_range.py), the oracle tables they are
checked against, and the checker of the contract of sfmx_ransac_score_ex as include/sfmx.h states it.  No files and no device;
tests/test_ransac_inputs_cpu.py runs the CPU oracle on every scene class and asserts the properties the GPU cases rely on (the
ill-conditioned octets really are ill-conditioned, the planted points really sit a few ulp from the threshold, ...), so that no
GPU case can pass on an input that misses its point.

A scene is a correspondence set xi, xj [n][2] with K = identity (norm_point is then exact, so the same arrays serve the kernel
level and the find_E_ransac seam), a threshold, and the octets of the stream find_E_ransac itself draws: mt19937(12345), 8 * iters
draws below n.  The reference for everything is the oracle (orc_ransac_hypotheses, orc_ransac_counts, orc_sampson_err,
orc_find_E_ransac); NumPy only CLASSIFIES octets (eigh of AtA, svd of the null vector), it never stands in for the Jacobi.

Scene classes (second-image noise sigma; 30 % uniform outliers):
  general0, general   3-D points at depth 3..8, small rotation + translation, sigma = 0 / 1e-3.  general0's outliers are kept 0.1
                      away from their epipolar lines: its all-inlier octets tie at the maximal count (lowest iteration wins)
  planar0/6/3         points on a tilted plane, sigma = 0 / 1e-6 / 1e-3 (null space of dimension 3 for octets with <= 1 outlier)
  rot0, rot4          zero baseline, sigma = 0 / 1e-4
  dup                 general with points 300..599 bit-copies of 0..299: octets that hold i and i + 300 have distinct indices and
                      a rank-deficient AtA, so only the conditioning estimate can send them to the host
  wide                general with first-image coordinates up to 3
  pixel               general times 2000 (unnormalised coordinates), thr times 2000^2
  edge                general with planted points a few ulp either side of thr for the winner and the runner-up (_plant_edge)
  nan                 general with two all-NaN points, one drawn by some octet and one by none.  (The reference's Jacobi never picks
                      a NaN pivot, strict '>': a NaN octet yields the finite hypothesis of an unrotated matrix, with a count.)

What is said of the reference here was read off its source; tests/test_oracle_vs_reference_range.py asserts it on the reference
itself: hypotheses, counts, Sampson errors and find_E_ransac of every class at N0 and at the N_SIZES up to 1000, bit for bit.
"""
from __future__ import annotations

import ctypes
import functools
from typing import NamedTuple

import numpy as np

import helpers as H

N0 = 600            # base size
ITERS = 400
SEED = 12345        # find_E_ransac's own (T:657)
THR = 1e-3
MIN_INLIERS = 60
OUTLIER_SHARE = 0.3
PIXEL_SCALE = 2000.0
N_SIZES = (8, 9, 255, 256, 257, 513, 1000, 4097)   # around SC_THREADS = 256: one trip, exactly one, two, three, many
H_SIZES = (1, 3, 4, 5, 8, 9, 17, 400)              # around HPW = 4 and SC_HB = 8
CLASSES = ("general0", "general", "planar0", "planar6", "planar3", "rot0", "rot4", "dup", "wide", "pixel", "edge", "nan")
K_ID = np.eye(3)
DEV_EPS = 1e-16     # include/sfmx.h: |E_dev - E_ref| <= 1e-16 / cond per entry
MIN_COND = 1e-13    # include/sfmx.h: hypotheses with cond < 1e-13 are derived on the host
KEYS6 = ("E", "cond", "flags", "counts", "lo", "hi")   # the six outputs of sfmx_ransac_score_ex besides the winner
N_EDGE = (16, 8)    # planted pairs of each kind (just below / at or just above thr) for the winner and for the runner-up
N_SUPPORT = (32, 16)  # further planted pairs at 0.9 thr, which give the two a lead over the other near-true hypotheses


class Scene(NamedTuple):
    name: str
    xi: np.ndarray        # [n][2]
    xj: np.ndarray        # [n][2]
    thr: float
    outlier: np.ndarray   # [n] bool: x' is uniform noise (before planting)
    special: np.ndarray   # planted (edge) / NaN (nan) point indices, else empty

    @property
    def n(self):
        return self.xi.shape[0]


def _rodrigues(w):
    w = np.asarray(w, float)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


R_SMALL = _rodrigues([0.03, -0.05, 0.02])
T_BASE = np.array([1.5, 0.2, -0.4])   # parallax of about 0.3 between depth 3 and 8: ten times what thr = 1e-3 tolerates


def _two_views(n, sigma, shape="general", spread=0.45, baseline=True, seed=2024, gross=False):
    """n correspondences of a small rotation (+ translation): first-image points uniform in [-spread, spread]^2 at depth 3..8
    (shape "planar": on the plane 0.2 x - 0.1 y + z = 5), second-image noise sigma, OUTLIER_SHARE of the second-image points
    replaced by uniform ones (gross: redrawn until they are at least 0.1 away from their true epipolar line, so that no outlier
    is an inlier of the true E by accident)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-spread, spread, (n, 2))
    z = rng.uniform(3.0, 8.0, n)
    if shape == "planar":
        z = 5.0 / (1.0 + 0.2 * xy[:, 0] - 0.1 * xy[:, 1])
    X = np.column_stack([xy[:, 0] * z, xy[:, 1] * z, z])
    Y = X @ R_SMALL.T + (T_BASE if baseline else 0.0)
    xj = Y[:, :2] / Y[:, 2:3] + sigma * rng.standard_normal((n, 2))
    out = np.zeros(n, bool)
    out[rng.permutation(n)[: int(round(OUTLIER_SHARE * n))]] = True
    uni = rng.uniform(-spread, spread, (n, 2))
    if gross:
        t = T_BASE
        Et = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R_SMALL
        lines = np.column_stack([xy, np.ones(n)]) @ Et.T
        for i in np.nonzero(out)[0]:
            while abs(lines[i, 0] * uni[i, 0] + lines[i, 1] * uni[i, 1] + lines[i, 2]) < 0.1 * np.hypot(lines[i, 0], lines[i, 1]):
                uni[i] = rng.uniform(-spread, spread, 2)
    xj[out] = uni[out]
    return np.ascontiguousarray(xy), np.ascontiguousarray(xj), out


def draws(n, iters=ITERS):
    """the octets find_E_ransac draws for n points (T:657-665)"""
    return H.uniform_draws(H.oracle(), "orc", SEED, n, 8 * iters).reshape(iters, 8)


def hypotheses(xi, xj, idx8):
    """the reference's hypothesis of every octet (platform libm Jacobi)"""
    idx8 = H.i32(idx8)
    E = np.zeros((len(idx8), 3, 3))
    H.oracle().call("orc_ransac_hypotheses", None, H.f64(xi), H.f64(xj), idx8, len(idx8), E)
    return E


def counts(xi, xj, E, thr):
    c = np.zeros(len(E), np.int32)
    H.oracle().call("orc_ransac_counts", None, H.f64(xi), H.f64(xj), len(xi), H.f64(E), len(E), float(thr), c)
    return c


def sampson_all(E, xi, xj):
    """orc_sampson_err of every point for one E"""
    fn = H.oracle().dll.orc_sampson_err
    fn.restype = ctypes.c_double
    Ep = H.f64(E).ctypes.data_as(ctypes.c_void_p)
    d = ctypes.c_double
    return np.array([fn(Ep, d(a[0]), d(a[1]), d(b[0]), d(b[1])) for a, b in zip(xi.tolist(), xj.tolist())])


def winner_and_runner_up(cref):
    """the reference's winner (first maximum, T:673) and the iteration that would win without it"""
    w = int(np.argmax(cref))
    c = cref.copy()
    c[w] = -1
    return w, int(np.argmax(c))


def _plant_edge(xi, xj, outlier, thr):
    """points a few ulp either side of thr for the winner h* and the runner-up: outlier points that neither octet holds are replaced
    by a random x and an x' that starts on the epipolar line of x under E_h and is bisected along the line's normal with
    orc_sampson_err until two neighbouring offsets have err < thr <= err.  A planted point is on either side of thr for any other
    near-true hypothesis, so they alone would leave the winner to chance among a dozen hypotheses within a few counts of each
    other: N_SUPPORT more pairs at 0.9 thr, counted by a hypothesis close to E_h more often than not, give h* a lead over the
    runner-up and the runner-up a lead over the rest.  Repeated with the new winner and runner-up until they are stable."""
    idx8 = draws(len(xi))
    rng = np.random.default_rng(99)
    fn = H.oracle().dll.orc_sampson_err
    fn.restype = ctypes.c_double
    d = ctypes.c_double

    def pair(E, below, thr=thr):
        Ep = E.ctypes.data_as(ctypes.c_void_p)
        while True:
            x = rng.uniform(-0.4, 0.4, 2)
            l = E @ np.array([x[0], x[1], 1.0])
            nrm = np.hypot(l[0], l[1])
            p0 = rng.uniform(-0.4, 0.4, 2)
            p = p0 - (l[0] * p0[0] + l[1] * p0[1] + l[2]) / nrm ** 2 * l[:2]
            nh = l[:2] / nrm * (1.0 if rng.random() < 0.5 else -1.0)

            def err(t):
                return fn(Ep, d(x[0]), d(x[1]), d(p[0] + t * nh[0]), d(p[1] + t * nh[1]))
            a, b = 0.0, 0.2
            if not (abs(p).max() < 0.45 and err(a) < thr <= err(b)):
                continue
            while True:
                m = 0.5 * (a + b)
                if m == a or m == b:
                    break
                if err(m) < thr:
                    a = m
                else:
                    b = m
            t = a if below else b
            return x, np.array([p[0] + t * nh[0], p[1] + t * nh[1]])

    E = hypotheses(xi, xj, idx8)   # neither octet holds a replaced point, so these two rows are also the planted scene's
    guess = winner_and_runner_up(counts(xi, xj, E, thr))
    for _ in range(64):
        keep = set(idx8[guess[0]].tolist()) | set(idx8[guess[1]].tolist())
        free = [int(i) for i in np.nonzero(outlier)[0] if int(i) not in keep]
        yi, yj = xi.copy(), xj.copy()
        k = 0
        for h, m in zip(guess, N_EDGE):
            for below in (True, False):
                for _ in range(m):
                    yi[free[k]], yj[free[k]] = pair(np.ascontiguousarray(E[h]), below)
                    k += 1
        for h, m in zip(guess, N_SUPPORT):
            for _ in range(m):
                yi[free[k]], yj[free[k]] = pair(np.ascontiguousarray(E[h]), True, 0.9 * thr)
                k += 1
        now = winner_and_runner_up(counts(yi, yj, hypotheses(yi, yj, idx8), thr))   # octets that hold a replaced point have moved
        if now == guess:
            return yi, yj, np.array(free[:k], np.int64)
        guess = now
    raise AssertionError("edge scene: the oracle's winner did not settle")


@functools.lru_cache(maxsize=None)
def scene(name, n=N0) -> Scene:
    none = np.zeros(0, np.int64)
    thr = THR
    if name in ("general0", "general", "dup", "pixel", "edge", "nan"):
        xi, xj, out = _two_views(n, 0.0 if name == "general0" else 1e-3, gross=name == "general0")
    elif name in ("planar0", "planar6", "planar3"):
        xi, xj, out = _two_views(n, {"0": 0.0, "6": 1e-6, "3": 1e-3}[name[-1]], shape="planar")
    elif name in ("rot0", "rot4"):
        xi, xj, out = _two_views(n, 0.0 if name == "rot0" else 1e-4, baseline=False)
    elif name == "wide":
        xi, xj, out = _two_views(n, 1e-3, spread=3.0)
    else:
        raise KeyError(name)
    special = none
    if name == "dup":
        h = n // 2
        xi[h:2 * h], xj[h:2 * h], out[h:2 * h] = xi[:h], xj[:h], out[:h]
    elif name == "pixel":
        xi, xj, thr = xi * PIXEL_SCALE, xj * PIXEL_SCALE, THR * PIXEL_SCALE ** 2
    elif name == "edge":
        xi, xj, special = _plant_edge(xi, xj, out, thr)
    elif name == "nan":
        idx8 = draws(n)
        w, r = winner_and_runner_up(counts(xi, xj, hypotheses(xi, xj, idx8), thr))
        keep = set(idx8[w]) | set(idx8[r])
        drawn = np.bincount(idx8.ravel(), minlength=n)
        a = next(i for i in range(n) if drawn[i] > 0 and i not in keep)
        b = next(i for i in range(n) if drawn[i] == 0)
        special = np.array([a, b], np.int64)
        xi[special], xj[special] = np.nan, np.nan
    for a in (xi, xj, out, special):
        a.setflags(write=False)
    return Scene(name, xi, xj, thr, out, special)


class Tables(NamedTuple):
    idx8: np.ndarray   # [ITERS][8]
    E: np.ndarray      # [ITERS][3][3] the reference's hypotheses
    win: int
    runner_up: int


@functools.lru_cache(maxsize=None)
def tables(name, n=N0) -> Tables:
    """octets and reference hypotheses of scene(name, n) restricted to its first n points when n < N0 (octets drawn for that n)"""
    s = scene(name, max(n, N0))
    idx8 = draws(n)
    E = hypotheses(s.xi[:n], s.xj[:n], idx8)
    w, r = winner_and_runner_up(ref_counts(name, n, s.thr, E))
    for a in (idx8, E):
        a.setflags(write=False)
    return Tables(idx8, E, w, r)


_cref: dict = {}


def ref_counts(name, n, thr, E=None):
    """orc_ransac_counts of all ITERS reference hypotheses, computed once per (scene, n, thr)"""
    k = (name, n, float(thr))
    if k not in _cref:
        s = scene(name, max(n, N0))
        c = counts(s.xi[:n], s.xj[:n], tables(name, n).E if E is None else E, thr)
        c.setflags(write=False)
        _cref[k] = c
    return _cref[k]


def points(name, n=N0):
    s = scene(name, max(n, N0))
    return np.ascontiguousarray(s.xi[:n]), np.ascontiguousarray(s.xj[:n])


def repeated(idx8):
    """octets with a repeated sample index"""
    s = np.sort(idx8, axis=1)
    return (s[:, 1:] == s[:, :-1]).any(axis=1)


def ref_cond(xi, xj, idx8):
    """Conditioning of every octet as the reference sees it, from NumPy's eigh / svd (classification only): the minimum of the gap
    between the two smallest eigenvalues of AtA relative to the largest, and (s1^2 - s2^2) / s0^2 of the null vector.  NaN octets: 0."""
    out = np.zeros(len(idx8))
    for h, o in enumerate(idx8):
        x, y, xp, yp = xi[o, 0], xi[o, 1], xj[o, 0], xj[o, 1]
        A = np.column_stack([xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, np.ones(8)])
        if not np.isfinite(A).all():
            continue
        w, V = np.linalg.eigh(A.T @ A)
        s = np.linalg.svd(V[:, 0].reshape(3, 3), compute_uv=False)
        out[h] = max(0.0, min((w[1] - w[0]) / np.abs(w).max(), (s[1] ** 2 - s[2] ** 2) / s[0] ** 2))
    return out


def shard_range(n, rank, world):
    """sfmx_shard_range: contiguous, the first n % world ranks hold one more"""
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def rank_of(it, n, world):
    return next(r for r in range(world) if shard_range(n, r, world)[0] <= it < shard_range(n, r, world)[1])


class Contract(NamedTuple):
    worst: float       # largest max|E - Eref| * cond over device rows (0 if there is none)
    n_band: int        # rows with lo < hi
    n_exact_clean: int  # exact rows without a repeated index (second-round hypotheses)


def check_contract(res, Eref, cref, what, idx8=None, nan_equal=False, min_cond=MIN_COND) -> Contract:
    """The contract of sfmx_ransac_score_ex as include/sfmx.h states it, against the reference's hypotheses and counts of every
    iteration.  idx8 (optional) only serves the third returned figure."""
    Eref, cref = np.asarray(Eref), np.asarray(cref)
    ex = res["flags"].astype(bool)
    dev = ~ex
    lo, hi, cnt, cond = res["lo"], res["hi"], res["counts"], res["cond"]
    H.assert_bits_equal(res["E"][ex], Eref[ex], f"{what}: exact (host libm) hypotheses", nan_equal=nan_equal)
    bad = np.nonzero((lo > cref) | (cref > hi))[0]
    assert bad.size == 0, (what, "reference count outside [lo, hi]", bad[:5], lo[bad[:5]], cref[bad[:5]], hi[bad[:5]], cond[bad[:5]])
    assert np.array_equal(lo[ex], cref[ex]) and np.array_equal(hi[ex], cref[ex]) and np.array_equal(cnt[ex], cref[ex]), (what, "exact rows")
    tight = lo == hi
    assert np.array_equal(cnt[tight], cref[tight]), (what, "lo == hi but counts differ", np.nonzero(tight & (cnt != cref))[0][:5])
    assert np.all((lo <= cnt) & (cnt <= hi)), (what, "count outside its own bounds")
    assert np.all(np.isposinf(cond[ex])), (what, "cond of exact rows")
    assert np.all(cond[dev] >= min_cond), (what, "device row below the conditioning floor", cond[dev].min() if dev.any() else None)
    best = int(np.argmax(cnt))
    assert (res["best_iter"], res["best_count"]) == (best, int(cnt[best])), (what, "winner is not the first argmax of counts")
    dist = np.abs(res["E"] - Eref).max(axis=(1, 2))
    prod = dist[dev] * cond[dev]
    worst = float(prod.max()) if dev.any() else 0.0
    assert not dev.any() or worst <= DEV_EPS, (what, "max|E - Eref| * cond", worst, "rows", np.nonzero(dev)[0][np.argsort(-prod)[:5]])
    clean = ex & ~repeated(idx8) if idx8 is not None else np.zeros_like(ex)
    return Contract(worst, int((lo < hi).sum()), int(clean.sum()))


def summary_row(name, res, Eref, idx8, min_cond=MIN_COND):
    """the measured figures of one scene class that `ransac_child.py table` prints"""
    ex = res["flags"].astype(bool)
    dev = ~ex
    rep = repeated(idx8)
    dist = np.abs(res["E"] - Eref).max(axis=(1, 2))
    flip = np.minimum(dist, np.abs(res["E"] + Eref).max(axis=(1, 2)))
    n = len(ex)
    lo, hi = res["lo"], res["hi"]
    band = lo < hi
    return dict(name=name, worst=float((dist[dev] * res["cond"][dev]).max()) if dev.any() else 0.0,
                worst_up_to_sign=float((flip[dev] * res["cond"][dev]).max()) if dev.any() else 0.0,
                repeated=rep.sum() / n, second_round=(ex & ~rep).sum() / n, dev_low=(dev & (res["cond"] < 1e-8)).sum() / n,
                band=band.sum() / n, verify=int((band & (hi >= lo.max())).sum()))
