"""The cases on which the CPU oracle (oracle/sfm_oracle.cpp) is held to the real reference over the inputs of the range suites:
tests/test_oracle_vs_reference_range.py runs them, tests/golden/make_range_golden.py records the reference's results for them in
tests/golden/range_ref.json.  Inputs come from the generators of the range suites as they are (frontend_inputs, ba_inputs,
ransac_inputs, posegraph_inputs, solve_inputs): a table that grows there grows here.

A case is (family, id, run): run(lib, pre) calls the library `lib` through the wrappers of tests/helpers.py with the prefix `pre`
("orc" or "ref") and returns {name: ndarray | int}.  Arrays are compared bit for bit (any NaN equals any NaN) and recorded as one
SHA-256 per case, ints (return codes, counts) are compared for equality and recorded in clear, as are the shapes."""
from __future__ import annotations

import ctypes
import hashlib
import importlib
import os
from typing import Callable, NamedTuple

import numpy as np

import ba_inputs as B
import frontend_inputs as F
import helpers as H
import posegraph_inputs as P
import ransac_inputs as R
import solve_inputs as SI

synth = importlib.import_module(H.PKG_NAME + ".synth")


# Cases on which the reference's behaviour is undefined (an out-of-bounds read, say): "family/id" -> the reference line that makes
# it so.  Such a case is not compared with the reference; the fixture then holds the oracle's own record for it, marked as such.
# Empty: the reference needed no exclusion on any case below.
UNDEFINED_IN_REFERENCE: dict = {}


class Case(NamedTuple):
    family: str
    id: str
    run: Callable   # (lib, pre) -> {name: ndarray | int}


# ---- digests --------------------------------------------------------------------------------------------------------------------
def canonical(a):
    """a contiguous copy with every NaN replaced by the one canonical quiet NaN (x86 generates the negative one, other targets and
    numpy the positive one: NaN-ness is compared, its sign and payload are not)"""
    a = np.array(a, copy=True, order="C")
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.array(np.nan, a.dtype)
    return a


def record(result):
    """what the fixture holds for one case: the SHA-256 of all arrays (name, dtype, shape and canonical bytes, in name order), the
    shapes in clear (one string, in name order, to keep the file small) and the ints in clear"""
    h = hashlib.sha256()
    shapes, ints = [], {}
    for k in sorted(result):
        v = result[k]
        if isinstance(v, np.ndarray):
            a = canonical(v)
            h.update(f"{k}|{a.dtype.str}|{a.shape}|".encode())
            h.update(a.tobytes())
            shapes.append("x".join(str(n) for n in a.shape))
        else:
            ints[k] = int(v)
    return {"sha256": h.hexdigest(), "shapes": " ".join(shapes), "rc": ints}


def compare(family, cid, got, exp):
    """the bitwise comparison of two results of one case; a failure names the family, the case, the output and the first element"""
    assert sorted(got) == sorted(exp), (family, cid, sorted(got), sorted(exp))
    for k in sorted(got):
        a, b = got[k], exp[k]
        what = f"{family} {cid}: {k}"
        if not isinstance(a, np.ndarray):
            assert int(a) == int(b), (what, a, b)
        elif a.dtype.kind == "f":
            H.assert_bits_equal(a.astype(np.float64), np.asarray(b).astype(np.float64), what, nan_equal=True)   # float32 -> float64 is exact
        else:
            assert a.shape == b.shape, (what, a.shape, b.shape)
            ne = np.argwhere(a != b)
            assert ne.size == 0, (what, f"{len(ne)} of {a.size} differ; first at {ne[0].tolist()}", a[tuple(ne[0])], b[tuple(ne[0])])


# ---- pyramid --------------------------------------------------------------------------------------------------------------------
def _random_image(w, h):
    return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)


def _downsample_cases():
    def make(w, h):
        def run(lib, pre):
            out, cur = {}, _random_image(w, h)
            l = 0
            while min(cur.shape) >= 2:   # down to a level of one pixel in either axis
                cur = H.downsample2(lib, pre, cur)
                l += 1
                out[f"level{l}"] = cur
            out["levels"] = l
            return out
        return run
    return [Case("downsample2", f"{w}x{h}", make(w, h)) for w, h in F.SIZES]


# ---- corners --------------------------------------------------------------------------------------------------------------------
_caps: dict = {}


def _tied_caps(kind, w, h, quality, md):
    """caps that cut inside a run of picked corners of one score: the first such position and the middle one (none where no two
    consecutive picks tie: four grey levels at min_dist 8 and 16 on the smallest sizes)"""
    if (kind, w, h, quality, md) not in _caps:
        img = F.score_image(kind, w, h)
        full = H.shi_tomasi(H.oracle(), "orc", img, img.size, quality, md)
        s = F.oracle_score(img)[full[:, 1].astype(int), full[:, 0].astype(int)]
        inside = np.flatnonzero(s[1:] == s[:-1]) + 1   # a cap of k keeps picks 0 .. k-1: pick k-1 and pick k tie
        _caps[(kind, w, h, quality, md)] = sorted({int(inside[0]), int(inside[len(inside) // 2])}) if inside.size else []
    return _caps[(kind, w, h, quality, md)]


def _shi_cases():
    out = []

    def make(kind, w, h):
        def run(lib, pre):
            img = F.score_image(kind, w, h)
            return {f"md{md}/q{q}": H.shi_tomasi(lib, pre, img, w * h, q, md) for md in F.MIN_DIST for q in F.QUALITY}
        return run

    def make_cap(kind, w, h):
        def run(lib, pre):
            img = F.score_image(kind, w, h)
            res = {}
            for md in F.MIN_DIST:
                for cap in _tied_caps(kind, w, h, 0.01, md):
                    res[f"md{md}/cap{cap}"] = H.shi_tomasi(lib, pre, img, cap, 0.01, md)
            assert len(res) >= 4, "caps inside a tie at fewer than two values of min_dist"
            return res
        return run
    for kind in F.SCORE_KINDS:
        for w, h in F.SIZES:
            out.append(Case("shi_tomasi", f"{kind}/{w}x{h}", make(kind, w, h)))
    for kind in F.TIE_HEAVY:
        for w, h in F.TRACKER_SIZES:
            out.append(Case("shi_tomasi", f"{kind}/{w}x{h}/cap inside a tie", make_cap(kind, w, h)))
    return out


# ---- KLT ------------------------------------------------------------------------------------------------------------------------
def _klt(lib, pre, name, levels, r, iters, xy, fb=1.0):
    p = F.pair(name)
    with np.errstate(invalid="ignore"):   # the population holds inf and NaN coordinates
        fwd, back, keep = H.klt_track(lib, pre, p.a, p.b, levels, r, iters, xy, fb)
    return {"fwd": fwd, "back": back, "keep": keep}


def _level_counts(name):
    p = F.pair(name)
    return list(range(1, p.max_levels + 1)) + ([F.BELOW_2X2[1]] if name == F.BELOW_2X2[0] else [])


def _klt_cases():
    out = []
    for name in F.PAIRS:
        p = F.pair(name)
        for r in range(1, F.KLT_MAX_R + 1):
            out.append(Case("lk_step", f"{name}/r{r}", lambda lib, pre, name=name, r=r: {
                "step": np.array([H.lk_step(lib, pre, F.pair(name).a, F.pair(name).b, r, x, y) for x, y in F.pair_population(name, r)[0]])}))
            out.append(Case("klt_track", f"{name}/r{r}/levels{p.levels}", lambda lib, pre, name=name, r=r, lv=p.levels:
                            _klt(lib, pre, name, lv, r, F.VARIANT_ITERS, F.pair_population(name, r)[0])))
        for lv in _level_counts(name):
            out.append(Case("klt_track", f"{name}/r5/levels{lv}/iters4", lambda lib, pre, name=name, lv=lv:
                            _klt(lib, pre, name, lv, 5, 4, F.pair_population(name, 5, lv)[0])))

    def fb_values():
        e = F.fb_edge("small", 5, 3, F.VARIANT_ITERS)[1]
        return F.FB + (e, float(np.nextafter(e, 2.0)))

    def run_fb(lib, pre):
        xy = F.pair_population("small", 5, 3)[0]
        res = {}
        for k, fb in enumerate(fb_values()):
            for key, v in _klt(lib, pre, "small", 3, 5, F.VARIANT_ITERS, xy, fb).items():
                res[f"fb[{k}]/{key}"] = v
        for fb in (1.0, 0.0):
            for key, v in _klt(lib, pre, "small", 3, 5, 0, xy, fb).items():
                res[f"iters0/fb{fb}/{key}"] = v
        return res
    out.append(Case("klt_track", "small/r5/levels3/every fb", run_fb))
    for r in (2, 5, 6):
        def run_ragged(lib, pre, r=r):
            xy = F.pair_population("small", r)[0]
            res = {}
            for n in F.RAGGED_N:
                for key, v in _klt(lib, pre, "small", F.pair("small").levels, r, F.VARIANT_ITERS, np.ascontiguousarray(xy[:n])).items():
                    res[f"n{n}/{key}"] = v
            return res
        out.append(Case("klt_track", f"small/r{r}/ragged prefixes", run_ragged))
    return out


# ---- tracker --------------------------------------------------------------------------------------------------------------------
TRACKER_FRAMES = 3
TRACKER_MIN_DIST = (2, 4)   # at 8 and 16 the smallest images lose every track, and nothing survives to be replenished


def tracker_frames(kind, w, h):
    """the score image moved by one pixel per frame"""
    img = F.score_image(kind, w + TRACKER_FRAMES - 1, h)
    return [np.ascontiguousarray(img[:, k:k + w]) for k in range(TRACKER_FRAMES)]


def _tracker_cases():
    def make(kind, w, h, md):
        def run(lib, pre):
            T = H.Tracker(lib, pre, max_tracks=4000, min_tracks=3900, quality=0.01, min_distance=md, levels=3, radius=5, iters=10, fb=1.0)
            res = {}
            try:
                for f, img in enumerate(tracker_frames(kind, w, h)):
                    prev, cur, ids = T.step(img)
                    txy, tid = T.tracks()
                    res.update({f"f{f}/prev": prev, f"f{f}/cur": cur, f"f{f}/ids": ids, f"f{f}/tracks": txy, f"f{f}/track ids": tid,
                                f"f{f}/survivors": len(ids), f"f{f}/live": len(tid)})
            finally:
                T.close()
            return res
        return run
    return [Case("tracker", f"{kind}/{w}x{h}/md{md}", make(kind, w, h, md))
            for (w, h) in F.TRACKER_SIZES for kind in F.TIE_HEAVY + ("noisy",) for md in TRACKER_MIN_DIST]


# ---- dense solve ----------------------------------------------------------------------------------------------------------------
def _solve_run(A, b):
    """A, b: one system, or tuples of several (the sweep of solve_inputs: one case per n) -> rc and x of each under its name"""
    def run(lib, pre):
        if not isinstance(A, tuple):
            rc, x = H.solve_gauss(lib, pre, A, b)
            return {"rc": rc, "x": x if rc == 0 else np.zeros(0)}
        res = {}
        for name, Ak, bk in zip(SI.SWEEP_SYSTEMS, A, b):
            rc, x = H.solve_gauss(lib, pre, Ak, bk)
            res[f"{name}/rc"], res[f"{name}/x"] = rc, x if rc == 0 else np.zeros(0)
        return res
    return run


def _solve_cases():
    out = [Case("solve_gauss", cid, _solve_run(A, b)) for cid, A, b in SI.all_cases()]
    g = np.load(os.path.join(H.GOLDEN, "hotpath.npz"))   # the recorded systems test_solve_dense starts with
    for n in (6, 36, 60, 7):
        out.append(Case("solve_gauss", f"golden/n={n}", _solve_run(g[f"sg_A_{n}"], g[f"sg_b_{n}"])))
    out.append(Case("solve_gauss", "golden/singular", _solve_run(g["sg_A_sing"], np.ones(5))))
    return out


# ---- two-view geometry ----------------------------------------------------------------------------------------------------------
RANSAC_N = (R.N0,) + tuple(n for n in R.N_SIZES if n <= 1000)
K_PIXEL = np.array([[1520.4, 0.0, 302.32], [0.0, 1525.9, 246.87], [0.0, 0.0, 1.0]])
N_OTHER = 16   # evenly spaced hypotheses counted besides the winner and the runner-up


def _sampson_all(lib, pre, E, xi, xj):
    fn = getattr(lib.dll, f"{pre}_sampson_err")
    fn.restype = ctypes.c_double
    Ep = H.f64(E)
    ptr = Ep.ctypes.data_as(ctypes.c_void_p)
    d = ctypes.c_double
    return np.array([fn(ptr, d(a[0]), d(a[1]), d(b[0]), d(b[1])) for a, b in zip(xi.tolist(), xj.tolist())])


def _eight_point_all(lib, pre, xi, xj, idx8):
    return np.array([H.eight_point(lib, pre, xi, xj, o) for o in idx8]).reshape(-1, 3, 3)


def counted(name, n):
    """the hypotheses whose counts are compared: the winner, the runner-up and N_OTHER evenly spaced others"""
    t = R.tables(name, n)
    return sorted({t.win, t.runner_up} | {int(i) for i in np.linspace(0, R.ITERS - 1, N_OTHER).round()})


def _ransac_cases():
    out = []
    for name in R.CLASSES:
        for n in RANSAC_N:
            def run_norm(lib, pre, name=name, n=n):
                xi, xj = R.points(name, n)
                res = {}
                for tag, K in (("identity", R.K_ID), ("pixel", K_PIXEL)):
                    for side, x in (("i", xi), ("j", xj)):
                        rc, q = H.normalize_points(lib, pre, K, x * (1.0 if tag == "identity" else 1500.0))
                        res[f"{tag}/{side}/rc"], res[f"{tag}/{side}"] = rc, q
                res["singular K/rc"] = H.normalize_points(lib, pre, np.zeros((3, 3)), xi)[0]
                return res
            out.append(Case("normalize_points", f"{name}/n{n}", run_norm))

            def run_hyp(lib, pre, name=name, n=n):
                """orc_ransac_hypotheses (what the kernels are compared with) against the reference's eight_point_E of every octet"""
                xi, xj = R.points(name, n)
                idx8 = R.tables(name, n).idx8
                if pre == "orc":
                    E = np.zeros((len(idx8), 3, 3))
                    lib.call("orc_ransac_hypotheses", None, H.f64(xi), H.f64(xj), H.i32(idx8), len(idx8), E)
                    return {"E": E}
                return {"E": _eight_point_all(lib, pre, xi, xj, idx8)}
            out.append(Case("ransac_hypotheses", f"{name}/n{n}", run_hyp))

            def run_counts(lib, pre, name=name, n=n):
                """orc_ransac_counts against counts made from the reference's sampson_err (err < thr, T:669-671)"""
                xi, xj = R.points(name, n)
                t = R.tables(name, n)
                thr = R.scene(name, max(n, R.N0)).thr
                sel = counted(name, n)
                if pre == "orc":
                    E = np.ascontiguousarray(t.E[sel])
                    c = np.zeros(len(sel), np.int32)
                    lib.call("orc_ransac_counts", None, H.f64(xi), H.f64(xj), len(xi), E, len(sel), float(thr), c)
                    return {"counts": c}
                E = _eight_point_all(lib, pre, xi, xj, t.idx8[sel])
                return {"counts": np.array([int((_sampson_all(lib, pre, e, xi, xj) < thr).sum()) for e in E], np.int32)}
            out.append(Case("ransac_counts", f"{name}/n{n}", run_counts))

            def run_find(lib, pre, name=name, n=n):
                xi, xj = R.points(name, n)
                r = H.find_E_ransac(lib, pre, R.K_ID, xi, xj, R.ITERS, R.scene(name, max(n, R.N0)).thr, R.MIN_INLIERS)
                return {"ok": r["ok"], "inliers": r["inliers"], "R": r["R"], "t": r["t"]}
            out.append(Case("find_E_ransac", f"{name}/n{n}", run_find))

        def run_eight(lib, pre, name=name):
            xi, xj = R.points(name)
            return {"E": _eight_point_all(lib, pre, xi, xj, R.tables(name).idx8)}
        out.append(Case("eight_point", f"{name}/n{R.N0}", run_eight))

        def run_sampson(lib, pre, name=name):
            xi, xj = R.points(name)
            t = R.tables(name)
            return {f"h{h}": _sampson_all(lib, pre, t.E[h], xi, xj) for h in (t.win, t.runner_up)}
        out.append(Case("sampson", f"{name}/n{R.N0}", run_sampson))
    return out


# ---- small linear algebra -------------------------------------------------------------------------------------------------------
def hard_octets(name, most=4):
    """octets of a scene class with a rank-deficient design matrix (a repeated index, or both copies of a duplicated point) or a
    NaN point, and the first two others"""
    s, t = R.scene(name), R.tables(name)
    rep = R.repeated(t.idx8)
    nan = np.isnan(s.xi[t.idx8]).any(axis=(1, 2))
    twin = np.zeros(len(rep), bool)
    if name == "dup":
        m = np.sort(t.idx8 % (R.N0 // 2), axis=1)
        twin = (m[:, 1:] == m[:, :-1]).any(axis=1) & ~rep
    pick = list(np.flatnonzero(rep)[:most]) + list(np.flatnonzero(nan)[:most]) + list(np.flatnonzero(twin)[:most]) + list(np.flatnonzero(~rep & ~nan & ~twin)[:2])
    return [int(h) for h in pick]


def design_gram(name, h):
    """AtA [9][9] of octet h (numpy's products: an input, not a restatement), made exactly symmetric"""
    s, o = R.scene(name), R.tables(name).idx8[h]
    x, y, xp, yp = s.xi[o, 0], s.xi[o, 1], s.xj[o, 0], s.xj[o, 1]
    A = np.column_stack([xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, np.ones(8)])
    M = np.einsum("ki,kj->ij", A, A)
    return np.ascontiguousarray(np.triu(M) + np.triu(M, 1).T)


SO3_ANGLES = (0.0, 1e-12, 1.0, np.pi - 1e-9, np.pi)
SO3_AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 1.0), (0.3, -0.5, 0.8), (-1.0, 0.0, 0.0))


def triangulation_inputs():
    """(K, Ri, ti, Rj, tj, [(name, ui, uj)]): two ring cameras (camera -> world, t = centre) and the observations of an ordinary
    point, a point in the first camera's plane (depth 0: its own pixel does not exist, any pixel serves), a point behind both
    cameras, the same pixel twice and a NaN pixel"""
    K = synth.K_TEMPLE
    cams = []
    for a in (0.0, 3.0):
        Rw, tw = synth.ring_pose(a)
        cams.append((Rw, tw, np.ascontiguousarray(Rw.T), -Rw.T @ tw))

    def px(c, X):
        Xc = cams[c][0] @ X + cams[c][1]
        return np.array([K[0, 0] * Xc[0] / Xc[2] + K[0, 2], K[1, 1] * Xc[1] / Xc[2] + K[1, 2]])
    X0 = np.array([0.01, 0.02, 0.03])
    Xplane = cams[0][3] + cams[0][2] @ np.array([0.1, 0.05, 0.0])
    Xbehind = cams[0][3] + cams[0][2] @ np.array([0.02, -0.01, -0.5])
    obs = [("ordinary", px(0, X0), px(1, X0)), ("depth 0", np.array([K[0, 2] + 1000.0, K[1, 2] - 500.0]), px(1, Xplane)),
           ("behind", px(0, Xbehind), px(1, Xbehind)), ("same pixel", px(0, X0), px(0, X0)),
           ("nan pixel", np.array([np.nan, 10.0]), px(1, X0))]
    return K, cams[0][2], cams[0][3], cams[1][2], cams[1][3], obs


def _linalg_cases():
    out = []
    for name in R.CLASSES:
        def run_jacobi(lib, pre, name=name):
            res = {}
            for h in hard_octets(name):
                w, V = H.jacobi(lib, pre, design_gram(name, h), 120)
                res[f"h{h}/w"], res[f"h{h}/V"] = w, V
                E = np.ascontiguousarray(R.tables(name).E[h])
                w, V = H.jacobi(lib, pre, np.ascontiguousarray(np.triu(E.T @ E) + np.triu(E.T @ E, 1).T), 80)
                res[f"h{h}/EtE/w"], res[f"h{h}/EtE/V"] = w, V
            return res
        out.append(Case("jacobi", name, run_jacobi))

        def run_svd(lib, pre, name=name):
            res = {}
            for h in hard_octets(name):
                for tag, M in (("E", R.tables(name).E[h]), ("AtA[:3,:3]", design_gram(name, h)[:3, :3])):
                    U, s, V = H.svd3(lib, pre, np.ascontiguousarray(M))
                    res[f"h{h}/{tag}/U"], res[f"h{h}/{tag}/s"], res[f"h{h}/{tag}/V"] = U, s, V
            return res
        out.append(Case("svd3", name, run_svd))

    def run_svd_fixed(lib, pre):
        res = {}
        for tag, M in (("zero", np.zeros((3, 3))), ("identity", np.eye(3)), ("rank 1", np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0])),
                       ("reflection", np.diag([1.0, 1.0, -1.0])), ("nan", np.full((3, 3), np.nan))):
            U, s, V = H.svd3(lib, pre, M)
            res[f"{tag}/U"], res[f"{tag}/s"], res[f"{tag}/V"] = U, s, V
        return res
    out.append(Case("svd3", "fixed matrices", run_svd_fixed))

    def run_so3(lib, pre):
        res = {}
        for a in SO3_ANGLES:
            for k, ax in enumerate(SO3_AXES):
                u = np.array(ax) / np.linalg.norm(ax)
                Rm = H.so3_exp(lib, pre, a * u)
                res[f"angle {a!r}/axis {k}/exp"] = Rm
                res[f"angle {a!r}/axis {k}/log of exp"] = H.so3_log(lib, pre, Rm)
                res[f"angle {a!r}/axis {k}/log of numpy"] = H.so3_log(lib, pre, R._rodrigues(a * u) if a > 0 else np.eye(3))
        return res
    out.append(Case("so3", "angles 0, 1e-12, 1, pi - 1e-9, pi", run_so3))

    def run_tri(lib, pre):
        K, Ri, ti, Rj, tj, obs = triangulation_inputs()
        return {name: H.triangulate(lib, pre, K, Ri, ti, Rj, tj, ui, uj) for name, ui, uj in obs}
    out.append(Case("triangulate", "ordinary, depth 0, behind, same pixel, nan", run_tri))
    return out


# ---- bundle adjustment ----------------------------------------------------------------------------------------------------------
BA_ITERS = (1, 2)
BA_PARAM_PROBLEMS = {"W6-clean": lambda: B.window(6, "clean"), "W6-dup": lambda: B.window(6, "dup")}


class BaCase(NamedTuple):
    id: str
    prob: Callable      # () -> ba_inputs.Problem
    huber: object       # an entry of ba_inputs.HUBER, or a float
    lam: float
    max_points: object  # None: all points
    iters: tuple


def ba_cases():
    out = []
    for W, Pn, fl in B.WINDOWS:
        out.append(BaCase(f"window/W{W}-P{Pn}-{fl}", lambda W=W, fl=fl: B.window(W, fl), B.HUBER0, B.LAMBDA0, None, BA_ITERS))
    for W in B.P_EDGE_W:
        for Pn in B.P_EDGES:
            for fl in ("clean", "dup"):
                out.append(BaCase(f"edge/W{W}-P{Pn}-{fl}", lambda W=W, Pn=Pn, fl=fl: B.edge(W, Pn, fl), B.HUBER0, B.LAMBDA0, None, BA_ITERS))
    for W, Pn in B.BIG_P:
        out.append(BaCase(f"big/W{W}-P{Pn}", lambda W=W, Pn=Pn: B.big(W, Pn), B.HUBER0, B.LAMBDA0, None, (1,)))
    for pname, prob in BA_PARAM_PROBLEMS.items():
        for k, h in enumerate(B.HUBER):
            out.append(BaCase(f"huber/{pname}/{h}", prob, h, B.LAMBDA0, None, BA_ITERS))
        for lam in B.LAMBDA:
            out.append(BaCase(f"lambda/{pname}/{lam}", prob, B.HUBER0, lam, None, BA_ITERS))
        out.append(BaCase(f"zero system/{pname}", prob, 0.0, 0.0, None, BA_ITERS))
    for name in B.NONFINITE:
        for fl in ("clean", "dup"):
            out.append(BaCase(f"nonfinite/{name}/{fl}", lambda name=name, fl=fl: B.nonfinite_case(name, 64, fl)[0], B.HUBER0, B.LAMBDA0, None, BA_ITERS))
    for fl in ("clean", "dup"):
        out.append(BaCase(f"half behind/W6-{fl}", lambda fl=fl: B.window(6, fl, half_behind=3), B.HUBER0, B.LAMBDA0, None, BA_ITERS))
        for W in (3, 6, 10, 17):
            out.append(BaCase(f"skewed K/W{W}-{fl}", lambda W=W, fl=fl: B.window(W, fl, K="skewed"), B.HUBER0, B.LAMBDA0, None, BA_ITERS))
        for cap in (1, 2, 7, 150, 299):
            out.append(BaCase(f"max_points/W6-P300-{fl}/{cap}", lambda fl=fl: B.window(6, fl), B.HUBER0, B.LAMBDA0, cap, BA_ITERS))
    return out


def camera_to_world(poses_wc):
    """ba_inputs' world -> camera poses as the camera -> world poses bundle_adjust_window takes (R^T | centre); numpy's rounding,
    these are inputs"""
    out = np.zeros_like(poses_wc)
    for k, p in enumerate(poses_wc):
        Rm = p[:9].reshape(3, 3)
        out[k, :9] = Rm.T.ravel()
        out[k, 9:] = -Rm.T @ p[9:]
    return out


def ba_arguments(c: BaCase):
    """(K, poses camera -> world, X, ptr, li, uv, window, max_points, huber, lambda) of a case"""
    prob = c.prob()
    return (prob.K, camera_to_world(prob.poses), prob.X, prob.ptr, prob.li, prob.uv, prob.W, prob.P if c.max_points is None else c.max_points,
            B.huber_value(prob, c.huber), float(c.lam))


def _ba_cases():
    def make(c):
        def run(lib, pre):
            K, poses, X, ptr, li, uv, W, cap, huber, lam = ba_arguments(c)
            return {f"iters{it}": H.bundle_adjust_window(lib, pre, K, poses, X, ptr, li, uv, W, it, cap, huber, lam) for it in c.iters}
        return run
    return [Case("bundle_adjust_window", c.id, make(c)) for c in ba_cases()]


def ba_point_counts():
    return sorted({c.prob().P for c in ba_cases()})


def _map_order_cases():
    return [Case("map_iteration_order", f"P{n}", lambda lib, pre, n=n: {"order": H.map_iteration_order(lib, pre, n)}) for n in ba_point_counts()]


# ---- pose graph -----------------------------------------------------------------------------------------------------------------
def _posegraph_cases():
    graphs = [(f"{kind}/N{N}", lambda kind=kind, N=N: P.pipe_graph(kind, N)) for kind in P.PIPE_KINDS for N in P.PIPE_SIZES]
    graphs += [(f"cut/N{c[0]}-loops{c[1]}-seed{c[2]}", lambda c=c: P.cut_graph(*c)) for c in P.CUT_CASES]
    graphs += [(f"cut/N{N}-no loops", lambda N=N: P.cut_graph(N, 0, 0)) for N in (3, 33, 40, 129)]
    graphs += [(f"self-edge only/N{N}", lambda N=N: P.self_edge_only_graph(N)) for N in (3, 33, 129)]

    def make(g):
        def run(lib, pre):
            ok, c = H.posegraph(lib, pre, *g())
            return {"ok": ok, "centres": c}
        return run
    return [Case("posegraph_optimize_centers", cid, make(g)) for cid, g in graphs]


# ---- descriptor -----------------------------------------------------------------------------------------------------------------
def _desc_cases():
    out = []
    for w, h in F.SIZES:
        if w >= 32 and h >= 32:
            out.append(Case("global_desc", f"{w}x{h}", lambda lib, pre, w=w, h=h: {
                "random": H.global_desc(lib, pre, _random_image(w, h)), "noisy": H.global_desc(lib, pre, F.score_image("noisy", w, h)),
                "constant": H.global_desc(lib, pre, F.score_image("constant", w, h))}))
    return out


FAMILIES = {"downsample2": _downsample_cases, "shi_tomasi": _shi_cases, "klt": _klt_cases, "tracker": _tracker_cases,
            "solve_gauss": _solve_cases, "two_view": _ransac_cases, "linalg": _linalg_cases, "bundle_adjust_window": _ba_cases,
            "map_iteration_order": _map_order_cases, "posegraph_optimize_centers": _posegraph_cases, "global_desc": _desc_cases}

def all_cases(group=None):
    out = []
    for g, make in FAMILIES.items():
        if group is None or g == group:
            out += make()
    return out


def key(c: Case):
    return f"{c.family}/{c.id}"
