"""CPU suite: surface registration -- the NumPy restatement (tests/register_ref.py): its ordered sum against a plain Python loop
over the same tree at rows of 37, the solve at dimension 6 and 7 against np.linalg.solve, the update against composing the
similarity on sample points, the parameter check across capi, the library and the restatement, every Python-level refusal, the
branches the hand cases are named for, and the two calibrations of DESIGN.md 28."""
import importlib
import inspect
import math

import numpy as np
import pytest

import helpers as H
import register_ref as RG
import sdist_ref as SR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")


def _bound(x):
    """DESIGN.md 15's rule: 1.25 x the measured value, rounded up to two significant digits"""
    q = 10.0 ** (math.floor(math.log10(1.25 * x)) - 1)
    return math.ceil(1.25 * x / q - 1e-9) * q


# ---- the ordered sum -----------------------------------------------------------------------------------------------------------
def _plain_tree(vals):
    """the definition's tree in plain Python over one term's samples"""
    rows = []
    for b in range(0, len(vals), 256):
        blk = list(vals[b:b + 256]) + [0.0] * (256 - len(vals[b:b + 256]))
        t = [0.0] * 256
        for j, v in enumerate(blk):
            t[4 * (j % 64) + j // 64] = float(v)
        off = 128
        while off >= 1:
            t = [t[i] + t[i + off] for i in range(off)]
            off //= 2
        rows.append(t[0])
    while len(rows) > 1:
        nxt = []
        for g in range(0, len(rows), 256):
            t = rows[g:g + 256] + [0.0] * (256 - len(rows[g:g + 256]))
            off = 128
            while off >= 1:
                t = [t[i] + t[i + off] for i in range(off)]
                off //= 2
            nxt.append(t[0])
        rows = nxt
    return rows[0]


@pytest.mark.parametrize("n,k", [(1, 37), (63, 37), (64, 37), (65, 37), (255, 37), (256, 37), (257, 37), (1000, 37), (65537, 2)])
def test_ordered_sum_is_the_tree(n, k):
    rng = np.random.default_rng(n)
    T = rng.normal(size=(k, n)) * 10.0 ** rng.integers(-8, 8, size=(k, n))
    got = RG.ordered_sum(T)
    for t in range(k):
        assert got[t].tobytes() == np.float64(_plain_tree(T[t])).tobytes(), (n, t)
    assert got.tobytes() != T.sum(axis=1).tobytes() or n < 3, "the order matters on such data"


def test_ordered_sum_of_nothing_and_of_negative_zeros():
    assert RG.ordered_sum(np.zeros((37, 0))).tobytes() == np.zeros(37).tobytes()
    assert RG.ordered_sum(np.full((37, 256), -0.0)).tobytes() == np.full(37, -0.0).tobytes(), "a full block of -0.0 stays -0.0"
    assert RG.ordered_sum(np.full((37, 255), -0.0)).tobytes() == np.zeros(37).tobytes(), "padding is +0.0"


# ---- solve and update ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [6, 7])
def test_solve_against_linalg(dim):
    rng = np.random.default_rng(dim)
    for damping in (0.0, 0.5):
        Jm = rng.normal(size=(40, 7))
        A, b = Jm.T @ Jm, Jm.T @ rng.normal(size=40)
        sums = np.array([A[m, n] for m, n in RG.PAIRS] + list(b) + [1.0, 2.0])
        d = RG.solve(sums, damping, dim)
        ref = np.linalg.solve(A[:dim, :dim] + damping * np.eye(dim), -b[:dim])
        assert np.allclose(d[:dim], ref, rtol=1e-10, atol=1e-12) and (dim == 7 or d[6] == 0.0)
    sums[0] = -1.0
    assert RG.solve(sums, 0.0, dim) is None
    sums[0] = float("nan")
    assert RG.solve(sums, 0.0, dim) is None
    assert RG.solve(np.zeros(37), 0.0, dim) is None and RG.solve(np.zeros(37), 1.0, dim) == [0.0] * 7


def test_update_composes_the_similarity():
    rng = np.random.default_rng(5)
    p = [0.3, -0.2, 0.1]
    T = RG.disturb(p, 25.0, 1.3, 0.2, rng)
    delta = [0.02, -0.05, 0.03, 0.01, -0.02, 0.005, 0.04]
    N = RG.update(T, p, delta)
    D, g = np.array(RG.cayley(delta[:3])), 1.0 + delta[6]
    assert np.allclose(D @ D.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(D) - 1.0) < 1e-15
    X = rng.normal(size=(20, 3))
    Y = RG.apply(T, X)
    want = np.asarray(p) + g * ((Y - np.asarray(p)) @ D.T) + np.asarray(delta[3:6])
    assert np.allclose(RG.apply(N, X), want, rtol=0, atol=1e-14)
    assert N["s"] == g * T["s"]
    same = RG.update(T, p, [0.0] * 7)
    assert RG.same_transform(same, dict(T, t=(np.asarray(p) + (T["t"] - np.asarray(p))) + 0.0)), "a zero step leaves R and s alone"
    assert RG.apply(RG.identity(), X).tobytes() == (1.0 * X + 0.0).tobytes()


# ---- parameters ----------------------------------------------------------------------------------------------------------------
def test_check_params_field_by_field():
    d = capi.register_default_params()
    assert d == dict(d_max=0.0, **{k: (int(v) if isinstance(v, int) else v) for k, v in capi.REGISTER_DEFAULTS.items()})
    assert {k: v for k, v in d.items() if k != "d_max"} == RG.DEFAULTS == capi.REGISTER_DEFAULTS
    assert not capi.register_check_params(**d), "d_max has no default"
    assert capi.register_check_params(1e-3) and RG.check_params(1e-3)
    nan, inf = float("nan"), float("inf")
    cases = dict(d_max=[(1e-3, True), (2.0 ** 60, True), (2.0 ** -500, True), (0.0, False), (-1.0, False), (nan, False), (inf, False),
                        (2.0 ** 61, False), (2.0 ** -501, False)],
                 cell=[(0.0, True), (5.0, True), (-1.0, False), (nan, False), (inf, False)],
                 max_iters=[(1, True), (64, True), (0, False), (65, False), (-3, False)],
                 stride=[(1, True), (1000, True), (0, False), (-1, False)],
                 min_points=[(7, True), (10 ** 6, True), (6, False), (0, False)],
                 with_scale=[(0, True), (1, True)],
                 damping=[(0.0, True), (3.0, True), (-1e-9, False), (nan, False), (inf, False)],
                 eps_rot=[(0.0, True), (1.0, True), (-1e-9, False), (nan, False), (inf, False)],
                 eps_scale=[(0.0, True), (1.0, True), (-1e-9, False), (nan, False), (inf, False)],
                 eps_trans=[(0.0, True), (1.0, True), (-1e-9, False), (nan, False), (inf, False)])
    assert set(cases) == {k for k, _ in capi.RegisterParams._fields_}
    for field, vals in cases.items():
        for v, ok in vals:
            kw = dict(d_max=1e-3)
            kw[field] = v
            d_max = kw.pop("d_max")
            assert capi.register_check_params(d_max, **kw) == ok == RG.check_params(d_max, **kw), (field, v)
    lib = capi.load_library()
    assert lib.sfmx_register_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_register_default_params(None)  # tolerated
    p3 = np.ones(3)
    assert lib.sfmx_register_pivot(None, p3.ctypes.data_as(capi.POINTER(capi.c_double))) == capi.SFMX_ERR_INVALID and (p3 == 0).all()
    assert lib.sfmx_register_last_us(None) == 0.0 and lib.sfmx_register_last_query_us(None) == 0.0
    hdr = open(H.ROOT + "/include/sfmx.h").read()
    assert f"#define SFMX_REGISTER_ITERS_CAP {capi.REGISTER_ITERS_CAP} " in hdr and f"#define SFMX_REGISTER_TERMS {capi.REGISTER_TERMS}\n" in hdr
    assert RG.TERMS == capi.REGISTER_TERMS and RG.ITERS_CAP == capi.REGISTER_ITERS_CAP
    assert capi.REGISTER_STATUS == ("CONVERGED", "MAX_ITERS", "TOO_FEW", "DEGENERATE")


TRI_V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
TRI_F = np.array([[0, 1, 2]], np.int32)


def test_python_layer_refusals_and_keys():
    with pytest.raises(TypeError):
        capi.register_params(1.0, iterations=3)
    with pytest.raises(TypeError):
        capi.register_transform(dict(s=1.0, R=np.eye(3)))
    with pytest.raises(TypeError):
        capi.register_transform(dict(s=1.0, R=np.eye(3), t=np.zeros(3), q=1))
    t = capi.register_transform(None)
    assert t.s == 1.0 and list(t.R) == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0] and list(t.t) == [0.0] * 3
    with pytest.raises(TypeError):
        pipe.surface_register(None, TRI_V, TRI_F, TRI_V, TRI_F)  # no d_max
    with pytest.raises(TypeError):
        pipe.surface_register(None, TRI_V, TRI_F, TRI_V, TRI_F, d_max=1.0, iterations=3)
    with pytest.raises(ValueError):
        pipe.surface_register(None, TRI_V, TRI_F + 1, TRI_V, TRI_F, d_max=1.0)
    with pytest.raises(TypeError):
        pipe.surface_eval(None, TRI_V, TRI_F, TRI_V, TRI_F, d_max=1.0, tau=0.5, register=dict(iterations=3))
    with pytest.raises(TypeError):
        pipe.surface_eval(None, TRI_V, TRI_F, TRI_V, TRI_F, tau=0.5, register=True)  # the evaluation's own check comes first
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    gt = dict(gt_verts=TRI_V, gt_faces=TRI_F, d_max=1.0, tau=0.5)
    with pytest.raises(TypeError):
        pipe.fuse(*args, evaluate=dict(gt, register=dict(iterations=3)))
    with pytest.raises(TypeError):
        pipe.fuse(*args, evaluate=dict(gt, registered=True))
    assert inspect.signature(pipe.surface_eval).parameters["register"].default is None
    assert set(pipe.REGISTER_KEYS) == {"d_max", "init"} | set(capi.REGISTER_DEFAULTS)
    assert hasattr(capi.Context, "register")
    assert all(hasattr(capi.Register, k) for k in ("set_target", "system", "run", "apply", "pivot", "last_us", "last_query_us", "close"))
    blob = open(pipe.HOST_LIB_PATH, "rb").read()
    assert b"sfmx_sdist_query" in blob and b"sfmx_register" not in blob, "the host library does not reference the new entries"


# ---- hand targets: the branches by the restatement alone -----------------------------------------------------------------------
HAND_D_MAX = 0.5
HAND_V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [2.0, 0.0, 0.0]])
HAND_F = np.array([[0, 1, 2], [0, 1, 3], [1, 4, 0]], np.int32)  # z = 0, y = 0 (sharing the edge 0-1), and a collinear face


def hand_cases():
    """[(name, V, F, X, reasons, faces)]: targets of one to three faces; reasons = the restatement's branch counts at the identity,
    faces = sdist's face per point"""
    F1, F2, F3 = HAND_F[:1], HAND_F[:2], HAND_F
    F1r = HAND_F[:1, ::-1].copy()  # the same face seen from below: n = (0, 0, -1), so that h can be -0.0
    inplane = np.array([[0.3, 0.3, 0.0], [-0.1, -0.1, -0.0]])
    return [
        ("above the interior", HAND_V, F1, [[0.25, 0.25, 0.3], [0.6, 0.2, -0.1]], dict(clipped=0, collinear=0, used=2), [0, 0]),
        ("beyond an edge and a corner", HAND_V, F1, [[0.5, -0.2, 0.1], [-0.2, -0.2, 0.1], [1.2, -0.1, -0.2]], dict(clipped=0, collinear=0, used=3), [0, 0, 0]),
        ("in the plane", HAND_V, F1r, inplane, dict(clipped=0, collinear=0, used=2), [0, 0]),
        ("a block in the plane", HAND_V, F1r, np.repeat(inplane[1:], 256, axis=0), dict(clipped=0, collinear=0, used=256), [0] * 256),
        ("the bisector of a shared edge", HAND_V, F2, [[0.5, 0.1, 0.1], [0.5, -0.1, -0.1], [0.25, 0.05, 0.3]], dict(clipped=0, collinear=0, used=3), [0, 0, 1]),
        ("nearest to a collinear face", HAND_V, F3, [[1.7, -0.05, -0.05], [0.25, 0.25, 0.1]], dict(clipped=0, collinear=1, used=1), [2, 0]),
        ("beyond d_max", HAND_V, F1, [[0.25, 0.25, 0.6], [0.25, 0.25, 0.3]], dict(clipped=1, collinear=0, used=1), [-1, 0]),
        ("all clipped", HAND_V, F3, [[5.0, 5.0, 5.0], [0.2, 0.2, -0.7], [-3.0, 0.0, 0.0]] * 30, dict(clipped=90, collinear=0, used=0), [-1] * 90),
    ]


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_hand_cases_take_their_branches(case):
    name, V, F, X, reasons, faces = case
    X = np.asarray(X, np.float64)
    used, J, h, w, d2, got = RG.rows(RG.identity(), X, V, F, HAND_D_MAX)
    assert got == reasons
    assert list(SR.brute(X, V, F, HAND_D_MAX)[1]) == faces
    sums, n = RG.system(RG.identity(), X, V, F, HAND_D_MAX)
    assert n == reasons["used"]
    if name == "in the plane":
        assert h.tobytes() == np.array([0.0, -0.0]).tobytes(), "h = +0.0 and -0.0"
    if name == "a block in the plane":
        assert np.signbit(h).all() and sums[35].tobytes() == np.float64(0.0).tobytes() and np.signbit(sums[28:35]).any(), "-0.0 sums survive"
    if name == "all clipped":
        assert sums.tobytes() == np.zeros(37).tobytes()
        r = RG.register(X, V, F, HAND_D_MAX)
        assert (r["status"], r["iterations"]) == (RG.TOO_FEW, 1) and RG.same_transform(r["T"], RG.identity()) and r["trace"] == [(0, 0.0, 0.0, 0.0, 0.0, 0.0)]
    if name == "the bisector of a shared edge":
        both = [SR.tri(X[i], *V[F[f]]) for i in (0, 1) for f in (0, 1)]
        assert both[0] == both[1] and both[2] == both[3], "two faces at exactly the same distance: the smaller index wins"


def test_pivot_orders_the_zeros():
    assert RG.pivot(HAND_V, HAND_F) == [1.0, 0.5, 0.5] and RG.pivot(HAND_V, HAND_F[:0]) == [0.0, 0.0, 0.0]
    V = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, 1.0], [0.0, -0.0, -1.0], [9.0, 9.0, 9.0]])
    p = RG.pivot(V, np.array([[0, 1, 2]], np.int32))  # the unused vertex does not count
    assert np.array(p).tobytes() == np.array([0.0, -0.0, 0.0]).tobytes(), "min = -0.0, max = +0.0 on x; only -0.0 on y"


# ---- calibration --------------------------------------------------------------------------------------------------
# measured with this file's own code; bounds by _bound.  The device is held to bit equality, not to these.
MEASURED = dict(
    iters=(2, 3, 4), status=(RG.CONVERGED,) * 3, n=1467,
    rot=6.857e-2, scale=1.056e-3, trans=8.425e-5, rms_plane=4.987e-4, rms_point=4.987e-4, spread_rot=4.903e-4, spread_scale=1.796e-6, spread_trans=5.193e-7)
CALIB = {k: _bound(v) for k, v in MEASURED.items() if k not in ("iters", "status", "n")}

_calib = {}


def calibration():
    """the first calibration's fixture, built once: target, pivot and per start (true transform source -> target, source)"""
    if not _calib:
        V, F = RG.spheres_mesh(3)
        Xt = RG.spheres_source()
        p = RG.pivot(V, F)
        rng = np.random.default_rng(11)
        starts = []
        for deg, sc, sh in RG.STARTS:
            G = RG.disturb(p, deg, sc, sh, rng)
            X = RG.apply(RG.inverse(G), Xt)
            X.setflags(write=False)
            starts.append((G, X))
        V.setflags(write=False)
        F.setflags(write=False)
        _calib.update(V=V, F=F, p=p, starts=starts, results={})
    return _calib


def calibration_result(i, **kw):
    """the restatement's loop from start i, computed once per parameter set"""
    c = calibration()
    key = (i, tuple(sorted(kw.items())))
    if key not in c["results"]:
        its = []
        r = RG.register(c["starts"][i][1], c["V"], c["F"], RG.D_MAX, dist=SR.pruned, iterates=its, **kw)
        c["results"][key] = (r, its)
    return c["results"][key]


def test_calibration_four_spheres():
    c = calibration()
    assert not (set(map(bytes, np.round(c["starts"][0][1], 9))) & set(map(bytes, np.round(c["V"], 9)))), "no source point is a target vertex"
    finals = []
    for i, (G, X) in enumerate(c["starts"]):
        r, _ = calibration_result(i)
        err = RG.transform_error(r["T"], G, c["p"])
        rp, rq, n = RG.rms(r)
        print(f"start {RG.STARTS[i]}: status {r['status']} after {r['iterations']}, n {n}, rot {err[0]:.3e} deg, scale {err[1]:.3e}, "
              f"trans {err[2]:.3e}, rms plane {rp:.3e} point {rq:.3e}")
        assert (r["status"], r["iterations"], n) == (MEASURED["status"][i], MEASURED["iters"][i], MEASURED["n"])
        assert err[0] <= CALIB["rot"] and err[1] <= CALIB["scale"] and err[2] <= CALIB["trans"]
        assert rp <= CALIB["rms_plane"] and rq <= CALIB["rms_point"]
        finals.append(RG.compose(r["T"], RG.inverse(G)))
    spread = [max(RG.transform_error(a, b, c["p"])[k] for a in finals for b in finals) for k in range(3)]
    print("spread of the finals:", spread)
    assert spread[0] <= CALIB["spread_rot"] and spread[1] <= CALIB["spread_scale"] and spread[2] <= CALIB["spread_trans"]


def test_calibration_takes_every_branch():
    c = calibration()
    _, _, _, _, _, reasons = RG.rows(RG.identity(), c["starts"][2][1], c["V"], c["F"], RG.D_MAX, dist=SR.pruned)
    assert reasons["clipped"] > 50 and reasons["used"] > 1000 and reasons["collinear"] == 0, reasons


# the second calibration: DESIGN.md 19's four-sphere scene fused at 61^3, the ground truth in a disturbed frame
EVAL = dict(d_max=0.01, tau=0.0025)
# measured (accuracy, completeness): in the same frame, unregistered against the disturbed truth, registered against it
MEASURED2 = dict(same=(1.483e-3, 1.0), off=(6.512e-3, 0.4506), reg=(1.208e-3, 1.0), iters=3)

_scene = {}


def scene_mesh():
    """(verts, faces) of the four-sphere scene fused at 61^3 in NumPy, and the ground truth in its own and in a disturbed frame"""
    if not _scene:
        import align_ref as AL
        import fusion_ref as FR
        sc = AL.scene_volume()
        v, f = FR.extract(sc["sum"], sc["count"], AL.VOL["origin"], AL.VOL["voxel"])
        G = RG.spheres_mesh(3)
        p = RG.pivot(*G)
        M = RG.disturb(p, 3.0, 1.03, 0.006, np.random.default_rng(23))
        _scene.update(verts=v, faces=f, gt=G, moved=(RG.apply(M, G[0]), G[1]), M=M)
    return _scene


def test_calibration_scene_registered_evaluation():
    s = scene_mesh()
    v, f = s["verts"], s["faces"]
    same = SR.evaluate(v, f, *s["gt"], EVAL["d_max"], EVAL["tau"])
    off = SR.evaluate(v, f, *s["moved"], EVAL["d_max"], EVAL["tau"])
    r = RG.register(SR.used_vertices(v, f), *s["moved"], EVAL["d_max"], dist=SR.pruned)
    reg = SR.evaluate(RG.apply(r["T"], v), f, *s["moved"], EVAL["d_max"], EVAL["tau"])
    err = RG.transform_error(r["T"], s["M"], RG.pivot(*s["gt"]))
    print("same frame:", same, "\nunregistered:", off, "\nregistered:", reg, "\nstatus", r["status"], r["iterations"], "error", err, RG.rms(r))
    assert (r["status"], r["iterations"]) == (RG.CONVERGED, MEASURED2["iters"])
    for name, e in (("same", same), ("off", off), ("reg", reg)):
        assert e["accuracy"] == pytest.approx(MEASURED2[name][0], rel=2e-3) and e["completeness"] == pytest.approx(MEASURED2[name][1], rel=2e-3), name
    # the ground truth is 1.03 times larger in the disturbed frame: lengths are held to the same-frame figures times that
    assert reg["accuracy"] <= 1.25 * 1.03 * same["accuracy"] and reg["completeness"] >= same["completeness"] / 1.25
    assert off["accuracy"] > 2.0 * reg["accuracy"] and off["completeness"] < 0.5 * reg["completeness"], "what registration buys"
