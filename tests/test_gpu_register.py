"""GPU suite: surface registration.  Every comparison is byte for byte against the NumPy restatement (tests/register_ref.py): the
37 ordered sums and n_used of an evaluation, the pivot, and for the loop every iterate's transform, the status, the iteration
count and the trace; apply's output.  Sample counts around the wave, the block and the tree's second level with every stride,
hand targets of one to three faces where the restatement alone shows each branch taken (tests/test_register_cpu.py), every way
of feeding target and source, one object across sizes, the loop's end states from the calibration's starts, the degenerate
targets, the refusals, and the pipeline."""
import importlib
import json
import os

import numpy as np
import pytest

import align_ref as AL
import consist_ref as CR
import helpers as H
import register_ref as RG
import sdist_ref as SR
import visib_ref as VR
from test_register_cpu import EVAL, HAND_D_MAX, calibration, calibration_result, hand_cases, scene_mesh

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
PAIR = (2, 3)  # e2e_keyframes: the pair with valid disparity
SMALL = dict(num_disparities=32, census=5)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rg(ctx):
    """one object for the whole module: its target and buffers grow and shrink with the cases"""
    o = ctx.register()
    yield o
    o.close()


def _system(rg, X, V, F, d_max, what, T=None, dist=SR.brute, **kw):
    """one evaluation on the device against register_ref.system; the target must be set; returns (sums, n_used)"""
    sums, n = rg.system(X, T, **kw)
    rs, rn = RG.system(RG.identity() if T is None else T, X, V, F, d_max, kw.get("stride", 1), dist)
    assert n == rn, f"{what}: n_used {n} vs {rn}"
    H.assert_bits_equal(sums, rs, f"{what}: sums")
    return sums, n


def _same_loop(out, ref, what):
    assert (out["status"], out["iterations"]) == (ref["status"], ref["iterations"]), \
        f"{what}: {out['status']}, {out['iterations']} vs {ref['status']}, {ref['iterations']}"
    assert RG.same_result(out, ref), f"{what}: the device loop differs from register_ref.register: {out['trace']} vs {ref['trace']}"


def _loop(rg, X, V, F, d_max, what, init=None, dist=SR.brute, **kw):
    out = rg.run(X, init=init, **kw)
    ref = RG.register(X, V, F, d_max, init=init, dist=dist, **kw)
    _same_loop(out, ref, what)
    return out, ref


# ---- one evaluation: sizes and strides -----------------------------------------------------------------------------------------
BALL = SR.icosphere(1, 0.1)  # 42 vertices, 80 faces
BALL_D_MAX = 0.02
BALL_T = RG.disturb((0.0, 0.0, 0.0), 3.0, 1.02, 0.004, np.random.default_rng(2))


def _ball_points(n, seed=1):
    """points around the ball: most within d_max of it, some beyond"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return d * (0.1 + rng.uniform(-0.03, 0.03, n))[:, None]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 65537])
def test_system_sizes_and_strides(rg, n):
    X = _ball_points(n)
    rg.set_target(*BALL, BALL_D_MAX)
    H.assert_bits_equal(rg.pivot(), RG.pivot(*BALL), "pivot")
    dist = SR.pruned if n > 1000 else SR.brute
    for stride in (1, 2, 3, n + 1):
        sums, used = _system(rg, X, *BALL, BALL_D_MAX, f"n {n} stride {stride}", T=BALL_T, stride=stride, dist=dist)
        ns = (n + stride - 1) // stride
        assert used <= ns and (n < 63 or stride > 3 or 0 < used < ns), "some samples are used and some are clipped"
    if n == 0:
        assert sums.tobytes() == np.zeros(37).tobytes() and used == 0


# ---- hand targets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_hand_cases(rg, case):
    name, V, F, X, reasons, _ = case
    X = np.asarray(X, np.float64)
    rg.set_target(V, F, HAND_D_MAX)
    H.assert_bits_equal(rg.pivot(), RG.pivot(V, F), "pivot")
    sums, n = _system(rg, X, V, F, HAND_D_MAX, name)
    assert n == reasons["used"]
    # the same samples at a disturbed transform, and through the strides
    T = RG.disturb(RG.pivot(V, F), 1.0, 1.01, 0.01, np.random.default_rng(4))
    _system(rg, X, V, F, HAND_D_MAX, name + " disturbed", T=T)
    _system(rg, X, V, F, HAND_D_MAX, name + " stride 2", T=T, stride=2)
    if name == "all clipped":
        assert sums.tobytes() == np.zeros(37).tobytes()
        out, _ = _loop(rg, X, V, F, HAND_D_MAX, name)
        assert (out["status"], out["iterations"], out["trace"]) == (capi.REGISTER_STATUS.index("TOO_FEW"), 1, [(0, 0.0, 0.0, 0.0, 0.0, 0.0)])
        assert RG.same_transform(out["T"], RG.identity())
    if name == "a block in the plane":
        assert np.signbit(sums[28:35]).any(), "sums of -0.0 alone stay -0.0"


# ---- feeds and reuse -------------------------------------------------------------------------------------------------------------
def test_feeds_give_the_same_bits(ctx, rg):
    import torch
    c = calibration()
    V, F, X = c["V"], c["F"], c["starts"][1][1]
    rg.set_target(V, F, RG.D_MAX)
    want = _system(rg, X, V, F, RG.D_MAX, "host target, host source", dist=SR.pruned)
    loop = rg.run(X, max_iters=2)
    tv, tf, tx = (torch.from_numpy(np.array(a)).to("cuda:0") for a in (V, F, X))
    torch.cuda.synchronize()
    o = ctx.register()
    o.set_target(tv.data_ptr(), tf.data_ptr(), RG.D_MAX, nv=len(V), m=len(F))
    H.assert_bits_equal(o.pivot(), rg.pivot(), "pivot")
    for what, got in (("device target, host source", o.system(X)), ("device target, device source", o.system(tx.data_ptr(), n=len(X))),
                      ("host target, device source", rg.system(tx.data_ptr(), n=len(X)))):
        assert got[1] == want[1], what
        H.assert_bits_equal(got[0], want[0], what)
    assert RG.same_result(o.run(tx.data_ptr(), n=len(X), max_iters=2), loop)
    H.assert_bits_equal(o.apply(loop["T"], tx.data_ptr(), n=len(X)), RG.apply(loop["T"], X), "apply from a device pointer")
    o.close()


def test_device_meshes_as_source(ctx, rg):
    V, F = RG.spheres_mesh(2)
    rg.set_target(V, F, RG.D_MAX)
    # the simplified calibration target: its vertices lie near the target's
    sp = ctx.simplify()
    sp.run(*RG.spheres_mesh(3), cell=0.004)
    n, pv, _, _ = sp.device_mesh()
    Xs = sp.read()["verts"]
    assert n == len(Xs) > 100
    got = rg.system(pv, n=n)
    ref = RG.system(RG.identity(), Xs, V, F, RG.D_MAX, dist=SR.pruned)
    assert got[1] == ref[1] > 100
    H.assert_bits_equal(got[0], ref[0], "the simplify object's device vertices")
    _same_loop(rg.run(pv, n=n, max_iters=2), RG.register(Xs, V, F, RG.D_MAX, dist=SR.pruned, max_iters=2), "simplify, loop")
    sp.close()
    hc = VR.hand_cases()["two-views"]
    vb = ctx.visib()
    for cam in hc["cams"]:
        vb.add_view(cam)
    kept = vb.run(hc["verts"], hc["faces"], hc["z_min"], hc["depth_tol"])
    n, pv, _, _ = vb.device_mesh()
    assert n == len(kept["verts"]) > 0
    scale = float(np.abs(kept["verts"]).max())
    rg.set_target(hc["verts"], hc["faces"], 0.25 * scale)
    got = rg.system(pv, n=n)
    ref = RG.system(RG.identity(), kept["verts"], hc["verts"], hc["faces"], 0.25 * scale)
    assert got[1] == ref[1]
    H.assert_bits_equal(got[0], ref[0], "the visib object's device vertices")
    vb.close()


def test_one_object_across_sizes(ctx):
    o = ctx.register()
    big, small = RG.spheres_mesh(2), SR.icosphere(0, 0.1)
    Xb, Xs = _ball_points(3000, 5) * 0.45 + np.array(RG.SPHERES[0][0]), _ball_points(40, 6)
    for what, (V, F), X, d in (("large", big, Xb, RG.D_MAX), ("small", small, Xs, 0.03), ("large again", big, Xb, RG.D_MAX)):
        o.set_target(V, F, d)
        H.assert_bits_equal(o.pivot(), RG.pivot(V, F), what)
        _system(o, X, V, F, d, what, dist=SR.pruned)
    # one target, several sources
    for seed in (7, 8):
        _system(o, _ball_points(500, seed) * 0.45 + np.array(RG.SPHERES[0][0]), *big, RG.D_MAX, f"source {seed}", dist=SR.pruned)
    o.close()


# ---- the loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 1, 2])
@pytest.mark.parametrize("with_scale", [1, 0])
def test_loop_from_the_calibration_starts(rg, start, with_scale):
    c = calibration()
    rg.set_target(c["V"], c["F"], RG.D_MAX)
    X = c["starts"][start][1]
    ref, its = calibration_result(start, with_scale=with_scale)
    out = rg.run(X, with_scale=with_scale)
    _same_loop(out, ref, f"start {start} scale {with_scale}")
    assert out["status"] == RG.CONVERGED
    # every iterate: the loop cut after k evaluations ends at the transform the restatement made evaluation k + 1 at
    for k in range(1, ref["iterations"]):
        cut = rg.run(X, with_scale=with_scale, max_iters=k)
        assert (cut["status"], cut["iterations"]) == (RG.MAX_ITERS, k) and RG.same_transform(cut["T"], its[k]), k
        assert RG.same_result(dict(cut, status=ref["status"], iterations=k, T=ref["T"]), dict(ref, iterations=k, trace=ref["trace"][:k]))


@pytest.mark.parametrize("kw,status", [(dict(damping=1e-4), RG.CONVERGED), (dict(max_iters=1), RG.MAX_ITERS), (dict(max_iters=2), RG.MAX_ITERS),
                                       (dict(min_points=10 ** 6), RG.TOO_FEW), (dict(eps_rot=1.0, eps_scale=1.0, eps_trans=100.0), RG.CONVERGED),
                                       (dict(eps_rot=0.0, eps_scale=0.0, eps_trans=0.0, max_iters=6), RG.MAX_ITERS), (dict(stride=3), RG.CONVERGED)],
                         ids=lambda v: "-".join(v) if isinstance(v, dict) else str(v))
def test_loop_parameters(rg, kw, status):
    c = calibration()
    rg.set_target(c["V"], c["F"], RG.D_MAX)
    ref, _ = calibration_result(1, **kw)
    out = rg.run(c["starts"][1][1], **kw)
    _same_loop(out, ref, str(kw))
    assert out["status"] == status
    if "min_points" in kw:
        assert RG.same_transform(out["T"], RG.identity()) and out["iterations"] == 1
    if kw.get("eps_rot") == 1.0:
        assert out["iterations"] == 1


def test_loop_from_an_init(rg):
    c = calibration()
    rg.set_target(c["V"], c["F"], RG.D_MAX)
    G, X = c["starts"][2]
    near = RG.compose(RG.disturb(c["p"], 0.5, 1.005, 0.001, np.random.default_rng(9)), G)
    out, ref = _loop(rg, X, c["V"], c["F"], RG.D_MAX, "init", init=near, dist=SR.pruned)
    assert out["status"] == RG.CONVERGED and out["iterations"] <= calibration_result(2)[0]["iterations"]


def test_degenerate_targets(rg):
    # the single sphere: a rotation about its centre changes nothing but the discretisation; recorded, bytes pinned
    V, F = SR.icosphere(3, 0.05)
    X = RG.apply(RG.disturb((0.0, 0.0, 0.0), 2.0, 1.02, 0.003, np.random.default_rng(3)), _ball_points(800, 3) * np.array([0.5]))
    rg.set_target(V, F, RG.D_MAX)
    out, _ = _loop(rg, X, V, F, RG.D_MAX, "single sphere", dist=SR.pruned, max_iters=8)
    print("single sphere:", capi.REGISTER_STATUS[out["status"]], out["iterations"], out["T"]["s"])
    # a flat target: scale about the pivot and translation along the normal coincide, rotation about the normal is free
    g = np.arange(6, dtype=np.float64) * 0.1
    Vf = np.array([[x, y, 0.0] for y in g for x in g])
    Ff = np.array([[6 * j + i, 6 * j + i + 1, 6 * j + i + 7] for j in range(5) for i in range(5)] +
                  [[6 * j + i, 6 * j + i + 7, 6 * j + i + 6] for j in range(5) for i in range(5)], np.int32)
    rng = np.random.default_rng(10)
    Xf = np.column_stack([rng.uniform(0.05, 0.45, 300), rng.uniform(0.05, 0.45, 300), rng.normal(0.01, 0.002, 300)])
    rg.set_target(Vf, Ff, 0.05)
    H.assert_bits_equal(rg.pivot(), RG.pivot(Vf, Ff), "flat pivot")
    for ws in (1, 0):
        out, _ = _loop(rg, Xf, Vf, Ff, 0.05, f"flat target, scale {ws}", with_scale=ws, max_iters=4)
        print("flat target:", ws, capi.REGISTER_STATUS[out["status"]], out["iterations"])
    out, _ = _loop(rg, Xf, Vf, Ff, 0.05, "flat target, damped", damping=1e-3, max_iters=4)
    # a target without faces
    rg.set_target(Vf, Ff[:0], 0.05)
    assert rg.pivot().tobytes() == np.zeros(3).tobytes()
    sums, n = rg.system(Xf)
    assert n == 0 and sums.tobytes() == np.zeros(37).tobytes()
    out, _ = _loop(rg, Xf, Vf, Ff[:0], 0.05, "m = 0")
    assert (out["status"], out["iterations"]) == (RG.TOO_FEW, 1)
    rg.set_target(np.zeros((0, 3)), Ff[:0], 0.05)
    assert rg.run(Xf[:0])["status"] == RG.TOO_FEW


def test_apply(rg):
    rg.set_target(*BALL, BALL_D_MAX)
    for n in (0, 1, 257, 5000):
        X = _ball_points(n, 11) * 1e3
        H.assert_bits_equal(rg.apply(BALL_T, X), RG.apply(BALL_T, X), f"apply {n}")
    X = np.array([[0.0, -0.0, 1e300], [-1e-310, 5e-324, -0.0]])
    T = dict(s=2.0 ** -3, R=-np.eye(3), t=np.array([-0.0, 0.0, 1.0]))
    H.assert_bits_equal(rg.apply(T, X), RG.apply(T, X), "zeros, denormals, large")


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    o = ctx.register()
    X = _ball_points(100)

    def refused(fn, what):
        with pytest.raises(capi.SfmxError) as e:
            fn()
        assert e.value.status == capi.SFMX_ERR_INVALID, what

    def good(what):
        got = o.system(X, BALL_T)
        ref = RG.system(BALL_T, X, *BALL, BALL_D_MAX)
        assert got[1] == ref[1], what
        H.assert_bits_equal(got[0], ref[0], "after: " + what)

    for fn, what in ((lambda: o.system(X), "system"), (lambda: o.run(X), "run"), (lambda: o.apply(RG.identity(), X), "apply"), (o.pivot, "pivot")):
        refused(fn, what + " before set_target")
    o.set_target(*BALL, BALL_D_MAX)
    good("set_target")
    nan, inf = float("nan"), float("inf")
    for bad in (nan, inf, -inf):
        Xb = X.copy()
        Xb[37, 1] = bad
        refused(lambda: o.system(Xb), f"source {bad}")
        refused(lambda: o.run(Xb), f"source {bad}, run")
        refused(lambda: o.apply(RG.identity(), Xb), f"source {bad}, apply")
        good(f"source {bad}")
        H.assert_bits_equal(o.system(Xb, BALL_T, stride=2)[0], RG.system(BALL_T, Xb, *BALL, BALL_D_MAX, 2)[0], "an unsampled point is not read")
    for T in (dict(s=0.0, R=np.eye(3), t=np.zeros(3)), dict(s=-1.0, R=np.eye(3), t=np.zeros(3)), dict(s=nan, R=np.eye(3), t=np.zeros(3)),
              dict(s=1.0, R=np.full((3, 3), inf), t=np.zeros(3)), dict(s=1.0, R=np.eye(3), t=np.array([0.0, nan, 0.0]))):
        refused(lambda: o.system(X, T), f"T {T}")
        refused(lambda: o.run(X, init=T), f"init {T}")
        refused(lambda: o.apply(T, X), f"apply {T}")
        good("a bad transform")
    refused(lambda: o.system(X, dict(s=1e300, R=np.eye(3) * 1e300, t=np.zeros(3))), "a transform that overflows")
    good("overflow")
    import torch
    tx = torch.from_numpy(X).to("cuda:0")
    torch.cuda.synchronize()
    for n in (-1, 1 << 30):
        refused(lambda: o.system(tx.data_ptr(), n=n), f"n = {n}")
        refused(lambda: o.run(tx.data_ptr(), n=n), f"n = {n}")
        refused(lambda: o.apply(RG.identity(), tx.data_ptr(), n=n), f"n = {n}")
    good("n")
    for kw in (dict(max_iters=0), dict(max_iters=65), dict(stride=0), dict(min_points=6), dict(damping=-1.0), dict(eps_rot=nan), dict(eps_scale=-1.0),
               dict(eps_trans=inf)):
        refused(lambda: o.system(X, **kw), str(kw))
        refused(lambda: o.run(X, **kw), str(kw))
        good(str(kw))
    with pytest.raises(TypeError):
        o.run(X, d_max=1.0)
    with pytest.raises(TypeError):
        o.run(X, iterations=2)
    # another d_max than the target's, straight at the C entry
    p = capi.register_params(2 * BALL_D_MAX)
    sums, nu = np.zeros(37), capi.c_int32(0)
    rc = ctx.lib.sfmx_register_system(ctx.h_, o.h_, X.ctypes.data_as(capi.c_void_p), capi.c_int(len(X)), capi.c_int(0), None, capi.byref(p),
                                      sums.ctypes.data_as(capi.POINTER(capi.c_double)), capi.byref(nu))
    assert rc == capi.SFMX_ERR_INVALID
    good("d_max")
    # every refusal of sfmx_sdist_set_target; a failed set_target leaves no target
    V, F = BALL
    bad_targets = [((V, F + len(V)), dict(d_max=BALL_D_MAX), "a face index outside the vertices"),
                   ((np.where(np.arange(len(V))[:, None] == 3, nan, V), F), dict(d_max=BALL_D_MAX), "a non-finite used vertex"),
                   ((V * 2.0 ** 41, F), dict(d_max=1.0 / 1024), "a coordinate beyond 2^40 d_max"),
                   ((V, F), dict(d_max=BALL_D_MAX, cell=1e-9), "a cell that does not fit"),
                   ((V, F), dict(d_max=0.0), "d_max 0"), ((V, F), dict(d_max=BALL_D_MAX, cell=-1.0), "cell < 0")]
    for (bv, bf), kw, what in bad_targets:
        o.set_target(*BALL, BALL_D_MAX)
        refused(lambda: o.set_target(bv, bf, **kw), what)
        refused(lambda: o.system(X), what + ": no target is left")
        refused(o.pivot, what + ": no pivot is left")
    o.set_target(*BALL, BALL_D_MAX)
    good("a failed set_target")
    with pytest.raises(TypeError):
        o.set_target(V, 5, BALL_D_MAX)
    o.close()
    o.close()


def test_timing(ctx, rg):
    c = calibration()
    ctx.set_timing(True)
    rg.set_target(c["V"], c["F"], RG.D_MAX)
    assert rg.last_query_us() > 0.0 and rg.last_us() > 0.0
    rg.run(c["starts"][1][1])
    assert rg.last_us() > 0.0 and rg.last_query_us() > 0.0
    ctx.set_timing(False)
    rg.run(c["starts"][1][1], max_iters=1)
    assert rg.last_us() == 0.0 and rg.last_query_us() == 0.0


# ---- pipeline ----------------------------------------------------------------------------------------------------------------------
def _same_registration(got, ref, what):
    """a pipeline registration dict against the restatement's loop result"""
    _same_loop(got, ref, what)
    rp, rq, n = RG.rms(ref)
    assert got["n"] == n and (got["rms_plane"], got["rms_point"]) == (rp, rq) or (n == 0 and np.isnan(got["rms_plane"]))


def test_surface_register_and_eval_on_the_four_spheres(ctx):
    s = scene_mesh()
    fu = ctx.fusion(**AL.VOL)
    for cam, d16 in AL.scene_views():
        fu.add_view(cam, d16)
    v, f = fu.extract()
    fu.close()
    assert v.tobytes() == s["verts"].tobytes() and f.tobytes() == s["faces"].tobytes()
    gv, gf = s["moved"]
    ref = RG.register(SR.used_vertices(v, f), gv, gf, EVAL["d_max"], dist=SR.pruned)
    got = pipe.surface_register(ctx, v, f, gv, gf, d_max=EVAL["d_max"])
    assert set(got) == {"T", "status", "iterations", "n", "rms_plane", "rms_point", "trace", "verts"}
    _same_registration(got, ref, "surface_register")
    H.assert_bits_equal(got["verts"], RG.apply(ref["T"], v), "the moved vertices")
    off = pipe.surface_eval(ctx, v, f, gv, gf, **EVAL)
    assert off == SR.evaluate(v, f, gv, gf, EVAL["d_max"], EVAL["tau"]) and off == pipe.surface_eval(ctx, v, f, gv, gf, **EVAL, register=None)
    e = pipe.surface_eval(ctx, v, f, gv, gf, **EVAL, register=True)
    reg = e.pop("registration")
    assert "verts" not in reg
    _same_registration(reg, ref, "surface_eval(register=True)")
    assert e == SR.evaluate(RG.apply(ref["T"], v), f, gv, gf, EVAL["d_max"], EVAL["tau"])
    print("unregistered:", off, "\nregistered:", e)
    assert e["accuracy"] < 0.5 * off["accuracy"] and e["completeness"] == 1.0 > 2.0 * off["completeness"]
    # a dict: parameters, another trimming distance, a start
    kw = dict(d_max=0.02, max_iters=2, stride=5, init=RG.disturb((0.0, 0.0, 0.0), 0.5, 1.0, 0.0, np.random.default_rng(1)))
    e2 = pipe.surface_eval(ctx, v, f, gv, gf, **EVAL, register=kw)
    ref2 = RG.register(SR.used_vertices(v, f), gv, gf, 0.02, dist=SR.pruned, **{k: x for k, x in kw.items() if k != "d_max"})
    _same_registration(e2.pop("registration"), ref2, "surface_eval(register=dict)")
    assert e2 == SR.evaluate(RG.apply(ref2["T"], v), f, gv, gf, EVAL["d_max"], EVAL["tau"])
    with pytest.raises(TypeError):
        pipe.surface_eval(ctx, v, f, gv, gf, **EVAL, register=dict(iterations=2))
    with pytest.raises(capi.SfmxError):
        pipe.surface_eval(ctx, v, f, gv, gf, **EVAL, register=dict(max_iters=0))


def test_fuse_evaluate_register(ctx, tmp_path):
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    vol = CR.RING6_VOL
    args = (ctx, images, K, poses, pairs, vol["origin"], vol["voxel"], vol["dims"])
    G = synth.shell_mesh(4)
    M = RG.disturb(RG.pivot(*G), 2.0, 1.03, 0.004, np.random.default_rng(31))
    gv = RG.apply(M, G[0])
    ev = dict(gt_verts=gv, gt_faces=G[1], d_max=4 * vol["voxel"], tau=vol["voxel"])
    rkw = dict(max_iters=3, stride=4)
    p1, p2 = (str(tmp_path / n) for n in ("ev.ply", "reg.ply"))
    m1 = pipe.fuse(*args, num_disparities=64, ply_path=p1, evaluate=ev)
    m = pipe.fuse(*args, num_disparities=64, ply_path=p2, evaluate=dict(ev, register=rkw))
    assert set(m) == set(m1) and set(m["evaluation"]) == set(m1["evaluation"]) | {"registration"}
    for k in ("verts", "faces"):
        assert m1[k].tobytes() == m[k].tobytes(), k
    assert open(p1, "rb").read() == open(p2, "rb").read(), "the registration changes no output"
    ref = RG.register(SR.used_vertices(m1["verts"], m1["faces"]), gv, G[1], ev["d_max"], dist=SR.pruned, **rkw)
    e = dict(m["evaluation"])
    _same_registration(e.pop("registration"), ref, "fuse")
    assert e == SR.evaluate(RG.apply(ref["T"], m1["verts"]), m1["faces"], gv, G[1], ev["d_max"], ev["tau"])
    assert m1["evaluation"] == SR.evaluate(m1["verts"], m1["faces"], gv, G[1], ev["d_max"], ev["tau"])
    print("ring-6 unregistered:", m1["evaluation"], "\nregistered:", e, capi.REGISTER_STATUS[ref["status"]], RG.transform_error(ref["T"], M, RG.pivot(*G)))
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, evaluate=dict(ev, register=dict(iterations=3)))


def test_pipeline_run_evaluate_register(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in PAIR)
    sm = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][PAIR[0]], r0["kf_poses"][PAIR[1]], **SMALL)
    lo, hi = sm["verts"].min(0), sm["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    fz = dict(pairs=[PAIR], origin=tuple(lo), voxel=voxel, dims=dims, **SMALL)
    ev = dict(gt_verts=sm["verts"], gt_faces=sm["faces"], d_max=4 * voxel, tau=voxel)  # the pair's own stereo mesh as the truth
    rkw = dict(max_iters=2, stride=3)
    r = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None, fusion=dict(fz, evaluate=dict(ev, register=rkw)))
    assert r["log"] == r0["log"]
    m = r["fused_mesh"]
    assert len(m["faces"]) > 0
    ref = RG.register(SR.used_vertices(m["verts"], m["faces"]), sm["verts"], sm["faces"], ev["d_max"], dist=SR.pruned, **rkw)
    e = dict(m["evaluation"])
    _same_registration(e.pop("registration"), ref, "run")
    assert e == SR.evaluate(RG.apply(ref["T"], m["verts"]), m["faces"], sm["verts"], sm["faces"], ev["d_max"], ev["tau"])
