"""CPU suite: photometric registration of a camera to the textured mesh -- the NumPy restatement (tests/palign_ref.py): its
Jacobian against finite differences of the residual under the update, its ordered sum against a plain Python loop over the same
tree, the candidate rule against a brute-force window test, the pyramid's reduction and camera rule, the parameter check across
capi, the library and the restatement, every Python-level refusal, and the calibration of DESIGN.md 29."""
import importlib
import inspect
import math

import numpy as np
import pytest

import align_ref as AL
import helpers as H
import palign_ref as PA
import raycast_ref as RR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")


def _bound(x):
    """DESIGN.md 15's rule: 1.25 x the measured value, rounded up to two significant digits"""
    q = 10.0 ** (math.floor(math.log10(1.25 * x)) - 1)
    return math.ceil(1.25 * x / q - 1e-9) * q


# ---- the Jacobian ----------------------------------------------------------------------------------------------------------------
def _picture(u, v):
    """a smooth synthetic picture in place of I, with its gradient"""
    val = 100.0 + 40.0 * np.sin(0.11 * u + 0.3) * np.cos(0.07 * v - 0.2) + 0.5 * u - 0.25 * v
    gu = 40.0 * 0.11 * np.cos(0.11 * u + 0.3) * np.cos(0.07 * v - 0.2) + 0.5
    gv = -40.0 * 0.07 * np.sin(0.11 * u + 0.3) * np.sin(0.07 * v - 0.2) - 0.25
    return val, gu, gv


def _project(cam, X):
    R = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
    q = R @ (np.asarray(X, np.float64) - np.asarray(cam["c_left"], np.float64))
    return cam["f"] * q[0] / q[2] + cam["cx"], cam["f"] * q[1] / q[2] + cam["cy"]


def test_jacobian_against_finite_differences():
    """r(delta) = I(project(camera moved by delta, X)) - g for the fixed surface point X of a sample: J is dr / d delta at 0"""
    rng = np.random.default_rng(3)
    import fusion_ref as FR
    cam = dict(FR.look_at_cam((0.3, -0.2, -0.5), (0.02, 0.01, 0.0), 300.0, 160, 120, 0.05), w=160, h=120)
    pivot = [0.03, -0.02, 0.05]
    worst = 0.0
    for _ in range(20):
        x, y, z = float(rng.integers(1, 159)), float(rng.integers(1, 119)), float(rng.uniform(0.3, 0.9))
        _, gu, gv = _picture(x, y)
        J, X = PA.jacobian(np.array([gu]), np.array([gv]), np.array([x]), np.array([y]), np.array([z]), cam, pivot)
        J, X = [float(v[0]) for v in J], [float(v[0]) for v in X]
        u0, v0 = _project(cam, X)
        assert abs(u0 - x) < 1e-9 and abs(v0 - y) < 1e-9, "the surface point of a sample projects back onto its pixel centre"
        for m in range(6):
            h = 1e-6
            d = [0.0] * 6
            d[m] = h
            up = _picture(*_project(AL.update(cam, pivot, d), X))[0]
            d[m] = -h
            dn = _picture(*_project(AL.update(cam, pivot, d), X))[0]
            fd = (up - dn) / (2.0 * h)
            worst = max(worst, abs(fd - J[m]) / max(1.0, abs(J[m])))
    assert worst < 1e-5, worst  # central differences at h = 1e-6 on values of order 100: truncation h^2 and rounding 1e-14 / h


# ---- the ordered sum -------------------------------------------------------------------------------------------------------------
def _plain_sum(T):
    """the definition's tree in plain Python over one term [nsy][nsx]"""
    nsy, nsx = T.shape
    nby, nbx = (nsy + 15) // 16, (nsx + 15) // 16
    rows = []
    for by in range(nby):
        for bx in range(nbx):
            t = [0.0] * 256
            for wave in range(4):
                for lane in range(64):
                    i, j = bx * 16 + (wave & 1) * 8 + (lane & 7), by * 16 + (wave >> 1) * 8 + (lane >> 3)
                    if i < nsx and j < nsy:
                        t[4 * lane + wave] = float(T[j, i])
            off = 128
            while off >= 1:
                t = [t[k] + t[k + off] for k in range(off)]
                off //= 2
            rows.append(t[0])
    while len(rows) > 1:
        nxt = []
        for g in range(0, len(rows), 256):
            t = rows[g:g + 256] + [0.0] * (256 - len(rows[g:g + 256]))
            off = 128
            while off >= 1:
                t = [t[k] + t[k + off] for k in range(off)]
                off //= 2
            nxt.append(t[0])
        rows = nxt
    return rows[0]


@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (16, 16), (17, 33), (272, 272)])
def test_ordered_sum_is_the_view_alignments_tree(shape):
    assert PA.ordered_sum is AL.ordered_sum
    rng = np.random.default_rng(shape[0])
    k = 1 if shape[0] > 100 else 3
    T = rng.normal(size=(k,) + shape) * 10.0 ** rng.integers(-8, 8, size=(k,) + shape)
    got = PA.ordered_sum(T)
    for t in range(k):
        assert got[t].tobytes() == np.float64(_plain_sum(T[t])).tobytes(), (shape, t)


# ---- the candidate rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [1, 2, 8])
def test_candidates_against_a_window_test(margin):
    rng = np.random.default_rng(margin)
    for h, w in ((40, 37), (2 * margin + 1, 2 * margin + 1), (2 * margin, 50), (1, 1)):
        ok = rng.random((h, w)) < 0.995  # a few holes
        if h == 2 * margin + 1:
            ok[:] = True
        got = PA.candidates(ok, margin)
        want = np.zeros((h, w), bool)
        for y in range(h):
            for x in range(w):
                good = True
                for yy in range(y - margin, y + margin + 1):
                    for xx in range(x - margin, x + margin + 1):
                        good &= 0 <= yy < h and 0 <= xx < w and bool(ok[yy, xx])
                want[y, x] = good
        assert (got == want).all(), (margin, h, w)
        if h == 2 * margin + 1:
            assert got.sum() == 1 and got[margin, margin], "exactly the centre"
        if h == 2 * margin:
            assert not got.any(), "no pixel is margin away from both borders"


# ---- the pyramid -------------------------------------------------------------------------------------------------------------------
def test_pyramid_reduction_and_camera_rule():
    rng = np.random.default_rng(1)
    I = rng.integers(0, 256, (9, 7)).astype(np.uint8)  # odd sizes: the trailing row and column are dropped
    got = PA.reduce_image(I)
    assert got.shape == (4, 3) and got.dtype == np.uint8
    for j in range(4):
        for i in range(3):
            assert int(got[j, i]) == (int(I[2 * j, 2 * i]) + int(I[2 * j, 2 * i + 1]) + int(I[2 * j + 1, 2 * i]) + int(I[2 * j + 1, 2 * i + 1]) + 2) >> 2
    assert pipe.reduce_image(I).tobytes() == got.tobytes()
    # a linear ramp stays the ramp, sampled at the reduced pixels' centres 2 i + 0.5
    y, x = np.mgrid[0:20, 0:30]
    ramp = (10 + 2 * x + 2 * y).astype(np.uint8)
    red = PA.reduce_image(ramp)
    yy, xx = np.mgrid[0:10, 0:15]
    assert (red == 10 + 2 * (2 * xx + 0.5) + 2 * (2 * yy + 0.5)).all()
    # the camera rule: a point seen at (u, v) is seen at ((u - 0.5) / 2, (v - 0.5) / 2) by the reduced camera
    cam = dict(RR.axis_camera((0.1, 0.2, -1.0), 300.0, 31, 21, 14.25, 9.5), w=31, h=21)
    rc = PA.reduce_cam(cam)
    assert (rc["f"], rc["cx"], rc["cy"], rc["w"], rc["h"]) == (150.0, 6.875, 4.5, 15, 10)
    assert np.asarray(rc["R_rw"]).tobytes() == np.asarray(cam["R_rw"]).tobytes()
    X = np.array([0.13, 0.17, 0.4])
    (u, v), (ur, vr) = _project(cam, X), _project(rc, X)
    assert abs(ur - (u - 0.5) / 2.0) < 1e-12 and abs(vr - (v - 0.5) / 2.0) < 1e-12
    pc = pipe.reduce_camera(cam)
    assert {k: pc[k] for k in ("f", "cx", "cy", "w", "h")} == {k: rc[k] for k in ("f", "cx", "cy", "w", "h")}


# ---- parameters and refusals -------------------------------------------------------------------------------------------------------
def test_check_params_field_by_field():
    d = capi.palign_default_params()
    assert d == dict(z_min=0.0, pivot=(0.0, 0.0, 0.0), **capi.PALIGN_DEFAULTS)
    assert capi.PALIGN_DEFAULTS == PA.DEFAULTS
    assert not capi.palign_check_params(**d), "z_min has no default"
    assert capi.palign_check_params(0.05) and PA.check_params(0.05)
    for kw in PA.BAD_PARAMS:
        full = dict(dict(z_min=0.05), **kw)
        assert not capi.palign_check_params(**full) and not PA.check_params(**full), kw
    for kw in PA.GOOD_PARAMS:
        full = dict(dict(z_min=0.05), **kw)
        assert capi.palign_check_params(**full) and PA.check_params(**full), kw
    lib = capi.load_library()
    assert lib.sfmx_palign_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_palign_default_params(None)
    assert lib.sfmx_palign_last_us(None) == 0.0 and lib.sfmx_palign_last_zbuffer_us(None) == 0.0
    assert lib.sfmx_palign_sizes(None, None, None) == capi.SFMX_ERR_INVALID


def test_python_layer_refusals_and_keys():
    with pytest.raises(TypeError):
        capi.palign_params(0.05, iterations=3)
    tri_v, tri_f = np.array([[0.0, 0, 1], [0, 1, 1], [1, 0, 1]]), np.array([[0, 1, 2]], np.int32)
    cam, img = dict(R_rw=np.eye(3), c_left=np.zeros(3), f=100.0, cx=4.0, cy=4.0), np.zeros((8, 8), np.uint8)
    with pytest.raises(TypeError):
        pipe.view_register(None, None, tri_v, tri_f, cam, img)  # no z_min
    with pytest.raises(TypeError):
        pipe.view_register(None, None, tri_v, tri_f, cam, img, z_min=0.1, iterations=3)
    with pytest.raises(ValueError):
        pipe.view_register(None, None, tri_v, tri_f, cam, img, z_min=0.1, levels=0)
    with pytest.raises(ValueError):
        pipe.view_register(None, None, tri_v, np.array([[0, 1, 3]], np.int32), cam, img, z_min=0.1)
    with pytest.raises(ValueError):
        pipe.view_register(None, None, tri_v, tri_f[:0], cam, img, z_min=0.1)  # no box to take the pivot from
    with pytest.raises(TypeError):
        pipe.view_register(None, None, tri_v, tri_f, cam, np.zeros((2, 8, 8), np.uint8), z_min=0.1)
    sig = inspect.signature(pipe.view_register).parameters
    assert sig["levels"].default == 1 and sig["lv"].default is None and sig["init"].default is None and sig["pivot"].default is None
    assert hasattr(capi.Context, "palign")
    assert all(hasattr(capi.PAlign, k) for k in ("set_model", "set_image", "system", "view", "read", "last_us", "last_zbuffer_us", "close"))
    blob = open(pipe.HOST_LIB_PATH, "rb").read()
    assert b"sfmx_photo_run" in blob and b"sfmx_palign" not in blob, "the host library does not reference the new entries"
    # pipeline.fuse: refused before any device call (the context is None)
    assert set(pipe.PALIGN_KEYS) == {"cameras", "images", "levels", "z_min", "pivot"} | set(capi.PALIGN_DEFAULTS)
    assert inspect.signature(pipe.fuse).parameters["palign"].default is False
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    tex, req = dict(z_min=0.05), dict(cameras=[cam], images=[img])
    for bad in (True, dict(req, iterations=3), dict(cameras=[cam]), dict(images=[img]), dict(cameras=[cam, cam], images=[img])):
        with pytest.raises(TypeError):
            pipe.fuse(*args, texture=tex, palign=bad)
    for bad in (dict(req, margin=0), dict(req, levels=0), dict(req, z_min=-1.0), dict(req, pivot=(0.0, float("nan"), 0.0))):
        with pytest.raises(ValueError):
            pipe.fuse(*args, texture=tex, palign=bad)
    with pytest.raises(TypeError):
        pipe.fuse(*args, palign=req)  # palign without texture


def test_restatement_refusals():
    c = PA.calibration()
    with pytest.raises(ValueError):
        PA.model(c["verts"], c["faces"], None)
    with pytest.raises(ValueError):
        PA.model(c["verts"], c["faces"][:-1], c["tex"])
    with pytest.raises(ValueError):
        PA.model(c["verts"], c["faces"], c["tex"], atlas=np.zeros((3, 3), np.uint8))
    bad = c["faces"].copy()
    bad[7, 1] = len(c["verts"])
    with pytest.raises(ValueError):
        PA.model(c["verts"], bad, c["tex"])
    with pytest.raises(ValueError):
        PA.align(c["M"], c["cam"], c["image"], c["z_min"], c["pivot"], margin=0)


# ---- calibration ----------------------------------------------------------------------------------------------------
# measured with this file's own code on texture_ref.fidelity_scene(), held-out view 5; bounds by _bound.  The device is held to
# bit equality, not to these.  Step plateau of the restatement with eps = 0: |omega| <= 2.9e-6, |v| <= 5.1e-7 at full resolution;
# 1.9e-5 .. 4.5e-5 and 1.6e-6 .. 3.6e-6 on the half-resolution level.
MEASURED = dict(status=((PA.CONVERGED,), (PA.CONVERGED,), (PA.CONVERGED,), (PA.CONVERGED, PA.CONVERGED)), iters=((3,), (6,), (6,), (7, 4)),
                n=(9895, 9895, 9895, 9896), rot=3.5191e-2, centre=4.4186e-4, rms=3.615255e-1, spread_rot=6.1121e-4, spread_centre=4.0903e-6,
                cond=4.336e3)
CALIB = {k: _bound(MEASURED[k]) for k in ("rot", "centre", "rms", "spread_rot", "spread_centre", "cond")}


def test_calibration_held_out_view():
    c = PA.calibration()
    finals = []
    for i, (deg, metres, levels) in enumerate(PA.STARTS):
        r = PA.calibration_result(i)
        rot, centre = AL.pose_error(r["view"], c["cam"], 1.0)
        sums, _ = PA.system(c["M"], r["view"], c["image"], c["z_min"], c["pivot"], stride=2, margin=8)
        A = np.zeros((6, 6))
        for t, (a, b) in enumerate(AL.PAIRS):
            A[a, b] = A[b, a] = sums[t]
        cond = float(np.linalg.cond(A))
        print(f"start {deg} deg / {metres} m, levels {levels}: status {[l['status'] for l in r['levels']]} after "
              f"{[l['iterations'] for l in r['levels']]}, n {r['n']}, rot {rot:.4e} deg, centre {centre:.4e} m, rms {r['rms']:.6e}, cond {cond:.3e}")
        assert tuple(l["status"] for l in r["levels"]) == MEASURED["status"][i]
        assert tuple(l["iterations"] for l in r["levels"]) == MEASURED["iters"][i] and r["n"] == MEASURED["n"][i]
        assert r["status"] == PA.CONVERGED and r["iterations"] == sum(MEASURED["iters"][i])
        assert rot <= CALIB["rot"] and centre <= CALIB["centre"] and r["rms"] <= CALIB["rms"] and cond <= CALIB["cond"]
        finals.append(r["view"])
    sr = max(AL.pose_error(a, b, 1.0)[0] for a in finals for b in finals)
    sc = max(AL.pose_error(a, b, 1.0)[1] for a in finals for b in finals)
    print(f"spread of the finals: {sr:.4e} deg, {sc:.4e} m")
    assert sr <= CALIB["spread_rot"] and sc <= CALIB["spread_centre"]


def test_calibration_takes_every_state():
    c = PA.calibration()
    state, J, r = PA.rows(c["M"], c["starts"][2], c["image"], c["z_min"], c["pivot"], stride=2, margin=8, r_max=8.0)
    assert (state == 0).sum() > 1000 and (state == 1).sum() > 10 and (state == 2).sum() > 5000
    assert not r[state == 0].any() and (np.abs(r[state == 1]) > 8.0).all() and (np.abs(r[state == 2]) <= 8.0).all()
    assert all(not Jm[state != 2].any() for Jm in J)
