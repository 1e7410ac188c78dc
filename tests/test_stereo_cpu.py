"""CPU suite: keyframe-pair stereo -- host rectification and grid mesh (libsfmx_host.so) against the NumPy restatement,
parameter validation of the device stage, and the NumPy SGM itself on a hand-computed case."""
import importlib

import numpy as np
import pytest

import helpers as H
import stereo_ref as SR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipeline = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")


def _ring_pair(deg_a, deg_b, w=640, h=480):
    K = synth.K_TEMPLE.copy()
    K[0, :] *= w / 640.0
    K[1, :] *= h / 480.0
    out = []
    for d in (deg_a, deg_b):
        R, t = synth.ring_pose(d)
        out.append((R.T, -R.T @ t))
    return K, out[0], out[1]


@pytest.mark.parametrize("deg", [(0.0, 3.0), (3.0, 0.0), (10.0, 14.5), (-20.0, -17.0)])
def test_rectify_epipolar_geometry(deg):
    K, (Ra, ca), (Rb, cb) = _ring_pair(*deg)
    r = pipeline.stereo_rectify(K, (Ra, ca), (Rb, cb), 640, 480)
    R = r["R_rw"]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.det(R) - 1.0) < 1e-12
    rng = np.random.default_rng(3)
    X = rng.normal(size=(200, 3)) * 0.05  # points around the ring's centre, in front of both cameras
    Pl = (X - r["c_left"]) @ R.T
    Pr = (X - r["c_right"]) @ R.T
    assert (Pl[:, 2] > 0).all()
    f, cx, cy = r["f"], r["cx"], r["cy"]
    xl, yl = f * Pl[:, 0] / Pl[:, 2] + cx, f * Pl[:, 1] / Pl[:, 2] + cy
    xr, yr = f * Pr[:, 0] / Pr[:, 2] + cx, f * Pr[:, 1] / Pr[:, 2] + cy
    assert np.abs(yl - yr).max() < 1e-9
    assert np.abs((xl - xr) - f * r["B"] / Pl[:, 2]).max() < 1e-9
    # H_l / H_r take a rectified pixel to the pixel of the same point in the source view
    (Rl, cl), (Rr, cr) = ((Rb, cb), (Ra, ca)) if r["swapped"] else ((Ra, ca), (Rb, cb))
    for Hm, xs, ys, Rv, cv in ((r["H_l"], xl, yl, Rl, cl), (r["H_r"], xr, yr, Rr, cr)):
        src = np.stack([xs, ys, np.ones_like(xs)], 1) @ Hm.T
        src = src[:, :2] / src[:, 2:]
        pc = (X - cv) @ Rv  # world -> camera: R^T (X - c)
        proj = pc @ K.T
        assert np.abs(src - proj[:, :2] / proj[:, 2:]).max() < 1e-7
    ref = SR.rectify(K, Ra, ca, Rb, cb)
    assert ref["swapped"] == r["swapped"]
    for k in ("R_rw", "c_left", "c_right", "H_l", "H_r"):
        np.testing.assert_allclose(r[k], ref[k], rtol=1e-12, atol=1e-12)
    assert r["f"] == ref["f"] and r["B"] == ref["B"]


def test_rectify_swap_rule_both_orders():
    K, A, B = _ring_pair(0.0, 3.0)
    ab = pipeline.stereo_rectify(K, A, B, 640, 480)
    ba = pipeline.stereo_rectify(K, B, A, 640, 480)
    assert ab["swapped"] != ba["swapped"]
    for k in ("R_rw", "c_left", "c_right"):
        np.testing.assert_allclose(ab[k], ba[k], atol=1e-15)
    # the left camera lies on the -x side of the right one
    left_x = ab["R_rw"] @ (ab["c_right"] - ab["c_left"])
    assert left_x[0] > 0 and abs(left_x[1]) < 1e-15 and abs(left_x[2]) < 1e-15


def test_rectify_zero_baseline_is_an_error():
    K, A, _ = _ring_pair(0.0, 3.0)
    with pytest.raises(capi.SfmxError):
        pipeline.stereo_rectify(K, A, A, 640, 480)


def _mesh_case(d16, rect, **mp):
    v, f, warn = pipeline.stereo_grid_mesh(d16, rect, **mp)
    rv, rf, rwarn = SR.grid_mesh(d16, rect, **mp)
    assert warn == rwarn
    assert v.shape == rv.shape and f.shape == rf.shape
    H.assert_bits_equal(v, rv, "stereo grid mesh vertices")
    assert (f == rf).all()
    return v, f, warn


def test_grid_mesh_hand_made():
    K, A, B = _ring_pair(0.0, 3.0)
    rect = SR.rectify(K, *A, *B)
    d16 = np.full((9, 13), -16, np.int16)
    d16[0:5, 0:9] = 16 * 40
    d16[4, 4] = 16 * 40 + 7
    d16[0, 8] = 16 * 45  # a jump of 5 px: both faces of that cell go
    d16[8, 12] = 16 * 41
    v, f, warn = _mesh_case(d16, rect, step=4, disp_min=1.0, disp_jump=3.0, z_max_percentile=100.0)
    assert warn is None
    # grid (rows 0, 4, 8) x (cols 0, 4, 8, 12): vertices where valid, row-major
    assert len(v) == 7
    assert f.tolist() == [[0, 1, 4], [0, 4, 3]]


def test_grid_mesh_skip_paths():
    K, A, B = _ring_pair(0.0, 3.0)
    rect = SR.rectify(K, *A, *B)
    none = np.full((8, 8), -16, np.int16)
    assert _mesh_case(none, rect)[2] == "no valid disparity/depth"
    two = none.copy()
    two[0, 0] = two[0, 4] = 16 * 30
    assert _mesh_case(two, rect)[2] == "insufficient valid vertices"
    jumpy = none.copy()
    jumpy[0, 0], jumpy[0, 4], jumpy[4, 0], jumpy[4, 4] = 16 * 30, 16 * 40, 16 * 30, 16 * 30
    assert _mesh_case(jumpy, rect, z_max_percentile=100.0)[2] == "no faces survived filtering"
    low = np.full((8, 8), 8, np.int16)  # 0.5 px < disp_min
    assert _mesh_case(low, rect)[2] == "no valid disparity/depth"


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_grid_mesh_random_maps(seed):
    K, A, B = _ring_pair(0.0, 3.0)
    rect = SR.rectify(K, *A, *B)
    rng = np.random.default_rng(seed)
    h, w = 61, 83
    base = rng.integers(16 * 5, 16 * 60, size=(h // 6 + 1, w // 6 + 1))
    d16 = np.kron(base, np.ones((6, 6), np.int64))[:h, :w] + rng.integers(-20, 21, size=(h, w))
    d16[rng.random((h, w)) < 0.15] = -16
    d16 = d16.astype(np.int16)
    for mp in (dict(), dict(step=3, disp_min=20.0, disp_jump=1.5, z_max_percentile=90.0), dict(step=1, z_max_percentile=50.0)):
        v, f, warn = _mesh_case(d16, rect, **mp)
        assert warn is None and len(f) > 0


def test_device_parameter_validation():
    assert capi.stereo_check_params(640, 480)
    assert capi.stereo_check_params(160, 120, num_disparities=32, census=5)
    assert capi.stereo_check_params(64, 64, num_disparities=256, census=7, p1=1, p2=2048)
    assert not capi.stereo_check_params(640, 480, num_disparities=120)  # not a multiple of 16
    assert not capi.stereo_check_params(640, 480, num_disparities=0)
    assert not capi.stereo_check_params(640, 480, num_disparities=272)
    assert not capi.stereo_check_params(640, 480, census=4)  # even window
    assert not capi.stereo_check_params(640, 480, census=9)  # more than 48 bits
    assert not capi.stereo_check_params(640, 480, p1=96, p2=96)  # p1 >= p2
    assert not capi.stereo_check_params(640, 480, p1=0)
    assert not capi.stereo_check_params(640, 480, p2=4096)
    assert not capi.stereo_check_params(640, 480, uniqueness=101)
    assert not capi.stereo_check_params(0, 480)
    with pytest.raises(TypeError):
        capi.stereo_params(block_size=7)


def test_numpy_sgm_one_row_by_hand():
    # 1 x 3 image, D = 2, p1 = 1, p2 = 3.  Horizontal paths worked by hand; the vertical ones are the cost itself (h = 1).
    C = np.array([[[0, 4], [4, 0], [2, 2]]], np.uint8)
    # L_lr: [0,4] -> [4,1] -> [3,2];  L_rl: [1,4] <- [4,0] <- [2,2]
    S = SR.aggregate(C, 1, 3)
    assert S.tolist() == [[[1, 16], [16, 1], [9, 8]]]
    # winners: d* = 0, 1, 1; sub-pixel only where 0 < d* < D-1 (never for D = 2)
    cl = np.zeros((1, 3), np.uint64)
    d16 = SR.select(S, cl, 0, -1)
    assert d16.tolist() == [[0, 16, 16]]
    # right view: d_r(0) = argmin(S(0,0) = 1, S(1,1) = 1) = 0 (tie: smaller d), d_r(1) = argmin(16, S(2,1) = 8) = 1, d_r(2) = 0
    assert SR.right_disparity(S).tolist() == [[0, 1, 0]]
    # x = 1 (d* = 1) meets d_r(0) = 0: off by one, rejected only with lr_max_diff = 0
    assert SR.select(S, cl, 0, 0).tolist() == [[0, -16, 16]]
    assert SR.select(S, cl, 0, 1).tolist() == [[0, 16, 16]]
