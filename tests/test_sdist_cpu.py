"""CPU suite: the NumPy restatement of the point-to-mesh distance (tests/sdist_ref.py) against values worked out by hand, its
candidate-pruned variant against brute force, the evaluation's host arithmetic, the parameter and key checks that need no
device, synth.shell_mesh, and the calibration of DESIGN.md 17: accuracy and completeness of the sphere-26 and ring-6 surfaces
that tests/fusion_ref.py / consist_ref.py / clean_ref.py produce, re-measured here."""
import importlib
import inspect
import math
import sys

import numpy as np
import pytest

import clean_ref as LR
import consist_ref as CR
import fusion_ref as FR
import helpers as H
import sdist_ref as DR
import stereo_ref as SR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")

TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]], np.int32)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[1].dtype == np.int32


# ---- the definition, by hand -----------------------------------------------------------------------------------------------
def test_seven_regions_of_one_triangle():
    cases = [((0.25, 0.25, 0.5), 0.25), ((0.5, -1.0, 0.0), 1.0), ((1.0, 1.0, 0.0), 0.5), ((-1.0, 0.5, 0.0), 1.0),
             ((-1.0, -1.0, 0.0), 2.0), ((2.0, -1.0, 0.0), 2.0), ((-1.0, 2.0, 0.0), 2.0)]
    P = np.array([p for p, _ in cases])
    d2, face = DR.brute(P, TRI_V, TRI_F, 4.0)
    assert d2.tolist() == [d for _, d in cases] and (face == 0).all()
    for perm in ([1, 2, 0], [2, 0, 1], [0, 2, 1]):  # any corner order and either orientation
        assert DR.brute(P, TRI_V, np.array([perm], np.int32), 4.0)[0].tolist() == d2.tolist()
    assert DR.seg(np.array([0.5, 1.0, 0.0]), TRI_V[0], TRI_V[1]) == 1.0
    assert DR.seg(np.array([-3.0, 4.0, 0.0]), TRI_V[0], TRI_V[1]) == 25.0 and DR.seg(np.array([2.0, 0.0, 1.0]), TRI_V[0], TRI_V[1]) == 2.0


def test_degenerate_faces_are_their_segments():
    V = np.array([[0.0, 0, 0], [1, 0, 0], [3, 0, 0], [0, 2, 0], [0.5, 0.5, 0.5]])
    P = np.array([[0.5, 1.0, 0.0], [2.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [4.0, 3.0, 0.0], [0.5, 0.5, 0.5]])
    for f, want in (([4, 4, 4], [0.5, 2.75, 2.75, 18.75, 0.0]), ([0, 0, 1], [1.0, 2.0, 1.0, 18.0, 0.5]), ([0, 1, 0], [1.0, 2.0, 1.0, 18.0, 0.5]),
                    ([0, 1, 2], [1.0, 1.0, 1.0, 10.0, 0.5]), ([0, 2, 1], [1.0, 1.0, 1.0, 10.0, 0.5])):
        d2, face = DR.brute(P, V, np.array([f], np.int32), 8.0)
        assert d2.tolist() == want and (face == 0).all(), f
    rng = np.random.default_rng(0)
    x = rng.normal(size=(5000, 4, 3))
    x[:1000, 2] = x[:1000, 1]
    x[1000:2000, 3] = x[1000:2000, 1] + 2.5 * (x[1000:2000, 2] - x[1000:2000, 1])
    x[2000:3000, 1:] = x[2000:3000, 1:2]
    assert np.isfinite(DR.tri(x[:, 0], x[:, 1], x[:, 2], x[:, 3])).all(), "never NaN"


def test_tie_goes_to_the_smallest_index():
    V = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    P = np.array([[0.25, 0.25, 0.0], [0.5, 0.5, 1.0], [0.75, 0.25, 0.0], [0.25, 0.75, 2.0]])
    assert DR.brute(P, V, F, 4.0)[1].tolist() == [0, 0, 0, 1]
    assert DR.brute(P, V, F[::-1].copy(), 4.0)[1].tolist() == [0, 0, 1, 0]
    assert DR.pruned(P, V, np.concatenate([F, F]), 4.0)[1].tolist() == [0, 0, 0, 1], "a duplicated face never wins"
    # on an icosphere ordinary queries tie too: the rule is exercised by plain data
    Vs, Fs = DR.icosphere(2, 1.0)
    rng = np.random.default_rng(1)
    Q = rng.normal(size=(3000, 3))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True) / rng.uniform(0.5, 1.5, (3000, 1))
    D = DR.tri(Q[:200, None, :], Vs[Fs[:, 0]][None], Vs[Fs[:, 1]][None], Vs[Fs[:, 2]][None])
    assert ((D == D.min(axis=1, keepdims=True)).sum(axis=1) > 1).any()


def test_clip_at_d_max():
    h = 0.5
    below = math.nextafter(h, 0.0)
    P = np.array([[0.25, 0.25, h], [0.25, 0.25, below], [0.25, 0.25, -h], [5.0, 5.0, 5.0]])
    d2, face = DR.brute(P, TRI_V, TRI_F, h)
    assert d2.tolist() == [0.25, below * below, 0.25, 0.25] and face.tolist() == [-1, 0, -1, -1], "!(d2 < d_max^2) is clipped"
    d2, face = DR.brute(P, TRI_V, TRI_F, math.nextafter(h, 1.0))
    assert face.tolist() == [0, 0, 0, -1] and d2[0] == 0.25
    d2, face = DR.brute(P, TRI_V, np.zeros((0, 3), np.int32), h)
    assert (d2 == 0.25).all() and (face == -1).all(), "no faces: everything is clipped"
    assert DR.brute(np.zeros((0, 3)), TRI_V, TRI_F, h)[0].shape == (0,)


def test_icosphere_distances_within_the_sagitta():
    R = 0.1
    V, F = DR.icosphere(3, R)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n = DR.cross(b - a, c - a)
    sag = R - (np.abs(DR.dot(a, n)) / np.sqrt(DR.dot(n, n))).min()  # the deepest face plane below the sphere
    assert 0.0 < sag < 0.002
    rng = np.random.default_rng(2)
    P = rng.normal(size=(3000, 3))
    r = rng.uniform(0.05, 0.15, 3000)
    P *= (r / np.linalg.norm(P, axis=1))[:, None]
    d2, face = DR.brute(P, V, F, 1.0)
    err = np.abs(np.sqrt(d2) - np.abs(r - R))
    print("level-3 icosphere: sagitta %.3e, largest deviation from |r - R| %.3e" % (sag, err.max()))
    assert (face >= 0).all() and err.max() <= sag * (1.0 + 1e-9)


# ---- pruning ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ico_case():
    V, F = DR.icosphere(3, 0.1)
    rng = np.random.default_rng(11)
    d = rng.normal(size=(1500, 3))
    P = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.08, 0.12, (1500, 1))
    P = np.concatenate([P, [[1e3, 0, 0], [0, -1e6, 0], [0.0, 0.0, 0.0]], V[:50]])
    return P, V, F


@pytest.mark.parametrize("d_max", [0.002, 0.01, 0.05, 1.0])
def test_pruned_is_brute_force_bit_for_bit(ico_case, d_max):
    P, V, F = ico_case
    ref = DR.brute(P, V, F, d_max)
    assert _same(DR.pruned(P, V, F, d_max), ref)
    assert _same(DR.pruned(P, V, F, d_max, chunk=97), ref)
    assert _same(DR.brute(P, V, F, d_max, box=False), ref), "the grown-box rule drops no face that the plain minimum would choose"
    assert (ref[1] >= 0).sum() > 100
    if d_max == 0.01:  # the fallback grid agrees with scipy's tree
        saved = {k: sys.modules.get(k) for k in ("scipy", "scipy.spatial")}
        try:
            for k in saved:
                sys.modules[k] = None  # import raises ImportError
            assert _same(DR.pruned(P[:300], V, F, d_max), (ref[0][:300], ref[1][:300]))
        finally:
            for k, m in saved.items():
                if m is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = m


def test_box_rule_is_three_exact_comparisons():
    """a face counts for a query inside its bounding box grown by d_max (1 + 2^-10), borders included"""
    g = 0.25 * DR.GROW
    lo, hi = DR.boxes(TRI_V, TRI_F, 0.25)
    assert lo.tolist() == [[-g, -g, -g]] and hi.tolist() == [[1.0 + g, 1.0 + g, g]]
    P = np.array([[0.25, 0.25, g], [0.25, 0.25, math.nextafter(g, 1.0)], [-g, -g, 0.0], [0.25, -0.2, 0.0]])
    d2, face = DR.brute(P, TRI_V, TRI_F, 0.25)
    assert face.tolist() == [-1, -1, -1, 0] and d2.tolist() == [0.0625, 0.0625, 0.0625, 0.2 * 0.2]
    assert DR.brute(P, TRI_V, TRI_F, 0.25, box=False)[1].tolist() == face.tolist(), "beyond d_max either way: the rule is inert"


# ---- evaluation ------------------------------------------------------------------------------------------------------------
def test_evaluation_arithmetic():
    assert DR.nearest_rank(np.arange(1.0, 11.0), 90.0) == 9.0 and DR.nearest_rank(np.arange(1.0, 11.0), 91.0) == 10.0
    assert DR.nearest_rank(np.arange(1.0, 11.0), 100.0) == 10.0 and DR.nearest_rank(np.arange(1.0, 11.0), 0.001) == 1.0
    G = DR.icosphere(3, 0.1)
    V, F = DR.icosphere(2, 0.101)
    V = np.concatenate([V, [[9.0, 9.0, 9.0]]])  # a vertex no face uses is not sampled
    e = DR.evaluate(V, F, *G, 0.004, 0.002, dist=DR.brute)
    assert e == DR.evaluate(V, F, *G, 0.004, 0.002) and tuple(sorted(e)) == tuple(sorted(pipe.EVALUATION_FIELDS))
    assert e["n_rec"] == len(V) - 1 and e["n_gt"] == len(G[0]) and e["acc_within"] == e["n_rec"] and abs(e["accuracy"] - 0.001) < 1e-12
    e2 = DR.evaluate(*DR.icosphere(2, 0.1), *G, 0.004, 0.001)  # inscribed: its vertices are the truth's, its faces lie below
    assert e2["accuracy"] == 0.0 and 162 <= e2["comp_within"] < e2["n_gt"] and e2["completeness"] == e2["comp_within"] / e2["n_gt"]
    far = DR.evaluate(V * 2.0, F, *G, 0.004, 0.002)
    assert far["accuracy"] == far["acc_max"] == 0.004 and abs(far["acc_mean"] - 0.004) < 1e-15 and far["acc_within"] == 0 and far["completeness"] == 0.0
    none = DR.evaluate(V, np.zeros((0, 3), np.int32), *G, 0.004, 0.002)
    assert none["n_rec"] == 0 and math.isnan(none["accuracy"]) and none["comp_within"] == 0


# ---- library and Python layer ----------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.sdist_default_params() == dict(d_max=0.0, cell=0.0)
    assert not capi.sdist_check_params(**capi.sdist_default_params()), "d_max has no default"
    assert capi.sdist_check_params(1e-3) and capi.sdist_check_params(2.0 ** 60, 5.0) and capi.sdist_check_params(2.0 ** -500)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** 61, 2.0 ** -501, 1e-300):  # below 2^-500 d_max^2 would underflow
        assert not capi.sdist_check_params(bad), bad
    for bad in (-1.0, float("nan"), float("inf")):
        assert not capi.sdist_check_params(1.0, bad), bad
    lib = capi.load_library()
    assert lib.sfmx_sdist_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_sdist_default_params(None)  # tolerated
    assert lib.sfmx_sdist_stats(None, None, None, None, None, None) == capi.SFMX_ERR_INVALID
    assert capi.SDIST_CHUNK == int([ln for ln in open(H.ROOT + "/include/sfmx.h") if ln.startswith("#define SFMX_SDIST_CHUNK")][0].split()[2])


def test_python_layer_rejects_unknown_keys():
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    gt = dict(gt_verts=TRI_V, gt_faces=TRI_F)
    for bad in (dict(gt, d_max=1.0, tau=0.5, radius=1), dict(d_max=1.0, tau=0.5), dict(gt, d_max=1.0), dict(gt, tau=1.0)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, evaluate=bad)
    with pytest.raises(ValueError):
        pipe.fuse(*args, evaluate=dict(gt, d_max=1.0, tau=1.5))
    with pytest.raises(TypeError):
        pipe.surface_eval(None, TRI_V, TRI_F, TRI_V, TRI_F, tau=1.0)
    with pytest.raises(ValueError):
        pipe.surface_eval(None, TRI_V, TRI_F, TRI_V, TRI_F, d_max=1.0, tau=float("nan"))
    assert inspect.signature(pipe.fuse).parameters["evaluate"].default is None
    assert inspect.signature(pipe.surface_eval).parameters["percentile"].default == 90.0
    assert hasattr(capi.Context, "sdist") and all(hasattr(capi.Sdist, k) for k in ("set_target", "query", "stats", "close"))
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_ev") and hasattr(lib, "sfmx_host_surface_eval")


def test_shell_mesh_is_closed_and_on_the_shell():
    for level in (0, 2, 4):
        v, f = synth.shell_mesh(level)
        assert v.shape == (10 * 4 ** level + 2, 3) and f.shape == (20 * 4 ** level, 3) and f.dtype == np.int32
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        ue, cnt = np.unique(e, axis=0, return_counts=True)
        assert (cnt == 2).all() and len(v) - len(ue) + len(f) == 2, "closed, Euler characteristic 2"
        d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert len(np.unique(d, axis=0)) == len(d), "every edge once in each direction: consistently oriented"
        n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        assert ((n * v[f].mean(axis=1)).sum(axis=1) > 0).all(), "faces point outward"
        r = np.linalg.norm(v, axis=1)
        u = v / r[:, None]
        assert np.allclose(r, np.clip(0.085 + 0.012 * np.sin(7.0 * u[:, 0]) * np.cos(5.0 * u[:, 1]), 0.07, 0.10), rtol=1e-14, atol=0)
        assert np.allclose(synth.shell_mesh(level, 3.5)[0], 3.5 * v, rtol=1e-14, atol=0)
    # the scene's own points lie within its jitter of the mesh
    pts = synth.make_scene(2000, seed=7)["pts"]
    d = np.sqrt(DR.pruned(pts, *synth.shell_mesh(5), 0.02)[0])
    assert np.sqrt((d ** 2).mean()) < 0.0035 and d.max() < 0.013, "sigma 0.003, clipped at 0.07 / 0.10"


# ---- calibration --------------------------------------------------------------------------------------------
# d_max = 4 voxels (the truncation band), tau = 1 voxel; ground truth at level 5 (20 480 faces).  Accuracy bounds are 1.25 x
# the measured value rounded up to 1e-4; completeness bounds 1.25 x the distance to 100 %, rounded up to half a point.
SPHERE_RAW_ACC = (0.0190, 0.0200)      # the raw noisy sphere: measured 0.019039, more than a tenth of it is clipped at d_max = 0.02
SPHERE_FILT_ACC = 0.0012               # filtered: measured 0.000928
SPHERE_CLEAN_ACC = 0.0012              # filtered and cleaned: measured 0.000922
RING_OFF_ACC, RING_OFF_COMP = 0.0091, 0.340  # filter off: measured 0.007270 and 47.51 %
RING_ON_ACC, RING_ON_COMP = 0.0036, 0.120    # filter on: measured 0.002810 and 29.96 %


def _row(name, v, f, G, voxel):
    e = DR.evaluate(v, f, *G, 4 * voxel, voxel)
    print("%s: accuracy %.6f (mean %.6f, max %.6f, %d of %d within tau), completeness %.4f (%d of %d)"
          % (name, e["accuracy"], e["acc_mean"], e["acc_max"], e["acc_within"], e["n_rec"], e["completeness"], e["comp_within"], e["n_gt"]))
    return e


def test_sphere26_calibration():
    noisy, _ = CR.sphere26(True)
    vol = CR.SPHERE26_VOL
    G = DR.icosphere(5, CR.RADIUS)
    raw = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], noisy)
    filt = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(noisy, CR.filter_views(noisy)))
    cl = LR.clean(filt["verts"], filt["faces"])
    e_raw = _row("sphere-26, 5 % outliers, raw", raw["verts"], raw["faces"], G, vol["voxel"])
    e_filt = _row("sphere-26, filtered", filt["verts"], filt["faces"], G, vol["voxel"])
    e_cl = _row("sphere-26, filtered and cleaned", cl["verts"], cl["faces"], G, vol["voxel"])
    # the restatements are deterministic: the integer columns of the table are stated exactly
    assert (e_raw["n_rec"], e_raw["acc_within"], e_raw["comp_within"]) == (33415, 22955, 10242)
    assert (e_filt["n_rec"], e_filt["acc_within"], e_filt["comp_within"]) == (22850, 22792, 10242)
    assert (e_cl["n_rec"], e_cl["acc_within"], e_cl["comp_within"]) == (22792, 22792, 10242)
    assert SPHERE_RAW_ACC[0] <= e_raw["accuracy"] <= SPHERE_RAW_ACC[1] and e_raw["acc_max"] == 4 * vol["voxel"]
    assert e_filt["accuracy"] <= SPHERE_FILT_ACC and e_cl["accuracy"] <= SPHERE_CLEAN_ACC
    # the metric moves the way DESIGN.md 15 and 16 say the surfaces do
    assert e_raw["accuracy"] > 10 * e_cl["accuracy"], "the raw noisy sphere is worse than the filtered and cleaned one"
    assert e_cl["accuracy"] <= e_filt["accuracy"] and e_cl["acc_max"] < e_filt["acc_max"], "cleaning removes the far islands"
    assert e_raw["completeness"] == e_filt["completeness"] == e_cl["completeness"] == 1.0, "and nothing of the sphere is lost"


def test_ring6_calibration():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    views = []
    for a, b in pairs:
        r = SR.rectify(K, poses[a][0], poses[a][1], poses[b][0], poses[b][1])
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        views.append((r, SR.disparity(il, ir, r["H_l"], r["H_r"], dict(num_disparities=64))))
    vol = CR.RING6_VOL
    G = synth.shell_mesh(5)
    off = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], views)
    on = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(views, CR.filter_views(views)))
    e_off = _row("ring-6, filter off", off["verts"], off["faces"], G, vol["voxel"])
    e_on = _row("ring-6, filter on", on["verts"], on["faces"], G, vol["voxel"])
    assert (e_off["n_rec"], e_off["acc_within"], e_off["comp_within"]) == (18682, 13928, 4866)
    assert (e_on["n_rec"], e_on["acc_within"], e_on["comp_within"]) == (7552, 7293, 3068)
    assert e_off["accuracy"] <= RING_OFF_ACC and e_off["completeness"] >= RING_OFF_COMP
    assert e_on["accuracy"] <= RING_ON_ACC and e_on["completeness"] >= RING_ON_COMP
    # six pairs over 53 degrees see part of the shell only; the filter buys accuracy with coverage, and the metric says how much
    assert e_on["accuracy"] < 0.5 * e_off["accuracy"] and e_on["completeness"] < e_off["completeness"]
