"""CPU suite: multi-view consistency filtering of disparity maps -- properties of the NumPy restatement
(tests/consist_ref.py), its calibration on the sphere and ring fixtures of DESIGN.md 13, and parameter validation of the
device stage (sfmx_consist_check_params needs no device).

Bounds: 1.25 x the value the restatement gives on the fixture, rounded up to the next integer (counts), 0.05 (RMS) or half a
percentage point (shares, on the distance to 100 %); DESIGN.md 15 has the table.  The result is deterministic; the margin only
covers an honest difference in how a fixture is rendered."""
import importlib

import numpy as np
import pytest

import consist_ref as CR
import fusion_ref as FR
import helpers as H
import stereo_ref as SR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")

# measured -> bound
CLEAN_DROPPED = 8        # 6 of 1 224 808 valid pixels of the clean maps are dropped
OUTLIERS_SURVIVE = 687   # 549 of 133 537 replaced pixels survive
UNTOUCHED_DROPPED = 92   # 73 of 1 163 599 untouched valid pixels are dropped
OFF_SHELL = 73           # 58 vertices more than one voxel off the sphere after the filter (10 461 before)
RMS_FILTERED = 0.30      # 0.201 voxel (4.75 before, 0.104 on the clean maps)
RING6_OUTWARD = 0.97     # 97.69 % of the faces point outward with the filter (88.63 % without)
RING6_SHELL = 1.0        # every vertex in radius 0.065 .. 0.105 (99.15 % without)
RING6_KEPT = (0.36, 0.58)  # 113 926 of 249 324 valid pixels kept: 45.7 %


def _valid(d16, disp_min=1.0):
    return (d16 != -16) & (d16.astype(np.float64) / 16.0 >= disp_min)


@pytest.fixture(scope="module")
def small():
    return CR.sphere8()[:8]


# ---- properties ------------------------------------------------------------------------------------------------------------
def test_min_support_zero_keeps_exactly_the_valid_pixels(small):
    r = CR.filter_views(small, min_support=0)
    for (_, d16), out in zip(small, r["disp16"]):
        assert (out == np.where(_valid(d16), d16, -16)).all()
    assert (r["kept"] == r["valid"]).all() and r["valid"].sum() > 10000


def test_kept_is_monotone_in_min_support(small):
    prev = None
    for ms in range(0, 9):
        r = CR.filter_views(small, min_support=ms)
        if prev is not None:
            assert (r["kept"] <= prev["kept"]).all()
            for a, b in zip(r["disp16"], prev["disp16"]):
                assert ((a != -16) <= (b != -16)).all(), "a pixel kept at a higher min_support was dropped at a lower one"
            assert all((a == b).all() for a, b in zip(r["support"], prev["support"])), "support does not depend on min_support"
        prev = r
    assert prev["kept"].sum() == 0, "7 other views cannot give a support of 8"


def test_one_view_has_no_support(small):
    r = CR.filter_views(small[:1])
    assert (r["support"][0] == 0).all() and r["kept"][0] == 0 and r["valid"][0] > 0
    r0 = CR.filter_views(small[:1], min_support=0)
    assert r0["kept"][0] == r0["valid"][0]
    assert CR.filter_views([])["valid"].shape == (0,)


def test_a_view_added_twice_supports_itself(small):
    r = CR.filter_views([small[0], small[0]], min_support=1)
    valid = _valid(small[0][1])
    for k in range(2):
        assert (r["support"][k][valid] == 1).all(), "j != i is by index, not by camera"
        assert (r["disp16"][k] == np.where(valid, small[0][1], -16)).all()


def test_zero_disparity_under_nonpositive_disp_min(small):
    """d = 0 is Z = +inf: valid under disp_min <= 0, its point is not finite, every test skips it; nothing raises"""
    cam, d16 = small[0]
    d = d16.copy()
    d[10:20, 10:20] = 0
    d[30, 30:34] = -7
    with np.errstate(all="raise"):  # the restatement silences what it expects itself
        for disp_min in (0.0, -5.0):
            c = {}
            r = CR.filter_views([(cam, d)] + small[1:], disp_min=disp_min, min_support=0, counter=c)
            assert (r["support"][0][10:20, 10:20] == 0).all()
            assert (r["disp16"][0][10:20, 10:20] == 0).all(), "valid, and min_support 0 keeps it"
            assert sum(c.values()) == 7 * int(r["valid"].sum())
    r = CR.filter_views([(cam, d)] + small[1:], disp_min=-5.0, min_support=1)
    assert (r["disp16"][0][10:20, 10:20] == -16).all()


def test_only_selects_reference_views(small):
    full = CR.filter_views(small)
    part = CR.filter_views(small, only=[5, 2])
    assert (part["disp16"][0] == full["disp16"][5]).all() and (part["support"][1] == full["support"][2]).all()
    assert list(part["kept"]) == [full["kept"][5], full["kept"][2]]


def test_outcomes_all_taken():
    """the defaults and rel_tol 4.0 together take all seven outcomes (`back_behind` needs the wide tolerance)"""
    views = CR.sphere8()
    c0, c4 = {}, {}
    r = CR.filter_views(views, counter=c0)
    CR.filter_views(views, counter=c4, rel_tol=4.0)
    print("defaults", c0, "rel_tol 4.0", c4)
    assert all(c0[k] + c4[k] > 0 for k in CR.OUTCOMES)
    assert sum(c0.values()) == 8 * int(r["valid"].sum())
    c8 = {}
    CR.filter_views(views[:8], counter=c8, rel_tol=4.0)
    assert c8["back_behind"] == 232


# ---- calibration -----------------------------------------------------------------------------------------------------------
def test_sphere26_calibration():
    clean, _ = CR.sphere26(False)
    noisy, masks = CR.sphere26(True)
    rc = CR.filter_views(clean)
    rn = CR.filter_views(noisy)
    dropped_clean = int(rc["valid"].sum() - rc["kept"].sum())
    survive = sum(int(((o != -16) & m).sum()) for o, m in zip(rn["disp16"], masks))
    untouched = sum(int(((d != -16) & ~m).sum()) for (_, d), m in zip(noisy, masks))
    untouched_kept = sum(int(((o != -16) & ~m).sum()) for o, m in zip(rn["disp16"], masks))
    print("clean: %d of %d kept; noisy: %d of %d replaced survive, %d of %d untouched kept"
          % (rc["kept"].sum(), rc["valid"].sum(), survive, sum(int(m.sum()) for m in masks), untouched_kept, untouched))
    assert rc["valid"].sum() == 1224808
    assert dropped_clean <= CLEAN_DROPPED
    assert survive <= OUTLIERS_SURVIVE
    assert untouched - untouched_kept <= UNTOUCHED_DROPPED
    vol = CR.SPHERE26_VOL
    fig = {}
    for name, vs in (("clean", clean), ("noisy", noisy), ("filtered", CR.filtered_views(noisy, rn))):
        m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], vs)
        fig[name] = CR.off_shell(m["verts"])
        print(name, "vertices %d, off the shell %d, radius RMS %.3f voxel" % ((len(m["verts"]),) + fig[name]))
    assert fig["clean"][0] == 0
    assert fig["filtered"][0] <= OFF_SHELL and fig["filtered"][1] <= RMS_FILTERED
    assert fig["noisy"][0] > 10 * OFF_SHELL, "the unfiltered maps are not bad enough to show that the filter acts"


def test_ring6_calibration():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    views = []
    for a, b in pairs:
        r = SR.rectify(K, poses[a][0], poses[a][1], poses[b][0], poses[b][1])
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        views.append((r, SR.disparity(il, ir, r["H_l"], r["H_r"], dict(num_disparities=64))))
    res = CR.filter_views(views)
    hist = sum(np.bincount(s[d != -16].ravel(), minlength=6) for s, (_, d) in zip(res["support"], views))
    print("kept %d of %d; per view %s of %s; support histogram %s" % (res["kept"].sum(), res["valid"].sum(), list(res["kept"]),
                                                                      list(res["valid"]), list(hist)))
    assert ((res["kept"] > 0) & (res["kept"] < res["valid"])).all()
    share = res["kept"].sum() / res["valid"].sum()
    assert RING6_KEPT[0] <= share <= RING6_KEPT[1]
    assert hist.sum() == res["valid"].sum() and len(hist) == 6, "five other views: support 0 .. 5"
    vol = CR.RING6_VOL
    q = {}
    for name, vs in (("off", views), ("on", CR.filtered_views(views, res))):
        m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], vs)
        q[name] = CR.mesh_quality(m["verts"], m["faces"])
        print("filter %s: outward %.4f, shell %.4f, vertices %d" % ((name,) + q[name]))
    assert q["on"][0] >= RING6_OUTWARD and q["on"][1] >= RING6_SHELL
    assert q["on"][0] > q["off"][0] and q["on"][2] > 1000


# ---- library and Python layer ----------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.consist_default_params() == dict(rel_tol=0.01, reproj_px=1.0, disp_min=1.0, min_support=2)
    assert capi.consist_default_params() == capi.CONSIST_DEFAULTS == CR.DEFAULTS
    assert capi.consist_check_params()
    assert capi.consist_check_params(rel_tol=1e-12, reproj_px=0.0, disp_min=-5.0, min_support=0)
    assert capi.consist_check_params(rel_tol=4.0, reproj_px=1e6, disp_min=40.0, min_support=1000)
    nan, inf = float("nan"), float("inf")
    for bad in [dict(rel_tol=0.0), dict(rel_tol=-0.01), dict(rel_tol=nan), dict(rel_tol=inf), dict(reproj_px=-1e-9),
                dict(reproj_px=nan), dict(reproj_px=inf), dict(disp_min=nan), dict(min_support=-1)]:
        assert not capi.consist_check_params(**bad), bad
    lib = capi.load_library()
    assert lib.sfmx_consist_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_consist_default_params(None)  # tolerated


def test_python_layer_rejects_unknown_keys():
    with pytest.raises(TypeError):
        capi.consist_params(depth_tol=1.0)
    assert set(pipe.CONSISTENCY_KEYS) == set(capi.CONSIST_DEFAULTS) - {"disp_min"}
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    for bad in (dict(colour=1), dict(disp_min=1.0)):  # disp_min is the fusion's
        with pytest.raises(TypeError):
            pipe.fuse(*args, consistency=bad)
    import inspect
    assert inspect.signature(pipe.fuse).parameters["consistency"].default is False
    assert hasattr(capi.Context, "consist") and hasattr(capi.Fusion, "add_consist_view")
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_cs")
