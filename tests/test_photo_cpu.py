"""CPU suite for the photometric re-rendering: the NumPy restatement (tests/photo_ref.py) on hand cases whose
answers are known, its invariances in its own batching model, the containment property of the layout, the parameter validation
of the device stage (sfmx_photo_check_params needs no device), the key checks of pipeline.fuse, capi.photo_summary against hand
numbers, and the calibration of DESIGN.md 27 with its rule.  No GPU.
"""
import importlib
import math

import numpy as np
import pytest

import helpers as H
import level_ref as LR
import photo_ref as P
import raster_ref as R
import texture_ref as TR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")


def _bound(x):
    """DESIGN.md 15's rule: 1.25 x the restatement's figure, rounded up to 0.1 grey level"""
    return math.ceil(1.25 * x * 10.0 - 1e-9) / 10.0


# the restatement's figures on texture_ref.fidelity_scene() (z_min 0.05, depth_tol 0.002, patch 8)
MEASURED = dict(own=0.11293, cross=0.21369, held=0.19872, held_p90=1, held_untextured=0,  # 13 even views texture, all 26 render
                tx_cross=19.91614, lv_cross=15.21868, tx_own=0.13239, lv_own=8.47838)   # 26 disturbed views, 64 sweeps
BOUND_OWN, BOUND_CROSS, BOUND_HELD, BOUND_HELD_P90 = 0.2, 0.3, 0.3, 1.3
BOUND_TX_CROSS, BOUND_LV_CROSS = 24.9, 19.1


# ---- hand cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 4, 8, 64])
def test_pixels_on_texel_centres_reproduce_the_atlas(S):
    v, f, cam, img = P.aligned_face(S)
    tex = TR.run(v, f, [cam], [img], 0.5, 0.0, patch=S)
    res = P.run(v, f, [cam], [img], [0], tex, 0.5, patch=S)
    cls, out, face = (P.view_image(res, [cam], 0, k) for k in ("cls", "rendered", "face"))
    L = S - 2
    hit = 0
    for j in range(L + 1):
        for i in range(L + 1 - j):
            y, x = 1 + j, 1 + i
            if cls[y, x] == 0:  # an edge the top-left rule gives away
                continue
            hit += 1
            # pixel (1 + i, 1 + j) is texel (j, i) of half 0 of cell 0, and that texel was sampled at this very pixel centre
            assert cls[y, x] == 3 and face[y, x] == 0 and out[y, x] == tex["atlas"][i, j] == img[y, x], (S, i, j)
    assert hit == int((cls == 3).sum()) >= (L * (L + 1)) // 2 and res["classes"][0, 3] == hit
    assert res["stats"].tolist() == [[[hit, 0, 0], [0, 0, 0]]] and res["hist"][0, 0, 0] == hit and res["hist"].sum() == hit
    assert res["foreign_weight"] == 0.0


def test_the_five_classes():
    v, f, tc, ti, pc, pi, tv = P.five_classes()
    tex = TR.run(v, f, tc, ti, 0.5, 0.0, patch=4, fill=77)
    assert tex["face_view"].tolist() == [0, -1, -1]
    res = P.run(v, f, pc, pi, tv, tex, 0.5, patch=4, fill=77, background=9)
    assert res["classes"].tolist() == [[147, 15, 15, 15, 0], [147, 15, 15, 0, 15]]
    for q, own in ((0, 3), (1, 4)):
        cls, out, face = (P.view_image(res, pc, q, k) for k in ("cls", "rendered", "face"))
        assert (cls[:, :8].max(), cls[:, 8:16].max(), cls[:, 16:].max()) == (own, 2, 1)
        assert set(out[cls == 0]) == {9} and set(out[cls == 1]) == {9} and set(out[cls == 2]) == {77}
        assert set(face[cls == 0]) == {-1} and set(face[cls == own]) == {0} and set(face[cls == 2]) == {1} and set(face[cls == 1]) == {2}
        d = np.abs(out[cls == own].astype(int) - pi[q][cls == own].astype(int))
        assert res["stats"][q, own - 3].tolist() == [15, d.sum(), (d * d).sum()] and res["stats"][q, 4 - own].tolist() == [0, 0, 0]
        assert res["hist"][q, own - 3].tolist() == np.bincount(d, minlength=256).tolist()
    assert np.array_equal(P.view_image(res, pc, 0), P.view_image(res, pc, 1))  # the class changes, the picture does not


@pytest.mark.parametrize("S", [3, 4, 8, 64])
def test_containment(S):
    """no pixel reads a texel of another face with a weight above 2^-40: off-centre pixels of faces in both halves of many cells,
    the first and the last cell included (run() asserts it; here the weight is looked at too)"""
    w = h = 30
    v, f = P.quilt(5, 5, 6.0, seed=S)
    cams = [R.pixel_camera(w, h), R.pixel_camera(w, h, cx=0.375, cy=-0.25)]
    imgs = [np.random.default_rng(S + k).integers(0, 256, (h, w)).astype(np.uint8) for k in range(2)]
    tex = TR.run(v, f, cams, imgs, 0.5, 0.25, patch=S)
    assert tex["faces_textured"] == 50 and tex["cells"] == 25
    res = P.run(v, f, cams, imgs, [0, 1], tex, 0.5, patch=S)
    # equal areas in both views: every face takes view 0, so view 0 is all own and view 1 all cross
    assert res["classes"][0, 3] > 300 and res["classes"][1, 4] > 300 and res["foreign_weight"] <= P.CONTAIN_W
    with pytest.raises(AssertionError):  # the check can fail: a layout shifted by one texel makes every read foreign
        P.run(v, f, cams, imgs, [0, 1], dict(tex, uv_half=tex["uv_half"] + np.array([2 * (S + 1), 0], np.int32)), 0.5, patch=S)


@pytest.mark.parametrize("grey", [0, 255])
def test_errors_against_constant_images(grey):
    v, f, tc, ti, pc, _, tv = P.five_classes()
    tex = TR.run(v, f, tc, ti, 0.5, 0.0, patch=4)
    flat = [np.full((8, 24), grey, np.uint8), None]
    res = P.run(v, f, pc, flat, tv, tex, 0.5, patch=4)
    out, cls = P.view_image(res, pc, 0), P.view_image(res, pc, 0, "cls")
    d = np.abs(out[cls == 3].astype(int) - grey)
    assert d.max() <= 255 and res["stats"][0, 0].tolist() == [15, d.sum(), (d * d).sum()]
    assert res["hist"][0, 0].tolist() == np.bincount(d, minlength=256).tolist()
    assert not res["stats"][1].any() and not res["hist"][1].any() and res["classes"][1, 4] == 15  # no image: classes only
    atlas = np.full_like(tex["atlas"], 255 - grey)
    res = P.run(v, f, pc, flat, tv, tex, 0.5, patch=4, atlas=atlas)
    assert res["stats"][0, 0].tolist() == [15, 15 * 255, 15 * 65025] and res["hist"][0, 0, 255] == 15


def test_invariance_under_view_order_and_batch():
    v, f, cams, images = TR.fidelity_scene()
    sel = [0, 1, 2, 3, 4]
    cams, images = [dict(cams[k], w=80, h=80, f=cams[k]["f"] / 4, cx=cams[k]["cx"] / 4, cy=cams[k]["cy"] / 4) for k in sel], [
        np.ascontiguousarray(images[k][::4, ::4]) for k in sel]
    tex = TR.run(v, f, cams[:3], images[:3], 0.05, 0.002, patch=4)
    tv = [0, 1, 2, -1, -1]
    imgs = images[:4] + [None]
    a = P.run(v, f, cams, imgs, tv, tex, 0.05, patch=4)
    assert a["classes"][:, 3].min(initial=1) >= 0 and a["stats"][:3, 0, 0].min() > 0 and a["stats"][3, 1, 0] > 0 and not a["stats"][4].any()
    for batch in (1, 2, 4, 5):
        P.same(a, P.run(v, f, cams, imgs, tv, tex, 0.05, patch=4, batch=batch), f"batch {batch}")
    perm = [3, 0, 4, 2, 1]
    b = P.run(v, f, [cams[k] for k in perm], [imgs[k] for k in perm], [tv[k] for k in perm], tex, 0.05, patch=4, batch=2)
    for q, k in enumerate(perm):
        for key in ("classes", "stats", "hist"):
            assert np.array_equal(b[key][q], a[key][k]), (key, q, k)
        for key in ("rendered", "cls", "face"):
            assert np.array_equal(P.view_image(b, [cams[j] for j in perm], q, key), P.view_image(a, cams, k, key)), (key, q, k)


def test_refusals_and_empty_inputs():
    v, f, tc, ti, pc, pi, tv = P.five_classes()
    tex = TR.run(v, f, tc, ti, 0.5, 0.0, patch=4)
    for bad in (lambda: P.run(v, f, pc, pi, tv, None, 0.5, patch=4), lambda: P.run(v, f[:2], pc, pi, tv, tex, 0.5, patch=4),
                lambda: P.run(v, f, pc, pi, [0, 1], tex, 0.5, patch=4), lambda: P.run(v, f, pc, pi, [-2, 0], tex, 0.5, patch=4),
                lambda: P.run(v, f, pc, pi, tv, tex, 0.5, patch=4, atlas=np.zeros((3, 3), np.uint8)),
                lambda: P.run(v, np.array([[0, 1, 9], [3, 4, 5], [6, 7, 8]], np.int32), pc, pi, tv, tex, 0.5, patch=4),
                lambda: P.run(v, f, pc, pi, tv, tex, 0.0, patch=4),
                lambda: P.run(v, f, [R.pixel_camera(4096, 4096)] * 17, [None] * 17, [-1] * 17, tex, 0.5, patch=4)):
        with pytest.raises(ValueError):
            bad()
    res = P.run(v, f, [], [], [], tex, 0.5, patch=4)
    assert len(res["rendered"]) == 0 and res["classes"].shape == (0, 5) and res["offsets"].tolist() == [0]
    none = TR.run(np.zeros((0, 3)), np.zeros((0, 3), np.int32), tc, ti, 0.5, 0.0, patch=4)
    res = P.run(np.zeros((0, 3)), np.zeros((0, 3), np.int32), pc, pi, tv, none, 0.5, patch=4, background=3)
    assert res["classes"].tolist() == [[192, 0, 0, 0, 0]] * 2 and set(res["rendered"]) == {3} and set(res["face"]) == {-1}


# ---- library and Python layer ------------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.PHOTO_DEFAULTS == P.DEFAULTS == dict(background=0) and capi.PHOTO_CLASSES == P.CLASSES
    assert capi.photo_default_params() == dict(z_min=0.0, background=0)
    assert capi.PHOTO_MAX_PIXELS == P.PIXELS_MAX == 1 << 28
    assert not capi.photo_check_params() and not P.check_params()  # z_min has no default
    for good in P.GOOD_PARAMS:
        assert capi.photo_check_params(**good) and P.check_params(**good), good
    for bad in P.BAD_PARAMS:
        assert not capi.photo_check_params(**bad) and not P.check_params(**bad), bad
    with pytest.raises(TypeError):
        capi.photo_params(1.0, cull=1)
    with pytest.raises(TypeError):
        capi.photo_params(1.0, background=7.5)
    for b in (-1, 256):
        assert not P.check_params(1.0, background=b)
        with pytest.raises(ValueError):
            capi.photo_params(1.0, background=b)
    lib = capi.load_library()
    assert lib.sfmx_photo_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_photo_default_params(None)  # tolerated
    assert sum(s.startswith("sfmx_photo_") for s in capi.SYMBOLS) == 16
    assert lib.sfmx_photo_sizes(None, None, None) == capi.SFMX_ERR_INVALID and lib.sfmx_photo_device_rendered(None, None) == -1
    assert lib.sfmx_photo_view_count(None) == 0 and lib.sfmx_photo_set_batch(None, 1) == capi.SFMX_ERR_INVALID and lib.sfmx_photo_last_batch(None) == 0
    assert lib.sfmx_photo_last_us(None) == 0.0 and lib.sfmx_photo_last_resolve_us(None) == 0.0
    assert hasattr(capi.Context, "photo")
    assert all(hasattr(capi.Photo, k) for k in ("add_view", "add_texture_views", "set_batch", "run", "read", "sizes", "device_rendered", "last_us",
                                                "last_resolve_us", "last_batch", "view_count", "reset"))


def test_python_layer_key_checks():
    import inspect
    assert set(pipe.PHOTO_KEYS) == {"background", "pgm_prefix"}
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    tex = dict(z_min=0.05)
    for bad in (dict(z_min=0.1), dict(background=0, patch=8), dict(background=2.5)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, texture=tex, photo=bad)  # refused before any device call: the context is None
    with pytest.raises(ValueError):
        pipe.fuse(*args, texture=tex, photo=dict(background=256))
    for ph in (True, dict(background=3)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, photo=ph)  # photo without texture
        with pytest.raises(TypeError):
            pipe.fuse(*args, texture=False, level=False, photo=ph)
    assert inspect.signature(pipe.fuse).parameters["photo"].default is False
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_ph") and hasattr(lib, "sfmx_host_photo_free") and hasattr(lib, "sfmx_host_fusion_mesh_lv")
    lib.sfmx_host_photo_free(None)  # tolerated


STANDIN_MAIN = r"""
#include <cstdio>
#include "fusion.hpp"
int main() {
  sfmx_ctx* ctx = nullptr;
  if (sfmx_ctx_create(0, &ctx) != SFMX_OK) return 2;
  const double K[9] = {100, 0, 8, 0, 100, 8, 0, 0, 1};
  sfmx_stereo_params sp{};
  sfmx_fusion_params fp{};
  sfmx_fusion_result_ex res{};
  sfmx_photo_request pq{};
  const int with = sfmx_host_fusion_mesh_ph(ctx, nullptr, 0, 0, 16, 16, K, nullptr, nullptr, 0, &sp, &fp, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, &pq, &res, nullptr, nullptr, 0);
  const int without = sfmx_host_fusion_mesh_ph(ctx, nullptr, 0, 0, 16, 16, K, nullptr, nullptr, 0, &sp, &fp, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, &res, nullptr, nullptr, 0);
  sfmx_host_photo_free(&pq);
  std::printf("%d %d\n", with, without);
  sfmx_ctx_destroy(ctx);
  return 0;
}
"""


def test_stand_in_library_reports_unsupported(tmp_path):
    """the host layer on the CPU stand-in of libsfmx.so (tests/fake_sfmx), which has no photo stage: it links untouched, because the
    device entries are weak references, and a photo request says SFMX_ERR_UNSUPPORTED (before it looks for the texture request);
    without a request the call is the plain fusion, which the stand-in does not have either"""
    import os
    import subprocess
    host = os.path.join(H.ROOT, H.PKG_NAME, "csrc", "host")
    out = str(tmp_path)
    flags = ["-std=c++20", "-O0", "-ffp-contract=off", "-fPIC", "-I" + os.path.join(H.ROOT, "include")]
    with open(os.path.join(out, "main.cpp"), "w") as f:
        f.write(STANDIN_MAIN)
    subprocess.run(["g++", *flags, "-shared", "-o", os.path.join(out, "libsfmx.so"), os.path.join(H.ROOT, "tests", "fake_sfmx", "fake_sfmx.cpp"),
                    os.path.join(H.ROOT, "oracle", "sfm_oracle.cpp"), "-lrt", "-lpthread"], check=True)
    srcs = [os.path.join(host, n) for n in sorted(os.listdir(host)) if n.endswith(".cpp") and n != "main.cpp"]
    subprocess.run(["g++", *flags, "-I" + host, "-o", os.path.join(out, "standin"), os.path.join(out, "main.cpp"), *srcs, "-L" + out, "-lsfmx",
                    "-Wl,-rpath," + out, "-lpthread"], check=True)
    p = subprocess.run([os.path.join(out, "standin")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    with_photo, without = (int(x) for x in p.stdout.split())
    assert with_photo == capi.SFMX_ERR_UNSUPPORTED and without == capi.SFMX_ERR_UNSUPPORTED


def test_photo_summary_against_hand_numbers():
    stats = np.zeros((2, 2, 3), np.int64)
    hist = np.zeros((2, 2, 256), np.int64)
    hist[0, 0, [0, 1, 4]] = [7, 2, 1]  # ten pixels: d = 0 x 7, 1 x 2, 4 x 1
    stats[0, 0] = [10, 6, 18]
    hist[1, 1, [0, 10]] = [1, 9]
    stats[1, 1] = [10, 90, 900]
    hist[1, 0, 0] = 5
    stats[1, 0] = [5, 0, 0]
    s = capi.photo_summary(stats, hist)
    a = s["views"][0]["own"]
    assert a["count"] == 10 and a["mae"] == 0.6 and a["rmse"] == math.sqrt(1.8) and a["p90"] == 1
    assert a["psnr"] == 10.0 * math.log10(65025.0 * 10 / 18)
    assert s["views"][0]["cross"] == dict(count=0, mae=None, rmse=None, psnr=None, p90=None)
    b = s["views"][1]["cross"]
    assert b["mae"] == 9.0 and b["rmse"] == math.sqrt(90.0) and b["p90"] == 10
    z = s["views"][1]["own"]
    assert z["mae"] == 0.0 and z["psnr"] == float("inf") and z["p90"] == 0
    assert s["own"]["count"] == 15 and s["own"]["mae"] == 6 / 15 and s["own"]["p90"] == 1 and s["cross"] == b
    for q in range(2):
        for o, name in enumerate(("own", "cross")):
            assert s["views"][q][name] == P.measures(stats[q, o], hist[q, o])
    assert capi.photo_summary(np.zeros((0, 2, 3)), np.zeros((0, 2, 256)))["own"]["count"] == 0


# ---- calibration ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    return TR.fidelity_scene()


def test_held_out_views_of_the_textured_sphere(sphere):
    v, f, cams, img = sphere
    z, tol, S = TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"], TR.FIDELITY["patch"]
    even, odd = list(range(0, 26, 2)), list(range(1, 26, 2))
    tex = TR.run(v, f, [cams[k] for k in even], [img[k] for k in even], z, tol, patch=S)
    res = P.run(v, f, cams, img, [k // 2 if k % 2 == 0 else -1 for k in range(26)], tex, z, patch=S)
    own, cross, held = P.pooled(res, even, 0), P.pooled(res, even, 1), P.pooled(res, odd, 1)
    print("textured sphere, 13 texture views: own MAE %.5f (%d px), cross MAE %.5f (%d px); 13 held-out views: MAE %.5f, p90 %d (%d px), "
          "untextured %d" % (own["mae"], own["count"], cross["mae"], cross["count"], held["mae"], held["p90"], held["count"],
                             int(res["classes"][odd, 2].sum())))
    assert P.pooled(res, odd, 0)["count"] == 0 and res["foreign_weight"] <= P.CONTAIN_W
    assert abs(own["mae"] - MEASURED["own"]) < 5e-5 and abs(cross["mae"] - MEASURED["cross"]) < 5e-5 and abs(held["mae"] - MEASURED["held"]) < 5e-5
    assert held["p90"] == MEASURED["held_p90"] and int(res["classes"][odd, 2].sum()) == MEASURED["held_untextured"] == 0
    assert own["mae"] <= BOUND_OWN and cross["mae"] <= BOUND_CROSS and held["mae"] <= BOUND_HELD and held["p90"] <= BOUND_HELD_P90


def test_levelling_under_disturbed_images(sphere):
    v, f, cams, img = sphere
    z, tol, S = TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"], TR.FIDELITY["patch"]
    dimg = LR.disturb(img)
    tex = TR.run(v, f, cams, dimg, z, tol, patch=S)
    lev = LR.run(v, f, cams, dimg, tex, iterations=64, patch=S)
    allv = list(range(26))
    a = P.run(v, f, cams, dimg, allv, tex, z, patch=S)
    b = P.run(v, f, cams, dimg, allv, tex, z, patch=S, atlas=lev["atlas"])
    ta, tb, oa, ob = P.pooled(a, allv, 1)["mae"], P.pooled(b, allv, 1)["mae"], P.pooled(a, allv, 0)["mae"], P.pooled(b, allv, 0)["mae"]
    print("disturbed sphere: cross MAE %.5f with the texture's atlas, %.5f with the levelled one; own MAE %.5f -> %.5f" % (ta, tb, oa, ob))
    assert np.array_equal(a["cls"], b["cls"]) and np.array_equal(a["face"], b["face"])  # the atlas changes the grey only
    assert abs(ta - MEASURED["tx_cross"]) < 5e-5 and abs(tb - MEASURED["lv_cross"]) < 5e-5
    assert abs(oa - MEASURED["tx_own"]) < 5e-5 and abs(ob - MEASURED["lv_own"]) < 5e-5
    assert ta <= BOUND_TX_CROSS and tb <= BOUND_LV_CROSS
    assert tb < ta, "levelling lowers the cross-view error (and raises the own-view error: the offsets leave the own picture)"


def test_the_bounds_follow_the_rule():
    for bound, key in ((BOUND_OWN, "own"), (BOUND_CROSS, "cross"), (BOUND_HELD, "held"), (BOUND_HELD_P90, "held_p90"), (BOUND_TX_CROSS, "tx_cross"),
                       (BOUND_LV_CROSS, "lv_cross")):
        assert abs(bound - _bound(MEASURED[key])) < 1e-9, key
