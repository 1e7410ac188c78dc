"""CPU suite: exact multi-view visibility -- what the NumPy restatement (tests/visib_ref.py) gives on the hand cases and on the
nested spheres of DESIGN.md 24, the stated properties (face order, corner rotation, view order, and the two forms of the key
image), its calibration on the filtered ring-6 surface of DESIGN.md 15 raw and filled, and parameter validation of the device
stage (sfmx_visib_check_params needs no device).

Bounds (the rule of DESIGN.md 14 / 20 - 22): for a share, 1.25 x the distance to 100 % that the restatement gives on the fixture,
rounded up to half a percentage point; for back_pixels / hits, 1.25 x the measured share rounded up to 0.05 percentage points.
DESIGN.md 24 has the table.  The integer columns are stated exactly: the restatement is deterministic."""
import importlib

import numpy as np
import pytest

import consist_ref as CR
import fill_ref as FLR
import fusion_ref as FR
import helpers as H
import raster_ref as R
import smooth_ref as MR
import stereo_ref as SR
import visib_ref as VR

capi = importlib.import_module(H.PKG_NAME + ".capi")
synth = importlib.import_module(H.PKG_NAME + ".synth")

# ring-6, filter on, depth_tol = the voxel, min_views 1, the six left rectified cameras at 320 x 240; the first ring camera renders:
# (n, m) -> (n', m'), (faces_seen, faces_back_only, faces_unseen), outward share before, after -> bound, back_pixels / hits before,
# after -> bound
RING = {
    "raw": ((7552, 13622), (7495, 13271), (13271, 272, 79), 0.9769, 0.975, (63, 22380), (21, 22349), 0.0015),      # 98.29 %, 0.094 %
    "filled": ((7602, 14088), (7542, 13595), (13595, 388, 105), 0.9656, 0.970, (130, 23094), (28, 23047), 0.0020),  # 97.90 %, 0.122 %
}


@pytest.fixture(scope="module")
def spheres():
    v, f, nrm, no, mo = VR.nested_spheres()
    return dict(v=v, f=f, nrm=nrm, no=no, mo=mo, cams=VR.six_cameras())


def _hand(name, **kw):
    c = VR.hand_cases()[name]
    return VR.run(c["verts"], c["faces"], c["cams"], c["z_min"], c["depth_tol"], **kw), c


# ---- hand cases: what each one shows ---------------------------------------------------------------------------------------
def test_depth_tolerance_below_at_and_above():
    for name, far_visible in (("gap-below", 1), ("gap-at", 1), ("gap-ulp-above", 0)):
        r, c = _hand(name)
        assert c["depth_tol"] == 0.25 and c["verts"][0, 2] == 1.0
        assert r["vert_views"].tolist() == [1] * 4 + [far_visible] * 4, name
        assert r["face_views"].tolist() == [1, 1] + [far_visible] * 2 and r["pairs_occluded"] == 4 * (1 - far_visible), name
    assert VR.hand_cases()["gap-ulp-above"]["verts"][4, 2] == np.nextafter(1.25, 2.0), "q2 <= D + depth_tol: 1 + 0.25, one addition"


def test_half_pixel_goes_up_and_minus_half_is_pixel_zero():
    r, c = _hand("half-pixel")
    # the two vertices on x + 1/2 and y + 1/2 at depth 3 are seen at pixel (5, 5), where the plane is behind them; at (4, 5) or
    # (5, 4) it is in front
    assert r["vert_views"][4:7].tolist() == [1, 1, 1] and r["face_views"][2] == 1
    keys = VR.key_image(c["verts"], c["faces"].astype(np.int64), c["cams"][0], c["z_min"])[1]
    D = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert D[5, 5] >= 3.0 > D[5, 4] and D[4, 5] < 3.0
    assert r["vert_views"][7:].tolist() == [1, 1, 0] and r["pairs_off"] == 1, "(-0.5, 3) and (3, -0.5) are pixels 0; (7.5, 7.5) is off an 8 x 8 image"


def test_empty_pixels_borders_and_classes():
    r, _ = _hand("empty-pixel")
    assert r["vert_views"].tolist() == [1, 1, 1] and r["face_views"].tolist() == [0, 1] and r["face_back_views"].tolist() == [1, 0]
    assert (r["faces_seen"], r["faces_back_only"], r["faces_unseen"]) == (1, 1, 0)
    r, _ = _hand("off-borders")
    assert r["vert_views"].tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 1] and r["pairs_off"] == 4 and r["pairs_occluded"] == 0
    assert r["face_views"].tolist() == [1, 0, 0, 0, 0, 0, 0] and r["faces_kept"] == 1 and r["verts_kept"] == 3
    r, _ = _hand("z-min")
    assert r["vert_views"].tolist() == [1, 1, 1, 0, 1, 1] and r["face_views"].tolist() == [1, 0], "a vertex at z_min counts, one ulp below does not"
    r, _ = _hand("non-finite")
    assert r["vert_views"].tolist() == [1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0] and r["pairs_off"] == 3 and r["faces_seen"] == 1
    r, _ = _hand("no-centre")
    assert r["face_views"].tolist() == [1, 1, 1, 1], "a face that owns no pixel centre is seen through its corners"
    r, _ = _hand("collinear")
    assert r["vert_views"].min() == 1 and r["faces_unseen"] == 4 and r["faces_kept"] == 0 and r["verts_kept"] == 0, "A = 0: neither"
    r, _ = _hand("back-before-front")
    assert r["face_back_views"].tolist() == [1, 0] and r["face_views"].tolist() == [0, 0] and r["pairs_occluded"] == 3, "back faces occlude too"
    r, _ = _hand("two-views")
    assert r["face_views"].tolist() == [1, 1] and r["face_back_views"].tolist() == [1, 1] and r["vert_views"].tolist() == [2] * 4


def test_empty_inputs_and_min_views():
    for mv in (0, 1):
        r, c = _hand("no-faces", min_views=mv)
        assert r["faces"].shape == (0, 3) and r["verts"].shape == (0, 3) and r["vert_views"].tolist() == [1, 1, 0]
        r, c = _hand("no-verts", min_views=mv)
        assert VR.counts(r) == dict.fromkeys(VR.COUNTS, 0) and r["vert_views"].shape == (0,)
        c = VR.hand_cases()["two-views"]
        r = VR.run(c["verts"], c["faces"], [], c["z_min"], c["depth_tol"], min_views=mv)  # V = 0
        assert r["faces_unseen"] == 2 and r["faces_kept"] == (2 if mv == 0 else 0) and r["pairs_visible"] + r["pairs_off"] == 0
    r0 = _hand("two-views", min_views=0)[0]
    assert r0["verts"].tobytes() == VR.hand_cases()["two-views"]["verts"].tobytes(), "min_views 0 keeps everything and only measures"
    assert [_hand("two-views", min_views=k)[0]["faces_kept"] for k in (1, 2, 3)] == [2, 0, 0]
    with pytest.raises(ValueError):
        VR.run(np.zeros((2, 3)), [[0, 1, 2]], [], 1.0, 0.1)


def test_every_hand_case_both_forms_and_grey():
    for name, c in VR.hand_cases().items():
        n = len(c["verts"])
        nrm = np.random.default_rng(len(name)).standard_normal((n, 3))
        img = VR.images_for(c["cams"], 3)
        for kw in (dict(), dict(normals=nrm, images=img), dict(normals=nrm, images=img, cull=0, fill=9), dict(images=img, cull=0, min_views=0)):
            a = VR.run(c["verts"], c["faces"], c["cams"], c["z_min"], c["depth_tol"], **kw)
            b = VR.run(c["verts"], c["faces"], c["cams"], c["z_min"], c["depth_tol"], brute=True, **kw)
            VR.same(a, b, name)
            assert a["pairs_visible"] + a["pairs_occluded"] + a["pairs_off"] == n * len(c["cams"])
            if "grey" in a:
                assert (a["grey_views"] <= a["vert_views"]).all() and (a["grey"][a["grey_views"] == 0] == kw.get("fill", 0)).all()
                if kw.get("cull", 1) == 0:
                    assert (a["grey_views"] == a["vert_views"]).all()


def test_grey_is_the_rounded_mean():
    c = VR.hand_cases()["two-views"]
    img = [np.full((8, 8), 10, np.uint8), np.full((9, 5), 13, np.uint8)]
    r = VR.run(c["verts"], c["faces"], c["cams"], c["z_min"], c["depth_tol"], images=img, cull=0)
    assert r["grey"].tolist() == [12] * 4 and r["grey_views"].tolist() == [2] * 4, "(2 * 23 + 2) / 4 = 12: halves round up"
    nrm = np.tile([0.0, 0.0, -1.0], (4, 1))  # towards the first camera only
    r = VR.run(c["verts"], c["faces"], c["cams"], c["z_min"], c["depth_tol"], normals=nrm, images=img, cull=1)
    assert r["grey"].tolist() == [10] * 4 and r["grey_views"].tolist() == [1] * 4 and r["vert_views"].tolist() == [2] * 4


# ---- the nested spheres -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [0.002, 0.004])
def test_nested_spheres_culling_returns_the_outer_sphere(spheres, tol):
    s = spheres
    r = VR.run(s["v"], s["f"], s["cams"], VR.Z_MIN, tol, normals=s["nrm"])
    fv, fb, vv = r["face_views"], r["face_back_views"], r["vert_views"]
    assert (fv[:s["mo"]] >= 1).all() and (fb[:s["mo"]] == 0).all(), "every outer face is seen, none from behind"
    assert (fv[s["mo"]:] == 0).all() and (fb[s["mo"]:] == 0).all() and (vv[s["no"]:] == 0).all(), "nothing of the inner sphere is"
    assert r["verts"].tobytes() == s["v"][:s["no"]].tobytes() and r["faces"].tobytes() == s["f"][:s["mo"]].tobytes()
    assert r["normals"].tobytes() == s["nrm"][:s["no"]].tobytes()
    assert (r["vert_src"] == np.arange(s["no"])).all() and (r["face_src"] == np.arange(s["mo"])).all()
    assert (r["faces_seen"], r["faces_back_only"], r["faces_unseen"]) == (1280, 0, 320) and r["pairs_off"] == 0


def test_nested_spheres_a_tolerance_below_the_depth_slope(spheres):
    s = spheres
    r = VR.run(s["v"], s["f"], s["cams"], VR.Z_MIN, 0.0005)
    assert int((r["face_views"][:s["mo"]] == 0).sum()) == 152, "the grazing faces: the tolerance has to cover the depth slope inside a pixel"
    assert (r["face_views"][s["mo"]:] == 0).all()


def test_flipped_patch_and_inside_camera(spheres):
    v, f, _ = VR.flipped_patch(40)
    r = VR.run(v, f, spheres["cams"], VR.Z_MIN, 0.002)
    assert np.nonzero(r["face_views"] == 0)[0].tolist() == list(range(40)) and (r["face_back_views"][:40] >= 1).all()
    assert (r["faces_seen"], r["faces_back_only"], r["faces_unseen"]) == (1240, 40, 0) and (r["face_src"] == np.arange(40, 1280)).all()
    r = VR.run(spheres["v"], spheres["f"], [VR.inside_camera()], VR.Z_MIN, 0.002)
    assert (r["faces_seen"], r["faces_back_only"], r["faces_kept"]) == (0, 10, 0)


# ---- properties ------------------------------------------------------------------------------------------------------------
def test_face_order_corner_rotation_and_view_order(spheres):
    s = spheres
    img = VR.images_for(s["cams"], 1)
    for v, f, nrm in ((s["v"], s["f"], s["nrm"]), VR.soup(120)):
        cams = s["cams"] if v is s["v"] else VR.mixed_views()[1:5]
        im = img if v is s["v"] else VR.images_for(cams, 2)
        z, tol = (VR.Z_MIN, 0.002) if v is s["v"] else (0.5, 0.5)
        a = VR.run(v, f, cams, z, tol, normals=nrm, images=im, min_views=0)
        fp, perm = R.permute_faces(f, 4)
        b = VR.run(v, fp, cams, z, tol, normals=nrm, images=im, min_views=0)
        assert (b["face_views"] == a["face_views"][perm]).all() and (b["face_back_views"] == a["face_back_views"][perm]).all()
        for k in ("vert_views", "grey", "grey_views"):
            assert b[k].tobytes() == a[k].tobytes(), k
        assert VR.counts(a) == VR.counts(b)
        VR.same(VR.run(v, R.rotate_corners(f, 5), cams, z, tol, normals=nrm, images=im, min_views=0), {**a, "faces": R.rotate_corners(f, 5)}, "rotated")
        order = np.random.default_rng(6).permutation(len(cams))
        VR.same(VR.run(v, f, [cams[i] for i in order], z, tol, normals=nrm, images=[im[i] for i in order], min_views=0), a, "views permuted")


# ---- calibration --------------------------------------------------------------------------------------------
def test_ring6_calibration():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    views = []
    for a, b in pairs:
        r = SR.rectify(K, poses[a][0], poses[a][1], poses[b][0], poses[b][1])
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        views.append((r, SR.disparity(il, ir, r["H_l"], r["H_r"], dict(num_disparities=64))))
    vol = CR.RING6_VOL
    m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(views, CR.filter_views(views)))
    fl = FLR.fill(m["verts"], m["faces"], max_edges=32, unit=vol["voxel"], origin=vol["origin"])
    cams = [dict(R_rw=r["R_rw"], c_left=r["c_left"], f=r["f"], cx=r["cx"], cy=r["cy"], B=r["B"], w=320, h=240) for r, _ in views]
    first = dict(R_rw=poses[0][0].T, c_left=poses[0][1], f=K[0, 0], cx=K[0, 2], cy=K[1, 2], w=320, h=240)
    for name, (v, f) in (("raw", (m["verts"], m["faces"])), ("filled", (fl["verts"], fl["faces"]))):
        sizes, sizes_out, classes, out0, b_out, back0, back1, b_back = RING[name]
        r = VR.run(v, f, cams, 0.05, vol["voxel"])
        before, after = R.render(v, f, first, 0.05), R.render(r["verts"], r["faces"], first, 0.05)
        o0, o1 = MR.outward_share(v, f), MR.outward_share(r["verts"], r["faces"])
        print("%s: %d v / %d f -> %d / %d, %s; outward %.4f -> %.4f; back_pixels / hits %d / %d -> %d / %d"
              % (name, len(v), len(f), len(r["verts"]), len(r["faces"]), VR.counts(r), o0, o1, before["back_pixels"], before["hits"],
                 after["back_pixels"], after["hits"]))
        assert (len(v), len(f)) == sizes and (len(r["verts"]), len(r["faces"])) == sizes_out
        assert (r["faces_seen"], r["faces_back_only"], r["faces_unseen"]) == classes and r["pairs_off"] == 0
        assert (before["back_pixels"], before["hits"]) == back0 and (after["back_pixels"], after["hits"]) == back1
        assert abs(o0 - out0) < 5e-5 and o1 > o0, "the condition: culling raises the outward share"
        assert o1 >= b_out and after["back_pixels"] / after["hits"] <= b_back < before["back_pixels"] / before["hits"]
        assert CR.mesh_quality(r["verts"], r["faces"])[1] == 1.0, "vertices are copied: they stay in the shell"


def test_ring6_bounds_follow_the_rule():
    for name, measured_out, measured_back in (("raw", 0.9829, 21 / 22349), ("filled", 0.9790, 28 / 23047)):
        b_out, b_back = RING[name][4], RING[name][7]
        assert b_out == 1.0 - np.ceil(1.25 * (1.0 - measured_out) / 0.005 - 1e-9) * 0.005, name
        assert abs(b_back - np.ceil(1.25 * measured_back / 0.0005 - 1e-9) * 0.0005) < 1e-12, name


# ---- library and Python layer ----------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.visib_default_params() == dict(z_min=0.0, depth_tol=0.0, **capi.VISIB_DEFAULTS)
    assert capi.VISIB_DEFAULTS == VR.DEFAULTS and capi.VISIB_COUNTS == VR.COUNTS
    assert not capi.visib_check_params(**capi.visib_default_params()), "z_min has no default"
    assert not capi.visib_check_params() and not VR.check_params()
    for good in VR.GOOD_PARAMS:
        assert capi.visib_check_params(**good) and VR.check_params(**good), good
    for bad in VR.BAD_PARAMS:
        assert not capi.visib_check_params(**bad) and not VR.check_params(**bad), bad
    with pytest.raises(TypeError):
        capi.visib_params(1.0, 0.1, background=2)
    with pytest.raises(TypeError):
        capi.visib_params(1.0, 0.1, min_views=1.5)
    lib = capi.load_library()
    assert lib.sfmx_visib_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_visib_default_params(None)  # tolerated
    for s in capi.SYMBOLS:
        if s.startswith("sfmx_visib_"):
            assert hasattr(lib, s), s
    assert sum(s.startswith("sfmx_visib_") for s in capi.SYMBOLS) == 17
    assert lib.sfmx_visib_sizes(None, None, None, None, None) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_visib_counts(None, None, None) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_visib_device_mesh(None, None, None, None, None) == -1 and lib.sfmx_visib_device_surface(None, None, None) == -1
    assert lib.sfmx_visib_view_count(None) == 0 and lib.sfmx_visib_set_batch(None, 1) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_visib_last_batch(None) == 0 and capi.VISIB_MAX_BATCH == 64
    assert hasattr(capi.Context, "visib") and all(hasattr(capi.Visib, k) for k in ("add_view", "set_batch", "run", "read", "device_mesh"))


def test_python_layer_key_checks():
    import inspect
    pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
    assert set(pipe.VISIBILITY_KEYS) == {"z_min", "depth_tol", "min_views", "colour", "cull", "fill"}
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    # refused before any device call: the context is None
    for bad in (True, dict(depth_tol=0.1), dict(z_min=0.05, views=2), dict(z_min=0.05, background=1), dict(z_min=0.05, colour=True),
                dict(z_min=0.05, min_views=1.5)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, visibility=bad)
    assert inspect.signature(pipe.fuse).parameters["visibility"].default is False
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_vs") and hasattr(lib, "sfmx_host_visib_free")
    lib.sfmx_host_visib_free(None)  # tolerated


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
  sfmx_visib_request vq{};
  vq.params = sfmx_visib_params{0.1, 0.0, 1, 1, 0};
  const int with = sfmx_host_fusion_mesh_vs(ctx, nullptr, 0, 0, 16, 16, K, nullptr, nullptr, 0, &sp, &fp, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, &vq, &res, nullptr, nullptr, 0);
  std::printf("%d\n", with);
  sfmx_ctx_destroy(ctx);
  return 0;
}
"""


def test_stand_in_library_reports_unsupported(tmp_path):
    """the host layer on the CPU stand-in of libsfmx.so (tests/fake_sfmx), which has no device stage: it links untouched, because
    the device entries are weak references, and a visibility request says SFMX_ERR_UNSUPPORTED"""
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
    assert int(p.stdout.strip()) == capi.SFMX_ERR_UNSUPPORTED
