"""CPU suite: the best-view per-face texture atlas -- what the NumPy restatement (tests/texture_ref.py) gives: the layout (the two
halves tile a cell, the gutter, the corners), the best-view rule, an affine image on a fronto-parallel face, the proposition that
visibility culling leaves nothing untextured, the size refusals, parameter validation of the device stage
(sfmx_texture_check_params needs no device), the BMP and OBJ writers, and the fidelity calibration on the textured sphere.

Fidelity bounds (the rule of DESIGN.md 15): 1.25 x what the restatement gives on the fixture, rounded up to 0.1 grey level.
DESIGN.md 25 has the table."""
import importlib
import struct

import numpy as np
import pytest

import helpers as H
import raster_ref as R
import texture_ref as TR
import visib_ref as VR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")

# the textured sphere (texture_ref.FIDELITY): measured mean and 99th percentile of |texel - T|, and the mean of |vertex grey - T|
MEASURED = dict(mean=0.2792, p99=0.7611, vertex_mean=5.0416)
BOUND_MEAN, BOUND_P99 = 0.4, 1.0  # 1.25 x 0.2792 = 0.349 and 1.25 x 0.7611 = 0.951, rounded up to 0.1 grey level


def _bound(x):
    return np.ceil(1.25 * x / 0.1 - 1e-9) * 0.1


# ---- layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", range(3, 65))
def test_the_two_halves_tile_the_cell_and_the_corners_are_texel_centres(S):
    L = S - 2
    i, j = TR.half_texels(S)
    seen = np.zeros((S, S + 1), int)
    for half in (0, 1):
        x, y = TR.half_local(S, half, i, j)
        seen[y, x] += 1
        a, b, c = TR.corners_half(S, half)
        # the corner combination with weights (L - i - j, i, j) / L is the centre (2 x + 1, 2 y + 1) of the texel, in half-texels
        inner = i + j <= L
        cx = ((L - i - j) * a[0] + i * b[0] + j * c[0])[inner]
        cy = ((L - i - j) * a[1] + i * b[1] + j * c[1])[inner]
        assert (cx == L * (2 * x[inner] + 1)).all() and (cy == L * (2 * y[inner] + 1)).all()
    assert (seen == 1).all()
    i2, j2 = TR.gutter(S, i, j)
    inner = i + j <= L
    assert (i2 + j2 <= L).all() and (i2[inner] == i[inner]).all() and (j2[inner] == j[inner]).all()
    g = ~inner
    assert (i[g] + j[g] == S - 1).all() and (i2[g] + j2[g] == L).all(), "a gutter texel samples on the hypotenuse"


def test_layout_counts_sizes_and_refusals():
    assert TR.layout(0, 0) == dict(cells=0, cells_per_row=1, W=0, H=0)
    assert TR.layout(0, 5) == dict(cells=1, cells_per_row=1, W=9, H=8)
    assert TR.layout(3, 0) == dict(cells=2, cells_per_row=2, W=18, H=8)
    assert TR.layout(3, 1) == dict(cells=3, cells_per_row=2, W=18, H=16)
    assert TR.layout(9, 1, 3, 4) == dict(cells=6, cells_per_row=4, W=16, H=6)
    assert TR.layout(2 * 1820 ** 2 + 2, 0)["cells_per_row"] == 1820, "the automatic row length is capped at floor(16384 / 9)"
    assert TR.layout(10, 0, 8, 1820)["W"] == 16380
    for bad in ((10, 0, 8, 1821), (2 * 64528, 0, 64, 1), (2 * 64527, 1, 64, 1)):
        with pytest.raises(ValueError):
            TR.layout(*bad)
    assert TR.layout(2 * 64527, 0, 64, 1)["H"] == 64527 * 64


# ---- best view ---------------------------------------------------------------------------------------------------------------
def _three():
    uv = [(1.2, 1.1), (1.6, 7.3), (6.4, 2.2), (5.0, 3.0), (5.5, 8.5), (10.5, 4.0), (2.0, 6.0), (3.0, 9.0), (7.0, 8.0)]
    return R.at_pixels(uv, [1.0 + 0.125 * k for k in range(9)]), np.arange(9, dtype=np.int32).reshape(3, 3)


def _img(w, h, seed=0):
    y, x = np.mgrid[0:h, 0:w]
    return ((7 * x + 13 * y + np.random.default_rng(seed).integers(0, 40, (h, w))) % 256).astype(np.uint8)


def test_best_view_area_ties_and_view_order():
    v, f = _three()
    a, b, big = R.pixel_camera(12, 10), R.pixel_camera(12, 10), R.pixel_camera(24, 20, f=512.0)
    ia, ib, ibig = _img(12, 10, 1), _img(12, 10, 2), _img(24, 20, 3)
    r = TR.run(v, f, [a, big, b], [ia, ibig, ib], 0.5, 2.0)
    one = TR.run(v, f, [a], [ia], 0.5, 2.0)
    assert r["face_view"].tolist() == [1, 1, 1] and (r["face_area"] > 3 * one["face_area"]).all() and r["view_faces"].tolist() == [0, 3, 0]
    assert TR.run(v, f, [a, b], [ia, ib], 0.5, 2.0)["face_view"].tolist() == [0, 0, 0], "a tie goes to the smaller index"
    assert TR.run(v, f, [b, a], [ib, ia], 0.5, 2.0)["atlas"].tobytes() == TR.run(v, f, [b], [ib], 0.5, 2.0)["atlas"].tobytes()
    # no ties on the sphere under six cameras at different distances: permuting the views maps face_view through the permutation
    sv, sf, _, _, _ = VR.nested_spheres()
    cams = [dict(c, f=300.0 + 7.0 * k) for k, c in enumerate(VR.six_cameras())]
    img = VR.images_for(cams, 1)
    base = TR.run(sv, sf, cams, img, VR.Z_MIN, 0.002)
    order = np.random.default_rng(6).permutation(6)
    got = TR.run(sv, sf, [cams[i] for i in order], [img[i] for i in order], VR.Z_MIN, 0.002)
    tex = base["face_view"] >= 0
    assert ((got["face_view"] >= 0) == tex).all() and (order[got["face_view"][tex]] == base["face_view"][tex]).all()
    assert got["face_area"].tobytes() == base["face_area"].tobytes() and got["atlas"].tobytes() == base["atlas"].tobytes()


def test_an_affine_image_on_a_fronto_parallel_face():
    w, h = 40, 30
    y, x = np.mgrid[0:h, 0:w]
    img = (10 + 3 * x + 2 * y).astype(np.uint8)
    cam = R.pixel_camera(w, h)
    v = R.at_pixels([(3.3, 2.1), (5.9, 26.2), (36.4, 4.7)], 2.0)
    f = np.array([[0, 1, 2]], np.int32)
    for S in (3, 8, 64):
        r = TR.run(v, f, [cam], [img], 0.5, 0.25, patch=S)
        assert r["faces_textured"] == 1
        face, i, j = TR.texel_map(r["face_view"], {k: r[k] for k in ("cells", "cells_per_row", "W", "H")}, S)
        sel = np.nonzero(face >= 0)[0]
        X = TR.texel_points(v, f.astype(np.int64), face[sel], i[sel], j[sel], S)
        u, vv = 256.0 * X[0] / X[2], 256.0 * X[1] / X[2]
        want = 10.0 + 3.0 * u + 2.0 * vv
        assert np.abs(r["atlas"].ravel()[sel].astype(np.float64) - want).max() <= 0.5 + 1e-9
        assert len(sel) == S * (S + 1) // 2 and (r["atlas"].ravel()[face < 0] == 0).all()


# ---- the proposition ---------------------------------------------------------------------------------------------------------
def test_after_visibility_culling_every_face_is_textured():
    """removing faces only raises z-buffer keys, so a face that was seen stays seen: after visib_ref.run(min_views >= 1) with the same
    cameras, z_min and depth_tol nothing is untextured"""
    v, f, _, no, mo = VR.nested_spheres()
    cams = VR.six_cameras()
    img = VR.images_for(cams, 1)
    before = TR.run(v, f, cams, img, VR.Z_MIN, 0.002)
    assert before["faces_untextured"] == len(f) - mo
    for mv in (1, 2):
        c = VR.run(v, f, cams, VR.Z_MIN, 0.002, min_views=mv)
        after = TR.run(c["verts"], c["faces"], cams, img, VR.Z_MIN, 0.002)
        assert after["faces_untextured"] == 0 and after["faces_textured"] == c["faces_kept"] > 0
    sv, sf, _ = VR.soup(300, 5)
    cams = [R.pixel_camera(24, 20), R.pixel_camera(24, 20, f=200.0, cx=3.0)]
    img = VR.images_for(cams, 2)
    c = VR.run(sv, sf, cams, 0.5, 0.5)
    after = TR.run(c["verts"], c["faces"], cams, img, 0.5, 0.5)
    assert 0 < c["faces_kept"] < len(sf) and after["faces_untextured"] == 0


def test_after_visibility_culling_every_face_is_textured_ring2():
    """the same on the fused surface of two pairs of the ring-6 fixture with the pairs' left rectified cameras"""
    import consist_ref as CR
    import fusion_ref as FR
    import stereo_ref as SR
    synth = importlib.import_module(H.PKG_NAME + ".synth")
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    views = []
    for a, b in pairs[:2]:
        r = SR.rectify(K, poses[a][0], poses[a][1], poses[b][0], poses[b][1])
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        views.append((r, SR.disparity(il, ir, r["H_l"], r["H_r"], dict(num_disparities=64))))
    vol = CR.RING6_VOL
    m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], views)
    cams = [dict(R_rw=r["R_rw"], c_left=r["c_left"], f=r["f"], cx=r["cx"], cy=r["cy"], B=r["B"], w=320, h=240) for r, _ in views]
    img = VR.images_for(cams, 3)
    c = VR.run(m["verts"], m["faces"], cams, 0.05, vol["voxel"])
    before = TR.run(m["verts"], m["faces"], cams, img, 0.05, vol["voxel"])
    after = TR.run(c["verts"], c["faces"], cams, img, 0.05, vol["voxel"])
    print("ring-2: %d faces, %d untextured; culled to %d, %d untextured" % (len(m["faces"]), before["faces_untextured"], c["faces_kept"],
                                                                            after["faces_untextured"]))
    assert before["faces_untextured"] == len(m["faces"]) - c["faces_kept"] > 0 and after["faces_untextured"] == 0


# ---- library and Python layer ------------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.texture_default_params() == dict(z_min=0.0, depth_tol=0.0, **capi.TEXTURE_DEFAULTS)
    assert capi.TEXTURE_DEFAULTS == TR.DEFAULTS and capi.TEXTURE_COUNTS == TR.COUNTS
    assert not capi.texture_check_params(**capi.texture_default_params()), "z_min has no default"
    assert not capi.texture_check_params() and not TR.check_params()
    for good in TR.GOOD_PARAMS:
        assert capi.texture_check_params(**good) and TR.check_params(**good), good
    for bad in TR.BAD_PARAMS:
        assert not capi.texture_check_params(**bad) and not TR.check_params(**bad), bad
    for patch, ok in ((2, False), (3, True), (64, True), (65, False)):
        assert capi.texture_check_params(1.0, 0.1, patch=patch) == ok == TR.check_params(1.0, 0.1, patch=patch)
    with pytest.raises(TypeError):
        capi.texture_params(1.0, 0.1, background=2)
    with pytest.raises(TypeError):
        capi.texture_params(1.0, 0.1, patch=7.5)
    lib = capi.load_library()
    assert lib.sfmx_texture_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_texture_default_params(None)  # tolerated
    assert sum(s.startswith("sfmx_texture_") for s in capi.SYMBOLS) == 17
    assert lib.sfmx_texture_sizes(None, None, None, None, None, None) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_texture_counts(None, None) == capi.SFMX_ERR_INVALID and lib.sfmx_texture_device_atlas(None, None, None, None) == -1
    assert lib.sfmx_texture_view_count(None) == 0 and lib.sfmx_texture_set_batch(None, 1) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_texture_last_batch(None) == 0 and lib.sfmx_texture_last_us(None) == 0.0
    assert hasattr(capi.Context, "texture") and all(hasattr(capi.Texture, k) for k in ("add_view", "add_stereo_view", "set_batch", "run", "read"))


def test_python_layer_key_checks():
    import inspect
    assert set(pipe.TEXTURE_KEYS) == {"z_min", "depth_tol", "patch", "cells_per_row", "fill", "obj_path"}
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    for bad in (True, dict(depth_tol=0.1), dict(z_min=0.05, views=2), dict(z_min=0.05, min_views=1), dict(z_min=0.05, patch=7.5)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, texture=bad)  # refused before any device call: the context is None
    assert inspect.signature(pipe.fuse).parameters["texture"].default is False
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_tx") and hasattr(lib, "sfmx_host_texture_free")
    lib.sfmx_host_texture_free(None)  # tolerated


def test_write_bmp_parsed_back(tmp_path):
    for w, h in ((1, 1), (5, 3), (8, 2), (18, 16)):
        img = np.random.default_rng(w).integers(0, 256, (h, w)).astype(np.uint8)
        p = str(tmp_path / f"a{w}.bmp")
        pipe.write_bmp(p, img)
        b = open(p, "rb").read()
        magic, size, _, _, off = struct.unpack("<2sIHHI", b[:14])
        hs, bw, bh, planes, bpp, comp, isz, _, _, used, _ = struct.unpack("<IiiHHIIiiII", b[14:54])
        stride = (w + 3) & ~3
        assert (magic, size, off, hs, bw, bh, planes, bpp, comp, isz, used) == (b"BM", len(b), 1078, 40, w, h, 1, 8, 0, stride * h, 256)
        pal = np.frombuffer(b[54:1078], np.uint8).reshape(256, 4)
        assert (pal[:, :3] == np.arange(256)[:, None]).all() and (pal[:, 3] == 0).all()
        rows = np.frombuffer(b[off:], np.uint8).reshape(h, stride)
        assert (rows[::-1, :w] == img).all() and (rows[:, w:] == 0).all()


def test_the_obj_and_its_companions(tmp_path):
    v, f = _three()
    r = TR.run(v, f, [R.pixel_camera(12, 10)], [_img(12, 10)], 0.5, 2.0)
    uv = TR.uv(r["uv_half"], r["W"], r["H"])
    pipe.write_textured_obj(str(tmp_path / "mesh.obj"), v, f, uv, r["atlas"])
    lines = open(tmp_path / "mesh.obj").read().splitlines()
    kinds = [ln.split()[0] for ln in lines]
    assert kinds.count("v") == 9 and kinds.count("vt") == 9 and kinds.count("f") == 3 and lines[0] == "mtllib mesh.mtl"
    assert [float(x) for x in lines[2].split()[1:]] == v[0].tolist(), "%.17g round-trips a double"
    assert lines[-1] == "f 7/7 8/8 9/9" and [float(x) for x in lines[2 + 9].split()[1:]] == uv[0, 0].tolist()
    assert "map_Kd mesh_atlas.bmp" in open(tmp_path / "mesh.mtl").read()
    assert open(tmp_path / "mesh_atlas.pgm", "rb").read() == b"P5\n%d %d\n255\n" % (r["W"], r["H"]) + r["atlas"].tobytes()
    assert (uv >= 0).all() and (uv <= 1).all()


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
  sfmx_texture_request xq{};
  xq.params = sfmx_texture_params{0.1, 0.0, 8, 0, 0};
  const int with = sfmx_host_fusion_mesh_tx(ctx, nullptr, 0, 0, 16, 16, K, nullptr, nullptr, 0, &sp, &fp, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, &xq, &res, nullptr, nullptr, 0);
  std::printf("%d\n", with);
  sfmx_ctx_destroy(ctx);
  return 0;
}
"""


def test_stand_in_library_reports_unsupported(tmp_path):
    """the host layer on the CPU stand-in of libsfmx.so (tests/fake_sfmx), which has no texture stage: it links untouched, because
    the device entries are weak references, and a texture request says SFMX_ERR_UNSUPPORTED"""
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


# ---- fidelity calibration ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    v, f, cams, img = TR.fidelity_scene()
    res = TR.run(v, f, cams, img, TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"], patch=TR.FIDELITY["patch"])
    grey = VR.run(v, f, cams, TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"], normals=v / np.linalg.norm(v, axis=1)[:, None], images=img,
                  min_views=0)["grey"]
    return v, f, res, grey


def test_fidelity_on_the_textured_sphere(sphere):
    v, f, res, grey = sphere
    mean, p99, vmean = TR.fidelity(v, f, res, TR.FIDELITY["patch"], grey)
    print("textured sphere: %d faces textured of %d, atlas %d x %d; |texel - T| mean %.4f, p99 %.4f; |vertex grey - T| mean %.4f"
          % (res["faces_textured"], len(f), res["W"], res["H"], mean, p99, vmean))
    assert res["faces_untextured"] == 0
    assert mean <= BOUND_MEAN and p99 <= BOUND_P99
    assert mean < vmean, "the point of the feature: the atlas is closer to the pattern than the vertex grey of the same mesh"


def test_fidelity_bounds_follow_the_rule():
    assert abs(BOUND_MEAN - _bound(MEASURED["mean"])) < 1e-9 and abs(BOUND_P99 - _bound(MEASURED["p99"])) < 1e-9
