"""CPU suite: the exact z-buffer -- the NumPy restatement (tests/raster_ref.py) against itself (every face against every pixel
against the faces' boxes), the coverage rules on the hand cases, the stated properties (face order, corner rotation, closed
meshes), its calibration on a level-4 icosphere and on the fused sphere against the ray-cast volume, and the device stage's
parameter validation, Python key checks and exported symbols (none needs a device).

Bounds (the rule of DESIGN.md 14): 1.25 x the value the restatement gives on the fixture, rounded up to 0.5 as DESIGN.md 18 rounds;
DESIGN.md 23 has the table.  The integer columns of the icosphere are stated exactly."""
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import fusion_ref as FR
import helpers as H
import raster_ref as R
import raycast_ref as RR
import sdist_ref as DR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")


def _both(v, f, cam, z_min, normals=None, grey=None, **kw):
    a = R.brute(v, f, cam, z_min, normals, grey, **kw)
    b = R.render(v, f, cam, z_min, normals, grey, **kw)
    R.same(a, b, str(kw))
    assert a["keys"].tobytes() == b["keys"].tobytes()
    return a


# ---- the two forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.hand_cases()))
def test_forms_agree_on_the_hand_cases(name):
    c = R.hand_cases()[name]
    rng = np.random.default_rng(len(name))
    nrm, grey = rng.standard_normal(c["verts"].shape), rng.integers(0, 256, len(c["verts"])).astype(np.uint8)
    for cull in (0, 1, 2):
        _both(c["verts"], c["faces"], R.hand_camera(c), c["z_min"], cull=cull)
        _both(c["verts"], c["faces"], R.hand_camera(c), c["z_min"], nrm, grey, cull=cull, background=200)


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (7, 9), (8, 8), (17, 16), (64, 4), (4096, 1)])
def test_forms_agree_on_random_scenes(shape):
    w, h = shape
    v, f, nrm, grey = R.random_scene(w, h)
    a = _both(v, f, R.pixel_camera(w, h), 0.5, nrm, grey)
    assert a["hits"] > 0 and a["fragments"] > a["hits"]


def test_forms_agree_on_meshes():
    v, f = DR.icosphere(3, 0.1)
    for name, c in R.CALIB.items():
        a = _both(v, f, c["cam"](), R.CALIB_Z_MIN)
        assert a["back_pixels"] == 0 and a["fragments"] == 2 * a["hits"], name
    cam = RR.axis_camera((0.0, 0.0, 0.0), 40.0, 48, 32, 23.5, 15.5)
    a = _both(v, f, cam, 0.01)
    assert a["hits"] == a["back_pixels"] == 48 * 32 and a["faces_behind"] > len(f) // 3
    v, f = R.tiny_faces(3000, 32, 32)
    _both(v, f, R.pixel_camera(32, 32), 0.5)
    v, f = R.hot_pixel(2000)
    assert _both(v, f, R.pixel_camera(8, 8), 0.5)["faces_drawn"] == 2000


# ---- coverage: what the hand cases are there to show ---------------------------------------------------------------------------
def _hand(name, **kw):
    c = R.hand_cases()[name]
    return R.brute(c["verts"], c["faces"], R.hand_camera(c), c["z_min"], **kw), c


def test_top_left_rule():
    for name in ("top-left", "top-left-reversed"):
        a, _ = _hand(name)
        cov = a["face"] == 0
        # (2,2) (6,2) (2,6): the edges on y = 2 and x = 2 own their centres, the vertex (2,2) included; the slanted edge does not
        want = np.zeros((8, 8), bool)
        for y in range(2, 6):
            want[y, 2:2 + (6 - y)] = True
        want[2, 6] = False
        assert (cov == (want & (np.add.outer(np.arange(8), np.arange(8)) < 8))).all(), name
        assert cov[2, 2] and cov[2, 5] and cov[5, 2] and not cov[2, 6] and not cov[6, 2] and not cov[4, 4]
    for name in ("bottom-right", "bottom-right-reversed"):
        a, _ = _hand(name)
        cov = a["face"] == 0
        # (6,6) (2,6) (6,2): the bottom edge y = 6 and the right edge x = 6 own nothing; the slanted edge, a left edge here, does
        assert not cov[6, :].any() and not cov[:, 6].any() and cov[5, 3] and cov[3, 5] and cov[4, 4] and cov.sum() == 6
    assert _hand("top-left")[0]["faces_back"] == 1 and _hand("top-left-reversed")[0]["faces_back"] == 0


def test_shared_edges_and_the_fan():
    for name in ("shared-diagonal", "shared-antidiagonal", "shared-diagonal-mixed-winding"):
        a, c = _hand(name)
        n = R.fragments_per_pixel(c["verts"], c["faces"], R.hand_camera(c), c["z_min"])
        assert n.max() == 1 and n.sum() == a["fragments"] == a["hits"] == 36 and (n[1:7, 1:7] == 1).all(), name
    a, c = _hand("fan")
    n = R.fragments_per_pixel(c["verts"], c["faces"], R.hand_camera(c), c["z_min"])
    assert n.max() == 1 and n[4, 4] == 1 and a["fragments"] == a["hits"] and a["faces_drawn"] == 6


def test_classes():
    assert R.counts(_hand("no-centre")[0]) == dict.fromkeys(R.COUNTS + ("fragments",), 0) | dict(faces_back=1)
    a, _ = _hand("degenerate")
    assert (a["faces_degenerate"], a["faces_drawn"]) == (4, 1)
    a, _ = _hand("z-min")
    assert (a["faces_behind"], a["faces_drawn"]) == (1, 1) and (a["face"][a["face"] >= 0] == 0).all(), "exactly z_min is near"
    a, _ = _hand("band")
    assert (a["faces_outside"], a["faces_drawn"], a["hits"]) == (1, 1, 120) and (a["face"] == 0).all(), "exactly 16384 is inband"
    a, _ = _hand("non-finite")
    assert (a["faces_behind"], a["faces_outside"], a["faces_drawn"]) == (3, 0, 1)
    for name in ("no-faces", "no-faces-some-verts"):
        a, _ = _hand(name, background=7)
        assert a["hits"] == 0 and (a["face"] == -1).all() and (a["shaded"] == 7).all() and not a["depth"].any() and not a["points"].any()


def test_ties_and_culling():
    a, _ = _hand("coplanar-copies")
    assert a["fragments"] == 2 * a["hits"] and (a["face"][a["face"] >= 0] == 0).all()
    a, _ = _hand("same-float")
    assert (a["face"][a["face"] >= 0] == 0).all() and (a["depth"][a["face"] == 0] > 1.0).all(), "one float: the smaller index, though farther"
    a, _ = _hand("neighbouring-floats")
    assert (a["face"][a["face"] >= 0] == 1).all(), "neighbouring floats: the nearer"
    a0, _ = _hand("back-before-front")
    a1, _ = _hand("back-before-front", cull=1)
    a2, _ = _hand("back-before-front", cull=2)
    assert a0["back_pixels"] == 10 and (a0["face"] == 0).sum() == 10 and a0["faces_back"] == a1["faces_back"] == a2["faces_back"] == 1
    assert a1["back_pixels"] == 0 and (a1["face"] == 0).sum() == 0 and a1["hits"] == a0["hits"] and a1["faces_culled"] == 1
    assert a2["hits"] == a2["back_pixels"] == 10 and a2["faces_culled"] == 1
    assert a0["fragments"] == a1["fragments"] + a2["fragments"]


def test_box_sizes_around_the_small_path():
    """the cases the GPU suite uses at RS_SMALL - 1, RS_SMALL and RS_SMALL + 1 have boxes of exactly that many pixel centres"""
    src = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "hip", "raster.hip")).read()
    small = int(re.search(r"constexpr int RS_SMALL = (\d+);", src).group(1))
    for name, want in (("box-63", small - 1), ("box-64", small), ("box-65", small + 1)):
        c = R.hand_cases()[name]
        cam = R.hand_camera(c)
        pr = R.project(c["verts"], cam, c["z_min"])
        x0, y0, x1, y1 = R.boxes(c["faces"].astype(np.int64), np.array([0]), pr, c["w"], c["h"])
        assert int(((x1 - x0 + 1) * (y1 - y0 + 1))[0]) == want, name


# ---- the stated properties -----------------------------------------------------------------------------------------------------
def _mesh_and_attrs(level):
    v, f = DR.icosphere(level, 0.1)
    rng = np.random.default_rng(level)
    return v, f, rng.standard_normal(v.shape), rng.integers(0, 256, len(v)).astype(np.uint8)


def test_face_order_and_corner_rotation():
    v, f, nrm, grey = _mesh_and_attrs(3)
    soup = R.random_scene(40, 30, 60, seed=5)
    for (vv, ff, nn, gg), cam, z in (((v, f, nrm, grey), R.CALIB["oblique"]["cam"](), R.CALIB_Z_MIN), (soup, R.pixel_camera(40, 30), 0.5)):
        a = R.render(vv, ff, cam, z, nn, gg)
        f2, perm = R.permute_faces(ff, 1)
        b = R.render(vv, f2, cam, z, nn, gg)
        assert R.counts(a) == R.counts(b)
        assert all(a[k].tobytes() == b[k].tobytes() for k in ("depth", "points", "normals", "shaded", "grey"))
        assert (np.where(b["face"] >= 0, perm[b["face"]], -1) == a["face"]).all() and (b["face"] != a["face"]).any()
        c = R.render(vv, R.rotate_corners(ff, 2), cam, z, nn, gg)
        assert R.counts(a) == R.counts(c) and c["face"].tobytes() == a["face"].tobytes() and c["keys"].tobytes() == a["keys"].tobytes()
        # without vertex normals the face normal does not depend on the corner a face starts at, up to rounding; with them the
        # interpolation is the same sum in another order: equal to the last bits, not to the byte
        assert np.allclose(c["depth"], a["depth"], rtol=1e-12, atol=0) and np.allclose(c["normals"], a["normals"], atol=1e-9)


@pytest.mark.parametrize("name", list(R.CALIB))
def test_icosphere_calibration(name):
    """the anchor of DESIGN.md 23: hits, faces_back and the closed-mesh properties, exactly"""
    v, f, nrm, grey = _mesh_and_attrs(4)
    c = R.CALIB[name]
    cam = c["cam"]()
    a = R.render(v, f, cam, R.CALIB_Z_MIN, nrm, grey)
    assert (a["hits"], a["faces_back"], a["back_pixels"], a["fragments"]) == (c["hits"], c["faces_back"], 0, 2 * c["hits"])
    assert (a["faces_behind"], a["faces_outside"], a["faces_degenerate"]) == (0, 0, 0)
    n = R.fragments_per_pixel(v, f, cam, R.CALIB_Z_MIN)
    assert set(np.unique(n).tolist()) == {0, 2}, "a closed surface: a front and a back fragment, or none"
    one, two = R.render(v, f, cam, R.CALIB_Z_MIN, nrm, grey, cull=1), R.render(v, f, cam, R.CALIB_Z_MIN, nrm, grey, cull=2)
    assert one["fragments"] == two["fragments"] == a["fragments"] // 2
    assert all(one[k].tobytes() == a[k].tobytes() for k in R.ARRAYS + ("grey",)), "cull = 1 gives the image of cull = 0"
    assert two["back_pixels"] == two["hits"] == c["hits"] and (two["depth"][two["face"] >= 0] > a["depth"][a["face"] >= 0]).all()
    # against the analytic sphere: the chord at the silhouette (2.5 mm and 4.8 mm measured)
    dw, cc = RR.rays(cam, 160, 160), np.asarray(cam["c_left"], np.float64)
    A = sum(d * d for d in dw)
    B = 2.0 * sum(d * cc[i] for i, d in enumerate(dw))
    disc = B * B - 4.0 * A * (cc @ cc - 0.01)
    hit = a["face"] >= 0
    assert (disc[hit] > 0).all(), "the inscribed mesh lies inside the sphere's silhouette"
    zs = (-B - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * A)
    err = np.abs(a["depth"] - zs)[hit].max()
    assert err <= dict(axis=0.0032, oblique=0.0061)[name], err  # 1.25 x 2.54 mm and 4.85 mm, rounded up to 0.1 mm


# the fused sphere (26 views, 61^3 at 5 mm; 22 786 v / 45 568 f) against the ray-cast volume (raycast_ref.brute,
# DESIGN.md 18) from its two cameras: the depth difference in voxels at the pixels both hit, and the pixels only one of them hits.
# Measured with this file's own code; the bounds are 1.25 x the measured value rounded up to 0.5 (the rule of DESIGN.md 14, rounded
# as DESIGN.md 18 does).  The mesh hits a rim of pixels the rays miss: a face covers a pixel centre when the surface passes within
# the face's extent, the march needs two defined samples around the crossing.
FUSED = {
    RR.SPHERE_CAM["pos"]: dict(both=11731, max=5.0, mean=0.5, p99=0.5, mesh_only=62.5, volume_only=1.5),
    RR.CALIB_POS: dict(both=11871, max=3.5, mean=0.5, p99=0.5, mesh_only=36.5, volume_only=1.5),
}


def _bound(x):
    return np.ceil(1.25 * x / 0.5) * 0.5


def test_fused_bounds_follow_the_rule():
    """measured: depth difference in voxels max 3.61, mean 0.044, p99 0.34, 50 mesh-only and 1 volume-only pixels; and max 2.44,
    mean 0.044, p99 0.30, 29 and 1"""
    c = FUSED[RR.SPHERE_CAM["pos"]]
    assert (c["max"], c["mean"], c["p99"], c["mesh_only"], c["volume_only"]) == (_bound(3.6063), _bound(0.0445), _bound(0.3353), _bound(50), _bound(1))
    c = FUSED[RR.CALIB_POS]
    assert (c["max"], c["mean"], c["p99"], c["mesh_only"], c["volume_only"]) == (_bound(2.4419), _bound(0.0443), _bound(0.3029), _bound(29), _bound(1))


@pytest.fixture(scope="module")
def fused_sphere():
    s = RR.sphere_volume()
    v, f = FR.extract(s["sum"], s["count"], s["vol"]["origin"], s["vol"]["voxel"])
    assert (len(v), len(f)) == (22786, 45568)
    return s, v, f


@pytest.mark.parametrize("pos", list(FUSED))
def test_fused_sphere_against_the_ray_cast_volume(fused_sphere, pos):
    s, v, f = fused_sphere
    vol = s["vol"]
    cam = RR.camera(pos, (0.0, 0.0, 0.0), RR.SPHERE_CAM["f"], RR.SPHERE_CAM["w"], RR.SPHERE_CAM["h"])
    mesh = R.render(v, f, cam, RR.SPHERE_MARCH["z_min"])
    ray = RR.brute(s["sum"], s["count"], vol["origin"], vol["voxel"], cam, cam["w"], cam["h"], **RR.SPHERE_MARCH)
    mh, rh = mesh["face"] >= 0, ray["hit"]
    both = mh & rh
    d = np.abs(mesh["depth"] - ray["depth"])[both] / vol["voxel"]
    got = dict(both=int(both.sum()), max=float(d.max()), mean=float(d.mean()), p99=float(np.percentile(d, 99)),
               mesh_only=int((mh & ~rh).sum()), volume_only=int((rh & ~mh).sum()))
    print(pos, got)
    b = FUSED[pos]
    assert got["both"] == b["both"] and mesh["back_pixels"] == 0, "no inward-facing patch is visible from outside"
    assert all(got[k] <= b[k] for k in b if k != "both"), (got, b)


# ---- the library without a device ------------------------------------------------------------------------------------------------
def test_check_params_field_by_field():
    assert capi.raster_default_params() == dict(z_min=0.0, cull=0, background=0)
    assert not capi.raster_check_params(**capi.raster_default_params()), "z_min has no default"
    assert capi.RASTER_DEFAULTS == R.DEFAULTS and capi.RASTER_COUNTS == R.COUNTS
    assert (capi.RASTER_MAX_PIXELS, capi.RASTER_MAX_VERTS, capi.RASTER_MAX_FACES) == (R.WH_MAX, R.N_MAX, R.M_MAX)
    for p in R.GOOD_PARAMS:
        assert capi.raster_check_params(**p) and R.check_params(**p), p
    for p in R.BAD_PARAMS:
        assert not capi.raster_check_params(**p) and not R.check_params(**p), p
    with pytest.raises(ValueError):
        capi.raster_params(1.0, background=256)
    with pytest.raises(ValueError):
        capi.raster_params(1.0, background=-1)
    with pytest.raises(TypeError):
        capi.raster_params(1.0, cull=0.5)
    with pytest.raises(TypeError):
        capi.raster_params(1.0, z_max=2.0)
    assert capi.load_library().sfmx_raster_check_params(None) == capi.SFMX_ERR_INVALID


def test_symbols_and_python_keys():
    hdr = open(os.path.join(H.ROOT, "include", "sfmx.h")).read()
    names = set(re.findall(r"\b(sfmx_raster_[a-z_]+)\s*\(", hdr))
    assert names == {s for s in capi.SYMBOLS if s.startswith("sfmx_raster_")} and len(names) == 10
    lib = capi.load_library()
    assert all(hasattr(lib, s) for s in names)
    for m in ("render", "read", "counts", "device_surface", "last_us", "close"):
        assert callable(getattr(capi.Raster, m))
    assert "raster" in inspect.signature(pipe.fuse).parameters and inspect.signature(pipe.fuse).parameters["raster"].default is None
    assert pipe.RASTER_KEYS == ("cameras", "w", "h", "z_min", "cull", "background", "pgm_prefix")
    host = pipe.load_host_library()
    assert hasattr(host, "sfmx_host_fusion_mesh_rs") and hasattr(host, "sfmx_host_fusion_mesh_fl")


class _NoDevice:
    h_ = None


def test_fuse_refuses_bad_raster_keys_before_any_device_call():
    img = np.zeros((2, 16, 16), np.uint8)
    poses = [np.r_[np.eye(3).ravel(), 0, 0, 0], np.r_[np.eye(3).ravel(), 0.1, 0, 0]]
    cam = RR.axis_camera((0, 0, -1), 50.0, 8, 8, 3.5, 3.5)
    base = dict(cameras=[cam], w=8, h=8, z_min=0.1)

    def call(**raster):
        return pipe.fuse(_NoDevice(), img, np.eye(3), poses, [(0, 1)], (0, 0, 0), 0.1, (4, 4, 4), raster=raster)

    with pytest.raises(TypeError, match="unknown raster parameters"):
        call(**base, z_max=1.0)
    for k in base:
        with pytest.raises(TypeError, match="raster needs"):
            call(**{q: v for q, v in base.items() if q != k})
    for w, h in ((0, 8), (8, 0), (4097, 1), (4096, 4097)):
        with pytest.raises(ValueError, match="raster size"):
            call(**{**base, "w": w, "h": h})
    with pytest.raises(ValueError):
        call(**base, background=300)
    with pytest.raises(TypeError):
        call(**base, cull=1.5)


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
  sfmx_fusion_view cam{};
  sfmx_raster_out out{};
  sfmx_raster_request rq{&cam, 1, sfmx_raster_params{0.1, 0, 0}, &out};
  const int with = sfmx_host_fusion_mesh_rs(ctx, nullptr, 0, 0, 16, 16, K, nullptr, nullptr, 0, &sp, &fp, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            &rq, &res, nullptr, nullptr, 0);
  std::printf("%d\n", with);
  sfmx_ctx_destroy(ctx);
  return 0;
}
"""


def test_stand_in_library_reports_unsupported(tmp_path):
    """the host layer on the CPU stand-in of libsfmx.so (tests/fake_sfmx), which has no device stage: it links untouched, because
    the device entries are weak references, and a raster request says SFMX_ERR_UNSUPPORTED"""
    pkg = os.path.join(H.ROOT, H.PKG_NAME)
    host = os.path.join(pkg, "csrc", "host")
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
