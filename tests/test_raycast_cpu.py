"""CPU suite: TSDF ray casting -- the NumPy restatement (tests/raycast_ref.py) against itself (every sample against the samples
inside the grid alone), against the analytic sphere (the calibration of DESIGN.md 18), on hand-set volumes where samples land
exactly on grid points and on the grid's last plane, and the parts of the library that need no device: the parameter check and
the CPU stand-in, which must report that the stage is not there."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import appearance_ref as AR
import fusion_ref as FR
import helpers as H
import raycast_ref as RR

capi = importlib.import_module(H.PKG_NAME + ".capi")


def _both(s, c, origin, voxel, cam, **kw):
    b = RR.brute(s, c, origin, voxel, cam, cam["w"], cam["h"], **kw)
    r = RR.render(s, c, origin, voxel, cam, cam["w"], cam["h"], **kw)
    assert RR.same(b, r), "the clipped form differs from the one that evaluates every sample"
    return b


# ---- the two forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, pos, target, hits", [
    ("novel", RR.SPHERE_CAM["pos"], (0.0, 0.0, 0.0), True),
    ("inside the volume", (0.12, 0.02, -0.11), (0.0, 0.0, 0.0), True),
    ("inside the sphere", (0.01, 0.02, 0.0), (0.3, 0.1, 0.2), False),
    ("behind", (0.0, 0.05, 0.6), (0.0, 0.1, 1.2), False),
    ("looking away", (0.31, 0.22, -0.33), (0.62, 0.44, -0.66), False),
    ("beside", (0.45, 0.0, -0.1), (0.2, 0.0, 0.5), None),
])
def test_forms_agree_on_the_sphere(name, pos, target, hits):
    sp = RR.sphere_volume()
    cam = RR.camera(pos, target, 150.0, 80, 64)
    b = _both(sp["sum"], sp["count"], sp["vol"]["origin"], sp["vol"]["voxel"], cam, **RR.SPHERE_MARCH)
    if hits is not None:
        assert (b["hits"] > 0) == hits, name
    if not b["hits"]:
        assert not b["depth"].any() and not b["normals"].any() and not b["points"].any() and not b["shaded"].any()


def test_forms_agree_on_random_volumes():
    """30 % of the grid points undefined: defined and undefined cells interleave, a hit needs two defined samples in a row, and
    where those two straddle a cell with an undefined corner the hit point has no normal (N = 0)"""
    no_normal = 0
    for dims in ((9, 7, 5), (65, 5, 3)):
        hits = 0
        for step in RR.RANDOM_STEPS:
            for seed in RR.RANDOM_SEEDS:
                s, c, origin, voxel, cam, march = RR.random_case(dims, seed, step)
                b = _both(s, c, origin, voxel, cam, **march, background=7)
                assert (b["shaded"][~b["hit"]] == 7).all() and 0 < b["hits"] < cam["w"] * cam["h"]
                hits += b["hits"]
                lost = b["hit"] & ~b["normal_defined"]
                assert not b["normals"][lost].any() and not b["shaded"][lost].any() and b["depth"][lost].all()
                no_normal += int(lost.sum())
        assert hits >= 100, (dims, hits)
    assert no_normal > 0


def test_min_weight_and_background():
    sp = RR.sphere_volume()
    cam = RR.camera(RR.SPHERE_CAM["pos"], (0.0, 0.0, 0.0), 150.0, 80, 80)
    vol = sp["vol"]
    b1 = _both(sp["sum"], sp["count"], vol["origin"], vol["voxel"], cam, **RR.SPHERE_MARCH)
    b2 = _both(sp["sum"], sp["count"], vol["origin"], vol["voxel"], cam, **RR.SPHERE_MARCH, min_weight=2, background=200)
    assert 0 < b2["hits"] <= b1["hits"] and (b2["shaded"][~b2["hit"]] == 200).all() and (b1["shaded"][~b1["hit"]] == 0).all()


# ---- calibration ----------------------------------------------------------------------------------------------
# measured with this file's own code; the bounds are 1.25 x the measured value rounded up to 0.5 (the rule of DESIGN.md 14),
# a margin for a later change of the fixture and nothing else.  The device is held to bit equality, not to these.
CALIB = {
    "novel": dict(pos=RR.SPHERE_CAM["pos"], hits=11732, analytic=11620, mean=0.5, p99=1.0, max=2.5, angle=17.0, facing=False),
    "axis": dict(pos=RR.CALIB_POS, hits=11872, analytic=11780, mean=0.5, p99=1.0, max=2.5, angle=16.5, facing=True),
}


def _calibration(pos):
    sp = RR.sphere_volume()
    vol, radius = sp["vol"], sp["radius"]
    cam = RR.camera(pos, (0.0, 0.0, 0.0), RR.SPHERE_CAM["f"], RR.SPHERE_CAM["w"], RR.SPHERE_CAM["h"])
    w, h = cam["w"], cam["h"]
    b = RR.brute(sp["sum"], sp["count"], vol["origin"], vol["voxel"], cam, w, h, **RR.SPHERE_MARCH)
    hit_a, P = AR.sphere_hits(cam, w, h, radius)
    R, c0 = np.asarray(cam["R_rw"]), np.asarray(cam["c_left"])
    z_a = (P - c0) @ R[2]
    hit = b["hit"]
    err = np.abs(b["depth"] - z_a)[hit & hit_a] / vol["voxel"]
    n, pts = b["normals"][hit], b["points"][hit]
    radial = pts / np.linalg.norm(pts, axis=1)[:, None]
    angle = np.degrees(np.arccos(np.clip((n * radial).sum(1), -1.0, 1.0)))
    dw = np.stack(RR.rays(cam, w, h), -1)
    u = dw / np.linalg.norm(dw, axis=-1, keepdims=True)
    perp = np.linalg.norm(c0 - (u @ c0)[..., None] * u, axis=-1)  # distance of the pixel's ray from the sphere's centre
    n_dw = (b["normals"] * dw).sum(-1)
    return dict(hits=b["hits"], analytic=int(hit_a.sum()), mean=float(err.mean()), p99=float(np.percentile(err, 99)), max=float(err.max()),
                angle=float(angle.max()), zero_normals=int((np.linalg.norm(n, axis=1) == 0).sum()),
                deep_missed=int((hit_a & (perp < radius - 2.0 * vol["voxel"]) & ~hit).sum()),
                away=int((hit & (n_dw >= 0)).sum()), away_inside=int((hit & hit_a & (n_dw >= 0)).sum()),
                missed=int((hit_a & ~hit).sum()))


def _bound(x):
    return np.ceil(1.25 * x / 0.5) * 0.5


@pytest.mark.parametrize("name", list(CALIB))
def test_sphere_calibration(name):
    want = CALIB[name]
    m = _calibration(want["pos"])
    print(name, m)
    assert m["hits"] == want["hits"]
    # conditions, not measurements
    assert m["zero_normals"] == 0, "a hit pixel without a normal"
    assert m["deep_missed"] == 0, "an analytic hit more than 2 voxels inside the silhouette is not a hit"
    if want["facing"]:
        assert m["away"] == 0, "n . dw < 0 on every hit"
    else:
        # this camera's silhouette rays graze the surface: 19 hits just OUTSIDE the analytic silhouette have a normal that
        # faces away; inside it every normal faces the camera
        assert m["away"] == 19 and m["away_inside"] == 0
    assert m["analytic"] == want["analytic"] and m["missed"] == 0
    for k in ("mean", "p99", "max", "angle"):
        assert m[k] <= want[k], (k, m[k])


def test_calibration_bounds_follow_the_rule():
    """the constants above from the measured values: depth error in voxels mean 0.12, p99 0.70, max 1.94; normal
    against the radial direction at most 13.2 degrees"""
    c = CALIB["novel"]
    assert (c["mean"], c["p99"], c["max"], c["angle"]) == (_bound(0.1192), _bound(0.6962), _bound(1.9402), _bound(13.2042))
    c = CALIB["axis"]  # mean 0.12, p99 0.71, max 1.99, 13.2 degrees
    assert (c["mean"], c["p99"], c["max"], c["angle"]) == (_bound(0.1219), _bound(0.7093), _bound(1.9930), _bound(13.1632))


# ---- hand-set volumes --------------------------------------------------------------------------------------------------------
def _plane(level):
    """3 x 3 x 3 grid at the origin with voxel 1: s = level - z, every count 1"""
    s = np.broadcast_to((level - np.arange(3.0))[:, None, None], (3, 3, 3)).copy()
    return s, np.ones((3, 3, 3), np.int32)


def test_sample_exactly_on_grid_points():
    """R = I, the one pixel's ray runs down the grid line x = y = 1: the samples are the grid points themselves (f = 0)"""
    cam = RR.axis_camera((1.0, 1.0, -1.0), 1.0, 1, 1, 0.0, 0.0)
    s, c = _plane(1.0)  # 1, 0, -1
    b = _both(s, c, (0.0, 0.0, 0.0), 1.0, cam, z_min=1.0, z_max=3.0, step=1.0)
    # z = 1 is the grid point (1, 1, 0) with s = 1, z = 2 the grid point (1, 1, 1) with s = 0 <= 0: t = 1 / (1 - 0)
    assert b["hits"] == 1 and b["depth"][0, 0] == 2.0 and (b["points"][0, 0] == (1.0, 1.0, 1.0)).all()
    assert (b["normals"][0, 0] == (0.0, 0.0, -1.0)).all() and b["shaded"][0, 0] == 255


def test_last_plane_is_outside():
    """g = n - 1 is outside: the sample on the grid's last plane has no value, so a crossing that needs it is no hit"""
    cam = RR.axis_camera((1.0, 1.0, -1.0), 1.0, 1, 1, 0.0, 0.0)
    s, c = _plane(1.5)  # 1.5, 0.5, -0.5: the sign changes between z = 1 and the last plane z = 2
    b = _both(s, c, (0.0, 0.0, 0.0), 1.0, cam, z_min=1.0, z_max=3.0, step=1.0, background=9)
    assert b["hits"] == 0 and b["depth"][0, 0] == 0.0 and b["shaded"][0, 0] == 9
    # with half the step the sample at g = 1.5 is inside and holds exactly 0
    b = _both(s, c, (0.0, 0.0, 0.0), 1.0, cam, z_min=1.0, z_max=3.0, step=0.5)
    assert b["hits"] == 1 and b["depth"][0, 0] == 2.5 and (b["normals"][0, 0] == (0.0, 0.0, -1.0)).all()
    # the same along x: the ray x = 2 = n - 1 is outside whatever z is
    cam = RR.axis_camera((2.0, 1.0, -1.0), 1.0, 1, 1, 0.0, 0.0)
    assert _both(s, c, (0.0, 0.0, 0.0), 1.0, cam, z_min=1.0, z_max=3.0, step=0.5)["hits"] == 0


def test_one_sample_cannot_hit():
    cam = RR.axis_camera((1.0, 1.0, -1.0), 1.0, 1, 1, 0.0, 0.0)
    s, c = _plane(1.0)
    assert RR.sample_count(2.0, 2.5, 1.0) == 1
    assert _both(s, c, (0.0, 0.0, 0.0), 1.0, cam, z_min=2.0, z_max=2.5, step=1.0)["hits"] == 0


# ---- the library without a device ----------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.raycast_default_params() == dict(z_min=0.0, z_max=0.0, step=0.0, min_weight=0, background=0)
    assert not capi.raycast_check_params(**capi.raycast_default_params()), "z_min and z_max have no default"
    ok = dict(z_min=0.1, z_max=1.0)
    assert capi.raycast_check_params(**ok) and capi.raycast_check_params(**ok, step=0.01, min_weight=3, background=255)
    for bad in (dict(z_min=0.0), dict(z_min=-0.1), dict(z_min=float("nan")), dict(z_min=float("inf")), dict(z_max=0.1), dict(z_max=0.05),
                dict(z_max=float("inf")), dict(z_max=float("nan")), dict(step=-1e-3), dict(step=float("nan")), dict(step=float("inf")),
                dict(min_weight=-1)):
        assert not capi.raycast_check_params(**{**ok, **bad}), bad
    with pytest.raises(ValueError):
        capi.raycast_params(**ok, background=256)
    # K = floor((z_max - z_min) / step) + 1 <= 2^20
    top = float(capi.RAYCAST_MAX_SAMPLES)
    assert RR.K_MAX == capi.RAYCAST_MAX_SAMPLES and RR.WH_MAX == capi.RAYCAST_MAX_PIXELS
    assert capi.raycast_check_params(z_min=1.0, z_max=top, step=1.0), "K = 2^20"
    assert not capi.raycast_check_params(z_min=1.0, z_max=top + 1.0, step=1.0), "K = 2^20 + 1"
    assert not capi.raycast_check_params(z_min=1.0, z_max=2.0, step=1e-300)


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
  sfmx_render_out out{};
  sfmx_render_request rq{&cam, 1, sfmx_raycast_params{0.1, 1.0, 0.0, 0, 0}, &out};
  const int with = sfmx_host_fusion_mesh_rc(ctx, nullptr, 0, 0, 16, 16, K, nullptr, nullptr, 0, &sp, &fp, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, &rq, &res, nullptr, nullptr, 0);
  std::printf("%d\n", with);
  sfmx_ctx_destroy(ctx);
  return 0;
}
"""


def test_stand_in_library_reports_unsupported(tmp_path):
    """the host layer on the CPU stand-in of libsfmx.so (tests/fake_sfmx), which has no device stage: it links, because the
    device entries are weak references, and a request that needs one says SFMX_ERR_UNSUPPORTED"""
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
