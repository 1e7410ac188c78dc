"""CPU suite: the seam levelling of a texture atlas -- what the NumPy restatement (tests/level_ref.py) gives: the consequences of
the definition (no seam, no change; corner texels agree at a seam vertex; free offsets stay between the pinned ones of their
component and the 0 they start from; |g| <= 65 280) on the hand scenes and on the textured sphere, floor division on negative
odd sums, the roof and a strip against integers written out by hand, invariance under permuting faces, vertices and views,
parameter validation of the device stage (sfmx_level_check_params needs no device), the key checks of pipeline.fuse, the
stand-in library, and the calibration.

Calibration (the rule of DESIGN.md 15): a bound is 1.25 x what the restatement gives on the fixture, rounded up to 0.1 grey level.
DESIGN.md 26 has the table."""
import importlib

import numpy as np
import pytest

import helpers as H
import level_ref as LR
import raster_ref as R
import texture_ref as TR
import visib_ref as VR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")

# the disturbed textured sphere (level_ref.disturb, CALIBRATION): the seam step without and with levelling; the undisturbed one:
# the seam step without and with, and the mean and 99th percentile of |texel - T| of the levelled atlas
MEASURED = dict(before=19.7335, step=0.2663, plain_before=0.1730, plain_step=0.1533, mean=0.2817, p99=0.7794)
BOUND_STEP = 0.4                  # 1.25 x 0.2663 = 0.333, rounded up to 0.1 grey level
BOUND_MEAN, BOUND_P99 = 0.4, 1.0  # DESIGN.md 25's, unchanged: the levelled atlas stays within them
FACTOR = 10.0                     # a condition, not a measurement: the levelled step is at least this much smaller


def _bound(x):
    return np.ceil(1.25 * x / 0.1 - 1e-9) * 0.1


def _run(scene, z_min=0.5, tol=0.25, T=64, **kw):
    v, f, cams, img = scene
    tex = TR.run(v, f, cams, img, z_min, tol, **kw)
    return tex, LR.run(v, f, cams, img, tex, iterations=T, patch=kw.get("patch", 8), fill=kw.get("fill", 0))


# ---- the consequences --------------------------------------------------------------------------------------------------------
def _corner_texels(f, tex, atlas, patch):
    """vertex -> the corner texels of all its textured faces"""
    L = patch - 2
    lay = LR.layout_of(tex)
    out = {}
    for face in np.nonzero(tex["face_view"] >= 0)[0]:
        for c, (i, j) in enumerate(((0, 0), (L, 0), (0, L))):
            x, y = LR.texel_xy(tex["face_view"], lay, patch, int(face), i, j)
            out.setdefault(int(f[face, c]), []).append(int(atlas[y, x]))
    return out


def _components(n, lo, hi):
    label = np.arange(n)
    while True:
        new = label.copy()
        np.minimum.at(new, lo, label[hi])
        np.minimum.at(new, hi, label[lo])
        new = new[new]
        if (new == label).all():
            return label
        label = new


def _check_consequences(scene, z_min, tol, patch, T=(0, 1, 5, 64)):
    v, f, cams, img = scene
    tex = TR.run(v, f, cams, img, z_min, tol, patch=patch)
    F = np.asarray(f, np.int64)
    G = LR.graph(F, tex["face_view"], len(cams))
    for t in T:
        lev = LR.run(v, f, cams, img, tex, iterations=t, patch=patch)
        assert np.abs(lev["corner_adj"]).max(initial=0) <= LR.G_MAX
        assert lev["corner_sample"].min(initial=0) >= 0 and lev["corner_sample"].max(initial=0) <= LR.G_MAX
        seam = set(np.nonzero(lev["vertex_views"] >= 2)[0].tolist())
        for vert, texels in _corner_texels(F, tex, lev["atlas"], patch).items():
            if vert in seam:
                assert max(texels) - min(texels) <= 1, (t, vert, texels)
        if not seam:
            assert lev["atlas"].tobytes() == tex["atlas"].tobytes() and not lev["corner_adj"].any()
    # every free g^t lies between the smallest and the largest of its component's start values: the pinned g and the 0 every free
    # node starts from (0 belongs to the range: a component whose pinned offsets are all negative has its free nodes above them
    # until the sweeps have pulled them down); the rounded mean of numbers inside a range of integers stays inside it
    cn = G["corner_node"]
    texd = cn[:, 0] >= 0
    fx = np.zeros(len(G["node_v"]), np.int64)
    fx[cn[texd]] = lev["corner_sample"][texd]
    hist, pinned, vv, _ = LR.solve(fx, G["node_v"], len(v), G["lo"], G["hi"], max(T), history=True)
    label = _components(len(fx), G["lo"], G["hi"])
    lo_b, hi_b = np.zeros(len(fx), np.int64), np.zeros(len(fx), np.int64)  # a component without a pinned node stays at 0
    for c in np.unique(label):
        sel = label == c
        p = hist[0][sel & pinned]
        if len(p):
            lo_b[sel], hi_b[sel] = min(p.min(), 0), max(p.max(), 0)
    for g in hist:
        assert (g >= lo_b).all() and (g <= hi_b).all()
    return tex, lev


@pytest.mark.parametrize("patch", [3, 4, 8])
def test_consequences_on_the_hand_scenes(patch):
    for scene in (LR.roof(), LR.apex3(), LR.strip(12), LR.strip(12, unseen=True), LR.strip(40, binary=True), LR.fan(48)):
        tex, lev = _check_consequences(scene, 0.5, 0.25, patch)
        assert lev["seam_vertices"] >= 2
    v, f, cams, img = LR.strip(12)
    tex, lev = _check_consequences((v, f, cams[:1], img[:1]), 0.5, 0.25, patch)
    assert lev["seam_vertices"] == 0 and lev["free_nodes"] == lev["nodes"] > 0 and lev["atlas"].tobytes() == tex["atlas"].tobytes()


@pytest.fixture(scope="module")
def sphere():
    v, f, cams, img = TR.fidelity_scene()
    best = TR.best_views(v, f.astype(np.int64), cams, TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"])
    return v, f, cams, img, best


def test_consequences_on_the_textured_sphere(sphere):
    v, f, cams, img, _ = sphere
    tex, lev = _check_consequences((v, f, cams, LR.disturb(img)), TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"], 8, T=(64,))
    assert lev["seam_vertices"] > 500 and lev["free_nodes"] > 1000 and lev["pinned_nodes"] > 2 * lev["seam_vertices"] - 1


# ---- integers written out by hand ----------------------------------------------------------------------------------------------
def test_floor_division_on_negative_odd_sums():
    # node 0 is free with the pinned neighbours 1, 2 (and 3): the rounded mean of -1 and -2 is -1 (-1.5 rounds up), of -1, -2
    # and -2 it is -2 (-1.67), of 1 and 2 it is 2 (1.5 rounds up), of -3 and -4 it is -3, of -5 alone -5
    def one(gs):
        k = len(gs)
        g = np.array([0] + list(gs), np.int64)
        free = np.array([True] + [False] * k)
        lo, hi = np.zeros(k, np.int64), np.arange(1, k + 1, dtype=np.int64)
        deg = np.array([k] + [1] * k, np.int64)
        out = LR.sweep(g, free, lo, hi, deg)
        assert out[1:].tolist() == list(gs)
        return int(out[0])
    assert one([-1, -2]) == -1 and (2 * -3 + 2) // 4 == -1
    assert one([-1, -2, -2]) == -2 and (2 * -5 + 3) // 6 == -2
    assert one([1, 2]) == 2 and one([-3, -4]) == -3 and one([-5]) == -5 and one([-65280, -65279]) == -65279
    assert one([5120, 5120, 0, 0]) == 2560 and one([-5120, -5120, 0]) == -3413 and one([-5120, 0]) == -2560
    # the target of a seam vertex: samples 10 and 13 meet at (2 * 23 + 2) // 4 = 12, so the nodes are pinned at 2 and -1; 10, 13
    # and 14 at (2 * 37 + 3) // 6 = 12
    g, pinned, vv, target = LR.solve(np.array([10, 13, 7], np.int64), np.array([0, 0, 1]), 2, np.zeros(0, np.int64), np.zeros(0, np.int64), 0)
    assert g.tolist() == [2, -1, 0] and pinned.tolist() == [True, True, False] and vv.tolist() == [2, 1] and target.tolist() == [12, 0]
    g, _, _, target = LR.solve(np.array([10, 13, 14], np.int64), np.array([0, 0, 0]), 1, np.zeros(0, np.int64), np.zeros(0, np.int64), 3)
    assert g.tolist() == [2, -1, -2] and target.tolist() == [12]


def test_the_roof_under_two_constant_images():
    """view 0 shows 100 and takes face 0 = (0, 1, 2), view 1 shows 140 and takes face 1 = (0, 2, 3): the vertices 0 and 2 are seam
    vertices with the target 120 x 256, so face 0's nodes there are pinned at +20 x 256 and face 1's at -20 x 256.  Patch 4 (L =
    2): one cell of 5 x 4 texels, half 0 (face 0) top left, half 1 (face 1) the half turn."""
    scene = LR.roof(100, 140)
    tex, lev = _run(scene, T=0, patch=4)
    assert tex["face_view"].tolist() == [0, 1] and (tex["W"], tex["H"]) == (5, 4)
    assert tex["atlas"].tolist() == [[100, 100, 100, 100, 140], [100, 100, 100, 140, 140], [100, 100, 140, 140, 140], [100, 140, 140, 140, 140]]
    assert lev["corner_sample"].tolist() == [[25600] * 3, [35840] * 3] and lev["vertex_views"].tolist() == [2, 1, 2, 1]
    assert LR.counts(lev) == dict(nodes=6, seam_vertices=2, pinned_nodes=4, free_nodes=2, node_edges=6, iterations=0)
    # T = 0: the free corners (vertex 1 in face 0, vertex 3 in face 1) stay at 0; face 0's texel (i, j) is 100 + 20 (L - i') / L
    assert lev["corner_adj"].tolist() == [[5120, 0, 5120], [-5120, -5120, 0]]
    assert lev["atlas"].tolist() == [[120, 110, 100, 100, 140], [120, 110, 100, 130, 140], [120, 110, 120, 130, 130], [120, 120, 120, 120, 120]]
    # T = 1: each free corner takes the mean of its two pinned neighbours, and both faces are 120 throughout
    for T in (1, 2, 64):
        tex, lev = _run(scene, T=T, patch=4)
        assert lev["corner_adj"].tolist() == [[5120] * 3, [-5120] * 3] and (lev["atlas"] == 120).all() and lev["iterations"] == T
    for patch in (3, 8, 64):
        assert (_run(scene, T=1, patch=patch)[1]["atlas"] == 120).all()


def test_a_strip_against_a_hand_iterated_table():
    """eight faces on the vertices 0 .. 4 (top) and 6 .. 10 (bottom); view 0 (100) takes faces 0 .. 5, view 1 (140) faces 6 and 7; the
    seam vertices are 3 and 9.  In view 0 the nodes of 3 and 9 are pinned at 5120; vertex 2 has the neighbours 1, 8, 9, 3, vertex 8
    has 1, 7, 2, 9, and so on to the left.  In view 1 the nodes of 3 and 9 are pinned at -5120; vertex 10 has the neighbours 3, 9,
    4 and vertex 4 has 3, 10: (2 (-10240) + 3) // 6 = -3413 and (2 (-5120) + 2) // 4 = -2560 are the floor divisions of negative odd
    numerators."""
    v, f, cams, img = LR.strip(8)
    img = [np.full_like(img[0], 100), np.full_like(img[1], 140)]
    assert f.tolist() == [[0, 6, 7], [0, 7, 1], [1, 7, 8], [1, 8, 2], [2, 8, 9], [2, 9, 3], [3, 9, 10], [3, 10, 4]]
    tex = TR.run(v, f, cams, img, 0.5, 0.25, patch=4)
    assert tex["face_view"].tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    table = {
        0: [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 5120], [0, 5120, 5120], [-5120, -5120, 0], [-5120, 0, 0]],
        1: [[0, 0, 0], [0, 0, 0], [0, 0, 1280], [0, 1280, 2560], [2560, 1280, 5120], [2560, 5120, 5120], [-5120, -5120, -3413], [-5120, -3413, -2560]],
        2: [[0, 0, 320], [0, 320, 960], [960, 320, 1920], [960, 1920, 2880], [2880, 1920, 5120], [2880, 5120, 5120], [-5120, -5120, -4267],
            [-5120, -4267, -4266]],
        3: [[427, 160, 720], [427, 720, 1280], [1280, 720, 2320], [1280, 2320, 3280], [3280, 2320, 5120], [3280, 5120, 5120], [-5120, -5120, -4835],
            [-5120, -4835, -4693]],
    }
    for T, want in table.items():
        lev = LR.run(v, f, cams, img, tex, iterations=T, patch=4)
        assert lev["corner_adj"].tolist() == want, T
        assert lev["vertex_views"].tolist() == [1, 1, 1, 2, 1, 0, 1, 1, 1, 2, 1, 0]
    # the rows by hand: T = 1 vertex 8 = (0 + 0 + 0 + 5120) / 4, vertex 2 = (0 + 0 + 5120 + 5120) / 4; T = 2 vertex 7 = (0 + 0 + 0 +
    # 1280) / 4 = 320, vertex 1 = (0 + 0 + 1280 + 2560) / 4 = 960, vertex 8 = (0 + 0 + 2560 + 5120) / 4 = 1920, vertex 2 = (0 + 1280 +
    # 5120 + 5120) / 4 = 2880, vertex 10 = (-5120 - 5120 - 2560) / 3 = -4266.67 -> -4267, vertex 4 = (-5120 - 3413) / 2 = -4266.5 -> -4266
    assert (2 * -12800 + 3) // 6 == -4267 and (2 * -8533 + 2) // 4 == -4266


# ---- invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["apex", "fan", "spheres"])
def test_invariance_under_permuting_faces_vertices_and_views(name):
    if name == "spheres":
        v, f, _, _, _ = VR.nested_spheres()
        cams = VR.six_cameras()
        scene, z, tol, T = (v, f, cams, VR.images_for(cams, 1)), VR.Z_MIN, 0.002, 16
    else:
        scene, z, tol, T = (LR.apex3() if name == "apex" else LR.fan(64)), 0.5, 0.25, 7
    v, f, cams, img = scene
    tex, a = _run(scene, z, tol, T=T)
    rng = np.random.default_rng(8)
    fp, perm = R.permute_faces(f, 4)
    _, b = _run((v, fp, cams, img), z, tol, T=T)
    assert b["corner_adj"].tobytes() == a["corner_adj"][perm].tobytes() and b["corner_sample"].tobytes() == a["corner_sample"][perm].tobytes()
    assert b["vertex_views"].tobytes() == a["vertex_views"].tobytes() and LR.counts(b) == LR.counts(a)
    order = rng.permutation(len(v))  # new vertex i is old vertex order[i]
    inv = np.argsort(order)
    texc, c = _run((v[order], inv[f].astype(np.int32), cams, img), z, tol, T=T)
    assert texc["face_view"].tobytes() == tex["face_view"].tobytes()
    assert c["atlas"].tobytes() == a["atlas"].tobytes() and c["corner_adj"].tobytes() == a["corner_adj"].tobytes()
    assert c["vertex_views"].tobytes() == a["vertex_views"][order].tobytes() and LR.counts(c) == LR.counts(a)
    if name != "spheres":  # no two views tie on a face here, so the views' order cannot change a best view
        vo = rng.permutation(len(cams))
        texd, d = _run((v, f, [cams[i] for i in vo], [img[i] for i in vo]), z, tol, T=T)
        assert (vo[texd["face_view"]] == tex["face_view"]).all()
        for k in LR.ARRAYS:
            assert d[k].tobytes() == a[k].tobytes(), k
        assert LR.counts(d) == LR.counts(a)


# ---- library and Python layer ------------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.level_default_params() == capi.LEVEL_DEFAULTS == LR.DEFAULTS == dict(iterations=64)
    assert capi.LEVEL_COUNTS == LR.COUNTS
    assert capi.level_check_params() and LR.check_params()
    for good in LR.GOOD_PARAMS:
        assert capi.level_check_params(**good) and LR.check_params(**good), good
    for bad in LR.BAD_PARAMS:
        assert not capi.level_check_params(**bad) and not LR.check_params(**bad), bad
    for it, ok in ((-1, False), (0, True), (65536, True), (65537, False)):
        assert capi.level_check_params(iterations=it) == ok == LR.check_params(iterations=it)
    with pytest.raises(TypeError):
        capi.level_params(sweeps=2)
    with pytest.raises(TypeError):
        capi.level_params(iterations=7.5)
    with pytest.raises(ValueError):
        LR.run(*LR.roof(), TR.run(*LR.roof(), 0.5, 0.25), iterations=-1)
    lib = capi.load_library()
    assert lib.sfmx_level_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_level_default_params(None)  # tolerated
    assert sum(s.startswith("sfmx_level_") for s in capi.SYMBOLS) == 11
    assert sum(s.startswith("sfmx_texture_") for s in capi.SYMBOLS) == 17
    assert lib.sfmx_level_counts(None, None) == capi.SFMX_ERR_INVALID and lib.sfmx_level_device_atlas(None, None, None, None) == -1
    assert lib.sfmx_level_last_us(None) == 0.0 and lib.sfmx_level_last_sweeps_us(None) == 0.0 and lib.sfmx_level_last_bake_us(None) == 0.0
    assert hasattr(capi.Context, "level") and all(hasattr(capi.Level, k) for k in ("run", "read", "counts", "device_atlas", "last_sweeps_us"))


def test_python_layer_key_checks():
    import inspect
    assert set(pipe.LEVEL_KEYS) == {"iterations"}
    assert set(pipe.TEXTURE_KEYS) == {"z_min", "depth_tol", "patch", "cells_per_row", "fill", "obj_path"}
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    tex = dict(z_min=0.05)
    for bad in (dict(sweeps=3), dict(iterations=3, patch=8), dict(iterations=2.5)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, texture=tex, level=bad)  # refused before any device call: the context is None
    for lev in (True, dict(iterations=3)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, level=lev)  # level without texture
        with pytest.raises(TypeError):
            pipe.fuse(*args, texture=False, level=lev)
    assert inspect.signature(pipe.fuse).parameters["level"].default is False
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_lv") and hasattr(lib, "sfmx_host_level_free") and hasattr(lib, "sfmx_host_fusion_mesh_tx")
    lib.sfmx_host_level_free(None)  # tolerated


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
  sfmx_level_request lq{};
  lq.params = sfmx_level_params{64};
  const int with = sfmx_host_fusion_mesh_lv(ctx, nullptr, 0, 0, 16, 16, K, nullptr, nullptr, 0, &sp, &fp, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, &lq, &res, nullptr, nullptr, 0);
  const int without = sfmx_host_fusion_mesh_lv(ctx, nullptr, 0, 0, 16, 16, K, nullptr, nullptr, 0, &sp, &fp, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, &res, nullptr, nullptr, 0);
  std::printf("%d %d\n", with, without);
  sfmx_ctx_destroy(ctx);
  return 0;
}
"""


def test_stand_in_library_reports_unsupported(tmp_path):
    """the host layer on the CPU stand-in of libsfmx.so (tests/fake_sfmx), which has no level stage: it links untouched, because the
    device entries are weak references, and a level request says SFMX_ERR_UNSUPPORTED (before it looks at the texture request);
    without either request the call is the plain fusion, which the stand-in does not have either"""
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
    with_level, without = (int(x) for x in p.stdout.split())
    assert with_level == capi.SFMX_ERR_UNSUPPORTED and without == capi.SFMX_ERR_UNSUPPORTED


# ---- calibration ------------------------------------------------------------------------------------------------
def test_the_seam_step_on_the_disturbed_sphere(sphere):
    v, f, cams, img, best = sphere
    S, T = LR.CALIBRATION["patch"], LR.CALIBRATION["iterations"]
    z, tol = TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"]
    dimg = LR.disturb(img)
    assert all(d.dtype == np.uint8 and d.shape == i.shape for d, i in zip(dimg, img)) and dimg[0].tobytes() != img[0].tobytes()
    tex = TR.run(v, f, cams, dimg, z, tol, patch=S, best=best)
    lev = LR.run(v, f, cams, dimg, tex, iterations=T, patch=S)
    lay = LR.layout_of(tex)
    before, edges = LR.seam_step(f, tex["face_view"], tex["atlas"], lay, S)
    after, _ = LR.seam_step(f, tex["face_view"], lev["atlas"], lay, S)
    print("disturbed sphere: %s; seam step %.4f -> %.4f over %d edges, factor %.1f" % (LR.counts(lev), before, after, edges, before / after))
    assert edges == 573 and abs(before - MEASURED["before"]) < 5e-5 and abs(after - MEASURED["step"]) < 5e-5
    assert after <= BOUND_STEP and FACTOR * after <= before


def test_the_levelled_atlas_keeps_the_fidelity(sphere):
    v, f, cams, img, best = sphere
    S, T = LR.CALIBRATION["patch"], LR.CALIBRATION["iterations"]
    tex = TR.run(v, f, cams, img, TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"], patch=S, best=best)
    lev = LR.run(v, f, cams, img, tex, iterations=T, patch=S)
    lay = LR.layout_of(tex)
    before, _ = LR.seam_step(f, tex["face_view"], tex["atlas"], lay, S)
    after, _ = LR.seam_step(f, tex["face_view"], lev["atlas"], lay, S)
    mean, p99 = TR.fidelity(v, f, dict(tex, atlas=lev["atlas"]), S)
    print("textured sphere: seam step %.4f -> %.4f; |texel - T| of the levelled atlas: mean %.4f, p99 %.4f" % (before, after, mean, p99))
    assert abs(before - MEASURED["plain_before"]) < 5e-5 and abs(after - MEASURED["plain_step"]) < 5e-5 and after <= before
    assert abs(mean - MEASURED["mean"]) < 5e-5 and abs(p99 - MEASURED["p99"]) < 5e-5
    assert mean <= BOUND_MEAN and p99 <= BOUND_P99


def test_the_bounds_follow_the_rule():
    import test_texture_cpu as C
    assert abs(BOUND_STEP - _bound(MEASURED["step"])) < 1e-9
    assert (BOUND_MEAN, BOUND_P99) == (C.BOUND_MEAN, C.BOUND_P99), "the existing fidelity bounds, not new ones"
    assert FACTOR == 10.0
