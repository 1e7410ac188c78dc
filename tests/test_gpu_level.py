"""GPU suite: the seam levelling of a texture atlas on the device.  sfmx_level_* gives the levelled atlas, corner_adj,
corner_sample, vertex_views and all six counts byte for byte against the NumPy restatement (tests/level_ref.py): the hand scenes
(the roof, an apex of three views, a strip with a face no view sees) at four patch sizes, a fan of 4 096 faces about a free apex,
images of 0 and 255, one view, 2 to 65 views under two batch sizes, strips at the block and scan edges and past 2^16 faces, every
number of sweeps that matters, a random soup, the nested spheres as built, permuted, rotated and with the views permuted, every
invalid input followed by a good call, every feed, the calibrated seam step, and pipeline.fuse / pipeline.run."""
import ctypes
import importlib

import numpy as np
import pytest

import helpers as H
import level_ref as LR
import raster_ref as R
import texture_ref as TR
import visib_ref as VR

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tx(ctx):
    o = ctx.texture()
    yield o
    o.close()


@pytest.fixture(scope="module")
def lv(ctx):
    """one object for the whole module: its buffers grow and shrink with the cases"""
    o = ctx.level()
    yield o
    o.close()


def _load(tx, cams, images, batch=0):
    tx.reset()
    for cam, img in zip(cams, images):
        tx.add_view(cam, img)
    tx.set_batch(batch)


def _case(tx, lv, v, f, cams, images, z_min, tol, what, T=(64,), batch=0, tex=None, **kw):
    """the texture run, then one level run per T; returns (the texture reference, the last level reference)"""
    if tex is None:
        tex = TR.run(v, f, cams, images, z_min, tol, **kw)
    _load(tx, cams, images, batch)
    TR.same(tx.run(v, f, z_min, tol, **kw), tex, f"{what}: the texture run")
    want = None
    for t in T:
        want = LR.run(v, f, cams, images, tex, iterations=t, patch=kw.get("patch", 8), fill=kw.get("fill", 0))
        got = lv.run(tx, v, f, iterations=t)
        LR.same(got, want, f"{what} {kw} T {t} batch {batch}")
        assert lv.counts() == LR.counts(want) and lv.device_atlas()[0] == tex["W"] * tex["H"]
        assert want["nodes"] == want["pinned_nodes"] + want["free_nodes"] and np.abs(want["corner_adj"]).max(initial=0) <= LR.G_MAX
    TR.same(tx.read(), tex, f"{what}: the texture object after the level runs")
    return tex, want


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


# ---- hand scenes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", [3, 4, 8, 64])
def test_hand_scenes(tx, lv, patch):
    for name, (v, f, cams, img) in (("roof", LR.roof()), ("apex", LR.apex3()), ("strip", LR.strip(12)), ("unseen", LR.strip(12, unseen=True))):
        for fill in (0, 201):
            tex, want = _case(tx, lv, v, f, cams, img, 0.5, 0.25, name, T=(0, 1, 64), patch=patch, fill=fill)
        assert want["seam_vertices"] >= 2 and (tex["view_faces"] > 0).all(), name
        if name == "roof":
            assert (want["atlas"] == 120).all() and tex["face_view"].tolist() == [0, 1]
        if name == "apex":
            assert tex["face_view"].tolist() == [0, 1, 2] and want["vertex_views"].tolist() == [3, 2, 2, 2] and want["free_nodes"] == 0
        if name == "unseen":
            assert tex["face_view"][-1] == -1 and (want["corner_adj"][-1] == 0).all() and (want["corner_sample"][-1] == 0).all()
            S, C = patch, tex["cells_per_row"]
            c = tex["cells"] - 1
            cell = want["atlas"][(c // C) * S:(c // C + 1) * S, (c % C) * (S + 1):(c % C + 1) * (S + 1)]
            assert (cell == fill).all(), "the fill cell is kept"


def test_a_free_apex_of_4096_neighbours(tx, lv):
    v, f, cams, img = LR.fan(4096)
    tex, want = _case(tx, lv, v, f, cams, img, 0.5, 0.25, "fan", T=(0, 1, 2, 64), patch=3)
    assert want["vertex_views"][0] == 1 and (tex["face_view"][:4096] == 0).all() and tex["view_faces"][1] > 1000
    assert want["seam_vertices"] > 1000 and want["corner_adj"][0, 0] != 0, "the apex is a free node and has moved"


def test_images_of_0_and_255_take_both_clamps(tx, lv):
    v, f, cams, img = LR.strip(64, binary=True)
    tex, want = _case(tx, lv, v, f, cams, img, 0.5, 0.25, "binary", T=(0, 3, 64))
    lo, hi = LR.raw_range(v, f, cams, img, tex, want, 8)
    assert lo < 0 and hi > 255, (lo, hi)
    assert set(np.unique(img[0])) == {0, 255}


def test_one_view_gives_the_texture_atlas(tx, lv):
    v, f, cams, img = LR.strip(64)
    tex, want = _case(tx, lv, v, f, cams[:1], img[:1], 0.5, 0.25, "one view")
    assert want["atlas"].tobytes() == tex["atlas"].tobytes() and want["seam_vertices"] == 0 and not want["corner_adj"].any()
    assert 0 < tex["faces_textured"] < 64 and want["nodes"] == want["free_nodes"] > 0


# ---- batching and scale edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 64, 65])
def test_view_counts_with_the_texture_run_under_two_batch_sizes(tx, lv, V):
    v, f, _ = VR.soup(60, 7)
    base = [R.pixel_camera(24, 20, cx=3.0, cy=-2.0), R.pixel_camera(24, 20, f=200.0)] + VR.mixed_views()[1:5]
    cams = [base[k % len(base)] for k in range(V)]
    img = VR.images_for(cams, V)
    tex = TR.run(v, f, cams, img, 0.5, 0.5)
    for batch in (1, 0):
        _case(tx, lv, v, f, cams, img, 0.5, 0.5, f"{V} views", batch=batch, tex=tex)
    tx.set_batch(0)


@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 65537])
def test_strips_at_the_block_and_scan_edges(tx, lv, m):
    v, f, cams, img = LR.strip(m)
    tex, want = _case(tx, lv, v, f, cams, img, 0.5, 0.25, f"strip of {m}", T=(64,) if m > 1000 else (0, 5, 64), patch=3 if m > 1000 else 8)
    assert tex["faces_textured"] == m
    if m >= 255:
        assert want["seam_vertices"] == 2 and (tex["view_faces"] > 50).all() and want["nodes"] == len(np.unique(f)) + 2


def test_every_number_of_sweeps_that_matters(tx, lv):
    v, f, cams, img = LR.strip(300)
    _, want = _case(tx, lv, v, f, cams, img, 0.5, 0.25, "sweeps", T=(0, 1, 2, 63, 64, 1000))
    assert want["iterations"] == 1000


def test_random_soup(tx, lv):
    v, f, _ = VR.soup(2000, 11, 64, 48)
    cams = [R.pixel_camera(64, 48), R.pixel_camera(64, 48, f=200.0, cx=10.0, cy=8.0), R.pixel_camera(40, 40, f=300.0, cx=-20.0, cy=-10.0)]
    img = VR.images_for(cams, 12)
    tex, want = _case(tx, lv, v, f, cams, img, 0.5, 0.5, "soup")
    assert tex["faces_textured"] > 300 and tex["faces_untextured"] > 300
    _case(tx, lv, v, f, cams, img, 0.5, 0.5, "soup", T=(7,), patch=5, cells_per_row=7, fill=255)


# ---- the spheres -------------------------------------------------------------------------------------------------------------
def test_spheres_as_built_permuted_rotated_and_views_permuted(tx, lv):
    v, f, _, no, mo = VR.nested_spheres()
    cams = VR.six_cameras()
    img = VR.images_for(cams, 1)
    tex, a = _case(tx, lv, v, f, cams, img, VR.Z_MIN, 0.002, "nested")
    assert a["seam_vertices"] > 50 and a["free_nodes"] > 50 and (a["vertex_views"][no:] == 0).all() and not a["corner_adj"][mo:].any()
    fp, perm = R.permute_faces(f, 4)
    _, b = _case(tx, lv, v, fp, cams, img, VR.Z_MIN, 0.002, "faces permuted")
    assert b["corner_adj"].tobytes() == a["corner_adj"][perm].tobytes() and b["vertex_views"].tobytes() == a["vertex_views"].tobytes()
    assert LR.counts(b) == LR.counts(a)
    fr = R.rotate_corners(f, 5)
    _, c = _case(tx, lv, v, fr, cams, img, VR.Z_MIN, 0.002, "corners rotated")
    assert np.sort(c["corner_adj"], 1).tobytes() == np.sort(a["corner_adj"], 1).tobytes() and LR.counts(c) == LR.counts(a)
    order = np.random.default_rng(6).permutation(len(cams))
    _, d = _case(tx, lv, v, f, [cams[i] for i in order], [img[i] for i in order], VR.Z_MIN, 0.002, "views permuted")
    assert d["vertex_views"].sum() > 0 and d["nodes"] > 0


# ---- invalid inputs ------------------------------------------------------------------------------------------------------------
def test_invalid_inputs_each_followed_by_a_good_call(ctx, tx, lv):
    v, f, cams, img = LR.strip(12, unseen=True)
    z, tol = 0.5, 0.25
    tex = TR.run(v, f, cams, img, z, tol)
    want = LR.run(v, f, cams, img, tex, iterations=9)

    def good_call(what):
        _load(tx, cams, img)
        tx.run(v, f, z, tol)
        LR.same(lv.run(tx, v, f, iterations=9), want, "after " + what)

    def refused(fn, what):
        _invalid(fn)
        _invalid(lv.read)  # the failed run left no result
        with pytest.raises(capi.SfmxError):
            lv.counts()
        assert lv.device_atlas()[0] == -1
        good_call(what)

    good_call("nothing")
    fresh = ctx.texture()
    refused(lambda: lv.run(fresh, v, f), "a texture object that never ran")
    fresh.close()
    bad = f.copy()
    bad[3, 1] = len(v)
    _invalid(lambda: tx.run(v, bad, z, tol))
    refused(lambda: lv.run(tx, v, f), "a texture object whose last run failed")
    refused(lambda: lv.run(tx, v[:-1], f), "n - 1")
    refused(lambda: lv.run(tx, np.concatenate([v, v[:1]]), f), "n + 1")
    refused(lambda: lv.run(tx, v, f[:-1]), "m - 1")
    refused(lambda: lv.run(tx, v, np.concatenate([f, f[:1]])), "m + 1")
    for index in (-1, len(v), 2 ** 31 - 1, -2 ** 31):
        for corner in range(3):
            bad = f.copy()
            bad[5, corner] = index
            refused(lambda: lv.run(tx, v, bad), f"index {index}")
    for p in LR.BAD_PARAMS:
        assert not capi.level_check_params(**p) and not LR.check_params(**p)
        refused(lambda: lv.run(tx, v, f, **p), str(p))
    lib, P = ctx.lib, ctypes.c_void_p
    p = capi.level_params(iterations=9)
    args = (v.ctypes.data_as(P), ctypes.c_int(len(v)), f.ctypes.data_as(P), ctypes.c_int(len(f)), ctypes.c_int(0))
    refused(lambda: ctx._chk(lib.sfmx_level_run(ctx.h_, lv.h_, tx.h_, *args, None)), "NULL parameters")
    refused(lambda: ctx._chk(lib.sfmx_level_run(ctx.h_, lv.h_, None, *args, ctypes.byref(p))), "a NULL texture object")
    refused(lambda: ctx._chk(lib.sfmx_level_run(ctx.h_, lv.h_, tx.h_, None, args[1], args[2], args[3], args[4], ctypes.byref(p))), "NULL vertices")
    refused(lambda: ctx._chk(lib.sfmx_level_run(ctx.h_, lv.h_, tx.h_, args[0], args[1], None, args[3], args[4], ctypes.byref(p))), "NULL faces")
    assert lib.sfmx_level_run(ctx.h_, None, tx.h_, *args, ctypes.byref(p)) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_level_read(ctx.h_, lv.h_, None, None, None, None) == capi.SFMX_OK, "every pointer may be NULL"
    with pytest.raises(TypeError):
        lv.run(tx, v, f, sweeps=3)
    assert lv.read()["iterations"] == 9, "refused in Python, before the library: the result stays"
    for p in LR.GOOD_PARAMS[:3]:
        assert capi.level_check_params(**p) and LR.check_params(**p)
    assert capi.level_check_params(iterations=LR.ITER_MAX) and capi.level_default_params() == capi.LEVEL_DEFAULTS == LR.DEFAULTS


def test_empty_meshes_and_state_rules(ctx):
    s, t = ctx.level(), ctx.texture()
    _invalid(s.read)
    assert s.device_atlas() == (-1, None, 0, 0) and s.last_us() == 0.0 and s.last_sweeps_us() == 0.0 and s.last_bake_us() == 0.0
    v, f, cams, img = LR.strip(12)
    none = np.zeros((0, 3), np.int32)
    tex, want = _case(t, s, v, none, cams, img, 0.5, 0.25, "no faces")
    assert want["atlas"].shape == (0, 0) and want["nodes"] == 0 and want["vertex_views"].tolist() == [0] * len(v)
    _case(t, s, np.zeros((0, 3)), none, cams, img, 0.5, 0.25, "nothing")
    back = np.ascontiguousarray(f[:, ::-1])
    tex, want = _case(t, s, v, back, cams, img, 0.5, 0.25, "no textured face", fill=7)
    assert tex["faces_textured"] == 0 and (want["atlas"] == 7).all() and want["atlas"].size > 0 and want["nodes"] == 0
    ctx.set_timing(True)
    _case(t, s, v, f, cams, img, 0.5, 0.25, "timed")
    assert 0.0 < s.last_sweeps_us() <= s.last_us() and 0.0 < s.last_bake_us() <= s.last_us()
    ctx.set_timing(False)
    s.close()
    t.close()


# ---- feeds -------------------------------------------------------------------------------------------------------------------
def test_feeding_paths_and_sizes_large_small_large(ctx):
    """host pointers, device pointers, the device meshes of the visibility and the simplify objects; one object used large, small,
    large"""
    import torch
    import consist_ref as CR
    import simplify_ref as PR
    vol = CR.SPHERE26_VOL
    fu = ctx.fusion(**vol)
    views = CR.sphere8()[:8]
    for cam_, d16 in views:
        fu.add_view(cam_, d16)
    v, f, nrm = fu.extract_normals()
    cams = [dict(cam_, w=d16.shape[1], h=d16.shape[0]) for cam_, d16 in views[:5]]
    img = VR.images_for(cams, 5)
    tol = vol["voxel"]
    s, t = ctx.level(), ctx.texture()
    tex, ref = _case(t, s, v, f, cams, img, 0.05, tol, "host pointers", T=(8,), patch=4)
    assert ref["seam_vertices"] > 100 and ref["free_nodes"] > 100
    sv, sf, scams, simg = LR.roof()
    _case(t, s, sv, sf, scams, simg, 0.5, 0.25, "small after large")
    tv, tf = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, f))
    torch.cuda.synchronize()
    _load(t, cams, img)
    t.run(tv.data_ptr(), tf.data_ptr(), 0.05, tol, n=len(v), m=len(f), patch=4)
    LR.same(s.run(t, tv.data_ptr(), tf.data_ptr(), n=len(v), m=len(f), iterations=8), ref, "device pointers, large again")
    vb = ctx.visib()
    for cam in cams:
        vb.add_view(cam)
    vres = vb.run(v, f, 0.05, tol)
    n1, pv1, pf1, m1 = vb.device_mesh()
    t.run(pv1, pf1, 0.05, tol, n=n1, m=m1)
    tex1 = TR.run(vres["verts"], vres["faces"], cams, img, 0.05, tol)
    LR.same(s.run(t, pv1, pf1, n=n1, m=m1, iterations=8), LR.run(vres["verts"], vres["faces"], cams, img, tex1, iterations=8),
            "the visibility object's device mesh")
    sp = ctx.simplify()
    sp.run(tv.data_ptr(), tf.data_ptr(), n=len(v), m=len(f), cell=2 * vol["voxel"], origin=vol["origin"])
    pref = PR.simplify(v, f, None, cell=2 * vol["voxel"], origin=vol["origin"])
    n3, pv3, pf3, m3 = sp.device_mesh()
    t.run(pv3, pf3, 0.05, 2 * tol, n=n3, m=m3)
    tex3 = TR.run(pref["verts"], pref["faces"], cams, img, 0.05, 2 * tol)
    LR.same(s.run(t, pv3, pf3, n=n3, m=m3), LR.run(pref["verts"], pref["faces"], cams, img, tex3), "the simplify object's device mesh")
    for o in (sp, vb, s, t, fu):
        o.close()


def test_the_calibrated_seam_step_from_the_device(tx, lv):
    """the device's atlases of the disturbed and the undisturbed textured sphere give the CPU suite's figures (they are the same
    atlases)"""
    import test_level_cpu as C
    v, f, cams, img = TR.fidelity_scene()
    S, T = LR.CALIBRATION["patch"], LR.CALIBRATION["iterations"]
    z, tol = TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"]
    dimg = LR.disturb(img)
    tex, want = _case(tx, lv, v, f, cams, dimg, z, tol, "disturbed sphere", T=(T,), patch=S)
    got = lv.read()
    lay = LR.layout_of(tex)
    before, edges = LR.seam_step(f, tex["face_view"], tx.read()["atlas"], lay, S)
    after, _ = LR.seam_step(f, tex["face_view"], got["atlas"], lay, S)
    print("seam step on the disturbed sphere: %.4f -> %.4f over %d edges" % (before, after, edges))
    assert after <= C.BOUND_STEP and 10.0 * after <= before and abs(after - C.MEASURED["step"]) < 5e-5
    tex, want = _case(tx, lv, v, f, cams, img, z, tol, "textured sphere", T=(T,), patch=S)
    mean, p99 = TR.fidelity(v, f, dict(tex, atlas=lv.read()["atlas"]), S)
    print("fidelity of the levelled atlas: mean %.4f, p99 %.4f" % (mean, p99))
    assert mean <= C.BOUND_MEAN and p99 <= C.BOUND_P99


# ---- pipeline ----------------------------------------------------------------------------------------------------------------
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
LEV_KEYS = ("atlas", "corner_adj", "corner_sample", "vertex_views")


@pytest.fixture(scope="module")
def ring2(ctx):
    """two pairs of the ring-6 fixture with their left rectified cameras and images"""
    import consist_ref as CR
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    pairs = pairs[:2]
    st = ctx.stereo(320, 240, num_disparities=64)
    views, rects = [], []
    for a, b in pairs:
        r = pipe.stereo_rectify(K, poses[a], poses[b], 320, 240)
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        rects.append(st.disparity(il, ir, r["H_l"], r["H_r"], want_rect=True)["rect"][0].copy())
        views.append(dict(R_rw=r["R_rw"], c_left=r["c_left"], f=r["f"], cx=r["cx"], cy=r["cy"], B=r["B"], w=320, h=240))
    st.close()
    return dict(images=images, K=K, poses=poses, pairs=pairs, vol=CR.RING6_VOL, views=views, rects=rects)


def _fuse_args(ctx, r):
    vol = r["vol"]
    return (ctx, r["images"], r["K"], r["poses"], r["pairs"], vol["origin"], vol["voxel"], vol["dims"])


def _check_level(m, want, what):
    LR.same(m["level"], want, what)
    assert set(m["level"]) == set(LEV_KEYS) | set(LR.COUNTS), what


def _same_files(tmp_path, stem, m, tex, want):
    ref = tmp_path / "ref"
    ref.mkdir(exist_ok=True)
    pipe.write_textured_obj(str(ref / (stem + ".obj")), m["verts"], m["faces"], TR.uv(tex["uv_half"], tex["W"], tex["H"]), want["atlas"])
    for ext in (".obj", ".mtl", "_atlas.pgm", "_atlas.bmp"):
        assert open(tmp_path / (stem + ext), "rb").read() == open(ref / (stem + ext), "rb").read(), ext


def test_host_fuse_level(ctx, ring2, tmp_path):
    args = _fuse_args(ctx, ring2)
    voxel = ring2["vol"]["voxel"]
    p0, p1 = str(tmp_path / "tex.ply"), str(tmp_path / "lev.ply")
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0, texture=dict(z_min=0.05))
    again = pipe.fuse(*args, num_disparities=64, ply_path=p1, texture=dict(z_min=0.05), level=False)
    assert set(again) == set(m0) and open(p0, "rb").read() == open(p1, "rb").read(), "without level everything is what it was"
    TR.same(again["texture"], m0["texture"], "level=False")
    m = pipe.fuse(*args, num_disparities=64, ply_path=p1, texture=dict(z_min=0.05, obj_path=str(tmp_path / "mesh.obj")), level=True)
    assert set(m) == set(m0) | {"level"} and m["views"] == m0["views"] == 2 and m["warn"] == m0["warn"]
    assert m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read(), "the PLY is what it is without level"
    TR.same(m["texture"], m0["texture"], "the texture beside level")
    assert m["texture"]["uv"].tobytes() == m0["texture"]["uv"].tobytes()
    tex = TR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], 0.05, voxel)
    TR.same(m0["texture"], tex, "the texture reference")
    want = LR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], tex)
    print("fuse: %d v / %d f -> %s" % (len(m0["verts"]), len(m0["faces"]), LR.counts(want)))
    assert want["seam_vertices"] > 20 and want["free_nodes"] > 1000 and want["atlas"].tobytes() != tex["atlas"].tobytes()
    _check_level(m, want, "fuse")
    _same_files(tmp_path, "mesh", m, tex, want)
    # parameters of its own, on a texture with parameters of its own; no pairs; refused parameters
    xkw = dict(patch=5, cells_per_row=40, fill=99)
    m2 = pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05, depth_tol=2.5 * voxel, **xkw), level=dict(iterations=3))
    tex2 = TR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], 0.05, 2.5 * voxel, **xkw)
    _check_level(m2, LR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], tex2, iterations=3, patch=5, fill=99), "own")
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, texture=dict(z_min=0.05), level=True)
    assert empty["verts"].shape == (0, 3) and empty["level"]["atlas"].shape == (0, 0) and empty["level"]["corner_adj"].shape == (0, 3)
    assert {k: empty["level"][k] for k in LR.COUNTS} == dict.fromkeys(LR.COUNTS, 0) and len(empty["level"]["vertex_views"]) == 0
    for bad in (dict(iterations=-1), dict(iterations=65537)):
        with pytest.raises(capi.SfmxError):
            pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05), level=bad)
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05), level=dict(sweeps=1))
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, level=True)


def test_host_fuse_level_with_every_other_stage(ctx, ring2, tmp_path):
    """clean, fill, smooth, simplify, appearance and visibility: the seams are levelled on the final mesh, and everything else is
    what it is without level"""
    args = _fuse_args(ctx, ring2)
    voxel = ring2["vol"]["voxel"]
    stages = dict(appearance=True, clean=True, fill=True, smooth=dict(iters=3), simplify=True)
    for vis in (False, dict(z_min=0.05, depth_tol=2 * voxel)):
        p0, p1 = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
        xkw = dict(z_min=0.05, depth_tol=2 * voxel)
        m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0, visibility=vis, texture=xkw, **stages)
        m = pipe.fuse(*args, num_disparities=64, ply_path=p1, visibility=vis, texture=dict(xkw, obj_path=str(tmp_path / "s")), level=dict(iterations=16),
                      **stages)
        assert set(m) == set(m0) | {"level"} and open(p0, "rb").read() == open(p1, "rb").read()
        for k in ("verts", "faces", "normals", "grey", "vertex_views"):
            assert m[k].tobytes() == m0[k].tobytes(), k
        for k in ("clean", "fill", "smooth", "simplify"):
            assert m[k] == m0[k], k
        TR.same(m["texture"], m0["texture"], "the texture beside level")
        tex = TR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], 0.05, 2 * voxel)
        want = LR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], tex, iterations=16)
        _check_level(m, want, f"every stage, visibility {bool(vis)}")
        _same_files(tmp_path, "s", m, tex, want)
        assert want["seam_vertices"] > 10
    for one in (dict(clean=True), dict(fill=True), dict(smooth=dict(iters=2)), dict(simplify=True), dict(visibility=dict(z_min=0.05))):
        m0 = pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05), **one)
        m = pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05), level=dict(iterations=4), **one)
        assert m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes(), one
        TR.same(m["texture"], m0["texture"], str(one))
        tex = TR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], 0.05, voxel)
        _check_level(m, LR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], tex, iterations=4), str(one))


def test_pipeline_run_level(ctx, tmp_path):
    import json
    import os
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    pair, small = (2, 3), dict(num_disparities=32, census=5)
    plain, with_l = str(tmp_path / "tex"), str(tmp_path / "lev")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in pair)
    mesh = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][pair[0]], r0["kf_poses"][pair[1]], **small)
    lo, hi = mesh["verts"].min(0), mesh["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    fz = dict(pairs=[pair], origin=tuple(lo), voxel=voxel, dims=dims, texture=dict(z_min=1e-3), **small)
    h, w = g["images"].shape[1:]
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain, fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, with_l, fusion=dict(fz, level=dict(iterations=5)))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(with_l, "X") and sorted(os.listdir(with_l)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m) == set(m1) | {"level"} and len(m1["faces"]) > 0 and m["verts"].tobytes() == m1["verts"].tobytes()
    TR.same(m["texture"], m1["texture"], "pipeline.run: the texture beside level")
    rect = pipe.stereo_rectify(g["K"], r0["kf_poses"][pair[0]], r0["kf_poses"][pair[1]], w, h)
    view = dict(R_rw=rect["R_rw"], c_left=rect["c_left"], f=rect["f"], cx=rect["cx"], cy=rect["cy"], B=rect["B"], w=w, h=h)
    il, ir = (g["images"][fb], g["images"][fa]) if rect["swapped"] else (g["images"][fa], g["images"][fb])
    st = ctx.stereo(w, h, **small)
    left = st.disparity(il, ir, rect["H_l"], rect["H_r"], want_rect=True)["rect"][0].copy()
    st.close()
    tex = TR.run(m1["verts"], m1["faces"], [view], [left], 1e-3, voxel)
    want = LR.run(m1["verts"], m1["faces"], [view], [left], tex, iterations=5)
    print("run: %d f -> %s" % (len(m1["faces"]), LR.counts(want)))
    _check_level(m, want, "pipeline.run")
    assert want["atlas"].tobytes() == tex["atlas"].tobytes(), "one view: nothing to level"
