"""GPU suite: the exact z-buffer on the device.  sfmx_raster_* gives depth, face, points, normals, shaded, grey, the eight counts
and the fragment count byte for byte against the NumPy restatement (tests/raster_ref.py): the hand cases (every kind of edge and
vertex on a pixel centre, shared edges, a fan, degenerate faces, z_min and the band at and past their limits, non-finite
coordinates, ties in (float)depth, culling), the image shapes around the 8 x 8 and 16 x 16 tiles, boxes at RS_SMALL - 1, RS_SMALL
and RS_SMALL + 1, tiled faces off every border, face and vertex counts at the block edges and past 2^20, 65 536 faces on one
pixel, the calibration icosphere and the fused sphere as built, permuted and rotated, cameras inside the mesh, a random soup,
every invalid input, the state rules, and every way of feeding a mesh.

Where the restatement's brute form (every face against every pixel) would take minutes, its box form is the reference;
tests/test_raster_cpu.py holds the two to each other."""
import ctypes
import os
import importlib

import numpy as np
import pytest

import clean_ref as LR
import helpers as H
import raster_ref as R
import raycast_ref as RR
import sdist_ref as DR

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
Z = 0.5


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rs(ctx):
    """one object for the whole module: its buffers grow and shrink with the cases"""
    r = ctx.raster()
    yield r
    r.close()


def _case(rs, v, f, cam, what, z_min=Z, normals=None, grey=None, ref=R.brute, **kw):
    want = ref(v, f, cam, z_min, normals, grey, **kw)
    got = rs.render(v, f, cam, z_min, normals=normals, grey=grey, **kw)
    R.same(got, want, f"{what} {kw}")
    assert rs.counts() == R.counts(want) and rs.device_surface()[0] == want["face"].size
    return want


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


def _attrs(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3)), rng.integers(0, 256, n).astype(np.uint8)


# ---- hand cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.hand_cases()))
def test_hand_cases(rs, name):
    c = R.hand_cases()[name]
    v, f, cam = c["verts"], c["faces"], R.hand_camera(c)
    nrm, grey = _attrs(len(v), len(name))
    for cull in (0, 1, 2):
        _case(rs, v, f, cam, name, c["z_min"], cull=cull)
        _case(rs, v, f, cam, name + " with normals and grey", c["z_min"], nrm, grey, cull=cull, background=9)
    _case(rs, v, f, cam, name + " with grey", c["z_min"], None, grey)
    _case(rs, v, f, cam, name + " with normals", c["z_min"], nrm, None, background=255)
    if name.startswith("box-"):
        _case(rs, v, f, cam, name, c["z_min"])
        assert rs.last_big_faces() == (1 if name == "box-65" else 0), "RS_SMALL = 64: a box of 65 pixel centres is tiled"
    if name in ("band", "off-borders"):
        _case(rs, v, f, cam, name, c["z_min"])
        assert rs.last_big_faces() == (1 if name == "band" else 4)


# ---- image shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (7, 9), (8, 8), (17, 16), (64, 4), (4096, 1)])
def test_image_shapes(rs, shape):
    w, h = shape
    v, f, nrm, grey = R.random_scene(w, h)
    cam = R.pixel_camera(w, h)
    ref = _case(rs, v, f, cam, f"{w} x {h}", normals=nrm, grey=grey)
    assert ref["hits"] > 0 and ref["fragments"] > ref["hits"]
    _case(rs, v, f, cam, f"{w} x {h}", cull=1)
    # one face over the whole image and beyond, in front of everything
    cover = R.at_pixels([(-3.0 * (w + h), -5.0), (3.0 * (w + h), -5.0), (w / 2.0, 3.0 * (w + h))], 0.75)
    ref = _case(rs, np.concatenate([v, cover]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32), cam, "covered")
    assert (ref["face"] == len(f)).all() and ref["hits"] == w * h


# ---- scale edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [255, 256, 257])
def test_face_counts_at_the_block_edge(rs, count):
    v, f = R.tiny_faces(count, 16, 16)
    _case(rs, v, f, R.pixel_camera(16, 16), f"{count} faces")


@pytest.mark.parametrize("count", [65535, 65536, 65537, 1024 * 1024 + 1])
def test_face_counts_at_the_grid_edges(rs, count):
    side = 256 if count < 1 << 20 else 512
    v, f = R.tiny_faces(count, side, side)
    ref = _case(rs, v, f, R.pixel_camera(side, side), f"{count} faces", ref=R.render)
    assert ref["faces_drawn"] > count // 8 and rs.last_big_faces() == 0


@pytest.mark.parametrize("n", [255, 256, 257, 65535, 65536, 65537])
def test_vertex_counts_at_the_block_edges(rs, n):
    v, f = R.tiny_faces(80, 16, 16)
    pad = R.at_pixels(np.random.default_rng(n).uniform(-50, 50, (n - len(v), 2)), 1.5)
    v = np.concatenate([v, pad])
    f = np.concatenate([f, [[0, n - 1, n - 2], [n - 1, 5, n - 3]]]).astype(np.int32)  # the last vertices are used
    nrm, grey = _attrs(n, n)
    _case(rs, v, f, R.pixel_camera(16, 16), f"{n} vertices", normals=nrm, grey=grey)


def test_65536_faces_on_one_pixel(rs):
    v, f = R.hot_pixel()
    ref = _case(rs, v, f, R.pixel_camera(8, 8), "hot pixel", ref=R.render)
    assert ref["faces_drawn"] == 65536 and ref["fragments"] > 2 * 65536 and ref["face"][3, 3] >= 0


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def _variants(rs, v, f, cam, what, z_min, nrm, grey):
    """as built, faces permuted, corners rotated: against the restatement, and the stated properties against each other"""
    ref = _case(rs, v, f, cam, what, z_min, nrm, grey, ref=R.render)
    f2, perm = R.permute_faces(f, 3)
    a = _case(rs, v, f2, cam, what + ", faces permuted", z_min, nrm, grey, ref=R.render)
    assert R.counts(a) == R.counts(ref) and all(a[k].tobytes() == ref[k].tobytes() for k in ("depth", "points", "shaded", "normals", "grey"))
    assert (np.where(a["face"] >= 0, perm[a["face"]], -1) == ref["face"]).all(), "face follows the permutation"
    b = _case(rs, v, R.rotate_corners(f, 4), cam, what + ", corners rotated", z_min, nrm, grey, ref=R.render)
    assert R.counts(b) == R.counts(ref) and b["face"].tobytes() == ref["face"].tobytes()
    return ref


@pytest.mark.parametrize("name", list(R.CALIB))
def test_calibration_icosphere(rs, name):
    v, f = DR.icosphere(4, 0.1)
    nrm, grey = _attrs(len(v), 8)
    c = R.CALIB[name]
    cam = c["cam"]()
    ref = _variants(rs, v, f, cam, name, R.CALIB_Z_MIN, nrm, grey)
    assert (ref["hits"], ref["faces_back"], ref["back_pixels"], ref["fragments"]) == (c["hits"], c["faces_back"], 0, 2 * c["hits"])
    one = _case(rs, v, f, cam, name, R.CALIB_Z_MIN, nrm, grey, ref=R.render, cull=1)
    two = _case(rs, v, f, cam, name, R.CALIB_Z_MIN, nrm, grey, ref=R.render, cull=2)
    assert one["fragments"] == two["fragments"] == c["hits"] and two["back_pixels"] == two["hits"] == c["hits"]
    assert all(one[k].tobytes() == ref[k].tobytes() for k in R.ARRAYS + ("grey",)), "cull = 1 gives the image of cull = 0"


def test_cameras_inside_the_sphere(rs):
    v, f = DR.icosphere(3, 0.1)
    cam = RR.axis_camera((0.0, 0.0, 0.0), 40.0, 96, 64, 47.5, 31.5)
    ref = _case(rs, v, f, cam, "centre", 0.01)
    assert ref["hits"] == 96 * 64 == ref["back_pixels"] and ref["faces_behind"] > len(f) // 3, "half the mesh is behind the camera"
    assert _case(rs, v, f, cam, "centre", 0.01, cull=1)["hits"] == 0
    cam = RR.camera((0.02, -0.03, 0.06), (0.0, 0.05, -0.1), 60.0, 64, 48)
    ref = _case(rs, v, f, cam, "off centre", 0.02)
    assert 0 < ref["faces_behind"] < len(f) and ref["hits"] == ref["back_pixels"] > 0


def test_fused_sphere_from_two_cameras(ctx, rs):
    from test_fusion_cpu import SPHERE, VOL, sphere_views
    fu = ctx.fusion(**VOL)
    for cam, d16 in sphere_views(**SPHERE):
        fu.add_view(cam, d16)
    v, f, nrm = fu.extract_normals()
    fu.close()
    assert len(f) > 10000
    grey = _attrs(len(v), 2)[1]
    for pos in (RR.SPHERE_CAM["pos"], RR.CALIB_POS):
        cam = RR.camera(pos, (0.0, 0.0, 0.0), RR.SPHERE_CAM["f"], RR.SPHERE_CAM["w"], RR.SPHERE_CAM["h"])
        ref = _variants(rs, v, f, cam, f"sphere-26 from {pos}", 0.05, nrm, grey)
        assert ref["hits"] > 10000 and ref["fragments"] > ref["hits"], "the fused surface: a front and a back layer, with folds"


def test_soup(rs):
    v, f, nrm = LR.soup()
    assert (len(v), len(f)) == (20000, 15000)
    centre = v.mean(0)
    cam = RR.camera(centre + np.array([0.3, -0.2, -8.0]), centre, 60.0, 64, 48)
    grey = _attrs(len(v), 3)[1]
    ref = _case(rs, v, f, cam, "soup", 0.05, nrm, grey)
    assert ref["hits"] > 1000 and 0 < ref["back_pixels"] < ref["hits"] and rs.last_big_faces() > 0
    _case(rs, v, f, cam, "soup", 0.05, cull=2)


# ---- validation and state ----------------------------------------------------------------------------------------------------
def test_every_invalid_input_then_a_good_call(ctx, rs):
    import torch
    good = R.hand_cases()["fan"]
    gv, gf, cam = good["verts"], good["faces"], R.hand_camera(good)
    gref = R.brute(gv, gf, cam, Z)

    def good_call(what):
        R.same(rs.render(gv, gf, cam, Z), gref, "after " + what)

    def refused(fn, what):
        _invalid(fn)
        _invalid(rs.read)  # the failed run left no result
        with pytest.raises(capi.SfmxError):
            rs.counts()
        with pytest.raises(capi.SfmxError):
            rs.device_surface()
        good_call(what)

    good_call("nothing")
    for bad in (-1, len(gv), 2 ** 31 - 1, -2 ** 31):
        for corner in range(3):
            f = gf.copy()
            f[3, corner] = bad
            refused(lambda: rs.render(gv, f, cam, Z), f"index {bad}")
    for p in R.BAD_PARAMS:
        assert not capi.raster_check_params(**p)
        refused(lambda: rs.render(gv, gf, cam, **p), str(p))
    refused(lambda: rs.render(gv, gf, cam, Z, w=4097, h=1), "w over 4096")
    refused(lambda: rs.render(gv, gf, cam, Z, w=4096, h=4097), "w * h over 2^24")
    refused(lambda: rs.render(gv, gf, cam, Z, w=0, h=4), "w = 0")
    refused(lambda: rs.render(gv, gf, cam, Z, w=4, h=0), "h = 0")
    refused(lambda: rs.render(gv, gf, {**cam, "f": 0.0}, Z), "f = 0")
    refused(lambda: rs.render(gv, gf, {**cam, "cx": float("nan")}, Z), "cx NaN")
    # n and m at their limits: refused before anything is read
    tv, tf = torch.from_numpy(gv).to("cuda:0"), torch.from_numpy(gf).to("cuda:0")
    torch.cuda.synchronize()
    refused(lambda: rs.render(tv.data_ptr(), tf.data_ptr(), cam, Z, n=capi.RASTER_MAX_VERTS, m=len(gf)), "n = 2^24")
    refused(lambda: rs.render(tv.data_ptr(), tf.data_ptr(), cam, Z, n=len(gv), m=capi.RASTER_MAX_FACES), "m = 2^30")
    refused(lambda: rs.render(tv.data_ptr(), tf.data_ptr(), cam, Z, n=-1, m=len(gf)), "n < 0")
    refused(lambda: rs.render(tv.data_ptr(), tf.data_ptr(), cam, Z, n=len(gv), m=-1), "m < 0")
    R.same(rs.render(tv.data_ptr(), tf.data_ptr(), cam, Z, n=len(gv), m=len(gf)), gref, "device pointers")
    with pytest.raises(TypeError):
        rs.render(gv, gf, cam, Z, step=1.0)
    with pytest.raises(ValueError):
        rs.render(gv, gf, cam, Z, background=256)
    assert rs.read()["hits"] == gref["hits"], "refused in Python, before the library: the result stays"
    for p in R.GOOD_PARAMS:
        assert capi.raster_check_params(**p)
        R.same(rs.render(gv, gf, cam, **p), R.brute(gv, gf, cam, **p), str(p))


def test_one_object_large_small_large(ctx):
    s = ctx.raster()
    big = (*R.tiny_faces(40000, 200, 200), R.pixel_camera(200, 200))
    c = R.hand_cases()["fan"]
    small = (c["verts"], c["faces"], R.hand_camera(c))
    for what, (v, f, cam) in (("large", big), ("small", small), ("large again", big)):
        _case(s, v, f, cam, what, ref=R.render)
        assert s.last_us() == 0.0
    ctx.set_timing(True)
    _case(s, *big, "timed", ref=R.render)
    assert s.last_us() > 0.0
    ctx.set_timing(False)
    s.close()


def test_state_rules(ctx):
    s = ctx.raster()
    lib = ctx.lib
    _invalid(s.read)
    with pytest.raises(capi.SfmxError):
        s.counts()
    with pytest.raises(capi.SfmxError):
        s.device_surface()
    assert s.last_us() == 0.0 and s.last_big_faces() == 0
    c = R.hand_cases()["fan"]
    v, f, cam = c["verts"], c["faces"], R.hand_camera(c)
    ref = _case(s, v, f, cam, "first run")
    buf = np.zeros((8, 8), np.uint8)
    rc = lib.sfmx_raster_read(ctx.h_, s.h_, None, None, None, None, None, buf.ctypes.data_as(ctypes.c_void_p))
    assert rc == capi.SFMX_ERR_INVALID, "grey after a run without grey"
    assert lib.sfmx_raster_read(ctx.h_, s.h_, None, None, None, None, None, None) == capi.SFMX_OK, "every pointer may be NULL"
    face = np.zeros((8, 8), np.int32)
    assert lib.sfmx_raster_read(ctx.h_, s.h_, None, face.ctypes.data_as(ctypes.c_void_p), None, None, None, None) == capi.SFMX_OK
    assert face.tobytes() == ref["face"].tobytes()
    grey = _attrs(len(v), 1)[1]
    _case(s, v, f, cam, "with grey", grey=grey)
    assert lib.sfmx_raster_read(ctx.h_, s.h_, None, None, None, None, None, buf.ctypes.data_as(ctypes.c_void_p)) == capi.SFMX_OK
    assert buf.tobytes() == R.brute(v, f, cam, Z, grey=grey)["grey"].tobytes()
    # NULL arguments
    p, view = capi.raster_params(Z), capi.fusion_view({**cam, "B": 0.0}, 8, 8)
    args = (v.ctypes.data_as(ctypes.c_void_p), None, None, ctypes.c_int(len(v)), f.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(len(f)), ctypes.c_int(0))
    assert lib.sfmx_raster_run(ctx.h_, s.h_, *args, None, ctypes.byref(p)) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_raster_run(ctx.h_, s.h_, *args, ctypes.byref(view), None) == capi.SFMX_ERR_INVALID
    _invalid(s.read)
    assert lib.sfmx_raster_run(ctx.h_, s.h_, None, *args[1:], ctypes.byref(view), ctypes.byref(p)) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_raster_run(ctx.h_, s.h_, *args, ctypes.byref(view), ctypes.byref(p)) == capi.SFMX_OK
    s.close()


# ---- feeds -------------------------------------------------------------------------------------------------------------------
def test_feeding_paths_same_bytes(ctx):
    """host pointers, device pointers, and the device meshes of the fill, smooth and simplify objects (the fusion and clean
    objects publish no device faces through include/sfmx.h: their meshes are fed as the host arrays they return)"""
    import torch
    import consist_ref as CR
    import fill_ref as FLR
    import simplify_ref as PR
    import smooth_ref as MR
    vol = CR.SPHERE26_VOL
    fu = ctx.fusion(**vol)
    for cam_, d16 in CR.sphere8()[:8]:
        fu.add_view(cam_, d16)
    v, f, nrm = fu.extract_normals()
    cam = RR.camera((0.25, 0.2, -0.3), (0.0, 0.0, 0.0), 200.0, 120, 90)
    s = ctx.raster()
    grey = _attrs(len(v), 6)[1]
    ref = _case(s, v, f, cam, "host pointers", 0.05, nrm, grey, ref=R.render)
    assert ref["hits"] > 1000
    tv, tf, tn, tg = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, f, nrm, grey))
    torch.cuda.synchronize()
    got = s.render(tv.data_ptr(), tf.data_ptr(), cam, 0.05, normals=tn.data_ptr(), grey=tg.data_ptr(), n=len(v), m=len(f))
    R.same(got, ref, "device pointers")
    got = s.render(tv.data_ptr(), tf.data_ptr(), cam, 0.05, n=len(v), m=len(f))
    R.same(got, R.render(v, f, cam, 0.05), "device pointers, no attributes")
    # the cleaned surface (host arrays), then fill, smooth and simplify from their device meshes
    cl, fl, sm, sp = ctx.clean(), ctx.fill(), ctx.smooth(), ctx.simplify()
    cl.fusion(fu)
    cr = cl.read(normals=True)
    lref = LR.clean(v, f, nrm)
    assert cr["verts"].tobytes() == lref["verts"].tobytes() and cr["faces"].tobytes() == lref["faces"].tobytes()
    _case(s, cr["verts"], cr["faces"], cam, "cleaned", 0.05, cr["normals"], ref=R.render)
    kw = dict(unit=vol["voxel"], origin=vol["origin"])
    fl.clean(cl, max_edges=64, **kw)
    fref = FLR.fill(lref["verts"], lref["faces"], lref["normals"], max_edges=64, **kw)
    n, pv, pf, m = fl.device_mesh()
    pn = fl.device_surface()[2]
    want = R.render(fref["verts"], fref["faces"], cam, 0.05, fref["normals"])
    R.same(s.render(pv, pf, cam, 0.05, normals=pn, n=n, m=m), want, "the fill object's device mesh")
    R.same(s.render(fref["verts"], fref["faces"], cam, 0.05, normals=fref["normals"]), want, "the same from the host")
    sm.run(pv, pf, n=n, m=m, **kw)
    mref = MR.smooth(fref["verts"], fref["faces"], **kw)
    n2, pv2, pf2, m2 = sm.device_mesh()
    want = R.render(mref["verts"], fref["faces"], cam, 0.05, fref["normals"])
    R.same(s.render(pv2, pf2, cam, 0.05, normals=pn, n=n2, m=m2), want, "the smooth object's device mesh")
    sp.run(pv2, pf2, normals=pn, n=n2, m=m2, cell=2 * vol["voxel"], origin=vol["origin"])
    pref = PR.simplify(mref["verts"], fref["faces"], fref["normals"], cell=2 * vol["voxel"], origin=vol["origin"])
    n3, pv3, pf3, m3 = sp.device_mesh()
    want = R.render(pref["verts"], pref["faces"], cam, 0.05, pref["normals"])
    R.same(s.render(pv3, pf3, cam, 0.05, normals=sp.device_surface()[2], n=n3, m=m3), want, "the simplify object's device mesh")
    assert want["hits"] > 1000 and s.last_big_faces() >= 0
    for o in (cl, fl, sm, sp, s, fu):
        o.close()


def test_device_surface_into_shade(ctx):
    """the render's points and normals, on the device, shade as the same arrays from the host do"""
    from test_fusion_cpu import SPHERE, sphere_views
    views = sphere_views(**dict(SPHERE, w=64, h=64, f=120.0, n_views=6))
    sh, s = ctx.shade(), ctx.raster()
    rng = np.random.default_rng(12)
    for cam_, d16 in views:
        sh.add_view(cam_, d16, rng.integers(0, 256, d16.shape).astype(np.uint8))
    v, f = DR.icosphere(3, 0.1)
    cam = RR.camera((0.3, 0.1, -0.35), (0.0, 0.0, 0.0), 150.0, 80, 60)
    out = s.render(v, f, cam, 0.05)
    n, pp, pn = s.device_surface()
    assert n == 80 * 60
    dev = sh.shade(pp, pn, 0.01, n=n)
    host = sh.shade(out["points"].reshape(-1, 3), out["normals"].reshape(-1, 3), 0.01)
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes() and (host[1] > 0).any()
    sh.close()
    s.close()


# ---- pipeline ----------------------------------------------------------------------------------------------------------------
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")


@pytest.fixture(scope="module")
def ring2():
    """two pairs of the ring-6 fixture and two cameras on its ring"""
    import consist_ref as CR
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    cams = [dict(R_rw=poses[i][0].T, c_left=poses[i][1], f=0.3 * K[0, 0], cx=0.3 * K[0, 2], cy=0.3 * K[1, 2], w=96, h=72) for i in (0, 3)]
    return dict(images=images, K=K, poses=poses, pairs=pairs[:2], vol=CR.RING6_VOL, cams=cams)


def _read_pgm(path):
    raw = open(path, "rb").read()
    magic, size, top, data = raw.split(b"\n", 3)
    w, h = (int(x) for x in size.split())
    assert magic == b"P5" and top == b"255" and len(data) == w * h
    return np.frombuffer(data, np.uint8).reshape(h, w)


def _fuse_args(ctx, r):
    vol = r["vol"]
    return (ctx, r["images"], r["K"], r["poses"], r["pairs"], vol["origin"], vol["voxel"], vol["dims"])


def test_host_fuse_raster(ctx, ring2, tmp_path):
    args = _fuse_args(ctx, ring2)
    cams = ring2["cams"]
    p0, p1 = str(tmp_path / "plain.ply"), str(tmp_path / "raster.ply")
    prefix = str(tmp_path / "view")
    rkw = dict(cameras=cams, w=96, h=72, z_min=0.05, z_max=0.9)
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0, render=rkw)
    zkw = dict(cameras=cams, w=96, h=72, z_min=0.05, background=3, pgm_prefix=prefix)
    m = pipe.fuse(*args, num_disparities=64, ply_path=p1, render=rkw, raster=zkw)
    assert set(m) == set(m0) | {"rasters"} and m["warn"] == m0["warn"] and m["views"] == m0["views"] == 2
    assert m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes() and len(m["faces"]) > 1000
    assert open(p0, "rb").read() == open(p1, "rb").read(), "the PLY is the file without raster"
    for a, b in zip(m["renders"], m0["renders"]):
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a), "renders are what they are without raster"
    s = ctx.raster()
    assert len(m["rasters"]) == 2
    for i, (cam, got) in enumerate(zip(cams, m["rasters"])):
        ref = R.render(m["verts"], m["faces"], cam, 0.05, background=3)
        assert "grey" not in got and ref["hits"] > 500
        R.same(got, ref, f"fuse, camera {i}")
        R.same(s.render(m["verts"], m["faces"], cam, 0.05, background=3), ref, f"standalone, camera {i}")
        assert _read_pgm(f"{prefix}_{i}_mesh_shaded.pgm").tobytes() == ref["shaded"].tobytes()
        assert not os.path.exists(f"{prefix}_{i}_mesh_grey.pgm")
    s.close()
    # no pairs: nothing to render but the background; bad keys and parameters
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, raster=dict(zkw, pgm_prefix=None))
    assert empty["verts"].shape == (0, 3) and len(empty["rasters"]) == 2
    for got in empty["rasters"]:
        assert R.counts(got) == dict.fromkeys(R.COUNTS + ("fragments",), 0) and (got["shaded"] == 3).all() and (got["face"] == -1).all()
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, raster=dict(zkw, z_max=1.0))
    for bad in (dict(z_min=0.0), dict(cull=3), dict(z_min=float("nan"))):
        with pytest.raises(capi.SfmxError):
            pipe.fuse(*args, num_disparities=64, raster={**zkw, **bad, "pgm_prefix": None})


def test_host_fuse_raster_with_every_other_stage(ctx, ring2, tmp_path):
    """clean, fill, smooth, simplify and appearance in three combinations: the rendered mesh is the final one, with its
    appearance normals and grey, and everything else is what it is without raster"""
    import os
    args = _fuse_args(ctx, ring2)
    cams = ring2["cams"]
    prefix = str(tmp_path / "all")
    zkw = dict(cameras=cams, w=96, h=72, z_min=0.05, cull=1, background=250, pgm_prefix=prefix)
    for cl, fl, smo, simp in ((True, True, True, True), (True, True, True, False), (False, False, False, False)):
        stages = dict(appearance=True, clean=cl, fill=fl, smooth=dict(iters=3) if smo else False, simplify=simp)
        p0, p1 = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
        m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0, **stages)
        m = pipe.fuse(*args, num_disparities=64, ply_path=p1, raster=zkw, **stages)
        assert set(m) == set(m0) | {"rasters"} and open(p0, "rb").read() == open(p1, "rb").read()
        for k in set(m0) - {"warn", "views"}:
            assert (m[k] == m0[k] if isinstance(m0[k], dict) else m[k].tobytes() == m0[k].tobytes()), k
        for i, (cam, got) in enumerate(zip(cams, m["rasters"])):
            ref = R.render(m["verts"], m["faces"], cam, 0.05, m["normals"], m["grey"], cull=1, background=250)
            R.same(got, ref, f"{stages}, camera {i}")
            assert ref["hits"] > 500 and ref["faces_culled"] == ref["faces_back"] > 0 and ref["back_pixels"] == 0
            assert _read_pgm(f"{prefix}_{i}_mesh_shaded.pgm").tobytes() == ref["shaded"].tobytes()
            assert _read_pgm(f"{prefix}_{i}_mesh_grey.pgm").tobytes() == ref["grey"].tobytes() and len(np.unique(ref["grey"])) > 10
    # a surface with nothing left: the cleaning removes every component
    m5 = pipe.fuse(*args, num_disparities=64, clean=dict(min_faces=10 ** 8), appearance=True, raster=dict(zkw, pgm_prefix=None))
    assert m5["faces"].shape == (0, 3) and all(r["hits"] == 0 and (r["grey"] == 250).all() and (r["shaded"] == 250).all() for r in m5["rasters"])


def test_pipeline_run_raster(ctx, tmp_path):
    import json
    import os
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    pair, small = (2, 3), dict(num_disparities=32, census=5)
    plain, with_r = str(tmp_path / "plain"), str(tmp_path / "raster")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in pair)
    mesh = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][pair[0]], r0["kf_poses"][pair[1]], **small)
    lo, hi = mesh["verts"].min(0), mesh["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    fz = dict(pairs=[pair], origin=tuple(lo), voxel=voxel, dims=dims, **small)
    pose = r0["kf_poses"][pair[0]]
    K = np.asarray(g["K"], np.float64).reshape(3, 3)
    cam = dict(R_rw=pose[:9].reshape(3, 3).T, c_left=pose[9:], f=K[0, 0] / 4.0, cx=K[0, 2] / 4.0, cy=K[1, 2] / 4.0)
    h, w = g["images"].shape[1] // 4, g["images"].shape[2] // 4
    zkw = dict(cameras=[cam], w=w, h=h, z_min=1e-3)
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain, fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, with_r, fusion=dict(fz, raster=zkw))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(with_r, "X") and sorted(os.listdir(with_r)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m) == set(m1) | {"rasters"} and m["verts"].tobytes() == m1["verts"].tobytes() and len(m1["faces"]) > 0
    assert open(os.path.join(plain, "templeRing_mesh_fused.ply"), "rb").read() == open(os.path.join(with_r, "templeRing_mesh_fused.ply"), "rb").read()
    ref = R.render(m["verts"], m["faces"], dict(cam, w=w, h=h), 1e-3)
    print("run: %s" % R.counts(ref))
    R.same(m["rasters"][0], ref, "pipeline.run")
    assert ref["hits"] > 0
