"""GPU suite: exact multi-view visibility on the device.  sfmx_visib_* gives the culled mesh, vert_src / face_src, the per-face
and per-vertex view counts, grey and grey_views and all eight counts byte for byte against the NumPy restatement
(tests/visib_ref.py): the hand cases (the depth tolerance below, at and one ulp above the gap; snapped positions between two
pixel centres; empty pixels; every border; z_min; non-finite coordinates; faces without a pixel centre; collinear faces; a back
face that occludes; empty inputs), the nested spheres, the flipped patch and the camera inside as built, permuted and rotated,
every min_views, 1 to 65 views under every batch size, views of mixed sizes, face and vertex counts at the block and grid edges
and past 2^20, 65 536 faces on one pixel, a random soup, images and normals with cull and fill, every invalid input, the state
rules, and every way of feeding a mesh in and of handing the result on."""
import ctypes
import importlib

import numpy as np
import pytest

import helpers as H
import raster_ref as R
import raycast_ref as RR
import sdist_ref as DR
import visib_ref as VR

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vb(ctx):
    """one object for the whole module: its views and buffers grow and shrink with the cases"""
    o = ctx.visib()
    yield o
    o.close()


def _load(vb, cams, images=None, batch=0):
    vb.reset()
    for k, cam in enumerate(cams):
        vb.add_view(cam, None if images is None else images[k])
    assert vb.view_count() == len(cams)
    vb.set_batch(batch)


def _case(vb, v, f, cams, z_min, tol, what, normals=None, images=None, batch=0, want=None, **kw):
    if want is None:
        want = VR.run(v, f, cams, z_min, tol, normals=normals, images=images, **kw)
    _load(vb, cams, images, batch)
    got = vb.run(v, f, z_min, tol, normals=normals, **kw)
    VR.same(got, want, f"{what} {kw} batch {batch}")
    assert vb.counts() == VR.counts(want)
    assert vb.sizes() == (len(np.reshape(v, (-1, 3))), len(np.reshape(f, (-1, 3))), want["verts_kept"], want["faces_kept"])
    assert want["pairs_visible"] + want["pairs_occluded"] + want["pairs_off"] == vb.sizes()[0] * len(cams)
    assert vb.device_mesh()[0] == want["verts_kept"] and vb.device_mesh()[3] == want["faces_kept"]
    return want


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


def _normals(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 3))


# ---- hand cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VR.hand_cases()))
def test_hand_cases(vb, name):
    c = VR.hand_cases()[name]
    v, f, cams, z, tol = c["verts"], c["faces"], c["cams"], c["z_min"], c["depth_tol"]
    nrm, img = _normals(len(v), len(name)), VR.images_for(c["cams"], 3)
    for mv in (0, 1):
        _case(vb, v, f, cams, z, tol, name, min_views=mv)
        _case(vb, v, f, [], z, tol, name + ", no views", min_views=mv)
    _case(vb, v, f, cams, z, tol, name + " with normals", normals=nrm)
    _case(vb, v, f, cams, z, tol, name + " with images", normals=nrm, images=img)
    _case(vb, v, f, cams, z, tol, name + " with images", normals=nrm, images=img, cull=0, fill=9, min_views=2)
    _case(vb, v, f, cams, z, tol, name + " with images, no normals", images=img, cull=0, fill=255, min_views=0)


def test_hand_cases_show_what_they_should(vb):
    """the device on the three gap cases: the far quad is seen below and at the tolerance and not one ulp above it"""
    for name, seen in (("gap-below", 1), ("gap-at", 1), ("gap-ulp-above", 0)):
        c = VR.hand_cases()[name]
        _load(vb, c["cams"])
        got = vb.run(c["verts"], c["faces"], c["z_min"], c["depth_tol"])
        assert got["face_views"].tolist() == [1, 1, seen, seen] and got["vert_views"].tolist() == [1] * 4 + [seen] * 4, name


# ---- the spheres -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spheres():
    v, f, nrm, no, mo = VR.nested_spheres()
    cams = VR.six_cameras()
    img = VR.images_for(cams, 1)
    scenes = dict(nested=(v, f, nrm, cams), flipped=(*VR.flipped_patch(40), cams), inside=(v, f, nrm, [VR.inside_camera()]))
    refs = {k: VR.run(s[0], s[1], s[3], VR.Z_MIN, 0.002, normals=s[2], images=img[:len(s[3])], min_views=0) for k, s in scenes.items()}
    return dict(scenes=scenes, refs=refs, img=img, no=no, mo=mo)


@pytest.mark.parametrize("scene", ["nested", "flipped", "inside"])
def test_spheres_as_built_permuted_rotated_and_views_permuted(vb, spheres, scene):
    v, f, nrm, cams = spheres["scenes"][scene]
    img = spheres["img"][:len(cams)]
    a = spheres["refs"][scene]
    kw = dict(normals=nrm, images=img, min_views=0)
    _case(vb, v, f, cams, VR.Z_MIN, 0.002, scene, want=a, **kw)
    fp, perm = R.permute_faces(f, 4)
    _load(vb, cams, img)
    b = vb.run(v, fp, VR.Z_MIN, 0.002, normals=nrm, min_views=0)
    assert (b["face_views"] == a["face_views"][perm]).all() and (b["face_back_views"] == a["face_back_views"][perm]).all()
    for k in ("vert_views", "grey", "grey_views", "verts", "vert_src"):
        assert b[k].tobytes() == a[k].tobytes(), k
    assert vb.counts() == VR.counts(a)
    fr = R.rotate_corners(f, 5)
    VR.same(vb.run(v, fr, VR.Z_MIN, 0.002, normals=nrm, min_views=0), {**a, "faces": fr}, "corners rotated")
    order = np.random.default_rng(6).permutation(len(cams))
    _load(vb, [cams[i] for i in order], [img[i] for i in order])
    VR.same(vb.run(v, f, VR.Z_MIN, 0.002, normals=nrm, min_views=0), a, "views permuted")


def test_nested_spheres_culling_returns_the_outer_sphere(vb, spheres):
    v, f, nrm, cams = spheres["scenes"]["nested"]
    no, mo = spheres["no"], spheres["mo"]
    for tol in (0.002, 0.004):
        _load(vb, cams)
        got = vb.run(v, f, VR.Z_MIN, tol, normals=nrm)
        assert got["verts"].tobytes() == v[:no].tobytes() and got["faces"].tobytes() == f[:mo].tobytes()
        assert got["normals"].tobytes() == nrm[:no].tobytes() and (got["faces_seen"], got["faces_back_only"], got["faces_unseen"]) == (1280, 0, 320)
    want = _case(vb, v, f, cams, VR.Z_MIN, 0.0005, "below the depth slope")
    assert int((want["face_views"][:mo] == 0).sum()) == 152
    want = _case(vb, *spheres["scenes"]["flipped"][:2], cams, VR.Z_MIN, 0.002, "flipped patch")
    assert (want["faces_seen"], want["faces_back_only"], want["faces_unseen"]) == (1240, 40, 0)
    want = _case(vb, v, f, [VR.inside_camera()], VR.Z_MIN, 0.002, "inside")
    assert (want["faces_seen"], want["faces_back_only"], want["faces_kept"]) == (0, 10, 0)


@pytest.mark.parametrize("mv", [0, 1, 2, 6, 7])
def test_min_views(vb, spheres, mv):
    v, f, nrm, cams = spheres["scenes"]["nested"]
    a = spheres["refs"]["nested"]
    want = _case(vb, v, f, cams, VR.Z_MIN, 0.002, "min_views", normals=nrm, images=spheres["img"], min_views=mv)
    assert want["faces_kept"] == int((a["face_views"] >= mv).sum()) and want["face_views"].tobytes() == a["face_views"].tobytes()
    assert want["faces_kept"] == (len(f) if mv == 0 else 0 if mv == 7 else want["faces_kept"])


# ---- batching --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65])
def test_view_counts_and_batch_sizes(vb, V):
    v, f, nrm = VR.soup(60, 7)
    base = [R.pixel_camera(24, 20, cx=3.0, cy=-2.0), R.pixel_camera(24, 20, f=200.0)] + VR.mixed_views()[1:5]
    cams = [base[k % len(base)] for k in range(V)]
    img = VR.images_for(cams, V)
    want = VR.run(v, f, cams, 0.5, 0.5, normals=nrm, images=img)
    assert want["pairs_occluded"] > 0 and want["pairs_off"] > 0 and 0 < want["faces_kept"] < len(f)
    for batch in (1, 2, 64, 0):
        _case(vb, v, f, cams, 0.5, 0.5, f"{V} views", normals=nrm, images=img, batch=batch, want=want)
        assert vb.last_batch() == min(V, batch if batch else 64)
    with pytest.raises(capi.SfmxError):
        vb.set_batch(65)
    with pytest.raises(capi.SfmxError):
        vb.set_batch(-1)
    vb.set_batch(0)


def test_views_of_mixed_sizes(vb):
    v, f, nrm = VR.soup(150, 8)
    cams = VR.mixed_views()
    img = VR.images_for(cams, 9)
    want = None
    for batch in (0, 1, 3):
        want = _case(vb, v, f, cams, 0.5, 0.5, "mixed sizes", normals=nrm, images=img, batch=batch, want=want, min_views=0)
    assert want["pairs_visible"] > 0 and want["pairs_occluded"] > 0 and want["pairs_off"] > 0


# ---- scale edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [255, 256, 257])
def test_face_counts_at_the_block_edge(vb, count):
    v, f = R.tiny_faces(count, 16, 16)
    cams = [R.pixel_camera(16, 16), R.pixel_camera(16, 16, cx=0.5, cy=0.25)]
    want = _case(vb, v, f, cams, 0.5, 0.01, f"{count} faces")
    assert 0 < want["faces_kept"] < count


@pytest.mark.parametrize("count", [65535, 65536, 65537, 1024 * 1024 + 1])
def test_face_counts_at_the_grid_edges(vb, count):
    side = 256 if count < 1 << 20 else 512
    v, f = R.tiny_faces(count, side, side)
    want = _case(vb, v, f, [R.pixel_camera(side, side)], 0.5, 0.01, f"{count} faces")
    assert count // 8 < want["faces_kept"] < count and want["verts_kept"] == 3 * want["faces_kept"]


@pytest.mark.parametrize("n", [255, 256, 257, 65535, 65536, 65537])
def test_vertex_counts_at_the_block_edges(vb, n):
    v, f = R.tiny_faces(80, 16, 16)
    pad = R.at_pixels(np.random.default_rng(n).uniform(-50, 50, (n - len(v), 2)), 1.5)
    v = np.concatenate([v, pad])
    f = np.concatenate([f, [[0, n - 1, n - 2], [n - 1, 5, n - 3]]]).astype(np.int32)  # the last vertices are used
    cams = [R.pixel_camera(16, 16), R.pixel_camera(16, 16, f=128.0, cx=8.0, cy=8.0)]
    _case(vb, v, f, cams, 0.5, 0.5, f"{n} vertices", normals=_normals(n, n), images=VR.images_for(cams, n), min_views=0)


def test_many_faces_on_one_pixel(vb):
    v, f = R.hot_pixel(65536)
    back = _case(vb, v, f, [R.pixel_camera(8, 8)], 0.5, 0.5, "65 536 faces on one pixel")  # as built they all face away
    assert back["faces_seen"] == 0 and 1000 < back["faces_back_only"] < 65536 and back["pairs_occluded"] > 50000
    want = _case(vb, v, np.ascontiguousarray(f[:, ::-1]), [R.pixel_camera(8, 8)], 0.5, 0.5, "65 536 faces on one pixel, wound the other way")
    assert want["faces_seen"] == want["faces_kept"] == back["faces_back_only"] and want["vert_views"].tobytes() == back["vert_views"].tobytes()


def test_random_soup(vb):
    v, f, nrm = VR.soup(2000, 11, 64, 48)  # 4 000 faces of every size, half of them larger than the images
    cams = [R.pixel_camera(64, 48), R.pixel_camera(64, 48, f=200.0, cx=10.0, cy=8.0), R.pixel_camera(40, 40, f=300.0, cx=-20.0, cy=-10.0)]
    img = VR.images_for(cams, 12)
    for kw in (dict(), dict(cull=0, fill=77, min_views=2), dict(min_views=0)):
        want = _case(vb, v, f, cams, 0.5, 0.5, "soup", normals=nrm, images=img, **kw)
    assert want["faces_seen"] > 300 and want["faces_back_only"] > 300 and want["faces_unseen"] > 300


@pytest.mark.parametrize("n,m", [(300, 257), (700, 256), (70000, 65537)])  # the block edge, and the scans' second level
def test_compaction_agrees_between_clean_and_visibility(ctx, vb, n, m):
    """Both stages compact a mesh by keep flags.  Where every face is kept (clean without a threshold, visibility without views
    and min_views = 0) the flags are the same, so the five common arrays must be: byte for byte, and as tests/clean_ref.py has them."""
    import clean_ref as CR
    v, f, nrm = CR.soup(n, m, seed=n + m)
    want = CR.clean(v, f, normals=nrm, min_faces=0, min_permille=0)
    assert want["n_faces"] == m and 0 < want["n_verts"] < n, "a soup that leaves vertices unreferenced"
    cl = ctx.clean()
    try:
        cl.run(v, f, normals=nrm, min_faces=0, min_permille=0)
        a = cl.read(normals=True)
    finally:
        cl.close()
    _load(vb, [])
    b = vb.run(v, f, 0.5, 0.5, normals=nrm, min_views=0)
    for key in ("verts", "normals", "faces", "vert_src", "face_src"):
        assert a[key].dtype == b[key].dtype == want[key].dtype and a[key].shape == b[key].shape == want[key].shape, key
        assert a[key].tobytes() == b[key].tobytes(), f"{key}: clean and visibility differ at n = {n}, m = {m}"
        assert a[key].tobytes() == want[key].tobytes(), f"{key}: not the reference's at n = {n}, m = {m}"


# ---- invalid inputs ----------------------------------------------------------------------------------------------------------
def test_invalid_inputs_each_followed_by_a_good_call(ctx, vb):
    import torch
    c = VR.hand_cases()["two-views"]
    gv, gf, cams, z, tol = c["verts"], c["faces"], c["cams"], c["z_min"], c["depth_tol"]
    nrm, img = _normals(len(gv), 1), VR.images_for(cams, 2)
    gref = VR.run(gv, gf, cams, z, tol, normals=nrm, images=img)

    def good_call(what):
        _load(vb, cams, img)
        VR.same(vb.run(gv, gf, z, tol, normals=nrm), gref, "after " + what)

    def refused(fn, what):
        _invalid(fn)
        _invalid(vb.read)  # the failed run left no result
        for getter in (vb.counts, vb.sizes):
            with pytest.raises(capi.SfmxError):
                getter()
        assert vb.device_mesh()[0] == -1 and vb.device_surface()[0] == -1
        good_call(what)

    good_call("nothing")
    for bad in (-1, len(gv), 2 ** 31 - 1, -2 ** 31):
        for corner in range(3):
            f = gf.copy()
            f[1, corner] = bad
            refused(lambda: vb.run(gv, f, z, tol, normals=nrm), f"index {bad}")
    _load(vb, [])
    f = gf.copy()
    f[0, 0] = 4
    refused(lambda: vb.run(gv, f, z, tol), "a bad index without views")
    for p in VR.BAD_PARAMS:
        refused(lambda: vb.run(gv, gf, normals=nrm, **p), str(p))
    refused(lambda: vb.run(gv, gf, z, tol), "cull = 1 with images and no normals")
    _load(vb, cams, [img[0], None])
    refused(lambda: vb.run(gv, gf, z, tol, normals=nrm), "images on some views only")
    for bad_cam in ({**cams[0], "w": 4097, "h": 1}, {**cams[0], "w": 4096, "h": 4097}, {**cams[0], "w": 0}, {**cams[0], "h": 0},
                    {**cams[0], "f": 0.0}, {**cams[0], "cx": float("nan")}):
        n0 = vb.view_count()
        _invalid(lambda: vb.add_view(bad_cam))
        assert vb.view_count() == n0
    tv, tf = torch.from_numpy(gv).to("cuda:0"), torch.from_numpy(gf).to("cuda:0")
    torch.cuda.synchronize()
    _load(vb, cams)
    refused(lambda: vb.run(tv.data_ptr(), tf.data_ptr(), z, tol, n=capi.RASTER_MAX_VERTS, m=len(gf)), "n = 2^24")
    refused(lambda: vb.run(tv.data_ptr(), tf.data_ptr(), z, tol, n=len(gv), m=capi.RASTER_MAX_FACES), "m = 2^30")
    refused(lambda: vb.run(tv.data_ptr(), tf.data_ptr(), z, tol, n=-1, m=len(gf)), "n < 0")
    refused(lambda: vb.run(tv.data_ptr(), tf.data_ptr(), z, tol, n=len(gv), m=-1), "m < 0")
    _load(vb, cams)
    VR.same(vb.run(tv.data_ptr(), tf.data_ptr(), z, tol, n=len(gv), m=len(gf)), VR.run(gv, gf, cams, z, tol), "device pointers")
    with pytest.raises(TypeError):
        vb.run(gv, gf, z, tol, background=1)
    assert vb.read()["faces_kept"] == 2, "refused in Python, before the library: the result stays"
    for p in VR.GOOD_PARAMS:
        _case(vb, gv, gf, cams, p["z_min"], p["depth_tol"], str(p), normals=nrm, images=img, **{k: p[k] for k in p if k not in ("z_min", "depth_tol")})


def test_state_rules(ctx):
    s = ctx.visib()
    lib = ctx.lib
    _invalid(s.read)
    with pytest.raises(capi.SfmxError):
        s.counts()
    assert s.device_mesh() == (-1, None, None, 0) and s.last_us() == 0.0 and s.last_batch() == 0 and s.view_count() == 0
    c = VR.hand_cases()["two-views"]
    v, f, cams = c["verts"], c["faces"], c["cams"]
    ref = _case(s, v, f, cams, c["z_min"], c["depth_tol"], "first run")
    P = ctypes.c_void_p
    buf, ibuf = np.zeros(16, np.uint8), np.zeros(16, np.int32)

    def read(**kw):
        names = ("verts", "normals", "faces", "vert_src", "face_src", "face_views", "face_back_views", "vert_views", "grey", "grey_views")
        return lib.sfmx_visib_read(ctx.h_, s.h_, *[kw[k].ctypes.data_as(P) if k in kw else None for k in names])

    assert read() == capi.SFMX_OK, "every pointer may be NULL"
    assert read(grey=buf) == capi.SFMX_ERR_INVALID and read(grey_views=ibuf) == capi.SFMX_ERR_INVALID, "grey after a run without images"
    assert read(normals=np.zeros(12)) == capi.SFMX_ERR_INVALID, "normals after a run without normals"
    assert read(face_views=ibuf) == capi.SFMX_OK and ibuf[:2].tolist() == ref["face_views"].tolist()
    img = VR.images_for(cams, 4)
    ref = _case(s, v, f, cams, c["z_min"], c["depth_tol"], "with images", images=img, cull=0)
    assert read(grey=buf, grey_views=ibuf) == capi.SFMX_OK and buf[:4].tobytes() == ref["grey"].tobytes()
    # reset drops the views and keeps the result; a run without views sees nothing
    s.reset()
    assert s.view_count() == 0 and s.read()["faces_kept"] == 2
    assert s.run(v, f, c["z_min"], c["depth_tol"])["faces_kept"] == 0
    # NULL arguments
    p = capi.visib_params(0.5, 0.1)
    args = (v.ctypes.data_as(P), None, ctypes.c_int(len(v)), f.ctypes.data_as(P), ctypes.c_int(len(f)), ctypes.c_int(0))
    assert lib.sfmx_visib_run(ctx.h_, s.h_, *args, None) == capi.SFMX_ERR_INVALID
    _invalid(s.read)
    assert lib.sfmx_visib_run(ctx.h_, s.h_, None, *args[1:], ctypes.byref(p)) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_visib_add_view(ctx.h_, s.h_, None, None, ctypes.c_int(0)) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_visib_run(ctx.h_, s.h_, *args, ctypes.byref(p)) == capi.SFMX_OK
    ctx.set_timing(True)
    _case(s, v, f, cams, c["z_min"], c["depth_tol"], "timed")
    assert s.last_us() > 0.0
    ctx.set_timing(False)
    s.close()


# ---- feeds -------------------------------------------------------------------------------------------------------------------
def test_feeding_paths_and_handing_on(ctx):
    """host pointers, device pointers, device images, and the device meshes of the fill, smooth and simplify objects as input; the
    result's device mesh into sfmx_raster_run, sfmx_sdist_* and sfmx_shade_vertices equal to the host feed"""
    import torch
    import clean_ref as LR
    import consist_ref as CR
    import fill_ref as FLR
    import simplify_ref as PR
    import smooth_ref as MR
    vol = CR.SPHERE26_VOL
    fu = ctx.fusion(**vol)
    views = CR.sphere8()[:8]
    for cam_, d16 in views:
        fu.add_view(cam_, d16)
    v, f, nrm = fu.extract_normals()
    cams = [dict(cam_, w=d16.shape[1], h=d16.shape[0]) for cam_, d16 in views[:5]]
    img = VR.images_for(cams, 5)
    tol = vol["voxel"]
    s = ctx.visib()
    ref = _case(s, v, f, cams, 0.05, tol, "host pointers", normals=nrm, images=img)
    assert 1000 < ref["faces_kept"] < len(f)
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, f, nrm))
    timg = [torch.from_numpy(i).to("cuda:0") for i in img]
    torch.cuda.synchronize()
    s.reset()
    for cam, ti in zip(cams, timg):
        s.add_view(cam, ti.data_ptr())
    VR.same(s.run(tv.data_ptr(), tf.data_ptr(), 0.05, tol, normals=tn.data_ptr(), n=len(v), m=len(f)), ref, "device pointers and images")
    # hand the result on: raster, sdist and shade read the device mesh in place
    n1, pv1, pf1, m1 = s.device_mesh()
    pn1 = s.device_surface()[2]
    assert (n1, m1) == (ref["verts_kept"], ref["faces_kept"]) and s.device_surface()[:2] == (n1, pv1)
    rs, sd, sh = ctx.raster(), ctx.sdist(), ctx.shade()
    cam = RR.camera((0.25, 0.2, -0.3), (0.0, 0.0, 0.0), 200.0, 120, 90)
    R.same(rs.render(pv1, pf1, cam, 0.05, normals=pn1, n=n1, m=m1), R.render(ref["verts"], ref["faces"], cam, 0.05, ref["normals"]), "into raster")
    q = np.random.default_rng(3).uniform(-0.12, 0.12, (500, 3))
    sd.set_target(pv1, pf1, 4 * tol, nv=n1, m=m1)
    dev = sd.query(q)
    sd.set_target(ref["verts"], ref["faces"], 4 * tol)
    host = sd.query(q)
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes() and (host[1] >= 0).any(), "into sdist"
    rng = np.random.default_rng(12)
    for cam_, d16 in views:
        sh.add_view(cam_, d16, rng.integers(0, 256, d16.shape).astype(np.uint8))
    dev = sh.shade(pv1, pn1, 0.01, n=n1)
    host = sh.shade(ref["verts"], ref["normals"], 0.01)
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes() and (host[1] > 0).any(), "into shade"
    # the device meshes of fill, smooth and simplify as input
    cl, fl, sm, sp = ctx.clean(), ctx.fill(), ctx.smooth(), ctx.simplify()
    _load(s, cams, img)
    cl.fusion(fu)
    lref = LR.clean(v, f, nrm)
    kw = dict(unit=vol["voxel"], origin=vol["origin"])
    fl.clean(cl, max_edges=64, **kw)
    fref = FLR.fill(lref["verts"], lref["faces"], lref["normals"], max_edges=64, **kw)
    n, pv, pf, m = fl.device_mesh()
    pn = fl.device_surface()[2]
    VR.same(s.run(pv, pf, 0.05, tol, normals=pn, n=n, m=m), VR.run(fref["verts"], fref["faces"], cams, 0.05, tol, normals=fref["normals"], images=img),
            "the fill object's device mesh")
    sm.run(pv, pf, n=n, m=m, **kw)
    mref = MR.smooth(fref["verts"], fref["faces"], **kw)
    n2, pv2, pf2, m2 = sm.device_mesh()
    VR.same(s.run(pv2, pf2, 0.05, tol, normals=pn, n=n2, m=m2), VR.run(mref["verts"], fref["faces"], cams, 0.05, tol, normals=fref["normals"], images=img),
            "the smooth object's device mesh")
    sp.run(pv2, pf2, normals=pn, n=n2, m=m2, cell=2 * vol["voxel"], origin=vol["origin"])
    pref = PR.simplify(mref["verts"], fref["faces"], fref["normals"], cell=2 * vol["voxel"], origin=vol["origin"])
    n3, pv3, pf3, m3 = sp.device_mesh()
    want = VR.run(pref["verts"], pref["faces"], cams, 0.05, 2 * tol, normals=pref["normals"], images=img)
    VR.same(s.run(pv3, pf3, 0.05, 2 * tol, normals=sp.device_surface()[2], n=n3, m=m3), want, "the simplify object's device mesh")
    assert want["faces_kept"] > 500
    # and back into simplify from the visibility stage's device mesh
    n4, pv4, pf4, m4 = s.device_mesh()
    sp.run(pv4, pf4, normals=s.device_surface()[2], n=n4, m=m4, cell=4 * vol["voxel"], origin=vol["origin"])
    again = PR.simplify(want["verts"], want["faces"], want["normals"], cell=4 * vol["voxel"], origin=vol["origin"])
    got = sp.read(normals=True)
    assert got["verts"].tobytes() == again["verts"].tobytes() and got["faces"].tobytes() == again["faces"].tobytes()
    for o in (cl, fl, sm, sp, s, rs, sd, sh, fu):
        o.close()


# ---- pipeline ----------------------------------------------------------------------------------------------------------------
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
VIS_KEYS = ("face_views", "face_back_views", "vert_views")


@pytest.fixture(scope="module")
def ring2(ctx):
    """two pairs of the ring-6 fixture, their left rectified cameras and images, and two cameras on the ring"""
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
    cams = [dict(R_rw=poses[i][0].T, c_left=poses[i][1], f=0.3 * K[0, 0], cx=0.3 * K[0, 2], cy=0.3 * K[1, 2], w=96, h=72) for i in (0, 3)]
    return dict(images=images, K=K, poses=poses, pairs=pairs, vol=CR.RING6_VOL, views=views, rects=rects, cams=cams)


def _fuse_args(ctx, r):
    vol = r["vol"]
    return (ctx, r["images"], r["K"], r["poses"], r["pairs"], vol["origin"], vol["voxel"], vol["dims"])


def _check_visibility(m, want, n_in, m_in, what):
    vis = m["visibility"]
    assert m["verts"].tobytes() == want["verts"].tobytes() and m["faces"].tobytes() == want["faces"].tobytes(), what
    for k in VIS_KEYS:
        assert vis[k].dtype == np.int32 and vis[k].tobytes() == want[k].tobytes(), (what, k)
    assert {k: vis[k] for k in VR.COUNTS} == VR.counts(want), what
    assert vis["verts_removed"] == n_in - want["verts_kept"] and vis["faces_removed"] == m_in - want["faces_kept"], what
    assert set(vis) == set(VIS_KEYS) | set(VR.COUNTS) | {"verts_removed", "faces_removed"}


def test_host_fuse_visibility(ctx, ring2, tmp_path):
    args = _fuse_args(ctx, ring2)
    voxel = ring2["vol"]["voxel"]
    p0, p1 = str(tmp_path / "plain.ply"), str(tmp_path / "visib.ply")
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    again = pipe.fuse(*args, num_disparities=64, ply_path=p1, visibility=False)
    assert set(again) == set(m0) and all(again[k].tobytes() == m0[k].tobytes() for k in ("verts", "faces")) and again["warn"] == m0["warn"]
    assert open(p0, "rb").read() == open(p1, "rb").read(), "without visibility the file is what it was"
    m = pipe.fuse(*args, num_disparities=64, ply_path=p1, visibility=dict(z_min=0.05))
    assert set(m) == set(m0) | {"visibility"} and m["views"] == m0["views"] == 2 and m["warn"] == m0["warn"]
    want = VR.run(m0["verts"], m0["faces"], ring2["views"], 0.05, voxel)
    print("fuse: %d v / %d f -> %s" % (len(m0["verts"]), len(m0["faces"]), VR.counts(want)))
    assert 1000 < want["faces_kept"] < len(m0["faces"]) and want["faces_back_only"] > 0
    _check_visibility(m, want, len(m0["verts"]), len(m0["faces"]), "fuse")
    head = open(p1).read(400)
    assert f"element vertex {want['verts_kept']}\n" in head and f"element face {want['faces_kept']}\n" in head, "the PLY is the culled mesh"
    s = ctx.visib()
    _case(s, m0["verts"], m0["faces"], ring2["views"], 0.05, voxel, "standalone", want=want)
    s.close()
    # parameters of its own; measuring only; nothing left; no pairs; refused parameters
    m2 = pipe.fuse(*args, num_disparities=64, visibility=dict(z_min=0.05, depth_tol=2.5 * voxel, min_views=2))
    _check_visibility(m2, VR.run(m0["verts"], m0["faces"], ring2["views"], 0.05, 2.5 * voxel, min_views=2), len(m0["verts"]), len(m0["faces"]), "min_views 2")
    m3 = pipe.fuse(*args, num_disparities=64, visibility=dict(z_min=0.05, min_views=0))
    assert m3["verts"].tobytes() == m0["verts"].tobytes() and m3["faces"].tobytes() == m0["faces"].tobytes() and m3["visibility"]["faces_removed"] == 0
    m4 = pipe.fuse(*args, num_disparities=64, ply_path=str(tmp_path / "none.ply"), appearance=True, visibility=dict(z_min=0.05, min_views=3),
                   raster=dict(cameras=ring2["cams"], w=96, h=72, z_min=0.05, background=7))
    assert m4["verts"].shape == (0, 3) and m4["faces"].shape == (0, 3) and m4["grey"].shape == (0,) and m4["visibility"]["faces_kept"] == 0
    assert m4["visibility"]["faces_removed"] == len(m0["faces"]) and "no faces" in m4["warn"] and not (tmp_path / "none.ply").exists()
    assert all(r["hits"] == 0 and (r["shaded"] == 7).all() for r in m4["rasters"])
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, visibility=dict(z_min=0.05))
    assert empty["verts"].shape == (0, 3) and all(len(empty["visibility"][k]) == 0 for k in VIS_KEYS)
    assert {k: empty["visibility"][k] for k in VR.COUNTS} == dict.fromkeys(VR.COUNTS, 0)
    for bad in (dict(z_min=0.0), dict(z_min=0.05, depth_tol=-1.0), dict(z_min=0.05, cull=2), dict(z_min=0.05, fill=256)):
        with pytest.raises(capi.SfmxError):
            pipe.fuse(*args, num_disparities=64, visibility=bad)


def test_host_fuse_visibility_with_every_other_stage(ctx, ring2, tmp_path):
    """clean, fill, smooth, simplify, appearance, evaluate and raster: the stage culls the final mesh, a kept vertex keeps its normal,
    grey and views (or, with colour, gets this stage's), and the evaluation, the renders and the PLY take the culled mesh"""
    args = _fuse_args(ctx, ring2)
    voxel = ring2["vol"]["voxel"]
    gv, gf = DR.icosphere(3, 0.1)
    ekw = dict(gt_verts=gv, gt_faces=gf, d_max=4 * voxel, tau=voxel)
    zkw = dict(cameras=ring2["cams"], w=96, h=72, z_min=0.05, background=250)
    for cl, fl, smo, simp in ((True, True, True, True), (False, False, False, False)):
        stages = dict(appearance=True, clean=cl, fill=fl, smooth=dict(iters=3) if smo else False, simplify=simp)
        tol = 2 * voxel if simp else voxel
        m0 = pipe.fuse(*args, num_disparities=64, **stages)
        for colour in (False, True):
            p1 = str(tmp_path / "b.ply")
            m = pipe.fuse(*args, num_disparities=64, ply_path=p1, evaluate=ekw, raster=zkw,
                          visibility=dict(z_min=0.05, depth_tol=tol, colour=colour, fill=3), **stages)
            want = VR.run(m0["verts"], m0["faces"], ring2["views"], 0.05, tol, normals=m0["normals"], images=ring2["rects"], fill=3)
            _check_visibility(m, want, len(m0["verts"]), len(m0["faces"]), f"{stages} colour {colour}")
            src = want["vert_src"]
            assert 500 < want["faces_kept"] < len(m0["faces"]) and m["normals"].tobytes() == want["normals"].tobytes()
            if colour:
                assert m["grey"].tobytes() == want["grey"][src].tobytes() and m["vertex_views"].tobytes() == want["grey_views"][src].tobytes()
                assert len(np.unique(m["grey"])) > 10
            else:
                assert m["grey"].tobytes() == m0["grey"][src].tobytes() and m["vertex_views"].tobytes() == m0["vertex_views"][src].tobytes()
            for k in ("clean", "fill", "smooth", "simplify"):
                assert m.get(k) == m0.get(k), k
            for i, (cam, got) in enumerate(zip(ring2["cams"], m["rasters"])):
                R.same(got, R.render(m["verts"], m["faces"], cam, 0.05, m["normals"], m["grey"], background=250), f"raster {i}")
            assert m["evaluation"] == pipe.surface_eval(ctx, m["verts"], m["faces"], gv, gf, d_max=4 * voxel, tau=voxel)
            head = open(p1).read(600)
            assert f"element vertex {want['verts_kept']}\n" in head and f"element face {want['faces_kept']}\n" in head and "property uchar red" in head


def test_pipeline_run_visibility(ctx, tmp_path):
    import json
    import os
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    pair, small = (2, 3), dict(num_disparities=32, census=5)
    plain, with_v = str(tmp_path / "plain"), str(tmp_path / "visib")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in pair)
    mesh = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][pair[0]], r0["kf_poses"][pair[1]], **small)
    lo, hi = mesh["verts"].min(0), mesh["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    fz = dict(pairs=[pair], origin=tuple(lo), voxel=voxel, dims=dims, **small)
    h, w = g["images"].shape[1:]
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain, fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, with_v, fusion=dict(fz, visibility=dict(z_min=1e-3)))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(with_v, "X") and sorted(os.listdir(with_v)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    rect = pipe.stereo_rectify(g["K"], r0["kf_poses"][pair[0]], r0["kf_poses"][pair[1]], w, h)
    view = dict(R_rw=rect["R_rw"], c_left=rect["c_left"], f=rect["f"], cx=rect["cx"], cy=rect["cy"], B=rect["B"], w=w, h=h)
    want = VR.run(m1["verts"], m1["faces"], [view], 1e-3, voxel)
    print("run: %d f -> %s" % (len(m1["faces"]), VR.counts(want)))
    assert set(m) == set(m1) | {"visibility"} and len(m1["faces"]) > 0
    _check_visibility(m, want, len(m1["verts"]), len(m1["faces"]), "pipeline.run")
