"""GPU suite for the photometric re-rendering: every array and count of sfmx_photo is compared byte for byte with
the NumPy restatement (tests/photo_ref.py) -- hand meshes at every patch size, every class, view sizes around the tiles, view
counts around the batch, block edges and contention, scenes, both atlases, every refusal, the feeds and the pipeline.
"""
import ctypes
import importlib

import numpy as np
import pytest

import helpers as H
import level_ref as LR
import photo_ref as P
import raster_ref as R
import raycast_ref as RR
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
    o = ctx.level()
    yield o
    o.close()


@pytest.fixture(scope="module")
def ph(ctx):
    """one object for the whole module: its buffers grow and shrink with the cases"""
    o = ctx.photo()
    yield o
    o.close()


def _texture(tx, v, f, cams, images, z, tol, what, **kw):
    tex = TR.run(v, f, cams, images, z, tol, **kw)
    tx.reset()
    for cam, img in zip(cams, images):
        tx.add_view(cam, img)
    tx.set_batch(0)
    TR.same(tx.run(v, f, z, tol, **kw), tex, f"{what}: the texture run")
    return tex


def _views(ph, cams, images, tvs, batch=0):
    ph.reset()
    for cam, img, k in zip(cams, images, tvs):
        ph.add_view(cam, img, k)
    ph.set_batch(batch)
    assert ph.view_count() == len(cams)


def _photo(ph, tx, v, f, cams, images, tvs, tex, z, what, batches=(0,), lv=None, atlas=None, background=0, patch=8, fill=0):
    """one reference, one device run per batch size; returns the reference"""
    want = P.run(v, f, cams, images, tvs, tex, z, patch=patch, fill=fill, atlas=atlas, background=background)
    for batch in batches:
        _views(ph, cams, images, tvs, batch)
        got = ph.run(tx, v, f, z, lv=lv, background=background)
        P.same(got, want, f"{what}, batch {batch}")
        assert got["offsets"].tolist() == want["offsets"].tolist() and ph.sizes() == (len(cams), int(want["offsets"][-1]))
        assert ph.device_rendered()[0] == int(want["offsets"][-1])
        if cams:
            assert 1 <= ph.last_batch() <= (batch or 64)
    ph.set_batch(0)
    return want


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


# ---- hand meshes and views -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", [3, 4, 8, 64])
def test_hand_meshes(tx, ph, patch):
    v, f, cam, img = P.aligned_face(patch)
    tex = _texture(tx, v, f, [cam], [img], 0.5, 0.0, "aligned", patch=patch)
    want = _photo(ph, tx, v, f, [cam], [img], [0], tex, 0.5, "aligned", patch=patch)
    assert want["stats"][0, 0, 0] > 0 and want["stats"][0, 0, 1] == 0, "texel centres: the picture comes back"
    # both halves of every cell, the first and the last cell (the clamps at 0, W - 1 and H - 1), off-centre pixels, three faces
    for nx, ny in ((1, 1), (2, 1), (5, 5)):
        v, f = P.quilt(nx, ny, 6.0, seed=patch)
        if (nx, ny) == (2, 1):
            f = f[:3]
        w, h = 6 * nx, 6 * ny
        cams = [R.pixel_camera(w, h), R.pixel_camera(w, h, cx=0.375, cy=-0.25)]
        img = VR.images_for(cams, patch)
        for fill in (0, 201):
            tex = _texture(tx, v, f, cams, img, 0.5, 0.25, "quilt", patch=patch, fill=fill)
            want = _photo(ph, tx, v, f, cams, img, [0, 1], tex, 0.5, f"quilt {nx} x {ny}", patch=patch, fill=fill, background=17)
        assert want["classes"][0, 3] > 0 and want["classes"][1, 4] > 0 and want["foreign_weight"] <= P.CONTAIN_W


def test_every_class_an_empty_view_and_a_view_without_an_image(tx, ph):
    v, f, tc, ti, pc, pi, tv = P.five_classes()
    tex = _texture(tx, v, f, tc, ti, 0.5, 0.0, "classes", patch=4, fill=77)
    away = RR.axis_camera((0.0, 0.0, 50.0), 256.0, 9, 7, 0.0, 0.0)  # past the mesh, looking on: nothing in front of it
    cams, imgs, tvs = pc + [away, pc[0], pc[0]], pi + [VR.images_for([away], 1)[0], None, pi[0]], tv + [0, 0, -1]
    want = _photo(ph, tx, v, f, cams, imgs, tvs, tex, 0.5, "classes", batches=(0, 1, 2), patch=4, fill=77, background=9)
    assert want["classes"].tolist() == [[147, 15, 15, 15, 0], [147, 15, 15, 0, 15], [63, 0, 0, 0, 0], [147, 15, 15, 15, 0], [147, 15, 15, 0, 15]]
    assert not want["stats"][2:4].any() and want["stats"][4, 1, 0] == 15 and not want["hist"][3].any()


def test_view_sizes_around_the_tiles(tx, ph):
    v, f, _ = VR.soup(60, 7)
    tcams = [R.pixel_camera(24, 20, cx=3.0, cy=-2.0), R.pixel_camera(24, 20, f=200.0)]
    timg = VR.images_for(tcams, 3)
    tex = _texture(tx, v, f, tcams, timg, 0.5, 0.5, "sizes")
    cams = VR.mixed_views() + [R.pixel_camera(s, s, cx=1.0) for s in (7, 8, 9, 15, 16, 17, 33)] + tcams
    imgs = VR.images_for(cams, 4)
    imgs[3] = None
    tvs = [k % 3 - 1 for k in range(len(cams) - 2)] + [0, 1]
    want = _photo(ph, tx, v, f, cams, imgs, tvs, tex, 0.5, "sizes", batches=(0, 1, 3, 64), background=200)
    assert [int(c["w"]) * int(c["h"]) for c in cams[:6]] == [1, 63, 64, 272, 256, 4096]
    assert want["classes"][-2:, 3].min() > 0 and want["classes"][:, 4].sum() > 0 and want["classes"][:, 2].sum() > 0


# ---- batching --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 2, 63, 64, 65])
def test_view_counts_under_every_batch_size(tx, ph, Q):
    v, f, _ = VR.soup(60, 7)
    tcams = [R.pixel_camera(24, 20, cx=3.0, cy=-2.0), R.pixel_camera(24, 20, f=200.0)]
    tex = _texture(tx, v, f, tcams, VR.images_for(tcams, 3), 0.5, 0.5, "counts")
    base = tcams + VR.mixed_views()[1:5]
    cams = [base[k % len(base)] for k in range(Q)]
    imgs = VR.images_for(cams, Q)
    tvs = [(k % len(base)) if k % len(base) < 2 else -1 for k in range(Q)]
    want = _photo(ph, tx, v, f, cams, imgs, tvs, tex, 0.5, f"{Q} views", batches=(1, 2, 64, 0))
    assert want["stats"][0, 0, 0] > 0 and ph.last_batch() == min(Q, 64)


# ---- block edges and contention ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 65537])
def test_strips_at_the_block_edges(tx, ph, m):
    v, f, h = P.strips(m)
    cams = [R.pixel_camera(64, h), R.pixel_camera(64, h, cx=0.25, cy=0.125)]
    img = VR.images_for(cams, m)
    tex = _texture(tx, v, f, cams, img, 0.5, 0.25, f"strips {m}", patch=3)
    want = _photo(ph, tx, v, f, cams, img, [0, 1], tex, 0.5, f"strips {m}", patch=3)
    assert tex["faces_textured"] == m and want["classes"][:, 3:].sum() >= m // 2


def test_65536_faces_on_one_pixel(tx, ph):
    v, f = R.hot_pixel(65536)
    f[::2] = f[::2, ::-1].copy()  # as built every face is back-facing: turn every other one
    cams = [R.pixel_camera(8, 8)]
    img = VR.images_for(cams, 2)
    tex = _texture(tx, v, f, cams, img, 0.5, 2.0, "hot pixel", patch=3)  # the depths span 1 .. 2: no vertex counts as occluded
    want = _photo(ph, tx, v, f, cams + cams, img + img, [0, -1], tex, 0.5, "hot pixel", patch=3)
    assert want["classes"][0, 0] < 64 and tex["faces_textured"] == 32768 and want["classes"][0, 3] + want["classes"][0, 1] > 0


def test_every_pixel_adds_to_one_histogram_bin(tx, ph):
    """two faces over the whole of a 512 x 512 held-out view, textured from a wider camera that has their corners in its image"""
    v = R.at_pixels([(-2, -2), (-2, 514), (514, 514), (514, -2)])
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    wide = R.pixel_camera(520, 520, cx=3.0, cy=3.0)
    tex = _texture(tx, v, f, [wide], [np.full((520, 520), 100, np.uint8)], 0.5, 0.25, "one bin", fill=100)
    assert (tex["atlas"] == 100).all() and tex["faces_textured"] == 2
    cam = R.pixel_camera(512, 512)
    want = _photo(ph, tx, v, f, [cam], [np.full((512, 512), 93, np.uint8)], [-1], tex, 0.5, "one bin", fill=100)
    assert want["hist"][0, 1, 7] == 512 * 512 and want["stats"][0, 1].tolist() == [262144, 7 * 262144, 49 * 262144] and not want["stats"][0, 0].any()


# ---- scenes and atlases ----------------------------------------------------------------------------------------------------------
def test_random_soup(tx, ph):
    v, f, _ = VR.soup(2000, 11, 64, 48)
    cams = [R.pixel_camera(64, 48), R.pixel_camera(64, 48, f=200.0, cx=10.0, cy=8.0), R.pixel_camera(40, 40, f=300.0, cx=-20.0, cy=-10.0)]
    img = VR.images_for(cams, 12)
    tex = _texture(tx, v, f, cams, img, 0.5, 0.5, "soup")
    extra = R.pixel_camera(50, 30, f=220.0, cx=5.0, cy=3.0)
    want = _photo(ph, tx, v, f, cams + [extra], img + VR.images_for([extra], 13), [0, 1, 2, -1], tex, 0.5, "soup", batches=(0, 3))
    assert want["classes"][:, 1].sum() > 0 and want["classes"][:, 2].sum() > 0 and want["classes"][:3, 3].min() > 0
    assert want["classes"][3, 3] == 0 and want["classes"][3, 4] > 0
    tex = _texture(tx, v, f, cams, img, 0.5, 0.5, "soup", patch=5, cells_per_row=7, fill=255)
    _photo(ph, tx, v, f, cams, img, [0, 1, 2], tex, 0.5, "soup, own layout", patch=5, fill=255)


def test_spheres_as_built_permuted_rotated_and_views_permuted_under_both_atlases(tx, lv, ph):
    v, f, _, no, mo = VR.nested_spheres()
    cams = VR.six_cameras()
    img = VR.images_for(cams, 1)
    tvs = list(range(6))
    tex = _texture(tx, v, f, cams, img, VR.Z_MIN, 0.002, "nested")
    a = _photo(ph, tx, v, f, cams, img, tvs, tex, VR.Z_MIN, "nested", batches=(0, 4))
    assert a["classes"][:, 3].min() > 1000 and a["classes"][:, 4].min() > 100 and (a["face"] < mo).all(), "the inner sphere is never seen"
    lev = LR.run(v, f, cams, img, tex)
    LR.same(lv.run(tx, v, f), lev, "nested: the level run")
    b = _photo(ph, tx, v, f, cams, img, tvs, tex, VR.Z_MIN, "nested, levelled", lv=lv, atlas=lev["atlas"])
    assert b["cls"].tobytes() == a["cls"].tobytes() and b["rendered"].tobytes() != a["rendered"].tobytes()
    _photo(ph, tx, v, f, cams, img, tvs, tex, VR.Z_MIN, "nested, the texture's atlas again")
    fp, perm = R.permute_faces(f, 4)
    tp = _texture(tx, v, fp, cams, img, VR.Z_MIN, 0.002, "faces permuted")
    c = _photo(ph, tx, v, fp, cams, img, tvs, tp, VR.Z_MIN, "faces permuted")
    assert c["classes"].tobytes() == a["classes"].tobytes() and np.array_equal(perm[c["face"][c["face"] >= 0]], a["face"][a["face"] >= 0])
    fr = R.rotate_corners(f, 5)
    tr = _texture(tx, v, fr, cams, img, VR.Z_MIN, 0.002, "corners rotated")
    d = _photo(ph, tx, v, fr, cams, img, tvs, tr, VR.Z_MIN, "corners rotated")
    assert d["classes"].tobytes() == a["classes"].tobytes() and d["face"].tobytes() == a["face"].tobytes()
    tex = _texture(tx, v, f, cams, img, VR.Z_MIN, 0.002, "nested again")
    order = [int(i) for i in np.random.default_rng(6).permutation(6)]
    e = _photo(ph, tx, v, f, [cams[i] for i in order], [img[i] for i in order], order, tex, VR.Z_MIN, "views permuted", batches=(4,))
    assert e["stats"].tobytes() == a["stats"][order].tobytes() and e["hist"].tobytes() == a["hist"][order].tobytes()


# ---- errors and state ------------------------------------------------------------------------------------------------------------
def test_invalid_inputs_each_followed_by_a_good_call(ctx, tx, lv, ph):
    import torch
    v, f, tc, ti, pc, pi, tv = P.five_classes()
    z = 0.5
    tex = TR.run(v, f, tc, ti, z, 0.0, patch=4)
    want = P.run(v, f, pc, pi, tv, tex, z, patch=4)

    def textured():
        _texture(tx, v, f, tc, ti, z, 0.0, "refusals", patch=4)

    def good_call(what):
        textured()
        _views(ph, pc, pi, tv)
        P.same(ph.run(tx, v, f, z), want, "after " + what)

    def refused(fn, what):
        _invalid(fn)
        _invalid(ph.read)  # the failed run left no result
        with pytest.raises(capi.SfmxError):
            ph.sizes()
        assert ph.device_rendered() == (-1, None) and ph.last_batch() == 0
        good_call(what)

    good_call("nothing")
    fresh = ctx.texture()
    refused(lambda: ph.run(fresh, v, f, z), "a texture object that never ran")
    fresh.close()
    bad = f.copy()
    bad[1, 1] = len(v)
    _invalid(lambda: tx.run(v, bad, z, 0.0, patch=4))
    refused(lambda: ph.run(tx, v, f, z), "a texture object whose last run failed")
    refused(lambda: ph.run(tx, v[:-1], f, z), "n - 1")
    refused(lambda: ph.run(tx, np.concatenate([v, v[:1]]), f, z), "n + 1")
    refused(lambda: ph.run(tx, v, f[:-1], z), "m - 1")
    refused(lambda: ph.run(tx, v, np.concatenate([f, f[:1]]), z), "m + 1")
    fresh = ctx.level()
    refused(lambda: ph.run(tx, v, f, z, lv=fresh), "a level object that never ran")
    fresh.close()
    sv, sf, scams, simg = LR.roof()
    other = ctx.texture()
    _texture(other, sv, sf, scams, simg, 0.5, 0.25, "another atlas")
    lv.run(other, sv, sf)
    assert lv.device_atlas()[2:] != (tex["W"], tex["H"])
    refused(lambda: ph.run(tx, v, f, z, lv=lv), "a level object with another W and H")
    other.close()
    for k in (1, 2, 2 ** 31 - 1):
        textured()
        _views(ph, pc, pi, [0, k])
        refused(lambda: ph.run(tx, v, f, z), f"tex_view {k} of 1")
    for k in (-2, -2 ** 31):
        _invalid(lambda: ph.add_view(pc[0], pi[0], k))
    for index in (-1, len(v), 2 ** 31 - 1, -2 ** 31):
        for corner in range(3):
            bad = f.copy()
            bad[2, corner] = index
            refused(lambda: ph.run(tx, v, bad, z), f"index {index}")
    # more than 2^28 pixels: refused before anything is allocated (views without images take no memory)
    ph.reset()
    for _ in range(17):
        ph.add_view(R.pixel_camera(4096, 4096))
    free0 = torch.cuda.mem_get_info()[0]
    refused(lambda: ph.run(tx, v, f, z), "more than 2^28 pixels")
    assert free0 - torch.cuda.mem_get_info()[0] < (1 << 27), "refused before the outputs are allocated"
    for p in P.BAD_PARAMS:
        assert not capi.photo_check_params(**p) and not P.check_params(**p)
        refused(lambda: ph.run(tx, v, f, **p), str(p))
    lib, VP = ctx.lib, ctypes.c_void_p
    p = capi.photo_params(z)
    args = (v.ctypes.data_as(VP), ctypes.c_int(len(v)), f.ctypes.data_as(VP), ctypes.c_int(len(f)), ctypes.c_int(0))
    refused(lambda: ctx._chk(lib.sfmx_photo_run(ctx.h_, ph.h_, tx.h_, None, *args, None)), "NULL parameters")
    refused(lambda: ctx._chk(lib.sfmx_photo_run(ctx.h_, ph.h_, None, None, *args, ctypes.byref(p))), "a NULL texture object")
    refused(lambda: ctx._chk(lib.sfmx_photo_run(ctx.h_, ph.h_, tx.h_, None, None, *args[1:], ctypes.byref(p))), "NULL vertices")
    refused(lambda: ctx._chk(lib.sfmx_photo_run(ctx.h_, ph.h_, tx.h_, None, args[0], args[1], None, args[3], args[4], ctypes.byref(p))), "NULL faces")
    assert lib.sfmx_photo_run(ctx.h_, None, tx.h_, None, *args, ctypes.byref(p)) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_photo_read(ctx.h_, ph.h_, None, None, None, None, None, None) == capi.SFMX_OK, "every pointer may be NULL"
    for bad_cam in ({**pc[0], "w": 4097, "h": 1}, {**pc[0], "w": 0}, {**pc[0], "f": 0.0}, {**pc[0], "cx": float("nan")}):
        n0 = ph.view_count()
        _invalid(lambda: ph.add_view(bad_cam))
        assert ph.view_count() == n0
    for k in (-1, 65):
        with pytest.raises(capi.SfmxError):
            ph.set_batch(k)
    with pytest.raises(TypeError):
        ph.run(tx, v, f, z, cull=1)
    assert ph.sizes() == (2, 2 * 24 * 8), "refused in Python, before the library: the result stays"
    for p in P.GOOD_PARAMS[:2] + P.GOOD_PARAMS[3:]:
        assert capi.photo_check_params(**p) and P.check_params(**p)


def test_empty_inputs_and_state_rules(ctx):
    s, t = ctx.photo(), ctx.texture()
    _invalid(s.read)
    assert s.device_rendered() == (-1, None) and s.last_us() == 0.0 and s.last_resolve_us() == 0.0 and s.view_count() == 0
    v, f, tc, ti, pc, pi, tv = P.five_classes()
    tex = _texture(t, v, f, tc, ti, 0.5, 0.0, "state", patch=4)
    want = _photo(s, t, v, f, [], [], [], tex, 0.5, "no views", patch=4)
    assert len(want["rendered"]) == 0 and s.sizes() == (0, 0)
    none = np.zeros((0, 3), np.int32)
    tex0 = _texture(t, v, none, tc, ti, 0.5, 0.0, "no faces", patch=4)
    want = _photo(s, t, v, none, pc, pi, tv, tex0, 0.5, "no faces", patch=4, background=5)
    assert want["classes"].tolist() == [[192, 0, 0, 0, 0]] * 2 and set(want["rendered"]) == {5}
    tex0 = _texture(t, np.zeros((0, 3)), none, tc, ti, 0.5, 0.0, "nothing", patch=4)
    _photo(s, t, np.zeros((0, 3)), none, pc, pi, tv, tex0, 0.5, "nothing", patch=4)
    tex = _texture(t, v, f, tc, ti, 0.5, 0.0, "state", patch=4)
    # reset drops the views and keeps the result; views added after a run count from the next run on
    _photo(s, t, v, f, pc, pi, tv, tex, 0.5, "two views", patch=4)
    s.reset()
    assert s.view_count() == 0 and s.sizes() == (2, 384) and s.shapes == []
    ctx.set_timing(True)
    _photo(s, t, v, f, pc, pi, tv, tex, 0.5, "timed", batches=(1,), patch=4)
    assert 0.0 < s.last_resolve_us() <= s.last_us()
    ctx.set_timing(False)
    _photo(s, t, v, f, pc, pi, tv, tex, 0.5, "untimed", patch=4)
    assert s.last_us() == 0.0 and s.last_resolve_us() == 0.0
    s.close()
    t.close()


# ---- feeds -------------------------------------------------------------------------------------------------------------------
def test_feeding_paths_and_sizes_large_small_large(ctx):
    """host pointers, device pointers, add_texture_views, the device meshes of the visibility and the simplify objects; one object
    used large, small, large"""
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
    tvs = list(range(5))
    s, t = ctx.photo(), ctx.texture()
    tex = _texture(t, v, f, cams, img, 0.05, tol, "host pointers", patch=4)
    ref = _photo(s, t, v, f, cams, img, tvs, tex, 0.05, "host pointers", patch=4)
    assert ref["classes"][:, 3].min() > 100
    s.reset()
    s.add_texture_views(t)
    assert s.view_count() == 5 and s.shapes == t.shapes
    P.same(s.run(t, v, f, 0.05), ref, "add_texture_views")
    sv, sf, scams, simg = LR.roof()
    stex = _texture(t, sv, sf, scams, simg, 0.5, 0.25, "small")
    _photo(s, t, sv, sf, scams, simg, [0, 1], stex, 0.5, "small after large")
    tv_, tf_ = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, f))
    timg = [torch.from_numpy(i).to("cuda:0") for i in img]
    torch.cuda.synchronize()
    _texture(t, v, f, cams, img, 0.05, tol, "large again", patch=4)
    _views(s, cams, [int(i.data_ptr()) for i in timg], tvs)
    P.same(s.run(t, tv_.data_ptr(), tf_.data_ptr(), 0.05, n=len(v), m=len(f)), ref, "device pointers, large again")
    vb = ctx.visib()
    for cam in cams:
        vb.add_view(cam)
    vres = vb.run(v, f, 0.05, tol)
    n1, pv1, pf1, m1 = vb.device_mesh()
    t.run(pv1, pf1, 0.05, tol, n=n1, m=m1)
    tex1 = TR.run(vres["verts"], vres["faces"], cams, img, 0.05, tol)
    _views(s, cams, img, tvs)
    P.same(s.run(t, pv1, pf1, 0.05, n=n1, m=m1), P.run(vres["verts"], vres["faces"], cams, img, tvs, tex1, 0.05),
           "the visibility object's device mesh")
    sp = ctx.simplify()
    sp.run(tv_.data_ptr(), tf_.data_ptr(), n=len(v), m=len(f), cell=2 * vol["voxel"], origin=vol["origin"])
    pref = PR.simplify(v, f, None, cell=2 * vol["voxel"], origin=vol["origin"])
    n3, pv3, pf3, m3 = sp.device_mesh()
    t.run(pv3, pf3, 0.05, 2 * tol, n=n3, m=m3)
    tex3 = TR.run(pref["verts"], pref["faces"], cams, img, 0.05, 2 * tol)
    P.same(s.run(t, pv3, pf3, 0.05, n=n3, m=m3), P.run(pref["verts"], pref["faces"], cams, img, tvs, tex3, 0.05),
           "the simplify object's device mesh")
    for o in (sp, vb, s, t, fu):
        o.close()


def test_the_calibrated_errors_from_the_device(tx, ph):
    """the device's renders of the textured sphere give the CPU suite's figures (they are the same bytes)"""
    import test_photo_cpu as C
    v, f, cams, img = TR.fidelity_scene()
    z, tol, S = TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"], TR.FIDELITY["patch"]
    even, odd = list(range(0, 26, 2)), list(range(1, 26, 2))
    tex = _texture(tx, v, f, [cams[k] for k in even], [img[k] for k in even], z, tol, "sphere", patch=S)
    _views(ph, cams, img, [k // 2 if k % 2 == 0 else -1 for k in range(26)])
    got = ph.run(tx, v, f, z)
    s = capi.photo_summary(got["stats"][odd], got["hist"][odd])
    own = P.pooled(got, even, 0)
    print("held-out MAE %.5f, p90 %d; own MAE %.5f" % (s["cross"]["mae"], s["cross"]["p90"], own["mae"]))
    assert abs(s["cross"]["mae"] - C.MEASURED["held"]) < 5e-5 and s["cross"]["p90"] == C.MEASURED["held_p90"] and s["own"]["count"] == 0
    assert abs(own["mae"] - C.MEASURED["own"]) < 5e-5 and abs(P.pooled(got, even, 1)["mae"] - C.MEASURED["cross"]) < 5e-5
    assert s["cross"]["mae"] <= C.BOUND_HELD and own["mae"] <= C.BOUND_OWN and int(got["classes"][odd, 2].sum()) == 0


# ---- pipeline ----------------------------------------------------------------------------------------------------------------
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
PHOTO_KEYS = ("rendered", "cls", "face", "classes", "stats", "hist", "summary")


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


def _check_photo(m, views, rects, tex, what, atlas=None, prefix=None, **kw):
    want = P.run(m["verts"], m["faces"], views, rects, list(range(len(views))), tex, 0.05, atlas=atlas, **kw)
    got = m["photo"]
    assert set(got) == set(PHOTO_KEYS), what
    flat = dict(got, rendered=got["rendered"].ravel(), cls=got["cls"].ravel(), face=got["face"].ravel())
    P.same(flat, want, what)
    assert got["rendered"].shape == (len(views), 240, 320) and got["summary"] == capi.photo_summary(want["stats"], want["hist"])
    if prefix:
        for q in range(len(views)):
            assert open(f"{prefix}_{q}_photo.pgm", "rb").read() == P.pgm(P.view_image(want, views, q)), q
    return want


def test_host_fuse_photo(ctx, ring2, tmp_path):
    args = _fuse_args(ctx, ring2)
    voxel = ring2["vol"]["voxel"]
    views, rects = ring2["views"], ring2["rects"]
    p0, p1 = str(tmp_path / "tex.ply"), str(tmp_path / "pho.ply")
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0, texture=dict(z_min=0.05))
    again = pipe.fuse(*args, num_disparities=64, ply_path=p1, texture=dict(z_min=0.05), photo=False)
    assert set(again) == set(m0) and open(p0, "rb").read() == open(p1, "rb").read(), "without photo everything is what it was"
    prefix = str(tmp_path / "view")
    m = pipe.fuse(*args, num_disparities=64, ply_path=p1, texture=dict(z_min=0.05), photo=dict(pgm_prefix=prefix))
    assert set(m) == set(m0) | {"photo"} and m["views"] == m0["views"] == 2 and m["warn"] == m0["warn"]
    assert m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read(), "the PLY is what it is without photo"
    TR.same(m["texture"], m0["texture"], "the texture beside photo")
    tex = TR.run(m0["verts"], m0["faces"], views, rects, 0.05, voxel)
    want = _check_photo(m, views, rects, tex, "fuse", prefix=prefix)
    print("fuse: own %s, cross %s" % (m["photo"]["summary"]["own"], m["photo"]["summary"]["cross"]))
    assert want["classes"][:, 3].min() > 1000 and want["classes"][:, 4].min() > 100
    # with level the levelled atlas is rendered; a background and a texture layout of their own
    m1 = pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05), level=True)
    m2 = pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05), level=True, photo=True)
    assert set(m2) == set(m1) | {"photo"}
    LR.same(m2["level"], m1["level"], "the level beside photo")
    lev = LR.run(m0["verts"], m0["faces"], views, rects, tex)
    lw = _check_photo(m2, views, rects, tex, "fuse with level", atlas=lev["atlas"])
    assert lw["rendered"].tobytes() != want["rendered"].tobytes()
    xkw = dict(patch=5, cells_per_row=40, fill=99)
    m3 = pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05, depth_tol=2.5 * voxel, **xkw), photo=dict(background=200))
    tex3 = TR.run(m0["verts"], m0["faces"], views, rects, 0.05, 2.5 * voxel, **xkw)
    _check_photo(m3, views, rects, tex3, "own parameters", patch=5, fill=99, background=200)
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, texture=dict(z_min=0.05), photo=True)
    assert empty["verts"].shape == (0, 3) and empty["photo"]["rendered"].shape == (0, 0, 0) and empty["photo"]["classes"].shape == (0, 5)
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05), photo=dict(z_min=1.0))
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, photo=True)


def test_host_fuse_photo_with_every_other_stage(ctx, ring2, tmp_path):
    """clean, fill, smooth, simplify, appearance, visibility and level: the final mesh is rendered, and everything else is what it
    is without photo"""
    args = _fuse_args(ctx, ring2)
    voxel = ring2["vol"]["voxel"]
    views, rects = ring2["views"], ring2["rects"]
    stages = dict(appearance=True, clean=True, fill=True, smooth=dict(iters=3), simplify=True, level=dict(iterations=16))
    for vis in (False, dict(z_min=0.05, depth_tol=2 * voxel)):
        p0, p1 = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
        xkw = dict(z_min=0.05, depth_tol=2 * voxel)
        m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0, visibility=vis, texture=xkw, **stages)
        m = pipe.fuse(*args, num_disparities=64, ply_path=p1, visibility=vis, texture=xkw, photo=True, **stages)
        assert set(m) == set(m0) | {"photo"} and open(p0, "rb").read() == open(p1, "rb").read()
        for k in ("verts", "faces", "normals", "grey", "vertex_views"):
            assert m[k].tobytes() == m0[k].tobytes(), k
        for k in ("clean", "fill", "smooth", "simplify"):
            assert m[k] == m0[k], k
        TR.same(m["texture"], m0["texture"], "the texture beside photo")
        LR.same(m["level"], m0["level"], "the level beside photo")
        tex = TR.run(m0["verts"], m0["faces"], views, rects, 0.05, 2 * voxel)
        _check_photo(m, views, rects, tex, f"every stage, visibility {bool(vis)}", atlas=m0["level"]["atlas"])


def test_pipeline_run_photo(ctx, tmp_path):
    import json
    import os
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    pair, small = (2, 3), dict(num_disparities=32, census=5)
    plain, with_p = str(tmp_path / "tex"), str(tmp_path / "pho")
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
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, with_p, fusion=dict(fz, photo=True))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(with_p, "X") and sorted(os.listdir(with_p)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m) == set(m1) | {"photo"} and len(m1["faces"]) > 0 and m["verts"].tobytes() == m1["verts"].tobytes()
    TR.same(m["texture"], m1["texture"], "pipeline.run: the texture beside photo")
    rect = pipe.stereo_rectify(g["K"], r0["kf_poses"][pair[0]], r0["kf_poses"][pair[1]], w, h)
    view = dict(R_rw=rect["R_rw"], c_left=rect["c_left"], f=rect["f"], cx=rect["cx"], cy=rect["cy"], B=rect["B"], w=w, h=h)
    il, ir = (g["images"][fb], g["images"][fa]) if rect["swapped"] else (g["images"][fa], g["images"][fb])
    st = ctx.stereo(w, h, **small)
    left = st.disparity(il, ir, rect["H_l"], rect["H_r"], want_rect=True)["rect"][0].copy()
    st.close()
    tex = TR.run(m1["verts"], m1["faces"], [view], [left], 1e-3, voxel)
    want = P.run(m1["verts"], m1["faces"], [view], [left], [0], tex, 1e-3)
    flat = dict(m["photo"], rendered=m["photo"]["rendered"].ravel(), cls=m["photo"]["cls"].ravel(), face=m["photo"]["face"].ravel())
    P.same(flat, want, "pipeline.run")
    assert want["classes"][0, 3] > 0 and want["classes"][0, 4] == 0, "one view: every textured pixel is its own"
