"""GPU suite: the best-view per-face texture atlas on the device.  sfmx_texture_* gives the atlas, face_view, face_area, uv_half,
view_faces and all six counts byte for byte against the NumPy restatement (tests/texture_ref.py): hand meshes of one, two and
three faces and a face no view sees at four patch sizes, vertices on the image's clamps, a 1 x 1 and a 4 096 x 1 view, two views
with exactly the same area in both orders, the nested spheres as built, permuted, rotated and with the views permuted, 1 to 65
views under every batch size, views of mixed sizes, face counts at the block edges and past 2^16 under three row lengths, 65 536
faces on one pixel, a random soup, every invalid input followed by a good call, every feed, visibility culling first, the
fidelity on the textured sphere, and pipeline.fuse / pipeline.run."""
import ctypes
import importlib

import numpy as np
import pytest

import helpers as H
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
    """one object for the whole module: its views and buffers grow and shrink with the cases"""
    o = ctx.texture()
    yield o
    o.close()


def _load(tx, cams, images, batch=0):
    tx.reset()
    for cam, img in zip(cams, images):
        tx.add_view(cam, img)
    assert tx.view_count() == len(cams)
    tx.set_batch(batch)


def _case(tx, v, f, cams, images, z_min, tol, what, batch=0, want=None, **kw):
    if want is None:
        want = TR.run(v, f, cams, images, z_min, tol, **kw)
    _load(tx, cams, images, batch)
    got = tx.run(v, f, z_min, tol, **kw)
    TR.same(got, want, f"{what} {kw} batch {batch}")
    assert tx.counts() == TR.counts(want)
    assert tx.sizes() == (len(np.reshape(v, (-1, 3))), len(np.reshape(f, (-1, 3))), len(cams), want["W"], want["H"])
    assert got["uv"].tobytes() == TR.uv(want["uv_half"], want["W"], want["H"]).tobytes()
    assert tx.device_atlas()[0] == want["W"] * want["H"] and int(want["view_faces"].sum()) == want["faces_textured"]
    return want


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


def _ramp(w, h, seed=0):
    """an image with a gradient and noise: a wrong pixel, a wrong weight and a swapped axis all show"""
    y, x = np.mgrid[0:h, 0:w]
    return ((7 * x + 13 * y + np.random.default_rng(seed).integers(0, 40, (h, w))) % 256).astype(np.uint8)


# ---- hand meshes -------------------------------------------------------------------------------------------------------------
HAND_TOL = 2.0  # the hand faces overlap in the image between depths 1 and 3: with this tolerance no vertex is occluded


def _hand(faces, unseen=False):
    """`faces` front-facing faces over a 12 x 10 image and, with unseen, one wound the other way (no view sees it)"""
    tri = [[(1.2, 1.1), (1.6, 7.3), (6.4, 2.2)], [(5.0, 3.0), (5.5, 8.5), (10.5, 4.0)], [(2.0, 6.0), (3.0, 9.0), (7.0, 8.0)]][:faces]
    uv = [p for t in tri for p in t]
    z = [1.0 + 0.125 * k for k in range(len(uv))]
    if unseen:
        uv += [(8.0, 1.0), (10.0, 1.0), (9.0, 3.0)]
        z += [3.0] * 3
    return R.at_pixels(uv, z), np.arange(len(uv), dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("patch", [3, 4, 8, 64])
def test_hand_meshes(tx, patch):
    cams, img = [R.pixel_camera(12, 10)], [_ramp(12, 10)]
    for faces, unseen in ((1, False), (2, False), (3, False), (1, True), (2, True), (3, True)):
        v, f = _hand(faces, unseen)
        for fill in (0, 201):
            want = _case(tx, v, f, cams, img, 0.5, HAND_TOL, f"{faces} faces, unseen {unseen}", patch=patch, fill=fill)
        assert want["faces_textured"] == faces and want["faces_untextured"] == int(unseen)
        assert want["cells"] == (faces + 1) // 2 + int(unseen) and (want["face_view"][:faces] == 0).all()
        if unseen:
            assert want["face_view"][-1] == -1 and want["face_area"][-1] == 0 and len(np.unique(want["uv_half"][-1], axis=0)) == 1
    assert len(np.unique(want["atlas"])) > 2


def test_the_clamps(tx):
    """vertices whose nearest pixel is column 0 with u in [-0.5, 0) and column w - 1 with u in (w - 1, w - 0.5), and the same on
    rows: the texels near them sample with x0 = -1 or xi1 = w, both clamped"""
    w, h = 9, 7
    cams, img = [R.pixel_camera(w, h)], [_ramp(w, h, 3)]
    v = R.at_pixels([(-0.4, 1.0), (-0.3, 5.0), (4.0, 3.0), (w - 0.6, 1.0), (4.0, 2.0), (w - 0.7, 5.0), (1.0, -0.45), (4.0, 3.5), (7.0, -0.35),
                     (1.0, h - 0.6), (7.0, h - 0.55), (4.0, 2.5)], 1.0)
    f = np.arange(12, dtype=np.int32).reshape(4, 3)
    want = _case(tx, v, f, cams, img, 0.5, 0.25, "clamps", patch=8, fill=9)
    assert want["faces_textured"] == 4


def test_one_pixel_and_one_row_views(tx):
    v = R.at_pixels([(-0.4, -0.4), (-0.3, 0.4), (0.4, 0.1)], 1.0)
    f = np.array([[0, 1, 2]], np.int32)
    want = _case(tx, v, f, [R.pixel_camera(1, 1)], [np.full((1, 1), 77, np.uint8)], 0.5, 0.25, "1 x 1")
    assert want["faces_textured"] == 1 and set(np.unique(want["atlas"])) == {0, 77}
    v = R.at_pixels([(3.0, -0.4), (2.0, 0.4), (4090.2, 0.3)], 1.0)
    want = _case(tx, v, f, [R.pixel_camera(4096, 1)], [_ramp(4096, 1, 5)], 0.5, 0.25, "4096 x 1", patch=64)
    assert want["faces_textured"] == 1 and len(np.unique(want["atlas"])) > 20


def test_a_tie_goes_to_the_smaller_view_index(tx):
    v, f = _hand(3)
    a, b = R.pixel_camera(12, 10), R.pixel_camera(12, 10)
    big = R.pixel_camera(24, 20, f=512.0)
    ia, ib, ibig = _ramp(12, 10, 1), _ramp(12, 10, 2), _ramp(24, 20, 3)
    for cams, img, view in (([a, b], [ia, ib], 0), ([b, a], [ib, ia], 0), ([a, big, b], [ia, ibig, ib], 1), ([big, a], [ibig, ia], 0)):
        want = _case(tx, v, f, cams, img, 0.5, HAND_TOL, "tie")
        assert (want["face_view"] == view).all()


# ---- the spheres -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spheres():
    v, f, _, no, mo = VR.nested_spheres()
    cams = VR.six_cameras()
    img = VR.images_for(cams, 1)
    return dict(v=v, f=f, cams=cams, img=img, no=no, mo=mo, ref=TR.run(v, f, cams, img, VR.Z_MIN, 0.002))


def test_spheres_as_built_permuted_rotated_and_views_permuted(tx, spheres):
    v, f, cams, img, a = (spheres[k] for k in ("v", "f", "cams", "img", "ref"))
    mo = spheres["mo"]
    _case(tx, v, f, cams, img, VR.Z_MIN, 0.002, "nested", want=a)
    assert (a["face_view"][mo:] == -1).all() and (a["face_view"][:mo] >= 0).all() and a["faces_untextured"] == len(f) - mo
    fp, perm = R.permute_faces(f, 4)
    b = _case(tx, v, fp, cams, img, VR.Z_MIN, 0.002, "faces permuted")
    assert (b["face_view"] == a["face_view"][perm]).all() and (b["face_area"] == a["face_area"][perm]).all()
    assert b["view_faces"].tobytes() == a["view_faces"].tobytes() and TR.counts(b) == TR.counts(a)
    fr = R.rotate_corners(f, 5)
    c = _case(tx, v, fr, cams, img, VR.Z_MIN, 0.002, "corners rotated")
    assert c["face_view"].tobytes() == a["face_view"].tobytes() and c["face_area"].tobytes() == a["face_area"].tobytes()
    assert c["uv_half"].tobytes() == a["uv_half"].tobytes() and c["atlas"].tobytes() != a["atlas"].tobytes()
    order = np.random.default_rng(6).permutation(len(cams))
    d = _case(tx, v, f, [cams[i] for i in order], [img[i] for i in order], VR.Z_MIN, 0.002, "views permuted")
    assert d["face_area"].tobytes() == a["face_area"].tobytes() and ((d["face_view"] >= 0) == (a["face_view"] >= 0)).all()


def test_visibility_culling_first_leaves_nothing_untextured(ctx, tx, spheres):
    v, f, cams, img = (spheres[k] for k in ("v", "f", "cams", "img"))
    vb = ctx.visib()
    for cam in cams:
        vb.add_view(cam)
    got = vb.run(v, f, VR.Z_MIN, 0.002, read=False)
    n1, pv, pf, m1 = vb.device_mesh()
    assert (n1, m1) == (spheres["no"], spheres["mo"]) and got["faces_kept"] == m1
    _load(tx, cams, img)
    dev = tx.run(pv, pf, VR.Z_MIN, 0.002, n=n1, m=m1)
    TR.same(dev, TR.run(v[:n1], f[:m1], cams, img, VR.Z_MIN, 0.002), "the visib object's device mesh")
    assert dev["faces_untextured"] == 0 and dev["faces_textured"] == m1
    vb.close()


# ---- batching ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65])
def test_view_counts_and_batch_sizes(tx, V):
    v, f, _ = VR.soup(60, 7)
    base = [R.pixel_camera(24, 20, cx=3.0, cy=-2.0), R.pixel_camera(24, 20, f=200.0)] + VR.mixed_views()[1:5]
    cams = [base[k % len(base)] for k in range(V)]
    img = VR.images_for(cams, V)
    want = TR.run(v, f, cams, img, 0.5, 0.5)
    assert 0 < want["faces_textured"] < len(f)
    for batch in (1, 2, 64, 0):
        _case(tx, v, f, cams, img, 0.5, 0.5, f"{V} views", batch=batch, want=want)
        assert tx.last_batch() == min(V, batch if batch else 64)
    with pytest.raises(capi.SfmxError):
        tx.set_batch(65)
    with pytest.raises(capi.SfmxError):
        tx.set_batch(-1)
    tx.set_batch(0)


def test_views_of_mixed_sizes(tx):
    v, f, _ = VR.soup(150, 8)
    cams = VR.mixed_views()
    img = VR.images_for(cams, 9)
    want = None
    for batch in (0, 1, 3):
        want = _case(tx, v, f, cams, img, 0.5, 0.5, "mixed sizes", batch=batch, want=want, patch=5)
    assert (want["view_faces"] > 0).sum() >= 3


# ---- scale edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 65537])
def test_face_counts_and_row_lengths(tx, count):
    side = 16 if count < 1000 else 256
    v, f = R.tiny_faces(count, side, side)
    cams = [R.pixel_camera(side, side), R.pixel_camera(side, side, cx=0.5, cy=0.25)]
    img = VR.images_for(cams, count)
    patch = 8 if count < 1000 else 4
    F = f.astype(np.int64)
    best = TR.best_views(v, F, cams, 0.5, 0.01)
    n_tex = int((best[0] >= 0).sum())
    cells = (n_tex + 1) // 2 + int(n_tex < count)
    partial = max(2, int(np.sqrt(cells)) + 1)
    partial += int(cells % partial == 0 and cells > 2)
    for C in (1, 0, partial):
        want = TR.run(v, f, cams, img, 0.5, 0.01, patch=patch, cells_per_row=C, fill=5, best=best)
        _case(tx, v, f, cams, img, 0.5, 0.01, f"{count} faces, C {C}", want=want, patch=patch, cells_per_row=C, fill=5)
        assert want["cells"] == cells and want["cells_per_row"] == (C if C else want["cells_per_row"])
    assert n_tex > 0 and (count < 255 or n_tex < count)


def test_many_faces_on_one_pixel(tx):
    v, f = R.hot_pixel(65536)
    f = np.ascontiguousarray(f[:, ::-1])  # as built they all face away
    cams, img = [R.pixel_camera(8, 8)], [_ramp(8, 8, 4)]
    want = _case(tx, v, f, cams, img, 0.5, 0.5, "65 536 faces on one pixel", patch=3)
    assert 1000 < want["faces_textured"] < 65536


def test_random_soup(tx):
    v, f, _ = VR.soup(2000, 11, 64, 48)
    cams = [R.pixel_camera(64, 48), R.pixel_camera(64, 48, f=200.0, cx=10.0, cy=8.0), R.pixel_camera(40, 40, f=300.0, cx=-20.0, cy=-10.0)]
    img = VR.images_for(cams, 12)
    want = _case(tx, v, f, cams, img, 0.5, 0.5, "soup")
    assert want["faces_textured"] > 300 and want["faces_untextured"] > 300 and (want["view_faces"] > 50).all()
    _case(tx, v, f, cams, img, 0.5, 0.5, "soup", patch=5, cells_per_row=7, fill=255)


# ---- invalid inputs ------------------------------------------------------------------------------------------------------------
def test_invalid_inputs_each_followed_by_a_good_call(ctx, tx):
    import torch
    gv, gf = _hand(3, True)
    cams, img = [R.pixel_camera(12, 10), R.pixel_camera(12, 10, cx=1.0)], [_ramp(12, 10, 1), _ramp(12, 10, 2)]
    z, tol = 0.5, HAND_TOL
    gref = TR.run(gv, gf, cams, img, z, tol)

    def good_call(what):
        _load(tx, cams, img)
        TR.same(tx.run(gv, gf, z, tol), gref, "after " + what)

    def refused(fn, what):
        _invalid(fn)
        _invalid(tx.read)  # the failed run left no result
        for getter in (tx.counts, tx.sizes):
            with pytest.raises(capi.SfmxError):
                getter()
        assert tx.device_atlas()[0] == -1
        good_call(what)

    good_call("nothing")
    for bad in (-1, len(gv), 2 ** 31 - 1, -2 ** 31):
        for corner in range(3):
            f = gf.copy()
            f[1, corner] = bad
            refused(lambda: tx.run(gv, f, z, tol), f"index {bad}")
    _load(tx, [], [])
    refused(lambda: tx.run(gv, gf, z, tol), "no views")
    _load(tx, cams, [img[0], None])
    refused(lambda: tx.run(gv, gf, z, tol), "a view without an image")
    for p in TR.BAD_PARAMS:
        assert not capi.texture_check_params(**p) and not TR.check_params(**p)
        refused(lambda: tx.run(gv, gf, **p), str(p))
    refused(lambda: tx.run(gv, gf, z, tol, patch=8, cells_per_row=1821), "W = 16 389")
    with pytest.raises(ValueError):
        TR.run(gv, gf, cams, img, z, tol, patch=8, cells_per_row=1821)
    # 2^28 texels: patch 64 and one cell per row give 65 x 64 texels per cell, so 64 528 cells are too many.  130 000 disjoint
    # front-facing faces, one per pixel of a 500 x 260 grid, all seen: 65 000 cells
    count = 130000
    cell = np.arange(count)
    o = np.stack([cell % 500, cell // 500], 1).astype(np.float64)
    bv = R.at_pixels((o[:, None, :] + np.array([(0.1, 0.1), (0.2, 0.8), (0.8, 0.2)])[None]).reshape(-1, 2), 1.0)
    bf = np.arange(3 * count, dtype=np.int32).reshape(count, 3)
    big_cam, big_img = [R.pixel_camera(512, 512)], [_ramp(512, 512)]
    best = TR.best_views(bv, bf.astype(np.int64), big_cam, 0.5, 0.01)
    n_tex = int((best[0] >= 0).sum())
    assert n_tex == count
    with pytest.raises(ValueError):
        TR.layout(n_tex, count - n_tex, 64, 1)
    _load(tx, big_cam, big_img)
    free0 = torch.cuda.mem_get_info()[0]
    _invalid(lambda: tx.run(bv, bf, 0.5, 0.01, patch=64, cells_per_row=1))
    assert free0 - torch.cuda.mem_get_info()[0] < (1 << 27), "refused before the atlas is allocated"
    _invalid(tx.read)
    good_call("a layout above 2^28 texels")
    for bad_cam in ({**cams[0], "w": 4097, "h": 1}, {**cams[0], "w": 0}, {**cams[0], "f": 0.0}, {**cams[0], "cx": float("nan")}):
        n0 = tx.view_count()
        _invalid(lambda: tx.add_view(bad_cam))
        assert tx.view_count() == n0
    with pytest.raises(TypeError):
        tx.run(gv, gf, z, tol, background=1)
    assert tx.read()["faces_textured"] == 3, "refused in Python, before the library: the result stays"
    for p in TR.GOOD_PARAMS[:3]:
        assert capi.texture_check_params(**p)
        _case(tx, gv, gf, cams, img, p["z_min"], p["depth_tol"], str(p), **{k: p[k] for k in p if k not in ("z_min", "depth_tol")})
    assert capi.texture_default_params() == dict(z_min=0.0, depth_tol=0.0, **capi.TEXTURE_DEFAULTS)


def test_view_set_refusals_agree(ctx):
    """The visibility and the texture object keep the same kind of view list: the same sequence of bad views, bad batch sizes, a
    reset and one good view gives the same status and the same view_count() on both at every step, and both then run."""
    good, img = R.pixel_camera(12, 10), _ramp(12, 10)
    bad_R = np.array(good["R_rw"], np.float64).copy()
    bad_R.flat[4] = np.nan
    steps = [("w = 0", lambda o: o.add_view({**good, "w": 0})), ("w = 4097", lambda o: o.add_view({**good, "w": 4097})),
             ("f = 0", lambda o: o.add_view({**good, "f": 0.0})), ("f = NaN", lambda o: o.add_view({**good, "f": float("nan")})),
             ("a NaN in R_rw", lambda o: o.add_view({**good, "R_rw": bad_R})), ("set_batch(-1)", lambda o: o.set_batch(-1)),
             ("set_batch(65)", lambda o: o.set_batch(65)), ("a good view", lambda o: o.add_view(good, img)), ("reset", lambda o: o.reset()),
             ("a good view after the reset", lambda o: o.add_view(good, img))]

    def status(fn, o):
        try:
            fn(o)
        except capi.SfmxError as e:
            return e.status
        return capi.SFMX_OK

    vb, tx = ctx.visib(), ctx.texture()
    try:
        seen = []
        for what, fn in steps:
            sv, st = status(fn, vb), status(fn, tx)
            assert sv == st, f"{what}: visibility says {sv}, texture {st}"
            assert vb.view_count() == tx.view_count(), what
            seen.append((sv, vb.view_count()))
        I, OK = capi.SFMX_ERR_INVALID, capi.SFMX_OK
        assert seen == [(I, 0)] * 7 + [(OK, 1), (OK, 0), (OK, 1)]
        v, f = _hand(3)
        a = vb.run(v, f, 0.5, HAND_TOL, cull=0)
        b = tx.run(v, f, 0.5, HAND_TOL)
        assert a["faces_seen"] == b["faces_textured"] == 3
    finally:
        vb.close()
        tx.close()


def test_a_non_finite_vertex_is_no_error(tx):
    v, f = _hand(3)
    v = v.copy()
    v[0, 0], v[4, 2] = np.nan, np.inf
    want = _case(tx, v, f, [R.pixel_camera(12, 10)], [_ramp(12, 10)], 0.5, HAND_TOL, "non-finite")
    assert want["face_view"].tolist() == [-1, -1, 0] and want["cells"] == 2


def test_empty_meshes_and_state_rules(ctx):
    s = ctx.texture()
    _invalid(s.read)
    with pytest.raises(capi.SfmxError):
        s.counts()
    assert s.device_atlas() == (-1, None, 0, 0) and s.last_us() == 0.0 and s.last_batch() == 0 and s.view_count() == 0
    cams, img = [R.pixel_camera(12, 10)], [_ramp(12, 10)]
    v, f = _hand(2)
    want = _case(s, v, np.zeros((0, 3), np.int32), cams, img, 0.5, 0.25, "no faces")
    assert (want["W"], want["H"], want["cells"]) == (0, 0, 0) and want["atlas"].shape == (0, 0)
    _case(s, np.zeros((0, 3)), np.zeros((0, 3), np.int32), cams, img, 0.5, 0.25, "nothing")
    _case(s, v, f, cams, img, 0.5, 0.25, "two faces")
    lib, P = ctx.lib, ctypes.c_void_p
    assert lib.sfmx_texture_read(ctx.h_, s.h_, None, None, None, None, None) == capi.SFMX_OK, "every pointer may be NULL"
    s.reset()
    assert s.view_count() == 0 and s.read()["faces_textured"] == 2, "reset drops the views and keeps the result"
    p = capi.texture_params(0.5, 0.1)
    args = (v.ctypes.data_as(P), ctypes.c_int(len(v)), f.ctypes.data_as(P), ctypes.c_int(len(f)), ctypes.c_int(0))
    assert lib.sfmx_texture_run(ctx.h_, s.h_, *args, None) == capi.SFMX_ERR_INVALID
    _invalid(s.read)
    assert lib.sfmx_texture_add_view(ctx.h_, s.h_, None, None, ctypes.c_int(0)) == capi.SFMX_ERR_INVALID
    ctx.set_timing(True)
    _case(s, v, f, cams, img, 0.5, 0.25, "timed")
    assert s.last_us() > 0.0 and 0.0 < s.last_bake_us() <= s.last_us()
    ctx.set_timing(False)
    s.close()


# ---- feeds -------------------------------------------------------------------------------------------------------------------
def test_feeding_paths_and_sizes_large_small_large(ctx):
    """host pointers, device pointers and images, the simplify object's device mesh; one object used large, small, large"""
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
    s = ctx.texture()
    ref = _case(s, v, f, cams, img, 0.05, tol, "host pointers", patch=4)
    assert 1000 < ref["faces_textured"] < len(f)
    sv, sf = _hand(3, True)
    _case(s, sv, sf, [R.pixel_camera(12, 10)], [_ramp(12, 10)], 0.5, HAND_TOL, "small after large")
    tv, tf = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, f))
    timg = [torch.from_numpy(i).to("cuda:0") for i in img]
    torch.cuda.synchronize()
    s.reset()
    for cam, ti in zip(cams, timg):
        s.add_view(cam, ti.data_ptr())
    TR.same(s.run(tv.data_ptr(), tf.data_ptr(), 0.05, tol, n=len(v), m=len(f), patch=4), ref, "device pointers and images, large again")
    k, pa, W, H = s.device_atlas()
    assert (k, W, H) == (ref["W"] * ref["H"], ref["W"], ref["H"])
    assert pa is not None
    sp = ctx.simplify()
    sp.run(tv.data_ptr(), tf.data_ptr(), n=len(v), m=len(f), cell=2 * vol["voxel"], origin=vol["origin"])
    pref = PR.simplify(v, f, None, cell=2 * vol["voxel"], origin=vol["origin"])
    n3, pv3, pf3, m3 = sp.device_mesh()
    want = TR.run(pref["verts"], pref["faces"], cams, img, 0.05, 2 * tol)
    TR.same(s.run(pv3, pf3, 0.05, 2 * tol, n=n3, m=m3), want, "the simplify object's device mesh")
    assert want["faces_textured"] > 500
    for o in (sp, s, fu):
        o.close()


def test_fidelity_on_the_textured_sphere_from_the_device(tx):
    """the device's atlas of the textured sphere gives the CPU suite's figures exactly (it is the same atlas)"""
    import test_texture_cpu as C
    v, f, cams, img = TR.fidelity_scene()
    kw = dict(patch=TR.FIDELITY["patch"])
    want = _case(tx, v, f, cams, img, TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"], "textured sphere", **kw)
    got = tx.read()
    mean, p99 = TR.fidelity(v, f, got, TR.FIDELITY["patch"])
    assert (mean, p99) == TR.fidelity(v, f, want, TR.FIDELITY["patch"]) and got["faces_untextured"] == 0
    assert mean <= C.BOUND_MEAN and p99 <= C.BOUND_P99 and abs(mean - C.MEASURED["mean"]) < 5e-5 and abs(p99 - C.MEASURED["p99"]) < 5e-5


# ---- pipeline ----------------------------------------------------------------------------------------------------------------
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
TEX_KEYS = ("atlas", "uv", "uv_half", "face_view", "face_area", "view_faces")


@pytest.fixture(scope="module")
def ring2(ctx):
    """two pairs of the ring-6 fixture with their left rectified cameras and images"""
    import consist_ref as CR
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    pairs = pairs[:2]
    st = ctx.stereo(320, 240, num_disparities=64)
    views, rects = [], []
    s = ctx.texture()
    for a, b in pairs:
        r = pipe.stereo_rectify(K, poses[a], poses[b], 320, 240)
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        rects.append(st.disparity(il, ir, r["H_l"], r["H_r"], want_rect=True)["rect"][0].copy())
        views.append(dict(R_rw=r["R_rw"], c_left=r["c_left"], f=r["f"], cx=r["cx"], cy=r["cy"], B=r["B"], w=320, h=240))
        s.add_stereo_view(views[-1], st)  # the image from where the stereo stage left it
    st.close()
    return dict(images=images, K=K, poses=poses, pairs=pairs, vol=CR.RING6_VOL, views=views, rects=rects, stereo_fed=s)


def _fuse_args(ctx, r):
    vol = r["vol"]
    return (ctx, r["images"], r["K"], r["poses"], r["pairs"], vol["origin"], vol["voxel"], vol["dims"])


def _check_texture(m, want, what):
    t = m["texture"]
    TR.same(t, want, what)
    assert t["uv"].tobytes() == TR.uv(want["uv_half"], want["W"], want["H"]).tobytes(), what
    assert set(t) == set(TEX_KEYS) | set(TR.COUNTS), what


def _same_files(tmp_path, stem, m, want):
    ref = tmp_path / "ref"
    ref.mkdir(exist_ok=True)
    pipe.write_textured_obj(str(ref / (stem + ".obj")), m["verts"], m["faces"], TR.uv(want["uv_half"], want["W"], want["H"]), want["atlas"])
    for ext in (".obj", ".mtl", "_atlas.pgm", "_atlas.bmp"):
        assert open(tmp_path / (stem + ext), "rb").read() == open(ref / (stem + ext), "rb").read(), ext


def test_host_fuse_texture(ctx, ring2, tmp_path):
    args = _fuse_args(ctx, ring2)
    voxel = ring2["vol"]["voxel"]
    p0, p1 = str(tmp_path / "plain.ply"), str(tmp_path / "tex.ply")
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    again = pipe.fuse(*args, num_disparities=64, ply_path=p1, texture=False)
    assert set(again) == set(m0) and all(again[k].tobytes() == m0[k].tobytes() for k in ("verts", "faces")) and again["warn"] == m0["warn"]
    assert open(p0, "rb").read() == open(p1, "rb").read(), "without texture the file is what it was"
    m = pipe.fuse(*args, num_disparities=64, ply_path=p1, texture=dict(z_min=0.05, obj_path=str(tmp_path / "mesh.obj")))
    assert set(m) == set(m0) | {"texture"} and m["views"] == m0["views"] == 2 and m["warn"] == m0["warn"]
    assert m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read(), "the PLY is what it is without texture"
    want = TR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], 0.05, voxel)
    print("fuse: %d v / %d f -> %s, view_faces %s" % (len(m0["verts"]), len(m0["faces"]), TR.counts(want), want["view_faces"].tolist()))
    assert want["faces_textured"] > 1000 and want["faces_untextured"] > 0 and (want["view_faces"] > 100).all()
    _check_texture(m, want, "fuse")
    _same_files(tmp_path, "mesh", m, want)
    s = ring2["stereo_fed"]
    TR.same(s.run(m0["verts"], m0["faces"], 0.05, voxel), want, "add_stereo_view")
    # parameters of its own; after the visibility culling nothing is untextured; no pairs; refused parameters
    m2 = pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05, depth_tol=2.5 * voxel, patch=5, cells_per_row=40, fill=99))
    _check_texture(m2, TR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], 0.05, 2.5 * voxel, patch=5, cells_per_row=40, fill=99), "own")
    mv = pipe.fuse(*args, num_disparities=64, visibility=dict(z_min=0.05))
    m3 = pipe.fuse(*args, num_disparities=64, visibility=dict(z_min=0.05), texture=dict(z_min=0.05))
    assert m3["verts"].tobytes() == mv["verts"].tobytes() and m3["faces"].tobytes() == mv["faces"].tobytes()
    assert {k: m3["visibility"][k] for k in VR.COUNTS} == {k: mv["visibility"][k] for k in VR.COUNTS}
    want3 = TR.run(mv["verts"], mv["faces"], ring2["views"], ring2["rects"], 0.05, voxel)
    _check_texture(m3, want3, "after visibility")
    assert want3["faces_untextured"] == 0 and want3["faces_textured"] == len(mv["faces"]) == want["faces_textured"]
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, texture=dict(z_min=0.05))
    assert empty["verts"].shape == (0, 3) and empty["texture"]["atlas"].shape == (0, 0) and len(empty["texture"]["face_view"]) == 0
    assert {k: empty["texture"][k] for k in TR.COUNTS} == dict.fromkeys(TR.COUNTS, 0)
    for bad in (dict(z_min=0.0), dict(z_min=0.05, depth_tol=-1.0), dict(z_min=0.05, patch=2), dict(z_min=0.05, patch=65), dict(z_min=0.05, fill=256),
                dict(z_min=0.05, cells_per_row=2000)):
        with pytest.raises(capi.SfmxError):
            pipe.fuse(*args, num_disparities=64, texture=bad)
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05, colour=True))


def test_host_fuse_texture_with_every_other_stage(ctx, ring2, tmp_path):
    """clean, fill, smooth, simplify, appearance and visibility: the atlas is baked for the final mesh, and everything else is what
    it is without texture"""
    args = _fuse_args(ctx, ring2)
    voxel = ring2["vol"]["voxel"]
    stages = dict(appearance=True, clean=True, fill=True, smooth=dict(iters=3), simplify=True)
    for vis in (False, dict(z_min=0.05, depth_tol=2 * voxel)):
        p0, p1 = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
        m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0, visibility=vis, **stages)
        m = pipe.fuse(*args, num_disparities=64, ply_path=p1, visibility=vis, texture=dict(z_min=0.05, depth_tol=2 * voxel, obj_path=str(tmp_path / "s")),
                      **stages)
        assert set(m) == set(m0) | {"texture"} and open(p0, "rb").read() == open(p1, "rb").read()
        for k in ("verts", "faces", "normals", "grey", "vertex_views"):
            assert m[k].tobytes() == m0[k].tobytes(), k
        for k in ("clean", "fill", "smooth", "simplify"):
            assert m[k] == m0[k], k
        want = TR.run(m0["verts"], m0["faces"], ring2["views"], ring2["rects"], 0.05, 2 * voxel)
        _check_texture(m, want, f"every stage, visibility {bool(vis)}")
        _same_files(tmp_path, "s", m, want)
        assert want["faces_textured"] > 500 and (want["faces_untextured"] == 0) == bool(vis)


def test_pipeline_run_texture(ctx, tmp_path):
    import json
    import os
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    pair, small = (2, 3), dict(num_disparities=32, census=5)
    plain, with_t = str(tmp_path / "plain"), str(tmp_path / "tex")
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
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, with_t, fusion=dict(fz, texture=dict(z_min=1e-3)))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(with_t, "X") and sorted(os.listdir(with_t)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m) == set(m1) | {"texture"} and len(m1["faces"]) > 0 and m["verts"].tobytes() == m1["verts"].tobytes()
    rect = pipe.stereo_rectify(g["K"], r0["kf_poses"][pair[0]], r0["kf_poses"][pair[1]], w, h)
    view = dict(R_rw=rect["R_rw"], c_left=rect["c_left"], f=rect["f"], cx=rect["cx"], cy=rect["cy"], B=rect["B"], w=w, h=h)
    il, ir = (g["images"][fb], g["images"][fa]) if rect["swapped"] else (g["images"][fa], g["images"][fb])
    st = ctx.stereo(w, h, **small)
    left = st.disparity(il, ir, rect["H_l"], rect["H_r"], want_rect=True)["rect"][0].copy()
    st.close()
    want = TR.run(m1["verts"], m1["faces"], [view], [left], 1e-3, voxel)
    print("run: %d f -> %s" % (len(m1["faces"]), TR.counts(want)))
    _check_texture(m, want, "pipeline.run")
