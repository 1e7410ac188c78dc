"""GPU suite for the photometric registration of a camera to the textured mesh: the 28 sums, n, the per-sample
state and r, and every iterate of the loop are compared byte for byte with the NumPy restatement (tests/palign_ref.py) -- hand
meshes at two patch sizes, picture sizes around the tiles and the tree's levels, strides, every way a sample is not a candidate,
the trimming threshold, both atlases, the feeds, one object across sizes, every refusal, and the calibrated loops."""
import importlib

import numpy as np
import pytest

import align_ref as AL
import helpers as H
import level_ref as LR
import palign_ref as PA
import photo_ref as P
import raster_ref as R
import texture_ref as TR
import visib_ref as VR

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")


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
def pa(ctx):
    """one object for the whole module: its buffers grow and shrink with the cases"""
    o = ctx.palign()
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


def _bits(x):
    return np.ascontiguousarray(x, np.float64).tobytes()


def _system(pa, M, cam, img, z, pivot, what, **kw):
    """one evaluation on the device against the restatement: sums, n, state and r; returns the reference's (sums, n, state, r)"""
    ref = {k: kw[k] for k in ("stride", "margin", "r_max") if k in kw}
    want = PA.system(M, cam, img, z, pivot, want_rows=True, **ref)
    sums, n = pa.system(cam, z, pivot, **kw)
    assert n == want[1], (what, n, want[1])
    assert _bits(sums) == _bits(want[0]), (what, sums, want[0])
    state, r = pa.read()
    assert state.shape == want[2].shape and state.tobytes() == want[2].tobytes(), what
    assert _bits(r) == _bits(want[3]), what
    return want


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


def _quilt_scene(tx, nx, ny, patch):
    """a quilt of nx x ny quads textured from two cameras over it, on the device and by the restatement"""
    v, f = P.quilt(nx, ny, 6.0, seed=patch)
    w, h = 6 * nx, 6 * ny
    cams = [R.pixel_camera(w, h), R.pixel_camera(w, h, cx=0.375, cy=-0.25)]
    imgs = VR.images_for(cams, patch)
    tex = _texture(tx, v, f, cams, imgs, 0.5, 0.25, "quilt", patch=patch)
    return v, f, tex, PA.model(v, f, tex)


# ---- one evaluation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", [8, 16])
def test_aligned_face_and_the_trimming_threshold(tx, pa, patch):
    v, f, cam, img = P.aligned_face(patch)
    tex = _texture(tx, v, f, [cam], [img], 0.5, 0.0, "aligned", patch=patch)
    M = PA.model(v, f, tex)
    pa.set_model(tx, v, f)
    pa.set_image(img)
    piv = [0.0, 0.0, 1.0]
    want = _system(pa, M, cam, img, 0.5, piv, "aligned", margin=1)
    assert want[1] > 0 and not want[3].any() and want[0][27] == 0.0, "texel centres: the picture comes back, r = 0 exactly"
    # g is an integer here, so |r| = 7 exactly at every candidate: r_max = 7 uses them all, r_max = 6 trims them all
    off = np.where(img >= 128, img.astype(np.int64) - 7, img.astype(np.int64) + 7).astype(np.uint8)
    pa.set_image(off)
    w7 = _system(pa, M, cam, off, 0.5, piv, "r_max = |r|", margin=1, r_max=7.0)
    assert w7[1] == want[1] and (np.abs(w7[3][w7[2] > 0]) == 7.0).all() and (w7[2][w7[2] > 0] == 2).all()
    w6 = _system(pa, M, cam, off, 0.5, piv, "r_max below |r|", margin=1, r_max=6.0)
    assert w6[1] == 0 and (w6[2] == 1).sum() == want[1] and not w6[0].any()
    # all trimmed: TOO_FEW after one evaluation, the view comes back; min_pixels one above n likewise
    for kw in (dict(r_max=6.0, min_pixels=1), dict(r_max=7.0, min_pixels=want[1] + 1)):
        got = pa.view(cam, 0.5, piv, margin=1, **kw)
        ref = PA.align(M, cam, off, 0.5, piv, margin=1, **kw)
        assert got["status"] == PA.TOO_FEW and got["iterations"] == 1 and PA.same_result(got, ref)
        assert _bits(got["view"]["R_rw"]) == _bits(cam["R_rw"])
    assert pa.view(cam, 0.5, piv, margin=1, r_max=7.0, min_pixels=want[1], max_iters=1)["status"] != PA.TOO_FEW


@pytest.mark.parametrize("patch", [3, 8])
def test_quilts_picture_sizes_and_strides(tx, pa, patch):
    for nx, ny in ((1, 1), (5, 5)):
        v, f, tex, M = _quilt_scene(tx, nx, ny, patch)
        assert len(f) == 2 * nx * ny
        pa.set_model(tx, v, f)
        total = 0
        for s in (7, 8, 9, 15, 16, 17, 33):
            cam = R.pixel_camera(s, s, cx=0.25)
            img = VR.images_for([cam], s)[0]
            pa.set_image(img)
            for stride in (1, 2, 3, s + 1):
                total += _system(pa, M, cam, img, 0.5, [0.05, 0.05, 1.5], f"quilt {nx} x {ny}, {s} px, stride {stride}", margin=1, stride=stride)[1]
        assert total > 0


def test_tree_levels_a_wide_picture_and_one_object_across_sizes(tx, pa):
    v, f, tex, M = _quilt_scene(tx, 46, 46, 8)
    pa.set_model(tx, v, f)
    cam = R.pixel_camera(272, 272)
    img = VR.images_for([cam], 5)[0]
    pa.set_image(img)  # large
    big = _system(pa, M, cam, img, 0.5, [0.5, 0.5, 1.5], "272 x 272: 289 blocks, the tree recurses", margin=1)
    assert big[1] > 256 and big[2].shape == (272, 272)
    small_cam = R.pixel_camera(9, 9)
    small = VR.images_for([small_cam], 2)[0]
    pa.set_image(small)  # small
    _system(pa, M, small_cam, small, 0.5, [0.5, 0.5, 1.5], "small after large", margin=1)
    pa.set_image(img)  # large again: set_image twice on one model
    again = pa.system(cam, 0.5, [0.5, 0.5, 1.5], margin=1)
    assert _bits(again[0]) == _bits(big[0]) and again[1] == big[1]
    _system(pa, M, cam, img, 0.5, [0.5, 0.5, 1.5], "margin 2 and stride 3", margin=2, stride=3)
    # 4 096 x 3: the widest picture; only the middle row can hold candidates
    v, f = P.quilt(682, 1, 6.0, seed=2)
    tcam = R.pixel_camera(4096, 6)
    timg = VR.images_for([tcam], 6)
    tex = _texture(tx, v, f, [tcam], timg, 0.5, 0.25, "wide")
    M = PA.model(v, f, tex)
    pa.set_model(tx, v, f)  # set_model on the picture set before ...
    _invalid(lambda: pa.system(R.pixel_camera(4096, 3, cy=-1.0), 0.5, [0.0, 0.0, 1.0]))  # ... whose size is another
    cam = R.pixel_camera(4096, 3, cy=-1.0)
    img = VR.images_for([cam], 7)[0]
    pa.set_image(img)
    wide = _system(pa, M, cam, img, 0.5, [8.0, 0.0, 1.5], "4096 x 3", margin=1)
    assert wide[1] > 500 and not wide[2][0].any() and not wide[2][2].any()


def test_every_way_a_sample_is_not_a_candidate(tx, pa):
    # face 0 textured; face 1 front-facing with a corner outside the texture camera's image: untextured; face 2 back-facing
    v = R.at_pixels([(1, 1), (1, 7), (7, 1), (13, 7), (7, -5), (1, 1)])
    f = np.array([[0, 1, 2], [2, 1, 3], [0, 4, 2]], np.int32)
    tcam, cam = R.pixel_camera(8, 8), R.pixel_camera(16, 9)
    timg = VR.images_for([tcam], 4)
    tex = _texture(tx, v, f, [tcam], timg, 0.5, 0.0, "neighbours", patch=4)
    assert tex["face_view"].tolist() == [0, -1, -1]
    M = PA.model(v, f, tex)
    ok, (px, fw, back, _, _), _ = PA.ok_mask(M, cam, 0.5)
    cls = np.zeros(16 * 9, int)
    cls[px] = np.where(back, 1, np.where(tex["face_view"][fw] < 0, 2, 3))
    cls = cls.reshape(9, 16)
    # ok pixels with an empty, a back-facing and an untextured neighbour exist
    assert cls[1, 1] == 3 and cls[0, 0] == 0 and cls[1, 2] == 3 and cls[0, 2] == 1 and cls[2, 5] == 3 and cls[2, 6] == 2
    img = VR.images_for([cam], 9)[0]
    pa.set_model(tx, v, f)
    pa.set_image(img)
    want = _system(pa, M, cam, img, 0.5, [0.0, 0.0, 1.0], "neighbours", margin=1)
    assert (want[2] > 0).sum() == 3
    # outside the image: a picture that cuts the face at its border
    cut = R.pixel_camera(5, 5, cx=-1.0, cy=-1.0)
    cimg = VR.images_for([cut], 3)[0]
    pa.set_image(cimg)
    w1 = _system(pa, M, cut, cimg, 0.5, [0.0, 0.0, 1.0], "border", margin=1)
    assert PA.ok_mask(M, cut, 0.5)[0][0, 0] and w1[2][0, 0] == 0 and w1[2][1, 1] > 0
    # the largest margin that leaves exactly one candidate, and one more that leaves none
    v2, f2, cam2, img2 = P.aligned_face(64, x0=3, y0=3, w=70, h=70)
    tex2 = _texture(tx, v2, f2, [cam2], [img2], 0.5, 0.0, "aligned 64", patch=64)
    M2 = PA.model(v2, f2, tex2)
    pa.set_model(tx, v2, f2)
    pa.set_image(img2)
    counts = [int(PA.candidates(PA.ok_mask(M2, cam2, 0.5)[0], m).sum()) for m in range(1, 40)]
    m1 = 1 + max(i for i, c in enumerate(counts) if c >= 1)
    assert counts[m1 - 1] >= 1 and counts[m1] == 0
    for m in (m1, m1 + 1):
        wm = _system(pa, M2, cam2, img2, 0.5, [0.1, 0.1, 1.0], f"margin {m}", margin=m)
        assert (wm[2] > 0).sum() == counts[m - 1]


def test_constant_picture_damping_and_negative_zero_blocks(tx, pa):
    v, f, cam, img = P.aligned_face(64, x0=15, y0=15, w=96, h=96)
    img = np.minimum(img, 254)
    tex = _texture(tx, v, f, [cam], [img], 0.5, 0.0, "aligned 64", patch=64)
    M = PA.model(v, f, tex)
    flat = np.full_like(img, 255)
    pa.set_model(tx, v, f)
    pa.set_image(flat)
    piv = [0.1, 0.1, 1.0]
    want = _system(pa, M, cam, flat, 0.5, piv, "constant picture", margin=1)
    assert (want[2][16:32, 16:32] == 2).all(), "block (1, 1) is all used: its b sums are -0.0 or +0.0 by sign alone"
    assert not want[0][:27].any() and want[0][27] > 0.0, "A = 0 and b = 0, e > 0"
    for kw, status in ((dict(), PA.DEGENERATE), (dict(damping=1.0), PA.CONVERGED)):
        got = pa.view(cam, 0.5, piv, margin=1, **kw)
        ref = PA.align(M, cam, flat, 0.5, piv, margin=1, **kw)
        assert got["status"] == status == ref["status"] and got["iterations"] == 1 and PA.same_result(got, ref)
        assert _bits(got["view"]["R_rw"]) == _bits(cam["R_rw"]) and _bits(got["view"]["c_left"]) == _bits(cam["c_left"])


# ---- feeds, atlases, refusals ------------------------------------------------------------------------------------------------------
def test_feeds_both_atlases_and_every_refusal(ctx, tx, pa):
    import torch
    v, f, tex, M = _quilt_scene(tx, 5, 5, 8)
    cam = R.pixel_camera(30, 30, cx=0.25)
    img = VR.images_for([cam], 11)[0]
    piv = [0.05, 0.05, 1.5]
    fresh = ctx.palign()
    try:
        _invalid(lambda: fresh.system(cam, 0.5, piv))  # nothing set
        fresh.set_image(img)
        _invalid(lambda: fresh.system(cam, 0.5, piv))  # no model
        _invalid(fresh.read)
        fresh.set_model(tx, v, f)
        _invalid(fresh.read)  # no evaluation yet
        host = _system(fresh, M, cam, img, 0.5, piv, "host feeds", margin=1)
    finally:
        fresh.close()
    # device feeds for mesh and picture
    dv, df = torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda()
    di = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    torch.cuda.synchronize()
    pa.set_model(tx, dv.data_ptr(), df.data_ptr(), n=len(v), m=len(f))
    pa.set_image(di.data_ptr(), shape=img.shape)
    dev = pa.system(cam, 0.5, piv, margin=1)
    assert _bits(dev[0]) == _bits(host[0]) and dev[1] == host[1]
    # the levelled atlas, on a roof whose two faces share an edge (the quilt's quads share nothing, so levelling moves nothing)
    sv, sf, scams, simg = LR.roof()
    rtx, lv = ctx.texture(), ctx.level()
    try:
        rtex = _texture(rtx, sv, sf, scams, simg, 0.5, 0.25, "roof")
        lev = LR.run(sv, sf, scams, simg, rtex)
        LR.same(lv.run(rtx, sv, sf), lev, "roof: the level run")
        pa.set_model(rtx, sv, sf)
        pa.set_image(simg[0])
        plain = _system(pa, PA.model(sv, sf, rtex), scams[0], simg[0], 0.5, [0.0, 0.0, 1.0], "the texture's atlas", margin=1)
        Ml = PA.model(sv, sf, rtex, atlas=lev["atlas"])
        pa.set_model(rtx, sv, sf, lv=lv)  # set_model twice on one picture
        got = _system(pa, Ml, scams[0], simg[0], 0.5, [0.0, 0.0, 1.0], "the levelled atlas", margin=1)
        assert got[1] > 0 and _bits(got[0]) != _bits(plain[0]), "the two atlases differ on this scene"
        other = ctx.level()
        try:
            _invalid(lambda: pa.set_model(rtx, sv, sf, lv=other))  # a level object without a run
            _invalid(lambda: pa.set_model(tx, v, f, lv=lv))  # a level object with another W and H
        finally:
            other.close()
        _system(pa, Ml, scams[0], simg[0], 0.5, [0.0, 0.0, 1.0], "the model stays after a refused set_model", margin=1)
        pa.set_model(tx, v, f)
    finally:
        lv.close()
        rtx.close()
    pa.set_image(img)
    good = lambda: _system(pa, M, cam, img, 0.5, piv, "a good call after a refusal", margin=1)
    empty = ctx.texture()
    try:
        _invalid(lambda: pa.set_model(empty, v, f))  # a texture object without a run
    finally:
        empty.close()
    good()
    _invalid(lambda: pa.set_model(tx, v[:-1], f))  # n other than the run's
    _invalid(lambda: pa.set_model(tx, v, f[:-1]))  # m other than the run's
    bad = f.copy()
    bad[3, 2] = len(v)
    _invalid(lambda: pa.set_model(tx, v, bad))  # a face index outside [0, n)
    bad[3, 2] = -1
    _invalid(lambda: pa.set_model(tx, v, bad))
    good()
    _invalid(lambda: pa.system(dict(cam, w=31), 0.5, piv))  # not the picture's size
    _invalid(lambda: pa.system(dict(cam, f=0.0), 0.5, piv))  # the z-buffer refuses it
    _invalid(lambda: pa.system(dict(cam, f=float("nan")), 0.5, piv))
    nanR = np.array(cam["R_rw"], np.float64).copy()
    nanR.flat[4] = float("inf")
    _invalid(lambda: pa.view(dict(cam, R_rw=nanR), 0.5, piv))
    _invalid(lambda: pa.view(dict(cam, c_left=[0.0, float("nan"), 0.0]), 0.5, piv))
    for kw in PA.BAD_PARAMS:
        full = dict(dict(z_min=0.5, pivot=piv), **kw)
        _invalid(lambda: pa.system(cam, **full))
        _invalid(pa.read)  # a failed call leaves no result
    good()
    _invalid(lambda: pa.set_image(np.zeros((2, 4097), np.uint8)))
    good()
    # a view that sees nothing is TOO_FEW, not an error
    away = dict(cam, c_left=[0.0, 0.0, 50.0])
    got = pa.view(away, 0.5, piv)
    assert got["status"] == PA.TOO_FEW and got["trace"] == [(0, 0.0, 0.0, 0.0)]
    # the texture object run again on another mesh: the model no longer holds
    v2, f2, _, _ = P.aligned_face(8)
    _texture(tx, v2, f2, [R.pixel_camera(9, 9)], [VR.images_for([R.pixel_camera(9, 9)], 1)[0]], 0.5, 0.0, "another mesh", patch=8)
    _invalid(lambda: pa.system(cam, 0.5, piv))


def test_device_meshes_of_visib_and_simplify_as_input(ctx, tx, pa):
    v, f = P.quilt(5, 5, 6.0, seed=8)
    cams = [R.pixel_camera(30, 30), R.pixel_camera(30, 30, cx=0.375, cy=-0.25)]
    imgs = VR.images_for(cams, 8)
    cam = R.pixel_camera(30, 30, cx=0.25)
    img = VR.images_for([cam], 11)[0]
    vb = ctx.visib()
    try:
        for c in cams:
            vb.add_view(c)
        out = vb.run(v, f, 0.5, 0.25)
        nv, pv, pf, nf = vb.device_mesh()
        tex = _texture(tx, out["verts"], out["faces"], cams, imgs, 0.5, 0.25, "visib's mesh")
        M = PA.model(out["verts"], out["faces"], tex)
        pa.set_model(tx, pv, pf, n=nv, m=nf)
        pa.set_image(img)
        _system(pa, M, cam, img, 0.5, [0.05, 0.05, 1.5], "visib's device mesh", margin=1)
    finally:
        vb.close()
    import simplify_ref as SR
    sp = ctx.simplify()
    try:
        sp.run(v, f, cell=1e-3, origin=(-1.0, -1.0, 0.0))
        n3, pv3, pf3, m3 = sp.device_mesh()
        pref = SR.simplify(v, f, None, cell=1e-3, origin=(-1.0, -1.0, 0.0))
        tex = TR.run(pref["verts"], pref["faces"], cams, imgs, 0.5, 0.25)
        tx.reset()
        for c, im in zip(cams, imgs):
            tx.add_view(c, im)
        TR.same(tx.run(pv3, pf3, 0.5, 0.25, n=n3, m=m3), tex, "simplify's mesh: the texture run")
        pa.set_model(tx, pv3, pf3, n=n3, m=m3)
        want = _system(pa, PA.model(pref["verts"], pref["faces"], tex), cam, img, 0.5, [0.05, 0.05, 1.5], "simplify's device mesh", margin=1)
        assert want[1] > 50
    finally:
        sp.close()


# ---- the loop --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calib(tx):
    c = PA.calibration()
    tx.reset()
    for cam, img in zip(c["cams"], c["images"]):
        tx.add_view(cam, img)
    TR.same(tx.run(c["verts"], c["faces"], c["z_min"], c["depth_tol"], patch=c["patch"]), c["tex"], "calibration: the texture run")
    return c


def test_calibration_loops_levels_and_cut_iterates(ctx, tx, pa, calib):
    import test_palign_cpu as CPU
    c = calib
    finals = []
    for i, (deg, metres, levels) in enumerate(PA.STARTS):
        want = PA.calibration_result(i)
        got = pipe.view_register(ctx, tx, c["verts"], c["faces"], c["starts"][i], c["image"], z_min=c["z_min"], levels=levels,
                                 **PA.CALIB_PARAMS)
        assert len(got["levels"]) == levels and all(PA.same_result(a, b) for a, b in zip(got["levels"], want["levels"])), (i, got, want)
        assert (got["status"], got["iterations"], got["n"]) == (want["status"], want["iterations"], want["n"]) and got["rms"] == want["rms"]
        # the calibrated figures, from the device
        rot, centre = AL.pose_error(got["view"], c["cam"], 1.0)
        assert tuple(l["status"] for l in got["levels"]) == CPU.MEASURED["status"][i]
        assert tuple(l["iterations"] for l in got["levels"]) == CPU.MEASURED["iters"][i] and got["n"] == CPU.MEASURED["n"][i]
        assert rot <= CPU.CALIB["rot"] and centre <= CPU.CALIB["centre"] and got["rms"] <= CPU.CALIB["rms"]
        finals.append(got["view"])
    assert max(AL.pose_error(a, b, 1.0)[0] for a in finals for b in finals) <= CPU.CALIB["spread_rot"]
    assert max(AL.pose_error(a, b, 1.0)[1] for a in finals for b in finals) <= CPU.CALIB["spread_centre"]
    # levels = 2 is two manual calls, on the reduced and on the full picture
    start = c["starts"][3]
    kw = dict(PA.CALIB_PARAMS, eps_trans=1e-5 * c["diag"])
    pa.set_model(tx, c["verts"], c["faces"])
    pa.set_image(PA.reduce_image(c["image"]))
    half = pa.view(PA.reduce_cam(start), c["z_min"], c["pivot"], **kw)
    pa.set_image(c["image"])
    full = pa.view(dict(start, R_rw=half["view"]["R_rw"], c_left=half["view"]["c_left"]), c["z_min"], c["pivot"], **kw)
    want = PA.calibration_result(3)
    assert PA.same_result(half, want["levels"][0]) and PA.same_result(full, want["levels"][1])
    # every iterate: the loop cut after k evaluations, from the 2 degree start; a pivot of its own at k = 2
    for k in range(1, 7):
        piv = c["pivot"] if k != 2 else [0.01, -0.02, 0.03]
        got = pa.view(c["starts"][2], c["z_min"], piv, max_iters=k, **kw)
        ref = PA.align(c["M"], c["starts"][2], c["image"], c["z_min"], piv, max_iters=k, **kw)
        assert PA.same_result(got, ref) and got["iterations"] == k, k
        assert got["status"] == (PA.CONVERGED if k == 6 and piv is c["pivot"] else ref["status"])
    assert pa.last_us() >= 0.0 and pa.last_zbuffer_us() >= 0.0
    state, r = pa.read()
    ws = PA.system(c["M"], PA.align(c["M"], c["starts"][2], c["image"], c["z_min"], c["pivot"], max_iters=5, **kw)["view"], c["image"], c["z_min"],
                   c["pivot"], stride=2, margin=8, want_rows=True)
    assert state.tobytes() == ws[2].tobytes() and _bits(r) == _bits(ws[3]), "read gives the last evaluation of the loop"


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring2(ctx):
    """two pairs of the ring with their rectified left views and images, as the host chain textures from them"""
    import consist_ref as CR
    synth = importlib.import_module(H.PKG_NAME + ".synth")
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
    vol = CR.RING6_VOL
    return dict(args=(ctx, images, K, poses, pairs, vol["origin"], vol["voxel"], vol["dims"]), voxel=vol["voxel"], views=views, rects=rects)


def _check_palign(m, tex, atlas, cam, img, z, what, levels=1, **kw):
    """out["palign"][0] against the restatement on the mesh and texture result of the call without palign"""
    M = PA.model(m["verts"], m["faces"], tex, atlas=atlas)
    piv, diag = PA.mesh_box(m["verts"], m["faces"])
    want = PA.view_register(M, cam, img, z, piv, levels=levels, **dict(dict(eps_trans=1e-5 * diag), **kw))
    got = m["palign"]
    assert len(got) == 1 and set(got[0]) == {"view", "status", "iterations", "n", "rms", "levels"}, what
    assert all(PA.same_result(a, b) for a, b in zip(got[0]["levels"], want["levels"])) and len(got[0]["levels"]) == levels, what
    assert (got[0]["status"], got[0]["iterations"], got[0]["n"], got[0]["rms"]) == (want["status"], want["iterations"], want["n"], want["rms"]), what
    return want


def test_host_fuse_palign_alone_and_with_other_stages(ctx, ring2, tmp_path):
    args, voxel, views, rects = ring2["args"], ring2["voxel"], ring2["views"], ring2["rects"]
    p0, p1 = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    req = dict(cameras=[views[0]], images=[rects[0]], stride=2, max_iters=3)
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0, texture=dict(z_min=0.05))
    m = pipe.fuse(*args, num_disparities=64, ply_path=p1, texture=dict(z_min=0.05), palign=req)
    assert set(m) == set(m0) | {"palign"} and open(p0, "rb").read() == open(p1, "rb").read() and m["warn"] == m0["warn"]
    assert m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes()
    TR.same(m["texture"], m0["texture"], "the texture beside palign")
    want = _check_palign(m, m0["texture"], None, views[0], rects[0], 0.05, "alone", stride=2, max_iters=3)
    assert want["n"] > 1000, "the ring's own view sees the textured surface"
    stages = dict(visibility=dict(z_min=0.05, depth_tol=2 * voxel), level=dict(iterations=16), photo=True)
    xkw = dict(z_min=0.05, depth_tol=2 * voxel)
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0, texture=xkw, **stages)
    m = pipe.fuse(*args, num_disparities=64, ply_path=p1, texture=xkw, palign=dict(req, levels=2), **stages)
    assert set(m) == set(m0) | {"palign"} and open(p0, "rb").read() == open(p1, "rb").read()
    assert m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes()
    TR.same(m["texture"], m0["texture"], "the texture beside palign")
    LR.same(m["level"], m0["level"], "the level beside palign")
    P.same({k: m["photo"][k].ravel() if k in ("rendered", "cls", "face") else m["photo"][k] for k in P.ARRAYS},
           {k: m0["photo"][k].ravel() if k in ("rendered", "cls", "face") else m0["photo"][k] for k in P.ARRAYS}, "the photo beside palign")
    _check_palign(m, m0["texture"], m0["level"]["atlas"], views[0], rects[0], 0.05, "with level, visibility and photo", levels=2, stride=2,
                  max_iters=3)
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05), palign=dict(req, iterations=3))
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, palign=req)
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, texture=dict(z_min=0.05), palign=dict(cameras=[views[0]], images=[]))


def test_pipeline_run_palign(ctx, tmp_path):
    import json
    import os
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    pair, small = (2, 3), dict(num_disparities=32, census=5)
    plain, with_p = str(tmp_path / "tex"), str(tmp_path / "pal")
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
    rect = pipe.stereo_rectify(g["K"], r0["kf_poses"][pair[0]], r0["kf_poses"][pair[1]], w, h)
    view = dict(R_rw=rect["R_rw"], c_left=rect["c_left"], f=rect["f"], cx=rect["cx"], cy=rect["cy"], B=rect["B"], w=w, h=h)
    il, ir = (g["images"][fb], g["images"][fa]) if rect["swapped"] else (g["images"][fa], g["images"][fb])
    st = ctx.stereo(w, h, **small)
    left = st.disparity(il, ir, rect["H_l"], rect["H_r"], want_rect=True)["rect"][0].copy()
    st.close()
    req = dict(cameras=[view], images=[left], stride=2, max_iters=2)
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain, fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, with_p, fusion=dict(fz, palign=req))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(with_p, "X") and sorted(os.listdir(with_p)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m) == set(m1) | {"palign"} and len(m1["faces"]) > 0 and m["verts"].tobytes() == m1["verts"].tobytes()
    TR.same(m["texture"], m1["texture"], "pipeline.run: the texture beside palign")
    _check_palign(m, m1["texture"], None, view, left, 1e-3, "pipeline.run", stride=2, max_iters=2)
