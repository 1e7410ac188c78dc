"""GPU suite: shape from silhouette.  sfmx_carve_* gives the signed squared distance maps, the hull, the view
counts, the carved or overwritten fusion volume and the counters byte for byte against the NumPy restatement (tests/carve_ref.py):
pictures around the row pass's tile and the column pass's 64 x 4 tile at every cap, volumes around the hull kernel's 64 x 4 block,
cameras that take every skip branch and both clamps, every batch size, the sphere-26 calibration of DESIGN.md 30 on the device, the
stages behind a stored hull, and every refusal."""
import importlib

import numpy as np
import pytest

import carve_ref as CV
import consist_ref as CR
import fusion_ref as FR
import helpers as H
import raycast_ref as RR

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
VOL = CR.SPHERE26_VOL
T = CV.ROW_TILE


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _cam(w, h, f=100.0, pos=(0.0, 0.0, -0.5), target=(0.0, 0.0, 0.0)):
    return FR.look_at_cam(pos, target, f, w, h)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert a.tobytes() == b.tobytes(), what


# ---- distance maps ------------------------------------------------------------------------------------------------------------
def _border_mask(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0, : max(1, w // 3)] = m[h - 1, w // 2:] = m[: max(1, h // 2), 0] = m[h // 3:, w - 1] = 255
    return m


def _pictures(cap):
    """(name, u8 [h][w]) around both passes' tiles"""
    rng = np.random.default_rng(100 + cap)
    shapes = [(1, 1), (1, 300), (300, 1), (4096, 2), (63, 3), (64, 4), (65, 5), (T - 1, 5), (T, 4), (T + 1, 3), (2 * T + 1, 2)]
    shapes += [(max(1, T - cap), 6), (T + cap, 6), (max(1, T - cap - 1), 2), (T + cap + 1, 2), (7, 2 * cap + 3)]
    out = []
    for w, h in shapes:
        # blobs: a random mask at a random density, so that distances up to the cap occur
        dens = rng.random()
        out.append((f"random {w} x {h}", (rng.random((h, w)) < dens).astype(np.uint8) * 255))
    for w, h in ((T + 3, 7), (5, 5)):
        out.append((f"sparse {w} x {h}", (rng.random((h, w)) < 0.01).astype(np.uint8) * 255))
        out.append((f"all outside {w} x {h}", np.zeros((h, w), np.uint8)))
        out.append((f"all inside {w} x {h}", np.full((h, w), 200, np.uint8)))
        out.append((f"checkerboard {w} x {h}", ((np.indices((h, w)).sum(0) & 1) * 255).astype(np.uint8)))
        one = np.zeros((h, w), np.uint8)
        one[h // 2, w // 2] = 1
        out.append((f"one inside pixel {w} x {h}", one))
        out.append((f"one outside pixel {w} x {h}", np.where(one, 0, 255).astype(np.uint8)))
        out.append((f"borders {w} x {h}", _border_mask(h, w)))
    return out


@pytest.mark.parametrize("cap", [1, 16, 64])
def test_distance_maps(ctx, cap):
    cv = ctx.carve()
    pics = _pictures(cap)
    for _, img in pics:
        cv.add_view(_cam(img.shape[1], img.shape[0]), img, threshold=1, cap=cap)
    assert cv.view_count() == len(pics)
    for i, (name, img) in enumerate(pics):
        got = cv.read_view(i)
        ref = CV.sd2_map(img, 1, cap)
        assert got.dtype == np.int16 and (got != 0).all() and ((got < 0) == (img >= 1)).all(), name
        _same_bits(got, ref, f"cap {cap}: {name}")
        if img.size <= 2048:
            _same_bits(got, CV.sd2_brute(img, 1, cap), f"cap {cap}: {name} (brute force)")
        if name.startswith("checkerboard") and img.size > 1:
            assert (np.abs(got) == 1).all()
        if name.startswith("all "):
            assert (np.abs(got) == cap * cap).all()
    cv.close()


def test_a_picture_taller_than_a_grid_dimension(ctx):
    """1 x 300 000 and 3 x 270 000: more than 65 535 blocks of four rows (the column pass runs on one grid dimension)"""
    rng = np.random.default_rng(9)
    cv = ctx.carve()
    for k, (w, h) in enumerate(((1, 300000), (3, 270000))):
        img = (rng.random((h, w)) < 0.02).astype(np.uint8) * 255
        img[-5:] = 255
        cv.add_view(_cam(w, h), img, threshold=1, cap=16)
        _same_bits(cv.read_view(k), CV.sd2_map(img, 1, 16), f"{w} x {h}")
        assert cv.inside_pixels()[k] == int((img >= 1).sum())
    cv.close()


def test_thresholds_and_feeds(ctx):
    import torch
    h, w = 37, T + 9
    ramp = ((np.arange(h)[:, None] * 5 + np.arange(w)[None, :]) % 256).astype(np.uint8)
    cv = ctx.carve()
    dev = torch.from_numpy(ramp).to("cuda:0")
    torch.cuda.synchronize()
    for thr in (1, 128, 255):
        cv.add_view(_cam(w, h), ramp, threshold=thr, cap=16)
        cv.add_view(_cam(w, h), dev.data_ptr(), shape=(h, w), threshold=thr, cap=16)
    for k, thr in enumerate((1, 128, 255)):
        ref = CV.sd2_map(ramp, thr, 16)
        _same_bits(cv.read_view(2 * k), ref, f"host feed, threshold {thr}")
        _same_bits(cv.read_view(2 * k + 1), ref, f"device feed, threshold {thr}")
        assert ((ref < 0) == (ramp >= thr)).all()
    cv.close()


# ---- hull -----------------------------------------------------------------------------------------------------------------
def _small_views(cap=16):
    """eight 64 x 64 silhouettes of the sphere; a camera inside the volume, one looking away from it (every point behind), one
    looking past it (projections outside the picture); an all-inside and an all-outside picture (every projection clamps to -1 / +1);
    pictures of other sizes"""
    out = []
    for cam, d16 in CR.sphere_views(8, 64, 64, 120.0):
        out.append((cam, ((d16 != -16) * 255).astype(np.uint8)))
    rng = np.random.default_rng(5)
    out.append((_cam(48, 40, 30.0, pos=(0.01, 0.0, 0.0), target=(0.0, 0.0, 1.0)), (rng.random((40, 48)) < 0.5).astype(np.uint8)))
    out.append((_cam(32, 32, 60.0, pos=(0.0, 0.0, -0.5), target=(0.0, 0.0, -1.0)), np.full((32, 32), 255, np.uint8)))
    out.append((_cam(16, 16, 200.0, pos=(0.0, 0.0, -0.5), target=(0.5, 0.0, -0.5)), np.zeros((16, 16), np.uint8)))
    out.append((_cam(300, 7, 120.0), np.full((7, 300), 255, np.uint8)))
    out.append((_cam(9, 200, 120.0, pos=(0.0, 0.0, 0.5)), np.zeros((200, 9), np.uint8)))
    return [(cam, img, CV.sd2_map(img, 1, cap)) for cam, img in out]


@pytest.fixture(scope="module")
def small_views():
    return _small_views()


def _feed(cv, views, cap=16):
    for cam, img, _ in views:
        cv.add_view(cam, img, threshold=1, cap=cap)


def _vol(nx, ny, nz, extent=0.3):
    voxel = extent / (max(nx, ny, nz) - 1)
    return dict(origin=(-0.5 * voxel * (nx - 1), -0.5 * voxel * (ny - 1), -0.5 * voxel * (nz - 1)), voxel=voxel, dims=(nx, ny, nz))


def _check_hull(cv, vol, views, what, **params):
    ref_h, ref_n = CV.hull(vol["origin"], vol["voxel"], vol["dims"], [(c, s) for c, _, s in views],
                           **{k: v for k, v in params.items() if k in ("cap", "min_views", "trunc")})
    cv.run(vol["origin"], vol["voxel"], vol["dims"], **params)
    got_h, got_n = cv.read()
    _same_bits(got_n, ref_n, what + ": views")
    _same_bits(got_h, ref_h, what + ": hull")
    return ref_h, ref_n


@pytest.mark.parametrize("ny", [3, 4, 5])
def test_hull_around_the_block(ctx, small_views, ny):
    cv = ctx.carve()
    _feed(cv, small_views)
    for nx in (63, 64, 65):
        vol = _vol(nx, ny, 3)
        counter = {}
        CV.hull(vol["origin"], vol["voxel"], vol["dims"], [(c, s) for c, _, s in small_views], counter=counter)
        assert all(counter[k] > 0 for k in ("behind", "outside", "clamp_hi", "clamp_lo")), counter
        _check_hull(cv, vol, small_views, f"{nx} x {ny} x 3")
    _check_hull(cv, _vol(2, 2, 2), small_views, "2 x 2 x 2")
    _check_hull(cv, _vol(33, 32, 3), small_views, "a 1024-point slice boundary", trunc=0.05)
    cv.close()


def test_hull_batches_order_and_sizes(ctx, small_views):
    views65 = [small_views[i % len(small_views)] for i in range(65)]
    vol = _vol(65, 5, 4)
    cv = ctx.carve()
    for n in (1, 2, 64, 65):
        cv.reset()
        _feed(cv, views65[:n])
        seen = set()
        for batch in (1, 2, 64, 0):
            cv.set_batch(batch)
            _check_hull(cv, vol, views65[:n], f"{n} views, batch {batch}")
            h, k = cv.read()
            seen.add(h.tobytes() + k.tobytes())
        assert len(seen) == 1
    # permuted: the same bytes
    base = cv.read()
    perm = [views65[i] for i in np.random.default_rng(11).permutation(65)]
    cv.reset()
    _feed(cv, perm)
    cv.run(vol["origin"], vol["voxel"], vol["dims"])
    again = cv.read()
    _same_bits(again[0], base[0], "permuted views: hull")
    _same_bits(again[1], base[1], "permuted views: views")
    # one object, large -> small -> large
    for dims in ((70, 40, 30), (3, 2, 2), (70, 40, 30), (64, 64, 17)):
        _check_hull(cv, _vol(*dims), perm, f"volume {dims}")
    cv.close()


def test_min_views(ctx, small_views):
    vol = _vol(40, 30, 20)
    cv = ctx.carve()
    _feed(cv, small_views)
    for mv, mw in ((1, 1), (2, 1), (2, 3), (len(small_views) + 1, 1)):
        ref_h, ref_n = _check_hull(cv, vol, small_views, f"min_views {mv}", min_views=mv)
        fu = ctx.fusion(vol["origin"], vol["voxel"], vol["dims"], min_weight=mw)
        cv.store(fu)
        s, c = fu.read()
        rs, rc = CV.store(ref_h, ref_n, mv, mw)
        _same_bits(s, rs, f"min_views {mv}: stored sum")
        _same_bits(c, rc, f"min_views {mv}: stored count")
        if mv > len(small_views):
            assert not c.any() and fu.counts() == (0, 0)
        cnt = cv.apply(fu, margin=0.25, mode="clear")
        s1, c1, rcnt = CV.apply(rs, rc, ref_h, ref_n, mv, 0.25, "clear", mw)
        assert cnt == rcnt
        _same_bits(fu.read()[0], s1, "cleared sum")
        _same_bits(fu.read()[1], c1, "cleared count")
        fu.close()
    cv.close()


# ---- apply and store on the sphere-26 volumes ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_carve(ctx):
    cv = ctx.carve()
    for (cam, _), img in zip(*CV.sphere_silhouettes()[:2]):
        cv.add_view(cam, img)
    cv.run(VOL["origin"], VOL["voxel"], VOL["dims"])
    h, n = cv.read()
    rh, rn = CV.sphere_hull(26)
    _same_bits(h, rh, "sphere-26 hull")
    _same_bits(n, rn, "sphere-26 views")
    for i in (0, 13, 25):
        _same_bits(cv.read_view(i), CV.sphere_silhouettes()[0][i][1], f"sphere-26 map {i}")
    yield cv
    cv.close()


EDGE = float(np.nextafter(1.0, 0.0))


@pytest.mark.parametrize("min_weight", [1, 3])
@pytest.mark.parametrize("noisy", [False, True])
def test_apply_on_the_sphere(ctx, sphere_carve, noisy, min_weight):
    cv = sphere_carve
    views, _ = CR.sphere26(noisy)
    S, C = CV.sphere_volume(noisy)
    rh, rn = CV.sphere_hull(26)
    fu = ctx.fusion(VOL["origin"], VOL["voxel"], VOL["dims"], min_weight=min_weight)
    for mode in CV.MODES:
        for margin in (0.0, 0.5, EDGE):
            fu.reset()
            for cam, d16 in views:
                fu.add_view(cam, d16)  # left pending: apply integrates them first
            cnt = cv.apply(fu, margin=margin, mode=mode)
            s1, c1, rcnt = CV.apply(S, C, rh, rn, 1, margin, mode, min_weight)
            assert cnt == rcnt, (mode, margin)
            s, c = fu.read()
            _same_bits(c, c1, f"{mode} {margin}: count")
            _same_bits(s, s1, f"{mode} {margin}: sum")
            if margin == 0.5 and min_weight == 1:
                v, f, nrm = fu.extract_normals()
                rv, rf = FR.extract(s1, c1, VOL["origin"], VOL["voxel"], min_weight)
                _same_bits(v, rv, f"{mode}: extracted vertices")
                _same_bits(f, rf, f"{mode}: extracted faces")
                v2, f2 = fu.extract()
                assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes() and len(nrm) == len(v)
                # the calibrated figures of DESIGN.md 30, from the device
                out, ins = CV.radius_error(v)[3:]
                if noisy:
                    assert (len(v), len(f), out, ins) == (30988, 55876, 0, 8034)
                else:
                    assert (len(v), len(f), out, ins) == (22786, 45568, 0, 0) and CV.radius_error(v)[0] <= 0.14
    fu.close()


def test_store_and_the_stages_behind_it(ctx, sphere_carve):
    cv = sphere_carve
    rh, rn = CV.sphere_hull(26)
    fu = ctx.fusion(VOL["origin"], VOL["voxel"], VOL["dims"])
    views, _ = CR.sphere26(False)
    fu.add_view(*views[0])  # pending, then overwritten
    v_before, _ = fu.extract()
    cv.store(fu)
    s, c = fu.read()
    rs, rc = CV.store(rh, rn)
    _same_bits(s, rs, "stored sum")
    _same_bits(c, rc, "stored count")
    v, f, nrm = fu.extract_normals()
    rv, rf = FR.extract(rs, rc, VOL["origin"], VOL["voxel"])
    _same_bits(v, rv, "hull vertices")
    _same_bits(f, rf, "hull faces")
    closed, euler = CV.closed_euler(f, len(v))
    rms, lo, hi, out, ins = CV.radius_error(v)
    assert (len(v), len(f)) == (22538, 45072) and closed and euler == 2 and len(v_before) != len(v)
    assert rms <= 0.072 and lo >= -0.20 and hi <= 0.43 and out == 0 and ins == 0
    # ray casting the stored hull
    cam = RR.camera(RR.SPHERE_CAM["pos"], (0.0, 0.0, 0.0), 150.0, 48, 40)
    rc_ = ctx.raycast()
    got = rc_.render(fu, cam, **RR.SPHERE_MARCH)
    ref = RR.render(rs, rc, VOL["origin"], VOL["voxel"], cam, 48, 40, **RR.SPHERE_MARCH)
    assert RR.same(got, ref) and got["hits"] > 0
    rc_.close()
    # clean -> simplify run on it
    fu.extract_normals()
    cl, sp = ctx.clean(), ctx.simplify()
    r = cl.fusion(fu)
    assert r["components"] == 1 and r["n_faces"] == 45072
    k = sp.clean(cl, cell=2 * VOL["voxel"])
    assert k["clusters"] > 0
    cl.close()
    sp.close()
    fu.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_object_usable(ctx, small_views):
    vol = _vol(20, 10, 5)
    cv = ctx.carve()
    fu = ctx.fusion(vol["origin"], vol["voxel"], vol["dims"])
    other = ctx.fusion(vol["origin"], vol["voxel"], (20, 10, 6))
    shifted = ctx.fusion((0.0, 0.0, 0.0), vol["voxel"], vol["dims"])

    def refused(fn, *a, **k):
        with pytest.raises(capi.SfmxError) as e:
            fn(*a, **k)
        assert e.value.status == capi.SFMX_ERR_INVALID

    refused(cv.run, vol["origin"], vol["voxel"], vol["dims"])  # no view
    refused(cv.read)
    refused(cv.apply, fu)
    refused(cv.store, fu)
    refused(cv.read_view, 0)
    cam, img, _ = small_views[0]
    for bad in (dict(threshold=0), dict(threshold=256), dict(cap=0), dict(cap=65)):
        refused(cv.add_view, cam, img, **bad)
    refused(cv.add_view, {**cam, "f": 0.0}, img)
    refused(cv.add_view, {**cam, "f": -120.0}, img)
    refused(cv.add_view, {**cam, "cx": float("nan")}, img)
    refused(cv.add_view, cam, np.zeros((2, 4097), np.uint8))
    assert cv.view_count() == 0
    _feed(cv, small_views[:3])
    cv.add_view(cam, img, cap=5)
    refused(cv.run, vol["origin"], vol["voxel"], vol["dims"])  # a view of another cap
    refused(cv.run, vol["origin"], vol["voxel"], vol["dims"], cap=5)
    refused(cv.read)
    cv.reset()
    assert cv.view_count() == 0
    _feed(cv, small_views[:3])
    for bad in (dict(cap=0), dict(cap=65), dict(min_views=0), dict(margin=1.0), dict(margin=-0.5), dict(trunc=-1.0), dict(mode=2)):
        refused(cv.run, vol["origin"], vol["voxel"], vol["dims"], **bad)
    refused(cv.run, vol["origin"], vol["voxel"], (1, 10, 5))
    refused(cv.run, vol["origin"], vol["voxel"], (1024, 1024, 129))  # beyond 2^27 points: refused before any allocation
    refused(cv.run, vol["origin"], 0.0, vol["dims"])
    refused(cv.run, (float("inf"), 0.0, 0.0), vol["voxel"], vol["dims"])
    refused(cv.read)  # a failed run leaves no result
    ref_h, ref_n = _check_hull(cv, vol, small_views[:3], "after the refusals")
    # a refused apply / store leaves the fusion object as it was: its cached surface is still there for the stages that take it
    other.add_view(_cam(64, 64, 120.0), np.full((64, 64), 192, np.int16))  # the plane z = 0 (Z = f B / 12 = 0.5), through the slab
    v_o, f_o, _ = other.extract_normals()
    assert len(f_o) > 0
    refused(cv.apply, other)
    refused(cv.store, other)
    refused(cv.apply, shifted)
    refused(cv.apply, fu, margin=1.0)
    cl = ctx.clean()
    assert cl.fusion(other)["n_faces"] > 0  # SFMX_ERR_INVALID had the refusals dropped the surface
    cl.close()
    v_o2, f_o2 = other.extract()
    assert v_o2.tobytes() == v_o.tobytes() and f_o2.tobytes() == f_o.tobytes()
    assert not shifted.read()[1].any()
    # the counters from the hull alone are apply's first two
    for margin in (0.0, 0.5):
        want = CV.apply(*CV.store(ref_h, ref_n), ref_h, ref_n, 1, margin, "clear")[2]
        assert cv.count(margin=margin) == dict(want, changed=0)
    refused(cv.count, margin=1.0)
    cv.store(fu)  # the result is still there
    _same_bits(fu.read()[0], CV.store(ref_h, ref_n)[0], "store after the refusals")
    assert cv.apply(fu, margin=0.0, mode="clear") == CV.apply(*CV.store(ref_h, ref_n), ref_h, ref_n, 1, 0.0, "clear")[2]
    cv.add_view(cam, img)  # a new view: the result is gone
    refused(cv.read)
    refused(cv.store, fu)
    for o in (cv, fu, other, shifted):
        o.close()


# ---- pipeline.fuse / pipeline.run ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring2(ctx):
    """two pairs of the ring-6 fixture: their left rectified cameras, pictures and disparity maps from the stereo
    stage (which its own suites hold to its restatement), the volume they integrate to, and the pictures' median as threshold"""
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    pairs = pairs[:2]
    st = ctx.stereo(320, 240, num_disparities=64)
    cv = ctx.carve()
    views, rects, maps = [], [], []
    for a, b in pairs:
        r = pipe.stereo_rectify(K, poses[a], poses[b], 320, 240)
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        out = st.disparity(il, ir, r["H_l"], r["H_r"], want_rect=True)
        rects.append(out["rect"][0].copy())
        maps.append(out["disp16"].copy())
        views.append(dict(R_rw=r["R_rw"], c_left=r["c_left"], f=r["f"], cx=r["cx"], cy=r["cy"], B=r["B"]))
    thr = int(np.median(np.stack(rects)))
    assert 1 <= thr <= 255 and all(0 < int((im >= thr).sum()) < im.size for im in rects)
    # the stereo-fed view, after a disparity and after the rectification alone
    r = pipe.stereo_rectify(K, poses[pairs[1][0]], poses[pairs[1][1]], 320, 240)
    cv.add_stereo_view(views[1], st, threshold=thr)
    st.rectify(il, ir, r["H_l"], r["H_r"])
    cv.add_stereo_view(views[1], st, threshold=thr)
    want = CV.sd2_map(rects[1], thr, 16)
    _same_bits(cv.read_view(0), want, "add_stereo_view after disparity")
    _same_bits(cv.read_view(1), want, "add_stereo_view after rectify")
    assert cv.inside_pixels() == [int((rects[1] >= thr).sum())] * 2
    st.close()
    cv.close()
    vol = CR.RING6_VOL
    S, C = FR.integrate(vol["origin"], vol["voxel"], vol["dims"], list(zip(views, maps)))
    sil = [(v, CV.sd2_map(im, thr, 16)) for v, im in zip(views, rects)]
    hull = CV.hull(vol["origin"], vol["voxel"], vol["dims"], sil)
    return dict(images=images, K=K, poses=poses, pairs=pairs, vol=vol, views=views, rects=rects, thr=thr, S=S, C=C, hull=hull)


def _fuse_args(ctx, r):
    vol = r["vol"]
    return (ctx, r["images"], r["K"], r["poses"], r["pairs"], vol["origin"], vol["voxel"], vol["dims"])


@pytest.mark.parametrize("mode", CV.MODES)
def test_fuse_carve(ctx, ring2, mode, tmp_path):
    args, vol, thr = _fuse_args(ctx, ring2), ring2["vol"], ring2["thr"]
    p0, p1 = str(tmp_path / "plain.ply"), str(tmp_path / "off.ply")
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    off = pipe.fuse(*args, num_disparities=64, ply_path=p1, carve=False)
    assert set(off) == set(m0) and all(off[k].tobytes() == m0[k].tobytes() for k in ("verts", "faces")) and off["warn"] == m0["warn"]
    assert open(p0, "rb").read() == open(p1, "rb").read(), "without carve the file is what it was"
    v0, f0 = FR.extract(ring2["S"], ring2["C"], vol["origin"], vol["voxel"])
    _same_bits(m0["verts"], v0, "the restated volume is the chain's")
    m = pipe.fuse(*args, num_disparities=64, carve=dict(threshold=thr, mode=mode))
    assert set(m) == set(m0) | {"carve"} and m["views"] == 2
    s1, c1, cnt = CV.apply(ring2["S"], ring2["C"], *ring2["hull"], 1, 0.5, mode)
    v1, f1 = FR.extract(s1, c1, vol["origin"], vol["voxel"])
    print(f"{mode}: {len(v0)} / {len(f0)} -> {len(v1)} / {len(f1)}, {cnt}")
    assert m["carve"] == dict(cnt, inside_pixels=[int((im >= thr).sum()) for im in ring2["rects"]])
    assert cnt["changed"] > 0 and cnt["outside"] > 0
    _same_bits(m["verts"], v1, f"carve {mode}: vertices")
    _same_bits(m["faces"], f1, f"carve {mode}: faces")
    # parameters of its own
    m2 = pipe.fuse(*args, num_disparities=64, carve=dict(threshold=thr, mode=mode, margin=0.25, min_views=2, cap=16))
    s2, c2, cnt2 = CV.apply(ring2["S"], ring2["C"], *ring2["hull"], 2, 0.25, mode)
    v2, f2 = FR.extract(s2, c2, vol["origin"], vol["voxel"])
    assert {k: m2["carve"][k] for k in cnt2} == cnt2
    _same_bits(m2["verts"], v2, f"carve {mode}, own parameters: vertices")
    _same_bits(m2["faces"], f2, f"carve {mode}, own parameters: faces")


def test_fuse_carve_with_other_stages_and_hull_only(ctx, ring2):
    args, vol, thr = _fuse_args(ctx, ring2), ring2["vol"], ring2["thr"]
    hull_h, hull_n = ring2["hull"]
    s1, c1, _ = CV.apply(ring2["S"], ring2["C"], hull_h, hull_n, 1, 0.5, "intersect")
    v1, f1 = FR.extract(s1, c1, vol["origin"], vol["voxel"])
    stages = dict(clean=True, visibility=dict(z_min=0.05), texture=dict(z_min=0.05))
    m = pipe.fuse(*args, num_disparities=64, carve=dict(threshold=thr), **stages)
    assert {"carve", "clean", "visibility", "texture"} <= set(m) and len(m["faces"]) > 0
    # the stages saw the carved surface: the clean stage's input is the carved extraction
    only = pipe.fuse(*args, num_disparities=64, carve=dict(threshold=thr), clean=True)
    assert only["clean"] == m["clean"] and only["clean"]["verts_removed"] + len(only["verts"]) == len(v1)
    # hull_only: no view integrated by disparity, the mesh is the stored hull's
    hs, hc = CV.store(hull_h, hull_n)
    hv, hf = FR.extract(hs, hc, vol["origin"], vol["voxel"])
    mh = pipe.fuse(*args, num_disparities=64, carve=dict(threshold=thr, hull_only=True, mode="clear"))
    assert len(hf) > 0
    assert mh["views"] == 0 and m["views"] == 2  # no pair was integrated: no disparity map was made, nothing entered the volume
    _same_bits(mh["verts"], hv, "hull_only: vertices")
    _same_bits(mh["faces"], hf, "hull_only: faces")
    cnt = dict(CV.apply(hs, hc, hull_h, hull_n, 1, 0.5, "clear")[2], changed=0)  # defined and outside do not depend on the mode
    assert mh["carve"] == dict(cnt, inside_pixels=[int((im >= thr).sum()) for im in ring2["rects"]])
    mh2 = pipe.fuse(*args, num_disparities=64, carve=dict(threshold=thr, hull_only=True), **stages)
    assert len(mh2["faces"]) > 0 and {"clean", "visibility", "texture"} <= set(mh2) and mh2["views"] == 0
    # no pairs: nothing to carve with
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, carve=True)
    assert empty["verts"].shape == (0, 3) and empty["carve"] == dict(defined=0, outside=0, changed=0, inside_pixels=[])
    for bad in (dict(hull_only=True, consistency=True), dict(hull_only=True, align=True), dict(hull_only=True, appearance=True)):
        with pytest.raises(ValueError):
            pipe.fuse(*args, num_disparities=64, carve=dict(hull_only=bad.pop("hull_only")), **bad)


def test_pipeline_run_carve(ctx, tmp_path):
    import json
    import os
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    pair, small = (2, 3), dict(num_disparities=32, census=5)
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
    rect = pipe.stereo_rectify(g["K"], r0["kf_poses"][pair[0]], r0["kf_poses"][pair[1]], w, h)
    view = dict(R_rw=rect["R_rw"], c_left=rect["c_left"], f=rect["f"], cx=rect["cx"], cy=rect["cy"], B=rect["B"])
    il, ir = (g["images"][fb], g["images"][fa]) if rect["swapped"] else (g["images"][fa], g["images"][fb])
    st = ctx.stereo(w, h, **small)
    out = st.disparity(il, ir, rect["H_l"], rect["H_r"], want_rect=True)
    st.close()
    left, d16 = out["rect"][0].copy(), out["disp16"].copy()
    thr = max(1, int(np.median(left)))
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, str(tmp_path / "plain"), fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, str(tmp_path / "carved"), fusion=dict(fz, carve=dict(threshold=thr)))
    assert r1["log"].replace(str(tmp_path / "plain"), "X") == r2["log"].replace(str(tmp_path / "carved"), "X")
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m) == set(m1) | {"carve"}
    S, C = FR.integrate(tuple(lo), voxel, dims, [(view, d16)])
    hh, hn = CV.hull(tuple(lo), voxel, dims, [(view, CV.sd2_map(left, thr, 16))])
    s1, c1, cnt = CV.apply(S, C, hh, hn)
    v1, f1 = FR.extract(s1, c1, tuple(lo), voxel)
    assert m["carve"] == dict(cnt, inside_pixels=[int((left >= thr).sum())])
    _same_bits(m["verts"], v1, "pipeline.run: vertices")
    _same_bits(m["faces"], f1, "pipeline.run: faces")


def test_fuse_carve_with_a_trunc_of_the_fusions_own(ctx, ring2):
    """a trunc given to the fusion is the hull's too (sfmx_carve_run alone would take 4 x voxel)"""
    args, vol, thr = _fuse_args(ctx, ring2), ring2["vol"], ring2["thr"]
    trunc = 2.5 * vol["voxel"]
    st = ctx.stereo(320, 240, num_disparities=64)
    maps = []
    for (a, b), v in zip(ring2["pairs"], ring2["views"]):
        r = pipe.stereo_rectify(ring2["K"], ring2["poses"][a], ring2["poses"][b], 320, 240)
        il, ir = (ring2["images"][b], ring2["images"][a]) if r["swapped"] else (ring2["images"][a], ring2["images"][b])
        maps.append(st.disparity(il, ir, r["H_l"], r["H_r"]).copy())
    st.close()
    S, C = FR.integrate(vol["origin"], vol["voxel"], vol["dims"], list(zip(ring2["views"], maps)), trunc=trunc)
    sil = [(v, CV.sd2_map(im, thr, 16)) for v, im in zip(ring2["views"], ring2["rects"])]
    hh, hn = CV.hull(vol["origin"], vol["voxel"], vol["dims"], sil, trunc=trunc)
    assert hh.tobytes() != ring2["hull"][0].tobytes()
    s1, c1, cnt = CV.apply(S, C, hh, hn)
    v1, f1 = FR.extract(s1, c1, vol["origin"], vol["voxel"])
    m = pipe.fuse(*args, num_disparities=64, trunc=trunc, carve=dict(threshold=thr))
    assert {k: m["carve"][k] for k in cnt} == cnt
    _same_bits(m["verts"], v1, "fusion trunc: vertices")
    _same_bits(m["faces"], f1, "fusion trunc: faces")
    mh = pipe.fuse(*args, num_disparities=64, trunc=trunc, carve=dict(threshold=thr, hull_only=True))
    hv, hf = FR.extract(*CV.store(hh, hn), vol["origin"], vol["voxel"])
    _same_bits(mh["verts"], hv, "fusion trunc, hull_only: vertices")
    _same_bits(mh["faces"], hf, "fusion trunc, hull_only: faces")


def test_host_chain_refuses_bad_requests(ctx):
    """sfmx_host_fusion_mesh_cv called directly: a threshold outside 1 .. 255, hull_only other than 0 / 1, bad parameters and
    hull_only with a consistency, align or appearance request are SFMX_ERR_INVALID; the same call with a good request is SFMX_OK"""
    from ctypes import POINTER, byref, c_double, c_int, c_void_p, create_string_buffer
    lib = pipe.load_host_library()
    K = np.ascontiguousarray([100.0, 0, 8, 0, 100.0, 8, 0, 0, 1])
    sp, fp = capi.stereo_params(num_disparities=32), capi.fusion_params((0.0, 0.0, 0.0), 0.1, (4, 4, 4))
    warn = create_string_buffer(256)
    imgs = np.zeros((2, 48, 64), np.uint8)
    ptrs = (c_void_p * 2)(imgs[0].ctypes.data, imgs[1].ctypes.data)
    poses = np.ascontiguousarray(np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (2, 1)))
    pairs = np.zeros((1, 2), np.int32)  # m = 0: none of it is read

    def call(kq, cs=None, al=None, app=None):
        rex = pipe.FusionResultEx()
        rc = lib.sfmx_host_fusion_mesh_cv(ctx.h_, ptrs, c_int(0), c_int(2), c_int(64), c_int(48), K.ctypes.data_as(POINTER(c_double)),
                                          poses.ctypes.data_as(POINTER(c_double)), pairs.ctypes.data_as(POINTER(c_int)),
                                          c_int(0), byref(sp), byref(fp), byref(app) if app is not None else None,
                                          byref(cs) if cs is not None else None, None, None, None, None, None, None,
                                          byref(al) if al is not None else None,
                                          None, None, None, None, None, None, None, None, None, None, None,  # simplify .. photo
                                          byref(kq), byref(rex), None, warn, c_int(len(warn)))
        lib.sfmx_host_fusion_free_ex(byref(rex))
        lib.sfmx_host_carve_free(byref(kq))
        if rc != capi.SFMX_OK:
            print("rc", rc, (ctx.lib.sfmx_last_error(ctx.h_) or b"").decode())
        return rc

    def req(threshold=1, hull_only=0, **kw):
        return pipe.CarveRequest(capi.carve_params(**kw), threshold, hull_only)

    assert call(req()) == capi.SFMX_OK and call(req(hull_only=1, mode="clear")) == capi.SFMX_OK
    for bad in (req(threshold=0), req(threshold=256), req(hull_only=2), req(hull_only=-1), req(cap=0), req(cap=65), req(margin=1.0),
                req(min_views=0), req(mode=2), req(trunc=-1.0)):
        assert call(bad) == capi.SFMX_ERR_INVALID
    cs = capi.consist_params()
    app = capi.shade_params(0.0)
    al = pipe.AlignRequest(1, capi.align_params(), None)
    assert call(req(hull_only=1), cs=cs) == capi.SFMX_ERR_INVALID
    assert call(req(hull_only=1), al=al) == capi.SFMX_ERR_INVALID
    assert call(req(hull_only=1), app=app) == capi.SFMX_ERR_INVALID
    assert call(req(), cs=cs) == capi.SFMX_OK and call(req(), app=app) == capi.SFMX_OK  # without hull_only they go together
    assert call(req()) == capi.SFMX_OK


def test_a_rectification_alone_leaves_no_disparity_map(ctx, ring2):
    """after Stereo.rectify the entries that take the stereo object's map refuse it; the carve entry takes the picture"""
    a, b = ring2["pairs"][0]
    r = pipe.stereo_rectify(ring2["K"], ring2["poses"][a], ring2["poses"][b], 320, 240)
    il, ir = (ring2["images"][b], ring2["images"][a]) if r["swapped"] else (ring2["images"][a], ring2["images"][b])
    vol = ring2["vol"]
    st, cv, cs, sh = ctx.stereo(320, 240, num_disparities=64), ctx.carve(), ctx.consist(), ctx.shade()
    fu = ctx.fusion(vol["origin"], vol["voxel"], vol["dims"])
    view = ring2["views"][0]
    st.rectify(il, ir, r["H_l"], r["H_r"])
    for fn in (fu.add_stereo_view, cs.add_stereo_view, sh.add_stereo_view):
        with pytest.raises(capi.SfmxError) as e:
            fn(view, st)
        assert e.value.status == capi.SFMX_ERR_INVALID
    cv.add_stereo_view(view, st, threshold=ring2["thr"])
    _same_bits(cv.read_view(0), CV.sd2_map(ring2["rects"][0], ring2["thr"], 16), "the rectified picture")
    st.disparity(il, ir, r["H_l"], r["H_r"])
    fu.add_stereo_view(view, st)
    cs.add_stereo_view(view, st)
    sh.add_stereo_view(view, st)
    assert fu.counts()[1] > 0
    for o in (st, cv, cs, sh, fu):
        o.close()
