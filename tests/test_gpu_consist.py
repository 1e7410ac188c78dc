"""GPU suite: multi-view consistency filtering of disparity maps.  sfmx_consist_* gives the filtered maps, the support counts
and the per-view counters byte for byte against the NumPy restatement (tests/consist_ref.py): a noisy sphere over the parameter
range with a camera inside it, views at the edges of the 64 x 4 tile, the u8 saturation of the support, every way of feeding
views, the state rules, ring pairs through the stereo kernels into the volume, pipeline.fuse / pipeline.run, and the quality
bound of DESIGN.md 15 on the device."""
import importlib
import json
import os

import numpy as np
import pytest

import appearance_ref as AR
import consist_ref as CR
import fusion_ref as FR
import helpers as H
from test_consist_cpu import OFF_SHELL, RMS_FILTERED

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
PAIR = (2, 3)  # e2e_keyframes: the pair with valid disparity
SMALL = dict(num_disparities=32, census=5)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _feed(cs, views):
    for cam, d16 in views:
        cs.add_view(cam, d16)


def _device_bytes(cs):
    """everything a filter leaves behind, as one byte string"""
    valid, kept = cs.counts()
    assert valid.dtype == np.int32 and kept.dtype == np.int32
    parts = [valid.tobytes(), kept.tobytes()]
    for i in range(cs.view_count()):
        d16, sup = cs.read(i)
        assert d16.dtype == np.int16 and sup.dtype == np.uint8
        parts += [d16.tobytes(), sup.tobytes()]
    return b"".join(parts)


def _ref_bytes(ref):
    parts = [ref["valid"].tobytes(), ref["kept"].tobytes()]
    for d16, sup in zip(ref["disp16"], ref["support"]):
        parts += [d16.tobytes(), sup.tobytes()]
    return b"".join(parts)


def _check(cs, ref, what):
    valid, kept = cs.counts()
    assert (valid == ref["valid"]).all(), what + ": valid counters"
    assert (kept == ref["kept"]).all(), what + ": kept counters"
    for i in range(cs.view_count()):
        d16, sup = cs.read(i)
        assert d16.shape == ref["disp16"][i].shape
        assert (sup == ref["support"][i]).all(), f"{what}: support of view {i}"
        assert (d16 == ref["disp16"][i]).all(), f"{what}: disp16 of view {i}"
    assert _device_bytes(cs) == _ref_bytes(ref), what


def _case(ctx, views, what, **params):
    ref = CR.filter_views(views, **params)
    cs = ctx.consist()
    _feed(cs, views)
    assert cs.view_count() == len(views)
    cs.filter(**params)
    _check(cs, ref, what)
    cs.close()
    return ref


# ---- sphere-8: the parameter range -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere8():
    return CR.sphere8()


PARAMS = [dict(), dict(rel_tol=4.0), dict(reproj_px=0.0), dict(min_support=0), dict(min_support=1), dict(min_support=3),
          dict(disp_min=-5.0), dict(disp_min=0.0), dict(disp_min=40.0)]


@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()) or "defaults")
def test_sphere8_bit_equal(ctx, sphere8, params):
    ref = _case(ctx, sphere8, f"sphere-8 {params}", **params)
    hand = sphere8[8][1]  # the ninth camera's hand-set map: 0, negative and extreme values
    base = int(((hand != -16) & (hand >= 16)).sum())
    if params.get("disp_min") == 40.0:  # above every disparity of the scene but int16's largest: whole waves leave early
        assert ref["valid"].sum() == 1 and ref["kept"].sum() == 0
        return
    assert ref["valid"][:8].sum() > 15000
    if params.get("min_support") == 0:
        assert (ref["kept"] == ref["valid"]).all()
    elif params.get("reproj_px") == 0.0:  # only an exact round trip counts: next to nothing survives
        assert ref["kept"].sum() < CR.filter_views(sphere8)["kept"].sum()
    else:
        assert 0 < ref["kept"].sum() < ref["valid"].sum()
    if "disp_min" in params:
        assert ref["valid"][8] > base, "disp_min <= 0 lets 0 (and at -5 the negative disparities) through"
    else:
        assert ref["valid"][8] == base


def test_sphere8_takes_every_outcome(sphere8):
    """counted in NumPy: the defaults and rel_tol 4.0, both compared with the device above, take all seven outcomes"""
    c0, c4 = {}, {}
    CR.filter_views(sphere8, counter=c0)
    CR.filter_views(sphere8, counter=c4, rel_tol=4.0)
    print("defaults", c0, "rel_tol 4.0", c4)
    assert all(c0[k] > 0 for k in CR.OUTCOMES if k != "back_behind"), c0
    assert c4["back_behind"] > 0 and all(c0[k] + c4[k] > 0 for k in CR.OUTCOMES)


# ---- shapes, saturation ----------------------------------------------------------------------------------------------------
def test_shapes_at_the_tile_edges(ctx):
    """1 x 1, 1 x 300, 300 x 1, 63 x 4, 64 x 4, 65 x 5 and 4096 x 2 pixels in one object, and in the reverse order"""
    views = CR.edge_shape_views()
    assert [d.shape[::-1] for _, d in views] == list(CR.EDGE_SHAPES)
    ref = _case(ctx, views, "tile edges")
    assert ref["kept"].sum() > 100 and (ref["valid"] - ref["kept"]).sum() > 100, "some pixels kept and some dropped"
    assert (ref["kept"] > 0).all()
    _case(ctx, views[::-1], "tile edges, reversed", min_support=1)


def test_support_saturates_at_255(ctx):
    views = CR.identical_views(300)
    ref = CR.filter_views(views, only=[0])
    valid = views[0][1] != -16
    assert valid.sum() > 10 and (ref["support"][0][valid] == 255).all() and (ref["support"][0][~valid] == 0).all()
    cs = ctx.consist()
    _feed(cs, views)
    cs.filter()
    v, k = cs.counts()
    assert (v == ref["valid"][0]).all() and (k == ref["kept"][0]).all() and len(v) == 300
    for i in (0, 1, 150, 298, 299):
        d16, sup = cs.read(i)
        assert (sup == ref["support"][0]).all() and (d16 == ref["disp16"][0]).all()
    cs.filter(min_support=299)  # the comparison is on the count, not on the saturated byte
    assert (cs.counts()[1] == ref["valid"][0]).all()
    cs.filter(min_support=300)
    assert (cs.counts()[1] == 0).all()
    cs.close()


# ---- ring pairs through the stereo kernels ---------------------------------------------------------------------------------
def _device_views(ctx, images, K, poses, pairs, **sp):
    """per pair: (rect, device disp16, device left rectified image, left source image, right source image)"""
    h, w = images.shape[1:]
    st = ctx.stereo(w, h, **sp)
    out = []
    for a, b in pairs:
        r = pipe.stereo_rectify(K, poses[a], poses[b], w, h)
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        d = st.disparity(il, ir, r["H_l"], r["H_r"], want_rect=True)
        out.append((r, d["disp16"], d["rect"][0].copy(), il, ir))
    st.close()
    return out


@pytest.fixture(scope="module")
def ring6(ctx):
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    full = _device_views(ctx, images, K, poses, pairs, num_disparities=64)
    views = [(r, d) for r, d, _, _, _ in full]
    ref = CR.filter_views(views)
    assert ((ref["kept"] > 0) & (ref["kept"] < ref["valid"])).all(), "precondition: the filter acts on every view"
    return dict(images=images, K=K, poses=poses, pairs=pairs, full=full, views=views, ref=ref, vol=CR.RING6_VOL)


def test_feeding_paths_same_bytes(ctx, ring6):
    """host maps, device maps and add_stereo_view; reset and reuse; the slab regrown with earlier views in it"""
    import torch
    views, full, want = ring6["views"], ring6["full"], _ref_bytes(ring6["ref"])
    h, w = views[0][1].shape
    cs = ctx.consist()
    small = CR.sphere8()[:2]
    _feed(cs, small)  # 2 x 64 x 64 first: the slab is regrown several times by the six larger views
    _feed(cs, views)
    cs.filter()
    _check(cs, CR.filter_views(small + views), "regrown slab")
    cs.reset()
    assert cs.view_count() == 0
    _feed(cs, views)
    cs.filter()
    host = _device_bytes(cs)
    cs.reset()
    dev = [torch.from_numpy(np.ascontiguousarray(d)).to("cuda:0") for _, d in views]
    torch.cuda.synchronize()
    for (r, _), td in zip(views, dev):
        cs.add_view(r, td.data_ptr(), shape=(h, w))
    cs.filter()
    devb = _device_bytes(cs)
    cs.reset()
    st = ctx.stereo(w, h, num_disparities=64)
    for r, _, _, il, ir in full:
        st.disparity(il, ir, r["H_l"], r["H_r"])
        cs.add_stereo_view(r, st)
    st.close()
    cs.filter()
    stv = _device_bytes(cs)
    cs.close()
    assert host == want, "host maps after reset"
    assert devb == want, "device maps after reset"
    assert stv == want, "add_stereo_view after reset"


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


def test_state_rules(ctx, sphere8):
    cs, fu = ctx.consist(), ctx.fusion(**CR.RING6_VOL)
    cs.filter()  # 0 views is not an error
    v, k = cs.counts()
    assert v.shape == (0,) and k.shape == (0,) and cs.last_us() == 0.0
    _invalid(lambda: cs.read(0))
    _invalid(lambda: fu.add_consist_view(cs, 0))
    cs.add_view(*sphere8[0])
    for fn in (lambda: cs.read(0), cs.counts, lambda: fu.add_consist_view(cs, 0)):
        _invalid(fn)  # before a filter
    cs.filter()  # 1 view: no other view, support 0 everywhere
    d16, sup = cs.read(0)
    v, k = cs.counts()
    assert (d16 == -16).all() and (sup == 0).all() and list(v) == [1990] and list(k) == [0]
    cs.filter(min_support=0)
    assert (cs.read(0)[0] == np.where(sphere8[0][1] != -16, sphere8[0][1], -16)).all() and list(cs.counts()[1]) == [1990]
    for i in (-1, 1, 1 << 20):
        _invalid(lambda: cs.read(i))
        _invalid(lambda: fu.add_consist_view(cs, i))
    fu.add_consist_view(cs, 0)
    cs.add_view(*sphere8[1])
    for fn in (lambda: cs.read(0), cs.counts, lambda: fu.add_consist_view(cs, 0)):
        _invalid(fn)  # after an add
    cs.filter()
    assert cs.read(1)[0].shape == (64, 64)
    cs.reset()
    for fn in (lambda: cs.read(0), cs.counts):
        _invalid(fn)  # after a reset
    with pytest.raises(capi.SfmxError):
        cs.filter(rel_tol=0.0)
    with pytest.raises(capi.SfmxError):
        cs.add_view(dict(sphere8[0][0], f=float("nan")), sphere8[0][1])
    cs.close()
    fu.close()


def test_ring6_into_the_volume(ctx, ring6):
    """the filter against NumPy; a volume fed by add_consist_view against one fed the filtered host maps against fusion_ref"""
    views, ref, vol = ring6["views"], ring6["ref"], ring6["vol"]
    cs = ctx.consist()
    _feed(cs, views)
    cs.filter()
    _check(cs, ref, "ring-6")
    want = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(views, ref))
    assert len(want["faces"]) > 5000
    fa, fb = ctx.fusion(**vol), ctx.fusion(**vol, max_views=4)  # fb: a full stack is integrated on the way
    for i in range(len(views)):
        fa.add_consist_view(cs, i)
        fb.add_consist_view(cs, i)
    fc = ctx.fusion(**vol)
    for cam, d16 in CR.filtered_views(views, ref):
        fc.add_view(cam, d16)
    for fu, what in ((fa, "add_consist_view"), (fb, "add_consist_view, max_views 4"), (fc, "filtered host maps")):
        s, c = fu.read()
        v, f = fu.extract()
        H.assert_bits_equal(s, want["sum"], what + ": sum")
        assert (c == want["count"]).all(), what + ": count"
        assert v.tobytes() == want["verts"].tobytes(), what + ": verts"
        assert f.tobytes() == want["faces"].tobytes(), what + ": faces"
        fu.close()
    cs.close()


# ---- pipeline --------------------------------------------------------------------------------------------------------------
def test_host_fuse_consistency(ctx, ring6, tmp_path):
    vol, ref, views = ring6["vol"], ring6["ref"], ring6["views"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain.ply", "false.ply", "on.ply"))
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    m1 = pipe.fuse(*args, num_disparities=64, ply_path=p1, consistency=False)
    assert set(m0) == set(m1) == {"verts", "faces", "views", "warn"}
    assert m0["verts"].tobytes() == m1["verts"].tobytes() and m0["faces"].tobytes() == m1["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read(), "consistency=False is the call without the argument"
    m = pipe.fuse(*args, num_disparities=64, ply_path=p2, consistency=True)
    assert set(m) == {"verts", "faces", "views", "warn", "consistency"} and m["views"] == 6 and m["warn"] is None
    assert m["consistency"] == dict(valid=[int(v) for v in ref["valid"]], kept=[int(v) for v in ref["kept"]])
    want = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(views, ref))
    assert m["verts"].tobytes() == want["verts"].tobytes() and m["faces"].tobytes() == want["faces"].tobytes()
    assert len(m["verts"]) < len(m0["verts"]) and open(p2).read().startswith("ply\nformat ascii 1.0\nelement vertex %d\n" % len(m["verts"]))
    # the manual chain
    h, w = views[0][1].shape
    st, cs, fu = ctx.stereo(w, h, num_disparities=64), ctx.consist(), ctx.fusion(**vol)
    for r, _, _, il, ir in ring6["full"]:
        st.disparity(il, ir, r["H_l"], r["H_r"])
        cs.add_stereo_view(r, st)
    cs.filter()
    for i in range(cs.view_count()):
        fu.add_consist_view(cs, i)
    v, f = fu.extract()
    assert m["verts"].tobytes() == v.tobytes() and m["faces"].tobytes() == f.tobytes()
    for o in (st, cs, fu):
        o.close()
    # parameters, a skipped pair, no pairs
    kw = dict(rel_tol=0.02, reproj_px=2.0, min_support=1)
    pairs = [ring6["pairs"][0], (0, 99)] + ring6["pairs"][1:]
    m3 = pipe.fuse(*args[:4], pairs, *args[5:], num_disparities=64, disp_min=2.0, consistency=kw)
    ref3 = CR.filter_views(views, disp_min=2.0, **kw)
    assert m3["views"] == 6 and "skipped" in m3["warn"]
    assert m3["consistency"] == dict(valid=[int(v) for v in ref3["valid"]], kept=[int(v) for v in ref3["kept"]])
    want3 = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(views, ref3), disp_min=2.0)
    assert m3["verts"].tobytes() == want3["verts"].tobytes() and m3["faces"].tobytes() == want3["faces"].tobytes()
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, consistency=dict(depth_tol=1.0))
    with pytest.raises(capi.SfmxError):
        pipe.fuse(*args, num_disparities=64, consistency=dict(rel_tol=-1.0))
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, consistency=True)
    assert empty["verts"].shape == (0, 3) and empty["consistency"] == dict(valid=[], kept=[])


def test_host_fuse_consistency_with_appearance(ctx, ring6):
    """the volume takes the filtered maps, the shade views keep the raw ones"""
    vol, ref, full = ring6["vol"], ring6["ref"], ring6["full"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    m = pipe.fuse(*args, num_disparities=64, consistency=True, appearance=True)
    assert set(m) == {"verts", "faces", "views", "warn", "normals", "grey", "vertex_views", "consistency"}
    want = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(ring6["views"], ref))
    nrm = AR.normals(want["sum"], want["count"])
    grey, cnt = AR.shade(want["verts"], nrm, [(r, d, im) for r, d, im, _, _ in full], FR.resolve(vol["voxel"]))
    assert m["verts"].tobytes() == want["verts"].tobytes() and m["faces"].tobytes() == want["faces"].tobytes()
    H.assert_bits_equal(m["normals"], nrm, "normals of the filtered volume")
    assert (m["grey"] == grey).all() and (m["vertex_views"] == cnt).all()
    assert m["consistency"]["kept"] == [int(v) for v in ref["kept"]]
    filt = [(r, f, im) for (r, _, im, _, _), f in zip(full, ref["disp16"])]
    _, cnt_f = AR.shade(want["verts"], nrm, filt, FR.resolve(vol["voxel"]))
    assert (cnt_f != cnt).any(), "shading from the filtered maps would give other view counts: the test can tell"


def test_pipeline_run_consistency(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    plain, filt = str(tmp_path / "plain"), str(tmp_path / "filt")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in PAIR)
    sm = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][PAIR[0]], r0["kf_poses"][PAIR[1]], **SMALL)
    lo, hi = sm["verts"].min(0), sm["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    # the pair listed twice: two views with one camera support each other (j != i is by index)
    fz = dict(pairs=[PAIR, PAIR], origin=tuple(lo), voxel=voxel, dims=dims, **SMALL)
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain, fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, filt, fusion=dict(fz, consistency=dict(min_support=1)))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(filt, "X")
    assert sorted(os.listdir(filt)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m1) == {"verts", "faces", "views", "warn"} and m["views"] == 2 and len(m["faces"]) > 0
    h, w = g["images"].shape[1:]
    rect = pipe.stereo_rectify(g["K"], r2["kf_poses"][PAIR[0]], r2["kf_poses"][PAIR[1]], w, h)
    il, ir = (g["images"][fb], g["images"][fa]) if rect["swapped"] else (g["images"][fa], g["images"][fb])
    d16 = ctx.stereo_disparity(il, ir, rect["H_l"], rect["H_r"], **SMALL)
    ref = CR.filter_views([(rect, d16), (rect, d16)], min_support=1)
    assert m["consistency"] == dict(valid=[int(v) for v in ref["valid"]], kept=[int(v) for v in ref["kept"]])
    assert 0 < ref["kept"][0] <= ref["valid"][0]
    want = FR.fuse(tuple(lo), voxel, dims, CR.filtered_views([(rect, d16), (rect, d16)], ref))
    assert m["verts"].tobytes() == want["verts"].tobytes() and m["faces"].tobytes() == want["faces"].tobytes()
    assert open(os.path.join(filt, "templeRing_mesh_fused.ply")).read().startswith(
        "ply\nformat ascii 1.0\nelement vertex %d\n" % len(m["verts"]))


# ---- quality ---------------------------------------------------------------------------------------------------------------
def test_noisy_sphere26_quality(ctx):
    """5 % outliers in all 26 maps, filtered and fused on the device: at most the recorded number of vertices off the shell"""
    noisy, _ = CR.sphere26(True)
    vol = CR.SPHERE26_VOL
    cs, fu, raw = ctx.consist(), ctx.fusion(**vol), ctx.fusion(**vol)
    _feed(cs, noisy)
    for cam, d16 in noisy:
        raw.add_view(cam, d16)
    cs.filter()
    valid, kept = cs.counts()
    for i in range(len(noisy)):
        fu.add_consist_view(cs, i)
    off, rms = CR.off_shell(fu.extract()[0])
    off_raw, rms_raw = CR.off_shell(raw.extract()[0])
    print("noisy sphere-26 on the device: kept %d of %d; off the shell %d (unfiltered %d), radius RMS %.3f (%.3f) voxel"
          % (kept.sum(), valid.sum(), off, off_raw, rms, rms_raw))
    assert off <= OFF_SHELL and rms <= RMS_FILTERED
    assert off_raw > 10 * OFF_SHELL
    for o in (cs, fu, raw):
        o.close()
