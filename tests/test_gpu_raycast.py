"""GPU suite: TSDF ray casting.  Every render is compared with the NumPy restatement that evaluates every sample of every ray
(tests/raycast_ref.py: brute): depth, points and normals bit for bit, shaded byte for byte, hits equal.  The sphere fixture from
novel cameras, every way of feeding a volume, random volumes whose defined and undefined cells interleave, image shapes around
the 8 x 8 / 16 x 16 tiles, rays on grid lines, box faces and box edges, cameras inside, behind and beside the volume, sample
lattices against the box entry, the composition with the shade stage, pipeline.fuse / pipeline.run, and the refusals."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

import appearance_ref as AR
import consist_ref as CR
import fusion_ref as FR
import helpers as H
import raycast_ref as RR

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


@pytest.fixture(scope="module")
def rc(ctx):
    r = ctx.raycast()
    yield r
    r.close()


def _same(out, ref, what):
    assert out["depth"].shape == ref["depth"].shape, what
    assert out["hits"] == ref["hits"], f"{what}: hits {out['hits']} vs {ref['hits']}"
    for k in ("depth", "points", "normals"):
        H.assert_bits_equal(out[k], ref[k], f"{what}: {k}")
    assert out["shaded"].dtype == np.uint8 and out["shaded"].tobytes() == ref["shaded"].tobytes(), what + ": shaded"


def _bytes(out):
    return b"".join(out[k].tobytes() for k in ("depth", "points", "normals", "shaded")) + str(out["hits"]).encode()


def _case(rc, s, c, origin, voxel, cam, what, **kw):
    """render_arrays from host arrays against brute(); returns (device result, reference)"""
    mw = kw.pop("min_weight", 0)
    ref = RR.brute(s, c, origin, voxel, cam, cam["w"], cam["h"], min_weight=max(mw, 1), **kw)
    out = rc.render((s, c, origin, voxel), cam, min_weight=mw, **kw)
    _same(out, ref, what)
    return out, ref


def _sphere_case(rc, cam, what, **kw):
    sp = RR.sphere_volume()
    return _case(rc, sp["sum"], sp["count"], sp["vol"]["origin"], sp["vol"]["voxel"], cam, what, **kw)


# ---- the sphere ------------------------------------------------------------------------------------------------------------
def test_sphere_novel_camera(rc):
    cam = RR.camera(RR.SPHERE_CAM["pos"], (0.0, 0.0, 0.0), RR.SPHERE_CAM["f"], RR.SPHERE_CAM["w"], RR.SPHERE_CAM["h"])
    out, _ = _sphere_case(rc, cam, "sphere", **RR.SPHERE_MARCH)
    assert out["hits"] == 11732
    assert rc.last_samples() > 0


def test_sphere_min_weight_2(rc):
    cam = RR.camera((-0.3, 0.25, 0.3), (0.0, 0.0, 0.0), 200.0, 96, 96)
    out, _ = _sphere_case(rc, cam, "sphere min_weight 2", **RR.SPHERE_MARCH, min_weight=2, background=31)
    assert 0 < out["hits"] < 96 * 96 and (out["shaded"][out["depth"] == 0.0] == 31).all()
    # and one where it matters: at 6 the silhouette loses cells
    few, _ = _sphere_case(rc, cam, "sphere min_weight 6", **RR.SPHERE_MARCH, min_weight=6)
    assert 0 < few["hits"] < out["hits"]


# ---- feeds -----------------------------------------------------------------------------------------------------------------
def test_feeds_give_the_same_bytes(ctx):
    import torch
    from test_fusion_cpu import SPHERE, VOL, sphere_views
    fu, r = ctx.fusion(**VOL), ctx.raycast()
    for cam, d16 in sphere_views(**SPHERE):
        fu.add_view(cam, d16)
    march = dict(z_min=0.05, z_max=0.9)  # step 0: voxel / 2
    cams = [RR.camera(RR.SPHERE_CAM["pos"], (0.0, 0.0, 0.0), f, w, h) for f, w, h in ((80.0, 40, 30), (200.0, 96, 96), (40.0, 17, 16))]
    first = r.render(fu, cams[0], **march)  # the views are still pending: render integrates them
    s, c = fu.read()
    sp = RR.sphere_volume()
    assert s.tobytes() == sp["sum"].tobytes() and c.tobytes() == sp["count"].tobytes()
    ts, tc = torch.from_numpy(s).cuda(), torch.from_numpy(c).cuda()
    torch.cuda.synchronize()
    for i, cam in enumerate(cams):  # one object across sizes: growing, then shrinking
        ref = RR.brute(s, c, VOL["origin"], VOL["voxel"], cam, cam["w"], cam["h"], **march)
        a = r.render(fu, cam, **march) if i else first
        _same(a, ref, f"fusion object {i}")
        b = r.render((s, c, VOL["origin"], VOL["voxel"]), cam, **march)
        d = r.render((ts.data_ptr(), tc.data_ptr(), VOL["origin"], VOL["voxel"], VOL["dims"]), cam, **march)
        assert _bytes(a) == _bytes(b) == _bytes(d), f"feeds differ at size {i}"
        n, pts, nrm = r.device_surface()
        assert n == cam["w"] * cam["h"] and pts and nrm
    fu.close()
    r.close()


# ---- random volumes --------------------------------------------------------------------------------------------------------
def test_random_volumes(rc):
    no_normal = 0
    for dims in ((9, 7, 5), (65, 5, 3)):
        for step in RR.RANDOM_STEPS:
            for seed in RR.RANDOM_SEEDS:
                s, c, origin, voxel, cam, march = RR.random_case(dims, seed, step)
                out, ref = _case(rc, s, c, origin, voxel, cam, f"random {dims} step {step} seed {seed}", **march, background=7)
                assert 0 < ref["hits"] < cam["w"] * cam["h"]
                no_normal += int((ref["hit"] & ~ref["normal_defined"]).sum())
    assert no_normal > 0, "two defined samples that straddle a cell with an undefined corner: N = 0"


def test_no_crossing_gives_background(rc):
    s, c, origin, voxel, cam, march = RR.random_case((9, 7, 5), 0)
    out, _ = _case(rc, np.abs(s) + 0.1, np.ones_like(c), origin, voxel, cam, "no crossing", **march, background=99)
    assert out["hits"] == 0 and (out["shaded"] == 99).all() and not out["depth"].any() and not out["normals"].any()


# ---- image shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w, h", [(1, 1), (1, 300), (300, 1), (7, 9), (8, 8), (17, 16), (64, 4)])
def test_image_shapes(rc, w, h):
    cam = RR.camera(RR.SPHERE_CAM["pos"], (0.0, 0.0, 0.0), 0.8 * max(w, h), w, h)
    out, _ = _sphere_case(rc, cam, f"{w} x {h}", **RR.SPHERE_MARCH)
    assert out["hits"] > 0


# ---- geometry --------------------------------------------------------------------------------------------------------------
def _unit_sphere():
    """the sphere fixture's numbers on a grid at (-30, -30, -30) with voxel 1: grid coordinates are exact"""
    sp = RR.sphere_volume()
    return sp["sum"], sp["count"], (-30.0, -30.0, -30.0), 1.0


GEOMETRY = {
    # R = I, integer cx / cy: dw_0 = dw_1 = 0 on the centre pixel, every sample of its ray is a grid point or a cell's middle
    "grid lines": (RR.axis_camera((0.0, 0.0, -80.0), 40.0, 17, 13, 8, 6), dict(z_min=20.0, z_max=140.0, step=0.5)),
    # the centre column lies in the face x = -30 (g = 0, inside) / x = 30 (g = n - 1, outside), the centre pixel on an edge
    "lower faces": (RR.axis_camera((-30.0, -30.0, -80.0), 40.0, 17, 13, 8, 6), dict(z_min=20.0, z_max=140.0, step=0.5)),
    "upper faces": (RR.axis_camera((30.0, 30.0, -80.0), 40.0, 17, 13, 8, 6), dict(z_min=20.0, z_max=140.0, step=0.5)),
    "one face": (RR.axis_camera((-30.0, 3.0, -80.0), 40.0, 17, 13, 8, 6), dict(z_min=20.0, z_max=140.0, step=0.5)),
    # the lattice is offset from the box entry (depth 50) by 1/4, 1/2 + 1/4 ... of a step, and by an amount that is no fraction
    "lattice offset": (RR.axis_camera((0.3, -0.2, -80.0), 40.0, 17, 13, 8, 6), dict(z_min=20.125, z_max=140.0, step=0.5)),
    "lattice offset, oblique": (RR.camera((41.0, 33.0, -52.0), (0.0, 0.0, 0.0), 60.0, 24, 20), dict(z_min=9.87, z_max=140.0, step=0.37)),
    "entry on the first sample": (RR.axis_camera((0.0, 0.0, -80.0), 40.0, 9, 9, 4, 4), dict(z_min=50.0, z_max=120.0, step=0.5)),
    "z_max inside the box": (RR.axis_camera((0.0, 0.0, -80.0), 40.0, 17, 13, 8, 6), dict(z_min=20.0, z_max=75.0, step=0.5)),
    "step 2.5 voxels": (RR.camera((41.0, 33.0, -52.0), (0.0, 0.0, 0.0), 60.0, 24, 20), dict(z_min=10.0, z_max=140.0, step=2.5)),
    "one sample": (RR.camera((41.0, 33.0, -52.0), (0.0, 0.0, 0.0), 60.0, 24, 20), dict(z_min=60.0, z_max=61.0, step=2.5)),
    "two samples": (RR.camera((41.0, 33.0, -52.0), (0.0, 0.0, 0.0), 60.0, 24, 20), dict(z_min=53.0, z_max=60.0, step=4.0)),
    "exact integer quotient": (RR.camera((41.0, 33.0, -52.0), (0.0, 0.0, 0.0), 60.0, 24, 20), dict(z_min=16.0, z_max=144.0, step=0.25)),
    "inside the volume": (RR.camera((24.0, 4.0, -22.0), (0.0, 0.0, 0.0), 30.0, 24, 20), dict(z_min=1.0, z_max=90.0, step=0.5)),
    "inside the sphere": (RR.camera((2.0, 4.0, 0.0), (30.0, 10.0, 20.0), 30.0, 24, 20), dict(z_min=1.0, z_max=90.0, step=0.5)),
    "behind": (RR.camera((0.0, 10.0, 120.0), (0.0, 20.0, 240.0), 30.0, 24, 20), dict(z_min=1.0, z_max=200.0, step=0.5)),
    "beside": (RR.camera((60.0, 0.0, -60.0), (38.0, 0.0, 0.0), 30.0, 24, 20), dict(z_min=1.0, z_max=200.0, step=0.5)),
    "far away": (RR.camera((4100.0, 3300.0, -5200.0), (0.0, 0.0, 0.0), 3000.0, 24, 20), dict(z_min=7300.0, z_max=7500.0, step=0.5)),
}
# what each case must show on the NumPy side: hits expected (True), excluded (False) or left open (None)
GEOMETRY_HITS = {"upper faces": False, "one sample": False, "inside the sphere": False, "behind": False, "beside": None, "two samples": None,
                 "lower faces": None}


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_geometry(rc, name):
    cam, march = GEOMETRY[name]
    s, c, origin, voxel = _unit_sphere()
    out, ref = _case(rc, s, c, origin, voxel, cam, name, **march, background=3)
    want = GEOMETRY_HITS.get(name, True)
    if want is not None:
        assert (ref["hits"] > 0) == want, (name, ref["hits"])
    if name == "grid lines":
        dw = RR.rays(cam, cam["w"], cam["h"])
        assert dw[0][6, 8] == 0.0 and dw[1][6, 8] == 0.0 and ref["hit"][6, 8]
    if name == "exact integer quotient":
        assert (march["z_max"] - march["z_min"]) / march["step"] == 512.0 and RR.sample_count(**march) == 513
    if name == "beside":
        assert 0 < ref["hits"] < ref["hit"].size // 2, "only part of the image crosses the box"


# ---- composition with the shade stage ----------------------------------------------------------------------------------------
def _shade_ref(ref, views, tol, background, **kw):
    g, v = AR.shade(ref["points"].reshape(-1, 3), ref["normals"].reshape(-1, 3), views, tol, **kw)
    hit = ref["hit"].ravel()
    return np.where(hit, g, background).astype(np.uint8).reshape(ref["hit"].shape), np.where(hit, v, 0).astype(np.int32).reshape(ref["hit"].shape)


def _scene(ctx, vol, views):
    fu, sh = ctx.fusion(**vol), ctx.shade()
    for cam, d16, img in views:
        fu.add_view(cam, d16)
        sh.add_view(cam, d16, img)
    return fu, sh


def test_shade_textured_sphere(ctx, rc):
    from test_fusion_cpu import SPHERE, VOL
    views = AR.textured_sphere_views(**SPHERE)
    fu, sh = _scene(ctx, VOL, views)
    cam = RR.camera(RR.SPHERE_CAM["pos"], (0.0, 0.0, 0.0), 150.0, 80, 80)
    out = rc.render(fu, cam, **RR.SPHERE_MARCH, background=17)
    s, c = fu.read()
    ref = RR.brute(s, c, VOL["origin"], VOL["voxel"], cam, 80, 80, **RR.SPHERE_MARCH, background=17)
    _same(out, ref, "textured sphere")
    tol = FR.resolve(VOL["voxel"])
    for kw in (dict(), dict(cull=0, fill=5)):
        g, v = rc.shade(sh, tol, **kw)
        eg, ev = _shade_ref(ref, views, tol, 17, **kw)
        assert g.dtype == np.uint8 and v.dtype == np.int32 and g.tobytes() == eg.tobytes() and v.tobytes() == ev.tobytes(), kw
    assert (g[~ref["hit"]] == 17).all() and (v[ref["hit"]] >= 1).all()
    fu.close()
    sh.close()


def test_shade_two_spheres(ctx, rc):
    """the conditions DESIGN.md 14 proves for vertices hold for ray-cast pixels as well (checked on the NumPy side first): with
    depth_tol = trunc every hit pixel is seen, and a pixel on A (B) is exactly 80 (200) -- no view that sees the other sphere
    through it contributes"""
    views = AR.two_sphere_views()
    V = AR.TWO_VOL
    fu, sh = _scene(ctx, V, views)
    cam = RR.camera((0.1, 0.15, -0.45), (0.06, 0.0, 0.0), 300.0, 128, 128)
    march = dict(z_min=0.2, z_max=0.8)
    out = rc.render(fu, cam, **march)
    s, c = fu.read()
    ref = RR.brute(s, c, V["origin"], V["voxel"], cam, 128, 128, **march)
    _same(out, ref, "two spheres")
    tol = FR.resolve(V["voxel"])
    eg, ev = _shade_ref(ref, views, tol, 0)
    hit = ref["hit"]
    A, B = (m.reshape(hit.shape) & hit for m in AR.two_sphere_labels(ref["points"].reshape(-1, 3)))
    assert ref["hits"] == 7433 and A.sum() == 6579 and B.sum() == 854 and not (hit & ~A & ~B).any()
    assert (ev[hit] >= 1).all() and (eg[A] == 80).all() and (eg[B] == 200).all()
    g, v = rc.shade(sh, tol)
    assert g.tobytes() == eg.tobytes() and v.tobytes() == ev.tobytes()
    fu.close()
    sh.close()


# ---- pipeline ----------------------------------------------------------------------------------------------------------------
def _pose_cam(K, pose):
    """the pinhole of a camera->world pose (R, c) with intrinsics K"""
    R, c = pose
    return dict(R_rw=np.asarray(R, np.float64).T.copy(), c_left=np.asarray(c, np.float64), f=float(K[0, 0]), cx=float(K[0, 2]), cy=float(K[1, 2]))


def _read_pgm(path):
    data = open(path, "rb").read()
    magic, size, maxval, body = data.split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    assert magic == b"P5" and maxval == b"255" and len(body) == w * h
    return np.frombuffer(body, np.uint8).reshape(h, w)


def test_fuse_render(ctx, tmp_path):
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES[:2], 320, 240)
    vol = CR.RING6_VOL
    args = (ctx, images, K, poses, pairs, vol["origin"], vol["voxel"], vol["dims"])
    cams = [_pose_cam(K, poses[0]), RR.camera((0.25, 0.2, -0.3), (0.0, 0.0, 0.0), 250.0, 96, 80)]
    dist = float(np.linalg.norm(poses[0][1]))
    rq = dict(cameras=cams, w=96, h=80, z_min=0.05, z_max=dist + 0.3, background=11)
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain.ply", "render.ply", "app.ply"))
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    m = pipe.fuse(*args, num_disparities=64, ply_path=p1, render=dict(rq, pgm_prefix=str(tmp_path / "r")))
    assert set(m) == set(m0) | {"renders"} and len(m["renders"]) == 2
    assert m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read(), "the render changes no other output"
    # the standalone object on the same volume: the same pairs through the stereo kernels, queued by hand
    st, fu, sh, r = ctx.stereo(320, 240, num_disparities=64), ctx.fusion(**vol), ctx.shade(), ctx.raycast()
    views = []
    for a, b in pairs:
        rect = pipe.stereo_rectify(K, poses[a], poses[b], 320, 240)
        il, ir = (images[b], images[a]) if rect["swapped"] else (images[a], images[b])
        d = st.disparity(il, ir, rect["H_l"], rect["H_r"], want_rect=True)
        fu.add_view(rect, d["disp16"])
        sh.add_view(rect, d["disp16"], d["rect"][0])
        views.append((rect, d["disp16"], d["rect"][0].copy()))
    s, c = fu.read()
    kw = {k: rq[k] for k in ("z_min", "z_max", "background")}
    own, refs = [], []
    for i, cam in enumerate(cams):
        own.append(r.render(fu, dict(cam, w=96, h=80), **kw))
        assert set(m["renders"][i]) == {"depth", "normals", "points", "shaded", "hits"}
        assert _bytes(m["renders"][i]) == _bytes(own[i]), f"fuse render {i} vs the standalone object"
        refs.append(RR.brute(s, c, vol["origin"], vol["voxel"], cam, 96, 80, **kw))
        _same(own[i], refs[i], f"ring render {i}")
        assert own[i]["hits"] > 500
        assert (_read_pgm(str(tmp_path / f"r_{i}_shaded.pgm")) == own[i]["shaded"]).all()
    assert not os.path.exists(str(tmp_path / "r_0_grey.pgm"))
    # with appearance: grey and pixel_views from the retained shade views
    ma = pipe.fuse(*args, num_disparities=64, ply_path=p2, appearance=True, render=dict(rq, pgm_prefix=str(tmp_path / "a")))
    ma0 = pipe.fuse(*args, num_disparities=64, appearance=True)
    for k in ("verts", "faces", "normals", "grey", "vertex_views"):
        assert ma[k].tobytes() == ma0[k].tobytes(), k
    tol = FR.resolve(vol["voxel"])
    for i in range(2):
        rr = ma["renders"][i]
        assert _bytes(rr) == _bytes(own[i])
        eg, ev = _shade_ref(refs[i], views, tol, 11)
        assert rr["grey"].tobytes() == eg.tobytes() and rr["pixel_views"].tobytes() == ev.tobytes() and rr["pixel_views"].dtype == np.int32
        assert (_read_pgm(str(tmp_path / f"a_{i}_grey.pgm")) == rr["grey"]).all()
        assert (_read_pgm(str(tmp_path / f"a_{i}_shaded.pgm")) == rr["shaded"]).all()
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, render=dict(rq, colour=1))
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, render=dict(cameras=cams, w=96, h=80))
    with pytest.raises(capi.SfmxError):
        pipe.fuse(*args, num_disparities=64, render=dict(rq, z_max=0.01))
    none = pipe.fuse(*args, num_disparities=64, render=dict(rq, cameras=[]))
    assert none["renders"] == [] and none["verts"].tobytes() == m0["verts"].tobytes()
    for o in (st, fu, sh, r):
        o.close()


def test_pipeline_run_render(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    plain, rend = str(tmp_path / "plain"), str(tmp_path / "render")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in PAIR)
    sm = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][PAIR[0]], r0["kf_poses"][PAIR[1]], **SMALL)
    lo, hi = sm["verts"].min(0), sm["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    fz = dict(pairs=[PAIR], origin=tuple(lo), voxel=voxel, dims=dims, **SMALL)
    pose = r0["kf_poses"][PAIR[0]]
    cam = _pose_cam(np.asarray(g["K"], np.float64).reshape(3, 3), (pose[:9].reshape(3, 3), pose[9:]))
    far = float(np.linalg.norm(np.maximum(np.abs(lo - pose[9:]), np.abs(hi - pose[9:]))))
    h, w = g["images"].shape[1:]
    rq = dict(cameras=[cam], w=w // 4, h=h // 4, z_min=far / 64.0, z_max=far, step=far / 256.0)
    rq["cameras"][0].update(f=cam["f"] / 4.0, cx=cam["cx"] / 4.0, cy=cam["cy"] / 4.0)
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain, fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, rend, fusion=dict(fz, render=rq))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(rend, "X")
    assert sorted(os.listdir(rend)) == sorted(os.listdir(plain))
    for fn in os.listdir(plain):
        assert open(os.path.join(plain, fn), "rb").read() == open(os.path.join(rend, fn), "rb").read(), fn
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m) == set(m1) | {"renders"} and m["verts"].tobytes() == m1["verts"].tobytes() and len(m["renders"]) == 1
    # the NumPy side: the same pair through the stereo kernels, integrated and rendered by the restatements
    rect = pipe.stereo_rectify(g["K"], r2["kf_poses"][PAIR[0]], r2["kf_poses"][PAIR[1]], w, h)
    il, ir = (g["images"][fb], g["images"][fa]) if rect["swapped"] else (g["images"][fa], g["images"][fb])
    st = ctx.stereo(w, h, **SMALL)
    d16 = st.disparity(il, ir, rect["H_l"], rect["H_r"])
    st.close()
    s, c = FR.integrate(tuple(lo), voxel, dims, [(rect, d16)])
    ref = RR.brute(s, c, tuple(lo), voxel, rq["cameras"][0], w // 4, h // 4, z_min=rq["z_min"], z_max=rq["z_max"], step=rq["step"])
    _same(m["renders"][0], ref, "pipeline.run render")
    assert ref["hits"] > 0


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    r, sh = ctx.raycast(), ctx.shade()
    sp = RR.sphere_volume()
    vol = (sp["sum"], sp["count"], sp["vol"]["origin"], sp["vol"]["voxel"])
    cam = RR.camera(RR.SPHERE_CAM["pos"], (0.0, 0.0, 0.0), 30.0, 16, 16)
    lib = ctx.lib

    def refused(fn):
        with pytest.raises(capi.SfmxError) as e:
            fn()
        assert e.value.status == capi.SFMX_ERR_INVALID and str(e.value).split(": ", 1)[1], "SFMX_ERR_INVALID with a message"

    refused(lambda: r.shade(sh, 0.02))  # before any render
    refused(r.read)
    with pytest.raises(capi.SfmxError):
        r.device_surface()
    p = capi.raycast_params(0.05, 0.9)
    fp = capi.fusion_params(sp["vol"]["origin"], sp["vol"]["voxel"], sp["vol"]["dims"])
    s, c = np.ascontiguousarray(sp["sum"]), np.ascontiguousarray(sp["count"])
    arrays = (ctypes.byref(fp), s.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(0))
    refused(lambda: ctx._chk(lib.sfmx_raycast_render_arrays(ctx.h_, r.h_, *arrays, None, ctypes.byref(p))))  # a NULL view
    refused(lambda: ctx._chk(lib.sfmx_raycast_render_arrays(ctx.h_, r.h_, *arrays, ctypes.byref(capi.fusion_view(cam, 16, 16)), None)))
    refused(lambda: r.render(vol, dict(cam, w=4096, h=4097), 0.05, 0.9))  # w * h over 2^24
    refused(lambda: r.render(vol, dict(cam, w=4097, h=1), 0.05, 0.9))
    refused(lambda: r.render(vol, dict(cam, w=0, h=4), 0.05, 0.9))
    refused(lambda: r.render(vol, dict(cam, f=0.0), 0.05, 0.9))
    refused(lambda: r.render(vol, cam, 0.05, 0.9, step=1e-9))  # K over the limit
    refused(lambda: r.render(vol, cam, 0.9, 0.05))
    refused(lambda: r.render((sp["sum"][:1], sp["count"][:1], sp["vol"]["origin"], sp["vol"]["voxel"]), cam, 0.05, 0.9))  # nz = 1
    # the object is still usable, and a failed render leaves no result behind
    ok = r.render(vol, cam, 0.05, 0.9)
    assert ok["hits"] > 0
    g, v = r.shade(sh, 0.02)  # no views: every hit pixel gets fill, every other the background
    assert not g.any() and not v.any()
    refused(lambda: r.render(vol, cam, 0.9, 0.05))
    refused(r.read)
    r.close()
    sh.close()
