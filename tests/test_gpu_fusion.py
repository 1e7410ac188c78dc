"""GPU suite: multi-pair depth fusion.  Device sum / count and the extracted surface bit for bit against the NumPy restatement
(tests/fusion_ref.py) on analytic sphere views and on real ring pairs (the device's own disparity maps, which
tests/test_gpu_stereo.py pins to tests/stereo_ref.py); every way of feeding views gives the same bytes; edge cases; the whole
ring; and the fusion request of pipeline.run with every pre-existing output unchanged."""
import importlib
import json
import os

import numpy as np
import pytest

import fusion_ref as FR
import helpers as H
from test_fusion_cpu import SPHERE, VOL, sphere_views

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
FILES = ("keyframes_camera_centers.csv", "posegraph_edges.csv", "templeRing_sparse_points.ply")
PAIR = (2, 3)  # e2e_keyframes: the pair with valid disparity
SMALL = dict(num_disparities=32, census=5)
RING_VOL = dict(origin=(-0.13, -0.13, -0.13), voxel=0.002, dims=(131, 131, 131))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _ring(angles_ab, w, h):
    """frames at the given (a, b) ring angles: (images [2m][h][w], K, poses [2m] camera->world, pairs [(2k, 2k+1)])"""
    angles = [a for ab in angles_ab for a in ab]
    seq = synth.make_sequence(len(angles), w, h, angles=angles)
    poses = [(seq["R"][i].T, -seq["R"][i].T @ seq["t"][i]) for i in range(len(angles))]
    return seq["images"], seq["K"], poses, [(2 * k, 2 * k + 1) for k in range(len(angles_ab))]


def _device_views(ctx, images, K, poses, pairs, **sp):
    """per pair: (rect, device disp16 on the host, left image, right image); the host library's rectification, as fuse uses"""
    h, w = images.shape[1:]
    st = ctx.stereo(w, h, **sp)
    out = []
    for a, b in pairs:
        r = pipe.stereo_rectify(K, poses[a], poses[b], w, h)
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        out.append((r, st.disparity(il, ir, r["H_l"], r["H_r"]), il, ir))
    st.close()
    return out


@pytest.fixture(scope="module")
def ring4(ctx):
    images, K, poses, pairs = _ring([(0.0, 3.0), (90.0, 93.0), (180.0, 183.0), (270.0, 273.0)], 320, 240)
    views = _device_views(ctx, images, K, poses, pairs, num_disparities=64)
    vol = dict(origin=(-0.13, -0.13, -0.13), voxel=0.004, dims=(66, 66, 66))
    ref = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], [(r, d) for r, d, _, _ in views])
    return dict(images=images, K=K, poses=poses, pairs=pairs, views=views, vol=vol, ref=ref)


def _check(fu, ref, what):
    s, c = fu.read()
    H.assert_bits_equal(s, ref["sum"], what + ": sum")
    assert (c == ref["count"]).all(), what + ": count"
    v, f = fu.extract()
    H.assert_bits_equal(v, ref["verts"], what + ": verts")
    assert f.shape == ref["faces"].shape and (f == ref["faces"]).all(), what + ": faces"


def test_sphere_bit_equal(ctx):
    views = sphere_views(**SPHERE)
    ref = FR.fuse(VOL["origin"], VOL["voxel"], VOL["dims"], views)
    fu = ctx.fusion(VOL["origin"], VOL["voxel"], VOL["dims"])
    for cam, d16 in views:
        fu.add_view(cam, d16)
    fu.integrate()
    _check(fu, ref, "sphere")
    assert len(ref["faces"]) > 10000
    fu.close()


def test_ring_pairs_bit_equal(ctx, ring4):
    ref = ring4["ref"]
    assert (ref["count"] > 0).mean() > 0.05 and len(ref["faces"]) > 1000
    fu = ctx.fusion(**ring4["vol"])
    for r, d16, _, _ in ring4["views"]:
        fu.add_view(r, d16)
    _check(fu, ref, "ring pairs")
    fu.close()


def _bytes(fu):
    s, c = fu.read()
    v, f = fu.extract()
    return s.tobytes() + c.tobytes() + v.tobytes() + f.tobytes()


def test_feeding_paths_same_bytes(ctx, ring4):
    import torch
    vol, views = ring4["vol"], ring4["views"]
    h, w = views[0][1].shape
    fu = ctx.fusion(**vol)
    for r, d16, _, _ in views:  # one view per launch
        fu.add_view(r, d16)
        fu.integrate()
    one = _bytes(fu)
    fu.reset()
    for r, d16, _, _ in views:  # batched, host maps
        fu.add_view(r, d16)
    fu.integrate()
    batched = _bytes(fu)
    fu.reset()
    dev = [torch.from_numpy(np.ascontiguousarray(d16)).to("cuda:0") for _, d16, _, _ in views]
    torch.cuda.synchronize()
    for (r, _, _, _), t in zip(views, dev):  # device maps
        fu.add_view(r, t.data_ptr(), shape=(h, w))
    devb = _bytes(fu)
    fu.reset()
    st = ctx.stereo(w, h, num_disparities=64)
    for r, _, il, ir in views:  # the stereo object's own device map
        st.disparity(il, ir, r["H_l"], r["H_r"])
        fu.add_stereo_view(r, st)
    stv = _bytes(fu)
    st.close()
    fu2 = ctx.fusion(**vol, max_views=1)  # a full stack integrates before it takes the next view
    for r, d16, _, _ in views:
        fu2.add_view(r, d16)
    small_stack = _bytes(fu2)
    fu.close()
    fu2.close()
    ref = ring4["ref"]
    want = ref["sum"].tobytes() + ref["count"].tobytes() + ref["verts"].tobytes() + ref["faces"].tobytes()
    assert one == batched == devb == stv == small_stack == want


def test_host_fuse_matches(ctx, ring4):
    vol = ring4["vol"]
    m = pipe.fuse(ctx, ring4["images"], ring4["K"], ring4["poses"], ring4["pairs"], vol["origin"], vol["voxel"], vol["dims"],
                  num_disparities=64)
    assert m["views"] == 4 and m["warn"] is None
    H.assert_bits_equal(m["verts"], ring4["ref"]["verts"], "fuse verts")
    assert (m["faces"] == ring4["ref"]["faces"]).all()
    bad = pipe.fuse(ctx, ring4["images"], ring4["K"], ring4["poses"], [(0, 1), (0, 9), (2, 2)], vol["origin"], vol["voxel"],
                    vol["dims"], num_disparities=64)
    assert bad["views"] == 1
    assert bad["warn"] == ("WARN: fusion pair (0, 9) skipped (out of range, images=8)\n"
                           "WARN: fusion pair (2, 2) skipped (zero baseline)\n")


def test_degenerate_pair_warning(ctx, ring4):
    """two cameras looking along their own baseline: rectification has no y axis; the WARN names that, not the baseline"""
    vol = ring4["vol"]
    images = np.concatenate([ring4["images"], ring4["images"][:2]])
    poses = list(ring4["poses"]) + [(np.eye(3), np.array([0.0, 0.0, -0.65])), (np.eye(3), np.array([0.0, 0.0, -0.5]))]
    m = pipe.fuse(ctx, images, ring4["K"], poses, [(8, 9), (0, 1)], vol["origin"], vol["voxel"], vol["dims"], num_disparities=64)
    assert m["views"] == 1
    assert m["warn"] == "WARN: fusion pair (8, 9) skipped (degenerate rectification)\n"


def test_edge_cases(ctx, ring4):
    vol, views = ring4["vol"], ring4["views"]
    fu = ctx.fusion(**vol)
    assert fu.counts() == (0, 0)  # no views
    v, f = fu.extract()
    assert v.shape == (0, 3) and f.shape == (0, 3)
    s, c = fu.read()
    assert not s.any() and not c.any()
    # a view that misses the volume: the camera looks away from it
    r0, d0 = views[0][0], views[0][1]
    away = dict(r0, R_rw=-np.asarray(r0["R_rw"]))
    fu.add_view(away, d0)
    s, c = fu.read()
    assert not c.any() and fu.counts() == (0, 0)
    # caps: too small -> INVALID with the counts set, then exact caps
    for r, d16, _, _ in views:
        fu.add_view(r, d16)
    nv, nf = fu.counts()
    assert (nv, nf) == (len(ring4["ref"]["verts"]), len(ring4["ref"]["faces"]))
    for vc, fc in ((nv - 1, nf), (nv, nf - 1)):
        rc, _, _, n1, n2 = fu.extract_into(vc, fc)
        assert rc == capi.SFMX_ERR_INVALID and (n1, n2) == (nv, nf)
    rc, vv, ff, _, _ = fu.extract_into(nv, nf)
    assert rc == capi.SFMX_OK
    H.assert_bits_equal(vv, ring4["ref"]["verts"], "exact caps")
    assert (ff == ring4["ref"]["faces"]).all()
    # reset: back to zero, and the same views again give the same bytes
    fu.reset()
    s, c = fu.read()
    assert not s.any() and not c.any()
    for r, d16, _, _ in views:
        fu.add_view(r, d16)
    _check(fu, ring4["ref"], "after reset")
    fu.close()
    # min_weight > 1
    ref = FR.extract(ring4["ref"]["sum"], ring4["ref"]["count"], vol["origin"], vol["voxel"], min_weight=2)
    fu = ctx.fusion(**vol, min_weight=2)
    for r, d16, _, _ in views:
        fu.add_view(r, d16)
    v, f = fu.extract()
    H.assert_bits_equal(v, ref[0], "min_weight 2")
    assert (f == ref[1]).all() and len(f) < len(ring4["ref"]["faces"])
    fu.close()
    # 2 x 2 x 2 around the sphere's surface point (0, 0, -0.1)
    views = sphere_views(**SPHERE)
    tiny = dict(origin=(-0.001, -0.001, -0.1013), voxel=0.002, dims=(2, 2, 2))
    ref = FR.fuse(tiny["origin"], tiny["voxel"], tiny["dims"], views)
    fu = ctx.fusion(**tiny)
    for cam, d16 in views:
        fu.add_view(cam, d16)
    _check(fu, ref, "2x2x2")
    assert len(ref["faces"]) > 0
    fu.close()
    with pytest.raises(capi.SfmxError):
        ctx.fusion(origin=(0, 0, 0), voxel=0.0, dims=(4, 4, 4))


def test_whole_ring(ctx):
    """36 pairs (10k, 10k + 3 degrees), VGA / D 128, ground-truth poses, [-0.13, 0.13]^3 at 2 mm, min_weight 6.
    Thresholds calibrated on the NumPy restatement before any GPU run."""
    images, K, poses, pairs = _ring([(10.0 * k, 10.0 * k + 3.0) for k in range(36)], 640, 480)
    vol = RING_VOL
    m = pipe.fuse(ctx, images, K, poses, pairs, vol["origin"], vol["voxel"], vol["dims"], min_weight=6)
    assert m["views"] == 36 and m["warn"] is None
    v, F = m["verts"], m["faces"]
    r = np.linalg.norm(v, axis=1)
    assert ((r >= 0.065) & (r <= 0.105)).mean() >= 0.95
    band = np.abs(v[:, 1]) < 0.04
    lon = np.degrees(np.arctan2(v[band, 0], -v[band, 2])) % 360
    assert (np.bincount((lon // 10).astype(int), minlength=36) > 0).all(), "every 10 degree longitude bin"
    n = np.cross(v[F[:, 1]] - v[F[:, 0]], v[F[:, 2]] - v[F[:, 0]])
    assert ((n * v[F].mean(1)).sum(1) > 0).mean() >= 0.95
    views = _device_views(ctx, images, K, poses, pairs)
    ref = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], [(rr, d) for rr, d, _, _ in views], min_weight=6)
    H.assert_bits_equal(v, ref["verts"], "whole ring verts")
    assert (F == ref["faces"]).all()


def _fixture():
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    return g, cfg, [str(s) for s in g["names"]]


def test_pipeline_fusion(ctx, tmp_path):
    g, cfg, names = _fixture()
    plain, fused = str(tmp_path / "plain"), str(tmp_path / "fused")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain)
    fa, fb = (int(r0["kf_frames"][k]) for k in PAIR)
    sm = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][PAIR[0]], r0["kf_poses"][PAIR[1]], **SMALL)
    assert len(sm["verts"]) > 0
    lo, hi = sm["verts"].min(0), sm["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)  # the box is ~7x deeper than wide (the run's diverged scale): size by the short side
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    fz = dict(pairs=[PAIR], origin=tuple(lo), voxel=voxel, dims=dims, **SMALL)
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, fused, fusion=fz)
    for fn in FILES:
        assert open(os.path.join(plain, fn)).read() == open(os.path.join(fused, fn)).read(), fn
    assert r0["log"].replace(plain, "X") == r1["log"].replace(fused, "X")
    assert (r0["centres"] == r1["centres"]).all() and (r0["kf_poses"] == r1["kf_poses"]).all()
    assert sorted(os.listdir(fused)) == sorted(os.listdir(plain) + ["templeRing_mesh_fused.ply"])
    m = r1["fused_mesh"]
    assert m["views"] == 1 and len(m["faces"]) > 0
    frames = [int(f) for f in r1["kf_frames"]]
    ref = pipe.fuse(ctx, g["images"][frames], g["K"], r1["kf_poses"], [PAIR], tuple(lo), voxel, dims, **SMALL)
    H.assert_bits_equal(m["verts"], ref["verts"], "pipeline fused mesh")
    assert (m["faces"] == ref["faces"]).all()
    head = open(os.path.join(fused, "templeRing_mesh_fused.ply")).read().split("end_header\n")[0]
    assert f"element vertex {len(m['verts'])}\n" in head and f"element face {len(m['faces'])}\n" in head
