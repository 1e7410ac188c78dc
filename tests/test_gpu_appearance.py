"""GPU suite: appearance of the fused surface.  sfmx_fusion_extract_normals gives sfmx_fusion_extract's vertices and faces
byte for byte plus normals, and sfmx_shade_* gives vertex grey and view counts, all bit for bit against the NumPy restatement
(tests/appearance_ref.py): analytic sphere scenes, real ring pairs through the stereo kernels with every way of feeding views,
host vertices against the device-resident ones, the parameter and shape ranges, pipeline.fuse / pipeline.run with the PLY
file, and the whole ring."""
import importlib
import json
import os

import numpy as np
import pytest

import appearance_ref as AR
import fusion_ref as FR
import helpers as H
import range_inputs as RI
from test_fusion_cpu import SPHERE, VOL

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
PAIR = (2, 3)  # e2e_keyframes: the pair with valid disparity
SMALL = dict(num_disparities=32, census=5)
RING_VOL = dict(origin=(-0.13, -0.13, -0.13), voxel=0.002, dims=(131, 131, 131))
# whole ring, measured on the NumPy side: share of vertices some view sees, share of normals that point away
# from the origin; the floors are 5 points below
RING_SEEN, RING_OUTWARD = 0.9902, 0.9744


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _ref(vol, views, **kw):
    with np.errstate(divide="ignore"):
        return AR.fuse(vol["origin"], vol["voxel"], vol["dims"], views, **kw)


def _feed(fu, sh, views):
    for cam, d16, img in views:
        fu.add_view(cam, d16)
        sh.add_view(cam, d16, img)


def _check(fu, sh, ref, what, depth_tol, **shade_kw):
    """every output of the two stages against the reference; returns the device arrays"""
    v0, f0 = fu.extract()
    v, f, n = fu.extract_normals()
    assert v.tobytes() == v0.tobytes() and f.tobytes() == f0.tobytes(), what + ": extract_normals changes verts / faces"
    H.assert_bits_equal(v, ref["verts"], what + ": verts")
    assert f.shape == ref["faces"].shape and (f == ref["faces"]).all(), what + ": faces"
    assert n.shape == ref["normals"].shape
    H.assert_bits_equal(n, ref["normals"], what + ": normals")
    g, c = sh.shade_fusion(fu, len(v), depth_tol, **shade_kw)
    assert g.dtype == np.uint8 and c.dtype == np.int32
    assert (c == ref["vertex_views"]).all(), what + ": views"
    assert (g == ref["grey"]).all(), what + ": grey"
    g2, c2 = sh.shade(v, n, depth_tol, **shade_kw)
    assert g2.tobytes() == g.tobytes() and c2.tobytes() == c.tobytes(), what + ": host vertices vs resident"
    return v, f, n, g, c


def _case(ctx, vol, views, what, depth_tol=None, shade_kw=None, **params):
    shade_kw = dict(shade_kw or {})
    ref_kw = {k: v for k, v in params.items() if k != "max_views"}
    ref = _ref(vol, views, depth_tol=depth_tol, **ref_kw, **shade_kw)
    tol = FR.resolve(vol["voxel"], params.get("trunc", 0.0)) if depth_tol is None else depth_tol
    fu, sh = ctx.fusion(**vol, **params), ctx.shade()
    _feed(fu, sh, views)
    assert sh.view_count() == len(views)
    _check(fu, sh, ref, what, tol, disp_min=params.get("disp_min", 1.0), **shade_kw)
    fu.close()
    sh.close()
    return ref


def _with_images(views, seed=7):
    rng = np.random.default_rng(seed)
    return [(cam, d16, rng.integers(0, 256, d16.shape, dtype=np.uint8)) for cam, d16 in views]


# ---- analytic scenes -------------------------------------------------------------------------------------------------------
def test_sphere_bit_equal(ctx):
    views = AR.textured_sphere_views(**SPHERE)
    ref = _case(ctx, VOL, views, "sphere")
    assert len(ref["verts"]) == 22786 and (ref["vertex_views"] >= 1).all()
    for tol, cull in ((1.0, 0), (1.0, 1)):
        _case(ctx, VOL, views, f"sphere tol {tol} cull {cull}", depth_tol=tol, shade_kw=dict(cull=cull))


def test_two_spheres_bit_equal(ctx):
    views = AR.two_sphere_views()
    ref = _case(ctx, AR.TWO_VOL, views, "two spheres")
    A, B = AR.two_sphere_labels(ref["verts"])
    assert (ref["grey"][A] == 80).all() and (ref["grey"][B] == 200).all() and (ref["vertex_views"] >= 1).all()
    ref1 = _case(ctx, AR.TWO_VOL, views, "two spheres, tolerance 1.0", depth_tol=1.0)
    assert (ref1["grey"][A] != 80).any() and (ref1["grey"][B] != 200).any()


# ---- ring pairs through the stereo kernels ---------------------------------------------------------------------------------
def _ring(angles_ab, w, h):
    """frames at the given (a, b) ring angles: (images [2m][h][w], K, poses [2m] camera->world, pairs [(2k, 2k+1)])"""
    angles = [a for ab in angles_ab for a in ab]
    seq = synth.make_sequence(len(angles), w, h, angles=angles)
    poses = [(seq["R"][i].T, -seq["R"][i].T @ seq["t"][i]) for i in range(len(angles))]
    return seq["images"], seq["K"], poses, [(2 * k, 2 * k + 1) for k in range(len(angles_ab))]


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
def ring4(ctx):
    images, K, poses, pairs = _ring([(0.0, 3.0), (90.0, 93.0), (180.0, 183.0), (270.0, 273.0)], 320, 240)
    views = _device_views(ctx, images, K, poses, pairs, num_disparities=64)
    vol = dict(origin=(-0.13, -0.13, -0.13), voxel=0.004, dims=(66, 66, 66))
    ref = _ref(vol, [(r, d, im) for r, d, im, _, _ in views])
    return dict(images=images, K=K, poses=poses, pairs=pairs, views=views, vol=vol, ref=ref)


def _bytes(fu, sh, tol):
    v, f, n = fu.extract_normals()
    g, c = sh.shade_fusion(fu, len(v), tol)
    return v.tobytes() + f.tobytes() + n.tobytes() + g.tobytes() + c.tobytes()


def test_feeding_paths_same_bytes(ctx, ring4):
    import torch
    vol, views, ref = ring4["vol"], ring4["views"], ring4["ref"]
    assert len(ref["faces"]) > 1000 and (ref["vertex_views"] >= 1).mean() > 0.5
    tol = FR.resolve(vol["voxel"])
    want = (ref["verts"].tobytes() + ref["faces"].tobytes() + ref["normals"].tobytes() + ref["grey"].tobytes()
            + ref["vertex_views"].tobytes())
    h, w = views[0][1].shape
    fu, sh = ctx.fusion(**vol), ctx.shade()
    for r, d16, im, _, _ in views:  # host maps
        fu.add_view(r, d16)
        sh.add_view(r, d16, im)
    host = _bytes(fu, sh, tol)
    fu.reset()
    sh.reset()
    assert sh.view_count() == 0
    dev = [(torch.from_numpy(np.ascontiguousarray(d16)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(im)).to("cuda:0"))
           for _, d16, im, _, _ in views]
    torch.cuda.synchronize()
    for (r, _, _, _, _), (td, ti) in zip(views, dev):  # device maps, into the same objects after reset
        fu.add_view(r, td.data_ptr(), shape=(h, w))
        sh.add_view(r, td.data_ptr(), ti.data_ptr(), shape=(h, w))
    devb = _bytes(fu, sh, tol)
    fu.reset()
    sh.reset()
    st = ctx.stereo(w, h, num_disparities=64)
    for r, _, _, il, ir in views:  # the stereo object's own device map and rectified image
        st.disparity(il, ir, r["H_l"], r["H_r"])
        fu.add_stereo_view(r, st)
        sh.add_stereo_view(r, st)
    stv = _bytes(fu, sh, tol)
    st.close()
    fu.close()
    sh.close()
    assert host == want, "host maps"
    assert devb == want, "device maps after reset"
    assert stv == want, "add_stereo_view after reset"


def test_resident_surface_rules(ctx, ring4):
    """shade_fusion needs the surface of the last extract_normals; a plain extract or a changed volume invalidates it"""
    vol, views = ring4["vol"], ring4["views"]
    fu, sh = ctx.fusion(**vol), ctx.shade()
    _feed(fu, sh, [(r, d, im) for r, d, im, _, _ in views])
    with pytest.raises(capi.SfmxError):
        sh.shade_fusion(fu, 1, 0.016)  # nothing extracted yet
    v, f, n = fu.extract_normals()
    g, c = sh.shade_fusion(fu, len(v), 0.016)
    assert (g == ring4["ref"]["grey"]).all()
    fu.extract()
    with pytest.raises(capi.SfmxError):
        sh.shade_fusion(fu, len(v), 0.016)
    fu.extract_normals()
    fu.add_view(views[0][0], views[0][1])
    fu.integrate()
    with pytest.raises(capi.SfmxError):
        sh.shade_fusion(fu, len(v), 0.016)
    with pytest.raises(capi.SfmxError):
        sh.shade(v, None, 0.016)  # cull needs normals
    with pytest.raises(capi.SfmxError):
        sh.shade(v, n, 0.0)  # depth_tol has no default
    fu.close()
    sh.close()


# ---- ranges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RI.BLOCK_SHAPES))
def test_volume_shapes_at_block_boundaries(ctx, name):
    vol, views, trunc = RI.shape_case(*RI.BLOCK_SHAPES[name])
    ref = _case(ctx, vol, _with_images(views), name, trunc=trunc)
    assert len(ref["faces"]) > 500


def test_volume_shape_past_scan_level_boundary(ctx):
    """1 024^2 grid points and one slice more: over a million vertices, normals and grey for each"""
    vol, views, trunc = RI.shape_case(*RI.BIG_SHAPES["s128x128x65"])
    ref = _case(ctx, vol, _with_images(views), "s128x128x65", trunc=trunc, depth_tol=0.002)
    assert len(ref["verts"]) > 10 ** 6 and (ref["vertex_views"] > 0).any() and (ref["vertex_views"] == 0).any()


def test_device_vertices(ctx, ring4):
    """sfmx_shade_vertices on vertices and normals that are already on the device (not the fusion object's own)"""
    import torch
    ref = ring4["ref"]
    sh = ctx.shade()
    for r, d16, im, _, _ in ring4["views"]:
        sh.add_view(r, d16, im)
    tv = torch.from_numpy(np.ascontiguousarray(ref["verts"])).to("cuda:0")
    tn = torch.from_numpy(np.ascontiguousarray(ref["normals"])).to("cuda:0")
    torch.cuda.synchronize()
    g, c = sh.shade(tv.data_ptr(), tn.data_ptr(), 0.016, n=len(ref["verts"]))
    assert (g == ref["grey"]).all() and (c == ref["vertex_views"]).all()
    views = [(r, d, im) for r, d, im, _, _ in ring4["views"]]
    g0, c0 = AR.shade(ref["verts"], None, views, 0.016, cull=0, fill=5)
    g, c = sh.shade(tv.data_ptr(), None, 0.016, n=len(ref["verts"]), cull=0, fill=5)
    assert (g == g0).all() and (c == c0).all()
    sh.close()


def test_views_of_different_sizes(ctx):
    """40 x 30, 640 x 480, 320 x 240 in one object and the reverse: the slabs regrown with earlier views in them"""
    for views in (RI.mixed_size_views(), RI.mixed_size_views()[::-1]):
        ref = _case(ctx, RI.SLAB_VOL, _with_images(views), "mixed sizes", trunc=RI.SLAB_TRUNC, depth_tol=0.01, shade_kw=dict(cull=0))
        assert len(ref["faces"]) > 10000 and (ref["vertex_views"] > 0).any()


def test_cameras_inside_behind_and_beside(ctx):
    views = _with_images([RI.slab_view(**RI.SLAB_VOL, seed=1), RI.inside_view(), RI.away_view(), RI.border_view()])
    for cull in (0, 1):
        ref = _case(ctx, RI.SLAB_VOL, views, f"special cameras, cull {cull}", trunc=RI.SLAB_TRUNC, depth_tol=0.01,
                    shade_kw=dict(cull=cull, fill=200))
        assert (ref["vertex_views"] == 0).any() and (ref["vertex_views"] > 0).any()
        assert (ref["grey"][ref["vertex_views"] == 0] == 200).all()


@pytest.mark.parametrize("disp_min", [-5.0, 0.0, 40.0])
def test_disp_min(ctx, disp_min):
    """disp_min <= 0 lets disparities of 0 (Z = +inf) and below through to the depth test, which rejects them"""
    views = _with_images(RI.slab_views3(extra=(-1, -32768, 32767)))
    _case(ctx, RI.SLAB_VOL, views, f"disp_min {disp_min}", trunc=RI.SLAB_TRUNC, disp_min=disp_min, depth_tol=0.02,
          shade_kw=dict(cull=0, fill=255))


@pytest.mark.parametrize("min_weight", [2, 3, 4])
def test_min_weight_takes_every_gradient_branch(ctx, min_weight):
    """undefined grid points next to the surface: one-sided differences on a real surface (4 = no surface at all).
    Counted in NumPy: the central, forward-only and backward-only branches are all taken.  The fourth branch (no defined
    neighbour, G = 0) cannot be reached from a vertex: both ends of its edge are corners of a meshed cell, whose 8 corners are
    all defined, so each end has a defined neighbour along every axis; the CPU suite covers it on a hand-set
    volume."""
    views = _with_images(RI.slab_views3())
    ref = _case(ctx, RI.SLAB_VOL, views, f"min_weight {min_weight}", trunc=RI.SLAB_TRUNC, min_weight=min_weight, depth_tol=0.01)
    if min_weight == 4:
        assert len(ref["verts"]) == 0
        return
    _, br = AR.normals(ref["sum"], ref["count"], min_weight, with_branches=True)
    counts = np.bincount(br.ravel(), minlength=4)
    assert counts[0] == 0 and (counts[1:] > 1000).all(), counts


def test_empty_inputs(ctx):
    """0 views, 0 vertices, an empty surface: counts 0, SFMX_OK, nothing launched"""
    views = _with_images(RI.slab_views3())
    fu, sh = ctx.fusion(**RI.SLAB_VOL, trunc=RI.SLAB_TRUNC), ctx.shade()
    v, f, n = fu.extract_normals()  # empty volume
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    g, c = sh.shade_fusion(fu, 0, 0.01)
    assert g.shape == (0,) and c.shape == (0,)
    g, c = sh.shade(np.zeros((0, 3)), np.zeros((0, 3)), 0.01)
    assert g.shape == (0,) and c.shape == (0,)
    for cam, d16, _ in views:
        fu.add_view(cam, d16)
    v, f, n = fu.extract_normals()
    assert len(v) > 1000
    g, c = sh.shade_fusion(fu, len(v), 0.01, fill=17)  # vertices, but no views
    assert (g == 17).all() and (c == 0).all()
    g, c = sh.shade(v, None, 0.01, cull=0, fill=18)
    assert (g == 18).all() and (c == 0).all()
    fu.close()
    sh.close()


# ---- pipeline --------------------------------------------------------------------------------------------------------------
def _ply_plain(verts, faces):
    """the file write_mesh_ply writes (default stream formatting of a double is %g)"""
    head = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces)))
    return head + "".join("%g %g %g\n" % tuple(p) for p in verts) + "".join("3 %d %d %d\n" % tuple(t) for t in faces)


def _check_ply(path, m):
    text = open(path).read()
    head, body = text.split("end_header\n")
    assert head == ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                    "property float nx\nproperty float ny\nproperty float nz\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                    "element face %d\nproperty list uchar int vertex_indices\n" % (len(m["verts"]), len(m["faces"])))
    lines = body.splitlines()
    nv = len(m["verts"])
    assert len(lines) == nv + len(m["faces"])
    for i in (0, nv // 2, nv - 1):
        assert lines[i].startswith("%g %g %g " % tuple(m["verts"][i])), "x y z as write_mesh_ply prints them"
    vals = np.array([ln.split() for ln in lines[:nv]], dtype=object)
    assert vals.shape == (nv, 9)
    nrm = vals[:, 3:6].astype(np.float64)
    assert (nrm.astype(np.float32) == m["normals"].astype(np.float32)).all(), "normals to float32 rounding"
    rgb = vals[:, 6:9].astype(np.int64)
    assert (rgb == m["grey"][:, None]).all()
    F = np.array([ln.split() for ln in lines[nv:]], dtype=np.int64)
    assert (F[:, 0] == 3).all() and (F[:, 1:] == m["faces"]).all()


def test_host_fuse_appearance(ctx, ring4, tmp_path):
    vol, ref = ring4["vol"], ring4["ref"]
    args = (ctx, ring4["images"], ring4["K"], ring4["poses"], ring4["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    plain_ply, app_ply = str(tmp_path / "plain.ply"), str(tmp_path / "app.ply")
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=plain_ply)
    assert set(m0) == {"verts", "faces", "views", "warn"}
    assert open(plain_ply).read() == _ply_plain(m0["verts"], m0["faces"]), "without appearance the file is what it was"
    m = pipe.fuse(*args, num_disparities=64, ply_path=app_ply, appearance=True)
    assert m["views"] == 4 and m["warn"] is None
    assert m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes()
    H.assert_bits_equal(m["normals"], ref["normals"], "fuse normals")
    assert (m["grey"] == ref["grey"]).all() and (m["vertex_views"] == ref["vertex_views"]).all()
    assert m["grey"].dtype == np.uint8 and m["vertex_views"].dtype == np.int32
    _check_ply(app_ply, m)
    views = [(r, d, im) for r, d, im, _, _ in ring4["views"]]
    m2 = pipe.fuse(*args, num_disparities=64, appearance=dict(depth_tol=1.0, cull=0, fill=9))
    g, c = AR.shade(ref["verts"], ref["normals"], views, 1.0, cull=0, fill=9)
    assert (m2["grey"] == g).all() and (m2["vertex_views"] == c).all()
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, appearance=dict(colour=1))
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, appearance=True)
    assert empty["verts"].shape == (0, 3) and empty["normals"].shape == (0, 3) and empty["grey"].shape == (0,)


def test_pipeline_fusion_appearance(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    plain, fused = str(tmp_path / "plain"), str(tmp_path / "fused")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in PAIR)
    sm = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][PAIR[0]], r0["kf_poses"][PAIR[1]], **SMALL)
    lo, hi = sm["verts"].min(0), sm["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    fz = dict(pairs=[PAIR], origin=tuple(lo), voxel=voxel, dims=dims, **SMALL)
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain, fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, fused, fusion=dict(fz, appearance=True))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(fused, "X")
    assert sorted(os.listdir(fused)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m1) == {"verts", "faces", "views", "warn"}
    assert open(os.path.join(plain, "templeRing_mesh_fused.ply")).read() == _ply_plain(m1["verts"], m1["faces"])
    assert m["views"] == 1 and len(m["faces"]) > 0
    assert m["verts"].tobytes() == m1["verts"].tobytes() and m["faces"].tobytes() == m1["faces"].tobytes()
    # the NumPy side: the same pair through the stereo kernels, then the restatement
    h, w = g["images"].shape[1:]
    rect = pipe.stereo_rectify(g["K"], r2["kf_poses"][PAIR[0]], r2["kf_poses"][PAIR[1]], w, h)
    il, ir = (g["images"][fb], g["images"][fa]) if rect["swapped"] else (g["images"][fa], g["images"][fb])
    st = ctx.stereo(w, h, **SMALL)
    d = st.disparity(il, ir, rect["H_l"], rect["H_r"], want_rect=True)
    st.close()
    ref = _ref(dict(origin=tuple(lo), voxel=voxel, dims=dims), [(rect, d["disp16"], d["rect"][0])])
    H.assert_bits_equal(m["verts"], ref["verts"], "pipeline verts")
    H.assert_bits_equal(m["normals"], ref["normals"], "pipeline normals")
    assert (m["grey"] == ref["grey"]).all() and (m["vertex_views"] == ref["vertex_views"]).all()
    _check_ply(os.path.join(fused, "templeRing_mesh_fused.ply"), m)


# ---- the whole ring --------------------------------------------------------------------------------------------------------
def test_whole_ring(ctx):
    """36 pairs (10k, 10k + 3 degrees), VGA / D 128, [-0.13, 0.13]^3 at 2 mm, min_weight 6, as test_gpu_fusion's whole ring.
    The device equals NumPy exactly; the floors are the NumPy values of DESIGN.md 14 minus 5 points."""
    images, K, poses, pairs = _ring([(10.0 * k, 10.0 * k + 3.0) for k in range(36)], 640, 480)
    vol = RING_VOL
    m = pipe.fuse(ctx, images, K, poses, pairs, vol["origin"], vol["voxel"], vol["dims"], min_weight=6, appearance=True)
    assert m["views"] == 36 and m["warn"] is None
    views = _device_views(ctx, images, K, poses, pairs)
    ref = _ref(vol, [(r, d, im) for r, d, im, _, _ in views], min_weight=6)
    seen = float((ref["vertex_views"] >= 1).mean())
    outward = float(((ref["normals"] * ref["verts"]).sum(1) > 0).mean())
    print("whole ring: vertices %d, views >= 1: %.4f, n . X > 0: %.4f, zero normals %d, views mean %.2f max %d"
          % (len(ref["verts"]), seen, outward, int((np.linalg.norm(ref["normals"], axis=1) == 0).sum()),
             ref["vertex_views"].mean(), ref["vertex_views"].max()))
    H.assert_bits_equal(m["verts"], ref["verts"], "whole ring verts")
    assert (m["faces"] == ref["faces"]).all()
    H.assert_bits_equal(m["normals"], ref["normals"], "whole ring normals")
    assert (m["grey"] == ref["grey"]).all() and (m["vertex_views"] == ref["vertex_views"]).all()
    assert float((m["vertex_views"] >= 1).mean()) >= RING_SEEN - 0.05
    assert float(((m["normals"] * m["verts"]).sum(1) > 0).mean()) >= RING_OUTWARD - 0.05
