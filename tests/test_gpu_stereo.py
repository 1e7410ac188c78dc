"""GPU suite: keyframe-pair stereo.  Device rectification and disparity bit for bit against the NumPy restatement
(tests/stereo_ref.py) stage by stage, host vs device-resident inputs, the geometry of a synthetic ring pair, and the stereo
request of the pipeline (sfmx_pipeline_run_ex) with every pre-existing output unchanged."""
import importlib
import json
import os

import numpy as np
import pytest

import helpers as H
import stereo_ref as SR

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
FILES = ("keyframes_camera_centers.csv", "posegraph_edges.csv", "templeRing_sparse_points.ply")
# e2e_keyframes (10 frames, 160x120): the pair and disparity range of the pipeline cases.  The run's keyframes 0 and 1
# rectify to views with no valid disparity at any D (the NumPy restatement agrees on the run's poses); keyframes 2 and 3
# give 328 vertices and 406 faces at D = 32.
PAIR = (2, 3)
SMALL = dict(num_disparities=32, census=5)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _cw(seq, i):
    R, t = seq["R"][i], seq["t"][i]
    return R.T, -R.T @ t


def _pair(w, h, fa=0, fb=10):
    """frames fa, fb of the default synthetic ring (0.3 deg per frame): (left, right, rect) in rectified order"""
    seq = synth.make_sequence(max(fa, fb) + 1, w, h, 0.3)
    A, B = _cw(seq, fa), _cw(seq, fb)
    rect = SR.rectify(seq["K"], *A, *B)
    il, ir = (seq["images"][fb], seq["images"][fa]) if rect["swapped"] else (seq["images"][fa], seq["images"][fb])
    return seq, il, ir, rect


@pytest.fixture(scope="module")
def vga():
    seq, il, ir, rect = _pair(640, 480)
    p = SR.DEFAULTS
    rl, vl = SR.remap(il, rect["H_l"])
    rr, vr = SR.remap(ir, rect["H_r"])
    cl, cr = SR.census(rl, vl, p["census"]), SR.census(rr, vr, p["census"])
    S = SR.aggregate(SR.cost_volume(cl, cr, p["num_disparities"], p["census"] ** 2 - 1), p["p1"], p["p2"])
    return dict(seq=seq, il=il, ir=ir, rect=rect, rl=rl, rr=rr, cl=cl, S=S)


def _ref_select(v, **kw):
    p = {**SR.DEFAULTS, **kw}
    d = SR.select(v["S"], v["cl"], p["uniqueness"], p["lr_max_diff"])
    return SR.speckle(d, p["speckle_window"], p["speckle_range"])


def _mismatch(a, b):
    bad = np.argwhere(a != b)
    return f"{len(bad)} pixels differ, first at {bad[:3].tolist()}"


def test_rectified_images_bit_equal(ctx, vga):
    st = ctx.stereo(640, 480)
    out = st.disparity(vga["il"], vga["ir"], vga["rect"]["H_l"], vga["rect"]["H_r"], want_rect=True)
    assert (out["rect"][0] == vga["rl"]).all(), _mismatch(out["rect"][0], vga["rl"])
    assert (out["rect"][1] == vga["rr"]).all(), _mismatch(out["rect"][1], vga["rr"])
    st.close()


def test_disparity_small_bit_equal_with_sums(ctx):
    seq, il, ir, rect = _pair(160, 120)
    ref = SR.disparity(il, ir, rect["H_l"], rect["H_r"], SMALL, want=True)
    st = ctx.stereo(160, 120, **SMALL)
    out = st.disparity(il, ir, rect["H_l"], rect["H_r"], want_rect=True, want_sum=True)
    assert (out["rect"] == ref["rect"]).all()
    assert (out["S"] == ref["S"]).all(), _mismatch(out["S"], ref["S"])
    assert (out["disp16"] == ref["disp16"]).all(), _mismatch(out["disp16"], ref["disp16"])
    assert (ref["disp16"] != -16).mean() > 0.2
    st.close()


@pytest.mark.parametrize("off", [None, "uniqueness", "lr_max_diff", "speckle_window"])
def test_disparity_vga_bit_equal(ctx, vga, off):
    """defaults, then each filter off in turn, so that a mismatch names its stage"""
    kw = {} if off is None else {off: (-1 if off == "lr_max_diff" else 0)}
    st = ctx.stereo(640, 480, **kw)
    out = st.disparity(vga["il"], vga["ir"], vga["rect"]["H_l"], vga["rect"]["H_r"], want_sum=off is None)
    ref = _ref_select(vga, **kw)
    if off is None:
        assert (out["S"] == vga["S"]).all(), "aggregation: " + _mismatch(out["S"], vga["S"])
        out = out["disp16"]
    assert (out == ref).all(), f"{off or 'defaults'}: " + _mismatch(out, ref)
    st.close()


def test_host_and_device_inputs_same_bytes(ctx, vga):
    import torch
    st = ctx.stereo(640, 480)
    a = st.disparity(vga["il"], vga["ir"], vga["rect"]["H_l"], vga["rect"]["H_r"])
    b = st.disparity(vga["il"], vga["ir"], vga["rect"]["H_l"], vga["rect"]["H_r"])
    dl = torch.from_numpy(np.ascontiguousarray(vga["il"])).to("cuda:0")
    dr = torch.from_numpy(np.ascontiguousarray(vga["ir"])).to("cuda:0")
    torch.cuda.synchronize()
    c = st.disparity(dl.data_ptr(), dr.data_ptr(), vga["rect"]["H_l"], vga["rect"]["H_r"])
    assert a.tobytes() == b.tobytes() == c.tobytes()
    st.close()


def test_ring_pair_geometry(ctx):
    """frames 0 and 10 of the ring (3 deg apart) with ground-truth poses: a dense mesh on the blob shell (radius 0.07-0.10)"""
    seq = synth.make_sequence(11, 640, 480, 0.3)
    m = pipe.stereo_mesh(ctx, seq["images"][0], seq["images"][10], seq["K"], _cw(seq, 0), _cw(seq, 10))
    assert m["warn"] is None
    v = m["verts"]
    r = np.linalg.norm(v, axis=1)
    assert len(v) >= 5000, len(v)
    assert ((r >= 0.065) & (r <= 0.105)).mean() >= 0.9
    ref_v, ref_f, _ = SR.grid_mesh(m["disp16"], m["rect"])
    H.assert_bits_equal(v, ref_v, "ring pair mesh")
    assert (m["faces"] == ref_f).all()


def _fixture():
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    return g, cfg, [str(s) for s in g["names"]]


def _same_outputs(a, b, log_a, log_b):
    for fn in FILES:
        assert open(os.path.join(a, fn)).read() == open(os.path.join(b, fn)).read(), fn
    assert log_a.replace(a, "X") == log_b.replace(b, "X")


@pytest.mark.parametrize("resident", [False, True])
def test_pipeline_stereo_pair(ctx, tmp_path, resident):
    g, cfg, names = _fixture()
    plain, ster = str(tmp_path / "plain"), str(tmp_path / "stereo")
    kw = {}
    if resident:
        import torch
        dev = torch.from_numpy(np.ascontiguousarray(g["images"])).to("cuda:0")
        torch.cuda.synchronize()
        kw = dict(images_dev=dev.data_ptr(), shape=tuple(dev.shape))
    imgs = None if resident else g["images"]
    r0 = pipe.run(ctx, imgs, names, g["K"], g["lat"], g["lon"], cfg, plain, **kw)
    r1 = pipe.run(ctx, imgs, names, g["K"], g["lat"], g["lon"], cfg, ster, stereo=dict(kf_pair=PAIR, **SMALL), **kw)
    _same_outputs(plain, ster, r0["log"], r1["log"])
    assert (r0["centres"] == r1["centres"]).all() and (r0["kf_poses"] == r1["kf_poses"]).all()
    assert (r1["kf_poses"][:, 9:] == r1["centres"]).all()
    ply = os.path.join(ster, f"templeRing_mesh_stereo_kf{PAIR[0]}_kf{PAIR[1]}.ply")
    assert os.path.exists(ply) and not os.path.exists(os.path.join(plain, os.path.basename(ply)))
    m = r1["stereo_mesh"]
    assert len(m["faces"]) > 0
    fa, fb = (int(r1["kf_frames"][k]) for k in PAIR)
    ref = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r1["kf_poses"][PAIR[0]], r1["kf_poses"][PAIR[1]], **SMALL)
    assert (m["disp16"] == ref["disp16"]).all()
    H.assert_bits_equal(m["verts"], ref["verts"], "pipeline stereo mesh")
    assert (m["faces"] == ref["faces"]).all()
    head = open(ply).read().split("end_header\n")[0]
    assert f"element vertex {len(m['verts'])}\n" in head and f"element face {len(m['faces'])}\n" in head


def test_pipeline_stereo_skip_path(ctx, tmp_path):
    """a disparity floor above every disparity: no file, one WARN line, everything else as without stereo"""
    g, cfg, names = _fixture()
    plain, ster = str(tmp_path / "plain"), str(tmp_path / "stereo")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain)
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, ster, stereo=dict(kf_pair=PAIR, disp_min=1e9, **SMALL))
    assert not os.path.exists(os.path.join(ster, f"templeRing_mesh_stereo_kf{PAIR[0]}_kf{PAIR[1]}.ply"))
    assert r1["log"] == r0["log"].replace(plain, ster) + "WARN: stereo mesh export skipped (no valid disparity/depth)\n"
    assert len(r1["stereo_mesh"]["verts"]) == 0 and len(r1["stereo_mesh"]["faces"]) == 0
    for fn in FILES:
        assert open(os.path.join(plain, fn)).read() == open(os.path.join(ster, fn)).read(), fn


def test_pipeline_stereo_pair_out_of_range(ctx, tmp_path):
    g, cfg, names = _fixture()
    with pytest.raises(capi.SfmxError, match=r"mesh_stereo.kf_pair \(0, 99\) out of range \(keyframes=5\)"):
        pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, str(tmp_path), stereo=dict(kf_pair=(0, 99), **SMALL))
