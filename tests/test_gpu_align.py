"""GPU suite: direct TSDF pose alignment.  Every comparison is bit for bit against the NumPy restatement (tests/align_ref.py):
the 28 ordered sums and n of an evaluation, and for the loop the refined R_rw and c_left, the status, the iteration count and
the trace.  The four-sphere fixture through every way of feeding a volume, random volumes with undefined cells where NumPy
shows every skip branch taken, map sizes and strides around the 8 x 8 / 16 x 16 tiles and past 256 blocks, special values,
one object across maps that grow and shrink, the loop's end states, pipeline.fuse / pipeline.run, and the refusals."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

import align_ref as AL
import consist_ref as CR
import fusion_ref as FR
import helpers as H
import raycast_ref as RR
from test_align_cpu import starts, uniform_view

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
def al(ctx):
    a = ctx.align()
    yield a
    a.close()


def _scene():
    sc = AL.scene_volume()
    return sc, (sc["sum"], sc["count"], AL.VOL["origin"], AL.VOL["voxel"])


def _system(al, feed, vol, cam, d16, what, min_weight=0, **kw):
    """one evaluation on the device against align_ref.system; returns (sums, n)"""
    sums, n = al.system(feed, cam, d16, min_weight=min_weight, **kw)
    rs, rn = AL.system(vol, cam, d16, kw.get("stride", 1), kw.get("disp_min", 1.0))
    assert n == rn, f"{what}: n {n} vs {rn}"
    H.assert_bits_equal(sums, rs, f"{what}: sums")
    return sums, n


def _loop(al, feed, vol, cam, d16, what, **kw):
    out = al.view(feed, cam, d16, **kw)
    ref = AL.align(vol, cam, d16, **{k: v for k, v in kw.items() if k != "min_weight"})
    assert (out["status"], out["iterations"]) == (ref["status"], ref["iterations"]), f"{what}: {out['status']}, {out['iterations']} vs {ref['status']}, {ref['iterations']}"
    assert AL.same_result(out, ref), f"{what}: the device loop differs from align_ref.align: {out['trace']} vs {ref['trace']}"
    for k in ("f", "cx", "cy", "B"):
        assert out["view"][k] == float(cam[k]), k
    return out, ref


# ---- the fixture, every feed -------------------------------------------------------------------------------------------------
def test_system_feeds_give_the_same_bits(ctx, al):
    import torch
    sc, arrays = _scene()
    fu = ctx.fusion(**AL.VOL)
    for cam, d16 in AL.scene_views():
        fu.add_view(cam, d16)
    cam, d16 = AL.novel_view(AL.NOVEL[0])
    first = _system(al, fu, sc["volume"], cam, d16, "fusion object, views pending")  # the call integrates them
    s, c = fu.read()
    assert s.tobytes() == sc["sum"].tobytes() and c.tobytes() == sc["count"].tobytes()
    assert first[1] == 8447
    ts, tc, td = torch.from_numpy(s).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(d16).cuda()
    torch.cuda.synchronize()
    dev = (ts.data_ptr(), tc.data_ptr(), AL.VOL["origin"], AL.VOL["voxel"], AL.VOL["dims"])
    for pos in AL.NOVEL:
        cam, d16 = AL.novel_view(pos)
        td.copy_(torch.from_numpy(d16))
        torch.cuda.synchronize()
        for k, start in enumerate(starts(cam, sc["volume"])):
            a = _system(al, fu, sc["volume"], start, d16, f"fusion object {pos} start {k}")
            b = al.system(arrays, start, d16)
            d = al.system(dev, start, d16)
            e = al.system(dev, start, td.data_ptr(), shape=d16.shape)
            for other in (b, d, e):
                assert other[1] == a[1] and other[0].tobytes() == a[0].tobytes(), "feeds differ"
    fu.close()


@pytest.mark.parametrize("min_weight", [2, 6])
def test_system_min_weight(al, min_weight):
    sc, arrays = _scene()
    vol = AL.volume(sc["sum"], sc["count"], AL.VOL["origin"], AL.VOL["voxel"], min_weight)
    cam, d16 = AL.novel_view(AL.NOVEL[1])
    why = AL.rows(vol, cam, d16)[3]
    _, n = _system(al, arrays, vol, cam, d16, f"min_weight {min_weight}", min_weight=min_weight)
    assert 0 < n <= 7796 and (min_weight == 2 or (why["undefined"] > 0 and n < 7796)), why


# ---- random volumes: every skip branch -----------------------------------------------------------------------------------------
def _grid_view(dims, c2, d):
    """voxel 1, R = I, f = 16, B = 1: disparity d gives the depth Z = 256 / d, and pixel (x, y) lifts to
    (x - 2, y - 2, c2 + Z) scaled by Z / 16 about the axis: with d = 16 every sample is a grid point or outside"""
    w, h = dims[0] + 4, dims[1] + 4
    cam = RR.axis_camera((0.0, 0.0, float(c2)), 16.0, w, h, 2.0, 2.0)
    cam["B"] = 1.0
    return cam, np.full((h, w), d, np.int16)


@pytest.mark.parametrize("dims", [(9, 7, 5), (65, 5, 3)])
def test_random_volumes_on_the_lattice(al, dims):
    seen = dict(invalid=0, outside=0, undefined=0, far=0, used=0)
    for seed in RR.RANDOM_SEEDS:
        s, c = RR.random_volume(dims, seed)
        s = s * 1.5  # some |s| >= 1: the "far" branch
        vol = AL.volume(s, c, (0.0, 0.0, 0.0), 1.0)
        feed = (s, c, (0.0, 0.0, 0.0), 1.0)
        # Z = 16: grid points; planes below the grid, g = 0, inside, g = n - 2, g = n - 1 (outside) and above
        for plane in (-1, 0, 1, dims[2] - 2, dims[2] - 1, dims[2]):
            cam, d16 = _grid_view(dims, plane - 16, 16)
            d16[0, :3] = -16
            why = AL.rows(vol, cam, d16)[3]
            _system(al, feed, vol, cam, d16, f"{dims} seed {seed} plane {plane}")
            if plane in (-1, dims[2] - 1, dims[2]):
                assert why["used"] == 0 and why["outside"] == d16.size - 3, (plane, why)
            for k in seen:
                seen[k] += why[k]
        # Z = 8: x and y in steps of half a voxel about the axis, z in the middle of a cell
        cam, d16 = _grid_view(dims, -7.5, 32)
        seen["used"] += _system(al, feed, vol, cam, d16, f"{dims} seed {seed} half cells")[1]
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("dims", [(9, 7, 5), (65, 5, 3)])
def test_random_volumes_oblique(al, dims):
    used = 0
    for seed in RR.RANDOM_SEEDS:
        s, c, origin, voxel, cam, _ = RR.random_case(dims, seed)
        cam["B"] = 0.05
        rng = np.random.default_rng(seed + 7)
        Z = rng.uniform(0.02, 0.3, (cam["h"], cam["w"]))
        d16 = np.clip(np.rint(16.0 * cam["f"] * cam["B"] / Z), 1, 32000).astype(np.int16)
        d16[rng.random(d16.shape) < 0.1] = -16
        vol = AL.volume(s, c, origin, voxel)
        why = AL.rows(vol, cam, d16)[3]
        assert why["outside"] > 0 and why["undefined"] > 0 and why["used"] > 0, why
        used += _system(al, (s, c, origin, voxel), vol, cam, d16, f"oblique {dims} seed {seed}")[1]
        _loop(al, (s, c, origin, voxel), vol, cam, d16, f"oblique loop {dims} seed {seed}", max_iters=3, min_pixels=1)
    assert used > 20


# ---- map sizes and strides ---------------------------------------------------------------------------------------------------
def _sized_view(w, h, pos=AL.NOVEL[0]):
    cam = FR.look_at_cam(pos, AL.SPHERES[0][0], AL.SCENE["f"], w, h, AL.SCENE["B"])  # the centre pixel sees the first sphere
    return cam, AL.scene_disp16(cam, w, h)


@pytest.mark.parametrize("w, h", [(1, 1), (1, 300), (300, 1), (7, 9), (8, 8), (17, 16), (64, 4)])
def test_map_sizes_and_strides(al, w, h):
    sc, arrays = _scene()
    cam, d16 = _sized_view(w, h)
    assert (d16 != -16).any()
    total = 0
    for stride in (1, 2, 3, max(w, h) + 1):
        total += _system(al, arrays, sc["volume"], cam, d16, f"{w} x {h} stride {stride}", stride=stride)[1]
    assert total > 0


def test_more_than_256_blocks(al):
    sc, arrays = _scene()
    cam, d16 = _sized_view(272, 272)
    assert ((272 + 15) // 16) ** 2 > 256, "the second level of the tree recurses"
    _, n = _system(al, arrays, sc["volume"], cam, d16, "272 x 272")
    assert n > 5000
    _system(al, arrays, sc["volume"], cam, d16, "272 x 272 stride 3", stride=3)


def test_only_the_last_lane_of_a_block(al):
    sc, arrays = _scene()
    cam, d16 = AL.novel_view(AL.NOVEL[0])
    used = AL.rows(sc["volume"], cam, d16)[0]
    ys, xs = np.nonzero(used[15::16, 15::16])
    y, x = 16 * int(ys[0]) + 15, 16 * int(xs[0]) + 15
    one = np.full_like(d16, -16)
    one[y, x] = d16[y, x]
    sums, n = _system(al, arrays, sc["volume"], cam, one, "one sample in a block's last lane")
    assert n == 1 and sums[27] > 0.0


def test_one_object_across_sizes(ctx):
    sc, arrays = _scene()
    a = ctx.align()
    seen = {}
    for w, h in ((17, 16), (272, 272), (1, 1), (64, 4), (272, 272), (17, 16)):
        cam, d16 = _sized_view(w, h)
        sums, n = _system(a, arrays, sc["volume"], cam, d16, f"reuse {w} x {h}")
        key = (w, h)
        assert seen.setdefault(key, (sums.tobytes(), n)) == (sums.tobytes(), n)
    a.close()


# ---- special values ------------------------------------------------------------------------------------------------------------
def test_all_invalid_map(al):
    sc, arrays = _scene()
    cam, d16 = AL.novel_view(AL.NOVEL[0])
    none = np.full_like(d16, -16)
    sums, n = _system(al, arrays, sc["volume"], cam, none, "all invalid")
    assert n == 0 and not sums.any() and not np.signbit(sums).any(), "all +0.0"
    out, _ = _loop(al, arrays, sc["volume"], cam, none, "all invalid loop")
    assert out["status"] == capi.ALIGN_TOO_FEW and out["iterations"] == 1
    assert out["view"]["R_rw"].tobytes() == np.asarray(cam["R_rw"], np.float64).tobytes()
    assert out["view"]["c_left"].tobytes() == np.asarray(cam["c_left"], np.float64).tobytes()


@pytest.mark.parametrize("disp_min", [0.0, -1.0])
def test_disparity_zero_under_a_disp_min_that_lets_it_through(al, disp_min):
    sc, arrays = _scene()
    cam, d16 = AL.novel_view(AL.NOVEL[0])
    z = d16.copy()
    z[::2] = 0  # depth f B / 0: the lift is not finite and the sample is outside
    z[1, :8] = -8
    why = AL.rows(sc["volume"], cam, z, 1, disp_min)[3]
    assert why["outside"] >= z.size // 2
    _, n = _system(al, arrays, sc["volume"], cam, z, f"zeros, disp_min {disp_min}", disp_min=disp_min)
    assert 0 < n < 8447


def test_negative_zero_terms(al):
    """s = -0.0 at a sample: it sits on a grid point (every fraction 0) whose value is -0.0 with negative neighbours, so each lerp
    is -0.0 + 0.0 * (negative) = -0.0; then b_m = J_m * -0.0 carries the sign of -J_m"""
    dims = (12, 12, 4)
    s = np.full(dims[::-1], -0.5)
    s[1, ::2, ::2] = -0.0
    c = np.ones(dims[::-1], np.int32)
    vol = AL.volume(s, c, (0.0, 0.0, 0.0), 1.0)
    cam, d16 = _grid_view(dims, 1 - 16, 16)
    used, J, sv, _ = AL.rows(vol, cam, d16)
    zero = used & (sv == 0.0)
    assert zero.any() and np.signbit(sv[zero]).all()
    T = AL.terms(used, J, sv)
    assert np.signbit(T[21:27][:, zero]).any() and not np.signbit(T[27]).any()
    _system(al, (s, c, (0.0, 0.0, 0.0), 1.0), vol, cam, d16, "-0.0")
    # a map of 16 x 16 samples, every one on such a grid point, where G is +0.0 along x and z: b_3 and b_5 are whole-block sums
    # of +0.0 * -0.0 = -0.0 and stay -0.0
    s2 = np.full((4, 40, 40), -0.5)
    s2[1, ::2, ::2] = -0.0
    vol2 = AL.volume(s2, np.ones_like(s2, np.int32), (0.0, 0.0, 0.0), 1.0)
    cam2 = RR.axis_camera((0.0, 0.0, -31.0), 16.0, 16, 16, -2.0, -2.0)  # Z = 32: pixel (x, y) lifts to (2 x + 4, 2 y + 4, 1)
    cam2["B"] = 1.0
    sums, n = _system(al, (s2, np.ones_like(s2, np.int32), (0.0, 0.0, 0.0), 1.0), vol2, cam2, np.full((16, 16), 8, np.int16), "-0.0 block",
                      disp_min=0.25)
    assert n == 256 and sums[27] == 0.0 and np.signbit(sums[21:27]).any()


# ---- the loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", AL.NOVEL)
def test_loop_from_the_far_start(al, pos):
    sc, arrays = _scene()
    cam, d16 = AL.novel_view(pos)
    start = starts(cam, sc["volume"])[2]
    out, _ = _loop(al, arrays, sc["volume"], start, d16, f"loop {pos}")
    assert out["status"] == capi.ALIGN_CONVERGED and out["iterations"] == 9
    e = AL.pose_error(out["view"], cam, AL.VOL["voxel"])
    assert e[0] < 0.25 and e[1] < 0.3


@pytest.mark.parametrize("kw, status", [
    (dict(stride=2), capi.ALIGN_CONVERGED),
    (dict(damping=1000.0), capi.ALIGN_CONVERGED),
    (dict(max_iters=1), capi.ALIGN_MAX_ITERS),
    (dict(max_iters=2), capi.ALIGN_MAX_ITERS),
    (dict(min_pixels=9000), capi.ALIGN_TOO_FEW),
    (dict(eps_rot=1e-2, eps_trans=10.0), capi.ALIGN_CONVERGED),
])
def test_loop_parameters(al, kw, status):
    sc, arrays = _scene()
    cam, d16 = AL.novel_view(AL.NOVEL[0])
    start = starts(cam, sc["volume"])[2]
    out, _ = _loop(al, arrays, sc["volume"], start, d16, f"loop {kw}", **kw)
    assert out["status"] == status
    if "max_iters" in kw:
        assert out["iterations"] == kw["max_iters"]


def test_loop_from_the_fusion_object_and_device_map(ctx, al):
    import torch
    sc, arrays = _scene()
    fu = ctx.fusion(**AL.VOL)
    for cam, d16 in AL.scene_views():
        fu.add_view(cam, d16)
    cam, d16 = AL.novel_view(AL.NOVEL[1])
    start = starts(cam, sc["volume"])[1]
    a, _ = _loop(al, fu, sc["volume"], start, d16, "loop, fusion object with views pending", max_iters=3)
    td = torch.from_numpy(d16).cuda()
    torch.cuda.synchronize()
    b = al.view(fu, start, td.data_ptr(), shape=d16.shape, max_iters=3)
    assert AL.same_result(a, b)
    ctx.set_timing(True)
    al.view(arrays, start, d16, max_iters=2)
    assert al.last_us() > 0.0
    ctx.set_timing(False)
    fu.close()


def test_degenerate_volume_returns_the_pose_unchanged(al):
    s, c = np.full((9, 9, 9), 0.5), np.ones((9, 9, 9), np.int32)
    vol = AL.volume(s, c, (0.0, 0.0, 0.0), 0.01)
    cam, d16 = uniform_view()
    out, _ = _loop(al, (s, c, (0.0, 0.0, 0.0), 0.01), vol, cam, d16, "uniform volume")
    assert out["status"] == capi.ALIGN_DEGENERATE and out["iterations"] == 1 and out["trace"][0][0] == 256
    assert out["view"]["R_rw"].tobytes() == np.asarray(cam["R_rw"], np.float64).tobytes()
    assert out["view"]["c_left"].tobytes() == np.asarray(cam["c_left"], np.float64).tobytes()
    out, _ = _loop(al, (s, c, (0.0, 0.0, 0.0), 0.01), vol, cam, d16, "uniform volume, damped", damping=1.0)
    assert out["status"] == capi.ALIGN_CONVERGED and out["iterations"] == 1


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
def _moved(pose, deg, shift):
    """a camera->world pose (R, c) carried along by a small rigid motion of the world about the origin"""
    th = np.radians(deg)
    D = np.array([[np.cos(th), 0.0, np.sin(th)], [0.0, 1.0, 0.0], [-np.sin(th), 0.0, np.cos(th)]])
    R, c = pose
    return D @ R, D @ c + np.asarray(shift)


def test_fuse_align(ctx, tmp_path):
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES[:4], 320, 240)
    vol = CR.RING6_VOL
    poses = list(poses)
    for i in pairs[2]:  # the third pair's rig is 1 degree and about a voxel off
        poses[i] = _moved(poses[i], 1.0, (0.003, -0.002, 0.002))
    args = (ctx, images, K, poses, pairs, vol["origin"], vol["voxel"], vol["dims"])
    akw = dict(max_iters=4, stride=2)
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain.ply", "again.ply", "align.ply"))
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    m1 = pipe.fuse(*args, num_disparities=64, ply_path=p1, align=False)
    assert set(m0) == set(m1) == {"verts", "faces", "views", "warn"}
    assert m0["verts"].tobytes() == m1["verts"].tobytes() and m0["faces"].tobytes() == m1["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read()
    m = pipe.fuse(*args, num_disparities=64, ply_path=p2, align=dict(seed=2, **akw))
    assert set(m) == set(m0) | {"alignment"} and [a["pair"] for a in m["alignment"]] == [pairs[2], pairs[3]] and m["views"] == 4
    # the standalone objects on the same maps, and NumPy on the same maps
    st, fu, al = ctx.stereo(320, 240, num_disparities=64), ctx.fusion(**vol), ctx.align()
    views = []
    for q, (a, b) in enumerate(pairs):
        rect = pipe.stereo_rectify(K, poses[a], poses[b], 320, 240)
        il, ir = (images[b], images[a]) if rect["swapped"] else (images[a], images[b])
        d16 = st.disparity(il, ir, rect["H_l"], rect["H_r"])
        if q >= 2:
            s, c = FR.integrate(vol["origin"], vol["voxel"], vol["dims"], views)
            ref = AL.align(AL.volume(s, c, vol["origin"], vol["voxel"]), rect, d16, **akw)
            own = al.view(fu, rect, d16, **akw)
            from_stereo = al.view(fu, rect, st, **akw)  # the same map, read in place on the device
            got = m["alignment"][q - 2]
            assert AL.same_result(own, ref), f"pair {q}: the standalone object differs from NumPy"
            assert AL.same_result(own, from_stereo), f"pair {q}: sfmx_align_stereo_view differs from the map by pointer"
            assert (got["status"], got["iterations"], got["n"]) == (own["status"], own["iterations"], own["trace"][-1][0])
            assert got["status"] in (capi.ALIGN_CONVERGED, capi.ALIGN_MAX_ITERS), got
            assert got["view"]["R_rw"].tobytes() == own["view"]["R_rw"].tobytes() and got["view"]["c_left"].tobytes() == own["view"]["c_left"].tobytes()
            assert got["rms"] == float(np.sqrt(own["trace"][-1][1] / own["trace"][-1][0]))
            rect = dict(rect, R_rw=own["view"]["R_rw"], c_left=own["view"]["c_left"])
        fu.add_view(rect, d16)
        views.append((rect, d16))
    s, c = fu.read()
    rs, rcnt = FR.integrate(vol["origin"], vol["voxel"], vol["dims"], views)
    assert s.tobytes() == rs.tobytes() and c.tobytes() == rcnt.tobytes(), "the volume holds the refined views"
    v, f = fu.extract()
    assert m["verts"].tobytes() == v.tobytes() and m["faces"].tobytes() == f.tobytes()
    # the third pair ends nearer to where it belongs
    true = pipe.stereo_rectify(K, *[CR.ring_frames(synth, CR.RING6_ANGLES[2:3], 320, 240)[2][i] for i in (0, 1)], 320, 240)
    given = pipe.stereo_rectify(K, poses[pairs[2][0]], poses[pairs[2][1]], 320, 240)
    e0, e1 = AL.pose_error(given, true, vol["voxel"]), AL.pose_error(m["alignment"][0]["view"], true, vol["voxel"])
    print("third pair: given", e0, "aligned", e1, m["alignment"][0]["status"], m["alignment"][0]["rms"])
    # with appearance the shade views take the refined views too
    ma = pipe.fuse(*args, num_disparities=64, appearance=True, align=dict(seed=2, **akw))
    assert ma["verts"].tobytes() == m["verts"].tobytes() and len(ma["grey"]) == len(ma["verts"])
    for o in (st, fu, al):
        o.close()


def test_fuse_align_refusals(ctx):
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES[:2], 320, 240)
    vol = CR.RING6_VOL
    args = (ctx, images, K, poses, pairs, vol["origin"], vol["voxel"], vol["dims"])
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, align=dict(iterations=3))
    for bad in (dict(seed=0), dict(max_iters=0), dict(stride=0)):
        with pytest.raises(capi.SfmxError) as e:
            pipe.fuse(*args, num_disparities=64, align=bad)
        assert e.value.status == capi.SFMX_ERR_INVALID
    with pytest.raises(capi.SfmxError) as e:
        pipe.fuse(*args, num_disparities=64, align=True, consistency=True)
    assert e.value.status == capi.SFMX_ERR_INVALID
    # a seed past the list aligns nothing and changes nothing
    m0 = pipe.fuse(*args, num_disparities=64)
    m = pipe.fuse(*args, num_disparities=64, align=dict(seed=5))
    assert m["alignment"] == [] and m["verts"].tobytes() == m0["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes()


def test_pipeline_run_align(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in PAIR)
    sm = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][PAIR[0]], r0["kf_poses"][PAIR[1]], **SMALL)
    lo, hi = sm["verts"].min(0), sm["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    akw = dict(max_iters=2, stride=2, min_pixels=1)
    # the one pair with valid disparity, listed twice: its second listing is aligned against the volume of the first
    fz = dict(pairs=[PAIR, PAIR], origin=tuple(lo), voxel=voxel, dims=dims, align=dict(seed=1, **akw), **SMALL)
    r = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None, fusion=fz)
    assert r["log"] == r0["log"]
    got = r["fused_mesh"]["alignment"]
    assert len(got) == 1 and got[0]["pair"] == PAIR
    h, w = g["images"].shape[1:]
    rect = pipe.stereo_rectify(g["K"], r["kf_poses"][PAIR[0]], r["kf_poses"][PAIR[1]], w, h)
    il, ir = (g["images"][fb], g["images"][fa]) if rect["swapped"] else (g["images"][fa], g["images"][fb])
    st = ctx.stereo(w, h, **SMALL)
    d16 = st.disparity(il, ir, rect["H_l"], rect["H_r"])
    st.close()
    s, c = FR.integrate(tuple(lo), voxel, dims, [(rect, d16)])
    ref = AL.align(AL.volume(s, c, tuple(lo), voxel), rect, d16, **akw)
    assert (got[0]["status"], got[0]["iterations"], got[0]["n"]) == (ref["status"], ref["iterations"], ref["trace"][-1][0])
    assert got[0]["view"]["R_rw"].tobytes() == np.asarray(ref["view"]["R_rw"], np.float64).tobytes()
    assert got[0]["view"]["c_left"].tobytes() == np.asarray(ref["view"]["c_left"], np.float64).tobytes()


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, al):
    sc, arrays = _scene()
    cam, d16 = AL.novel_view(AL.NOVEL[0])
    lib = ctx.lib

    def refused(fn):
        with pytest.raises(capi.SfmxError) as e:
            fn()
        assert e.value.status == capi.SFMX_ERR_INVALID and str(e.value).split(": ", 1)[1], "SFMX_ERR_INVALID with a message"

    refused(lambda: al.system(arrays, cam, d16, max_iters=0))
    refused(lambda: al.system(arrays, cam, d16, stride=0))
    refused(lambda: al.view(arrays, cam, d16, max_iters=65))
    refused(lambda: al.view(arrays, cam, d16, damping=-1.0))
    refused(lambda: al.system(arrays, dict(cam, f=float("nan")), d16))
    refused(lambda: al.system((sc["sum"][:1], sc["count"][:1], AL.VOL["origin"], AL.VOL["voxel"]), cam, d16))  # nz = 1
    p = capi.align_params()
    fp = capi.fusion_params(AL.VOL["origin"], AL.VOL["voxel"], AL.VOL["dims"])
    s, c = np.ascontiguousarray(sc["sum"]), np.ascontiguousarray(sc["count"])
    v = capi.fusion_view(cam, 160, 160)
    sums, n, out = np.zeros(28), ctypes.c_int32(0), capi.AlignResult()
    arr = (ctypes.byref(fp), s.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(0))
    pd = d16.ctypes.data_as(ctypes.c_void_p)
    dp = sums.ctypes.data_as(ctypes.c_void_p)
    refused(lambda: ctx._chk(lib.sfmx_align_system_arrays(ctx.h_, al.h_, *arr, None, pd, ctypes.c_int(0), ctypes.byref(p), dp, ctypes.byref(n))))
    refused(lambda: ctx._chk(lib.sfmx_align_system_arrays(ctx.h_, al.h_, *arr, ctypes.byref(v), None, ctypes.c_int(0), ctypes.byref(p), dp, ctypes.byref(n))))
    refused(lambda: ctx._chk(lib.sfmx_align_system_arrays(ctx.h_, al.h_, *arr, ctypes.byref(v), pd, ctypes.c_int(0), None, dp, ctypes.byref(n))))
    refused(lambda: ctx._chk(lib.sfmx_align_view_arrays(ctx.h_, al.h_, *arr, ctypes.byref(v), pd, ctypes.c_int(0), ctypes.byref(p), None)))
    refused(lambda: ctx._chk(lib.sfmx_align_view(ctx.h_, al.h_, None, ctypes.byref(v), pd, ctypes.c_int(0), ctypes.byref(p), ctypes.byref(out))))
    with pytest.raises(TypeError):
        al.system(arrays, cam, d16, iterations=2)
    # the object is still usable
    assert al.system(arrays, cam, d16)[1] == 8447
