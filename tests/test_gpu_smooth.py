"""GPU suite: exact Taubin lambda|mu smoothing of a triangle mesh on the device.  sfmx_smooth_* gives the vertices, the flags and
the five counts byte for byte against the NumPy restatement (tests/smooth_ref.py): hand meshes, every invalid input and refused
parameter set, the block and scan-level edges of vertices, faces and table slots, a vertex with 32 768 neighbours, one edge that
takes every counter update, a random soup as it is and permuted, the sphere-26 surface, every way of feeding a mesh, the state
rules, divergence, the simplify and distance stages fed from the device mesh, and pipeline.fuse / pipeline.run."""
import importlib
import json
import os

import numpy as np
import pytest

import clean_ref as LR
import consist_ref as CR
import fusion_ref as FR
import helpers as H
import sdist_ref as DR
import simplify_ref as PR
import smooth_ref as MR
from test_smooth_cpu import RING_EDGES, SPHERE_COUNTS

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
def sm(ctx):
    """one object for the whole module: its buffers grow and shrink with the cases"""
    s = ctx.smooth()
    yield s
    s.close()


def _check(sm, got, ref, what):
    """the counts a run returned and everything read() gives, against the restatement"""
    assert got == MR.counts(ref), what + ": counts"
    assert sm.sizes()[0] == len(ref["verts"])
    r = sm.read()
    for k in ("verts", "flags"):
        want = np.asarray(ref[k])
        assert r[k].dtype == want.dtype and r[k].shape == want.shape, f"{what}: {k} {r[k].shape} {want.shape}"
        assert r[k].tobytes() == want.tobytes(), f"{what}: {k}"
    return r


def _case(sm, v, f, what, **kw):
    ref = MR.smooth(v, f, **kw)
    _check(sm, sm.run(v, f, **kw), ref, f"{what} {kw}")
    return ref


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


# ---- hand meshes and refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MR.hand_cases()))
def test_hand_meshes(sm, name):
    c = dict(MR.hand_cases()[name])
    v, f = np.asarray(c.pop("verts"), np.float64).reshape(-1, 3), np.asarray(c.pop("faces"), np.int32).reshape(-1, 3)
    ref = _case(sm, v, f, name, **c)
    assert sm.device_mesh()[::3] == (len(v), len(f))
    for iters in (1, 2, 64):
        if "iters" not in c and name not in ("at-the-limit", "at-the-limit-origin"):
            _case(sm, v, f, name, **c, iters=iters)
    if name == "triangle-pinned":
        assert ref["flags"].tolist() == [1, 1, 1] and ref["verts"].tobytes() == v.tobytes()
    if name == "edge-used-three-times":
        assert ref["irregular_edges"] == 1 and ref["pinned"] == 3


def test_every_invalid_input_then_a_good_call(sm):
    bad, good = MR.invalid_inputs()
    gref = MR.smooth(**good)
    for name, c in bad:
        _invalid(lambda: sm.run(c["verts"], c["faces"], unit=c["unit"]))
        _invalid(sm.read)  # the failed run left no result
        with pytest.raises(capi.SfmxError):
            sm.sizes()
        with pytest.raises(capi.SfmxError):
            sm.counts()
        assert sm.device_mesh()[0] == -1 and sm.device_surface()[0] == -1, name
        _check(sm, sm.run(good["verts"], good["faces"], unit=1.0), gref, "after " + name)
    for p in MR.BAD_PARAMS:
        _invalid(lambda: sm.run(good["verts"], good["faces"], **p))
        _invalid(sm.read)
        _check(sm, sm.run(good["verts"], good["faces"], unit=1.0), gref, f"after {p}")
    _invalid(lambda: sm.run(good["verts"], good["faces"]))  # unit has no default
    with pytest.raises(TypeError):
        sm.run(good["verts"], good["faces"], unit=1.0, weights=3)
    sm.run(good["verts"], good["faces"], unit=1.0)
    with pytest.raises(TypeError):
        sm.run(good["verts"], good["faces"], unit=1.0, weights=3)
    assert sm.read()["verts"].shape == (5, 3), "refused in Python, before the library: the result stays"
    for p in MR.GOOD_PARAMS[5:]:
        _case(sm, good["verts"], good["faces"], "accepted", **p)
    # the limits themselves are inside
    v = good["verts"].copy()
    v[3] = (2.0 ** 18, -2.0 ** 18, 0.0)
    v[4] = (-2.0 ** 18, 2.0 ** 18, 2.0 ** 18)
    _case(sm, v, good["faces"], "|q| = 2^18", unit=1.0)
    _invalid(lambda: sm.run(v * 2.0, good["faces"], unit=1.0))
    _case(sm, v * 2.0, good["faces"], "|q| = 2^18 of two units", unit=2.0)
    f = good["faces"].copy()
    f[1, 1] = 4
    _case(sm, good["verts"], f, "the last vertex index", unit=1.0)


def test_divergence_is_refused_and_leaves_the_object_usable(sm):
    v, f = MR.UNIT_TRIANGLE
    ref = _case(sm, v, f, "32 pairs", iters=32, **MR.DIVERGING)
    assert np.abs(ref["verts"]).max() > 800.0
    with pytest.raises(ValueError, match="diverged"):
        MR.smooth(v, f, iters=64, **MR.DIVERGING)
    _invalid(lambda: sm.run(v, f, iters=64, **MR.DIVERGING))
    _invalid(sm.read)
    assert sm.device_mesh()[0] == -1
    _case(sm, v, f, "after the refused call", iters=33, **MR.DIVERGING)
    # in the middle of a larger mesh, and the first pair at which the restatement refuses
    first = next(i for i in range(33, 65) if not _passes(v, f, i))
    assert 50 < first <= 64
    bv, bf = MR.closed_tube(12, 30)
    vv, ff = np.concatenate([bv, v + 50.0]), np.concatenate([bf, f + len(bv)]).astype(np.int32)
    _case(sm, vv, ff, "tube and triangle, the last pair that passes", iters=first - 1, **MR.DIVERGING)
    _invalid(lambda: sm.run(vv, ff, iters=first, **MR.DIVERGING))


def _passes(v, f, iters):
    try:
        MR.smooth(v, f, iters=iters, **MR.DIVERGING)
        return True
    except ValueError:
        return False


# ---- block and scan edges --------------------------------------------------------------------------------------------------
SIZES = [255, 256, 257, 65535, 65536, 65537, 1024 * 1024 + 1]


@pytest.mark.parametrize("k", SIZES)
def test_disjoint_triangles_at_block_and_scan_edges(sm, k):
    """k faces over 3 k vertices, and k vertices of which 3 (k / 3) carry a face: every edge a boundary edge"""
    big = k > 100000
    v, f = MR.disjoint_triangles(k)
    ref = _case(sm, v, f, f"m={k}", unit=0.01, pin=0, iters=1 if big else 3)
    assert ref["edges"] == ref["boundary_edges"] == 3 * k and ref["isolated"] == 0
    v, f = MR.disjoint_triangles(k // 3, k)
    ref = _case(sm, v, f, f"n={k}", unit=0.01, pin=1, iters=1)
    assert ref["pinned"] == 3 * (k // 3) and ref["isolated"] == k - 3 * (k // 3)
    if not big:
        _case(sm, v, f, f"n={k} free", unit=0.01, pin=0, iters=2)


@pytest.mark.parametrize("k", SIZES)
def test_closed_strips_at_block_and_scan_edges(sm, k):
    """n = m = k: a closed band (an even number of faces; an odd k gets one more vertex and a face (a, a, a) over it)"""
    even = k - k % 2
    v, f = MR.closed_strip(even)
    if k % 2:
        v, f = np.concatenate([v, [[0.0, 0.0, 9.0]]]), np.concatenate([f, [[even, even, even]]]).astype(np.int32)
    assert len(v) == len(f) == k
    big = k > 100000
    ref = _case(sm, v, f, f"strip {k}", unit=0.01, pin=0, iters=1 if big else 4)
    assert ref["edges"] == 2 * even and ref["boundary_edges"] == even and ref["irregular_edges"] == 0 and ref["isolated"] == k % 2
    ref = _case(sm, v, f, f"strip {k} pinned", unit=0.01, pin=1, iters=1)
    assert ref["pinned"] == even, "every vertex lies on a rim"


def test_a_closed_tube_moves_everywhere(sm):
    v, f = MR.closed_tube(257, 255)
    ref = _case(sm, v, f, "tube", unit=0.01)
    assert ref["edges"] == 3 * len(v) and ref["boundary_edges"] == 0 and ref["pinned"] == 0 and (ref["verts"] != v).any(1).all()


# ---- one vertex with many neighbours, one edge with every update -----------------------------------------------------------
def test_hubs_with_32768_neighbours(sm):
    v, f = MR.double_cone()
    ref = _case(sm, v, f, "double cone", unit=0.5, iters=2)
    assert MR.counts(ref) == dict(edges=3 * 32768, boundary_edges=0, irregular_edges=0, pinned=0, isolated=0)
    assert (ref["verts"][-2:] != v[-2:]).all(), "the hubs move"
    v, f = MR.open_fan()
    ref = _case(sm, v, f, "open fan, rim pinned", unit=0.5, iters=2, pin=1)
    assert ref["pinned"] == 32768 and ref["boundary_edges"] == 32768 and ref["flags"][-1] == 0 and (ref["verts"][-1] != v[-1]).any()
    ref = _case(sm, v, f, "open fan, rim free", unit=0.5, iters=2, pin=0)
    assert ref["pinned"] == 0 and (ref["verts"] != v).any(1).all()
    # the hub as vertex 0, the smaller end of all its edges: 32 768 keys that start in one window of the table
    hub = len(v) - 1
    swap = np.arange(len(v))
    swap[[0, hub]] = [hub, 0]
    ref0 = _case(sm, v[swap], swap[f].astype(np.int32), "open fan, hub first", unit=0.5, iters=2, pin=0)
    assert ref0["verts"].tobytes() == ref["verts"][swap].tobytes()


def test_65536_faces_over_three_vertices(sm):
    v, f = MR.hot_edge()
    ref = _case(sm, v, f, "hot edge", unit=0.125, pin=1)
    assert MR.counts(ref) == dict(edges=3, boundary_edges=0, irregular_edges=3, pinned=3, isolated=0)
    ref = _case(sm, v, f, "hot edge, free", unit=0.125, pin=0)
    assert (ref["verts"] != v).any()
    _case(sm, v, np.concatenate([f, f[:, ::-1]]), "hot edge, both directions", unit=0.125, pin=0, iters=1)


# ---- random soup -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soup():
    v, f, _ = LR.soup()
    return v, f


@pytest.mark.parametrize("order", ["as-is", "vertices-permuted", "faces-permuted"])
def test_random_soup(sm, soup, order):
    v, f = soup
    if order == "vertices-permuted":
        v, f, _, _ = MR.permute_vertices(v, f, None, 8)
    elif order == "faces-permuted":
        f = f[np.random.default_rng(8).permutation(len(f))]
    for iters in (1, 10, 64):
        for pin in (0, 1):
            ref = _case(sm, v, f, "soup", unit=0.01, origin=(0.1, -0.2, 0.3), iters=iters, pin=pin)
    assert ref["irregular_edges"] >= 1 and ref["isolated"] > 1000 and ref["pinned"] > 10000
    _case(sm, v, f, "soup, other factors", unit=0.003, lam=0.9, mu=-0.2, iters=7, pin=0)


# ---- feeds and state -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ball(ctx):
    """eight small noisy views of the sphere in a volume: a surface with islands"""
    views = CR.sphere8()[:8]
    fu = ctx.fusion(**CR.SPHERE26_VOL)
    for cam, d16 in views:
        fu.add_view(cam, d16)
    yield fu, views
    fu.close()


def _bytes(r):
    return r["verts"].tobytes() + r["flags"].tobytes()


def test_feeding_paths_same_bytes(ctx, ball):
    import torch
    fu, _ = ball
    vol = CR.SPHERE26_VOL
    kw = dict(unit=vol["voxel"], origin=vol["origin"], iters=5)
    v, f, nrm = fu.extract_normals()
    ref = MR.smooth(v, f, **kw)
    assert ref["boundary_edges"] > 0 and 0 < ref["pinned"] < len(v), "precondition: an open surface with an interior"
    s, c = ctx.smooth(), ctx.clean()
    _check(s, s.fusion(fu, **kw), ref, "sfmx_smooth_fusion")
    resident = _bytes(s.read())
    n2, pv, pn = s.device_surface()
    assert n2 == len(v) and pv and pn and s.device_mesh()[::3] == (len(v), len(f)) and s.device_mesh()[1] == pv
    _check(s, s.run(v, f, **kw), ref, "host pointers")
    host = _bytes(s.read())
    assert s.device_surface()[2] is None, "plain pointers carry no normals"
    tv, tf = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, f))
    torch.cuda.synchronize()
    _check(s, s.run(tv.data_ptr(), tf.data_ptr(), n=len(v), m=len(f), **kw), ref, "device pointers")
    dev = _bytes(s.read())
    assert s.device_mesh()[2] == tf.data_ptr(), "device faces are handed on, not copied"
    assert resident == host == dev == _bytes(ref)
    # the cleaned surface, from the clean object
    lref = LR.clean(v, f, nrm)
    assert c.fusion(fu) == LR.counts(lref) and lref["n_faces"] < len(f)
    cref = MR.smooth(lref["verts"], lref["faces"], **kw)
    _check(s, s.clean(c, **kw), cref, "sfmx_smooth_clean")
    assert _bytes(s.read()) != resident and s.device_surface()[2] == c.device_surface()[2] is not None
    # a plain extract leaves the same surface without normals
    v2, f2 = fu.extract()
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    _check(s, s.fusion(fu, **kw), ref, "sfmx_smooth_fusion after a plain extract")
    assert s.device_surface()[2] is None
    s.close()
    c.close()


def test_one_object_large_small_large(ctx):
    s = ctx.smooth()
    big, small = MR.closed_tube(200, 200), MR.closed_tube(5, 4)
    for what, (v, f) in (("large", big), ("small", small), ("large again", big)):
        _case(s, v, f, what, unit=0.01, iters=3)
        assert s.last_us() == 0.0
    ctx.set_timing(True)
    _case(s, *big, "timed", unit=0.01, iters=3)
    assert s.last_us() > 0.0
    ctx.set_timing(False)
    s.close()


def test_state_rules(ctx, ball):
    _, views = ball
    vol = CR.SPHERE26_VOL
    kw = dict(unit=vol["voxel"], origin=vol["origin"], iters=2)
    s, c, fu = ctx.smooth(), ctx.clean(), ctx.fusion(**vol)
    _invalid(s.read)  # before a run
    for fn in (s.sizes, s.counts):
        with pytest.raises(capi.SfmxError):
            fn()
    assert s.device_surface()[0] == -1 and s.device_mesh() == (-1, None, None, 0)
    _invalid(lambda: s.fusion(fu, **kw))  # nothing extracted yet
    _invalid(lambda: s.clean(c, **kw))  # nothing cleaned yet
    fu.add_view(*views[0])
    assert fu.counts()[1] > 0
    _invalid(lambda: s.fusion(fu, **kw))  # counts alone leave no arrays
    v, f = fu.extract()
    ref = MR.smooth(v, f, **kw)
    _check(s, s.fusion(fu, **kw), ref, "after extract")
    assert s.sizes() == (len(v), len(f))
    fu.add_view(*views[1])
    fu.integrate()
    _invalid(lambda: s.fusion(fu, **kw))  # the volume changed
    _invalid(s.read)
    v, f, nrm = fu.extract_normals()
    ref = MR.smooth(v, f, **kw)
    _check(s, s.fusion(fu, **kw), ref, "after extract_normals")
    _invalid(lambda: s.fusion(fu, unit=0.0))  # refused for its parameters: no result left
    _invalid(s.read)
    assert s.device_mesh()[0] == -1
    _check(s, s.fusion(fu, **kw), ref, "after a refused call")
    c.fusion(fu)
    _invalid(lambda: c.fusion(fu, min_permille=1001))  # the clean object lost its result
    _invalid(lambda: s.clean(c, **kw))
    _invalid(s.read)
    fu.reset()
    _invalid(lambda: s.fusion(fu, **kw))  # after a reset
    v0, f0 = fu.extract()  # an empty volume: a current surface without faces
    assert len(f0) == 0
    assert s.fusion(fu, **kw) == dict(edges=0, boundary_edges=0, irregular_edges=0, pinned=0, isolated=0)
    r = s.read()
    assert r["verts"].shape == (0, 3) and r["flags"].shape == (0,)
    for o in (s, c, fu):
        o.close()


# ---- sphere-26 and the stages behind the smoothing -------------------------------------------------------------------------
def test_sphere26_then_simplify_and_distances(ctx):
    """all 26 clean maps fused, cleaned and smoothed on the device: NumPy's bytes and the exact integers of DESIGN.md 21; then
    the chain smooth -> sfmx_simplify_run(on_device = 1) -> sfmx_sdist_*, equal to the same chain fed from host arrays"""
    views, _ = CR.sphere26(False)
    vol = CR.SPHERE26_VOL
    fu, c, s, sp, sd = ctx.fusion(**vol), ctx.clean(), ctx.smooth(), ctx.simplify(), ctx.sdist()
    for cam, d16 in views:
        fu.add_view(cam, d16)
    v, f, nrm = fu.extract_normals()
    lref = LR.clean(v, f, nrm)
    assert c.fusion(fu) == LR.counts(lref) and lref["n_faces"] == len(f)
    ctx.set_timing(True)
    for iters in (5, 10, 20):
        ref = MR.smooth(lref["verts"], lref["faces"], unit=vol["voxel"], origin=vol["origin"], iters=iters)
        got = s.clean(c, unit=vol["voxel"], origin=vol["origin"], iters=iters)
        r = _check(s, got, ref, f"sphere-26, {iters} pairs")
        assert got == SPHERE_COUNTS
        print("sphere-26, %d pairs: %s; %.1f us" % (iters, got, s.last_us()))
    ctx.set_timing(False)
    n, pv, pf, m = s.device_mesh()
    assert (n, m) == (len(v), len(f)) and s.device_surface()[2] == c.device_surface()[2]
    cell = 2 * vol["voxel"]
    dev = sp.run(pv, pf, s.device_surface()[2], n=n, m=m, cell=cell, origin=vol["origin"])
    rd = sp.read(normals=True)
    host = sp.run(r["verts"], lref["faces"], lref["normals"], cell=cell, origin=vol["origin"])
    rh = sp.read(normals=True)
    pref = PR.simplify(ref["verts"], lref["faces"], lref["normals"], cell, vol["origin"])
    assert dev == host == PR.counts(pref) and 0 < pref["n_faces"] < m
    for k in PR.ARRAYS + ("normals",):
        assert rd[k].tobytes() == rh[k].tobytes() == np.asarray(pref[k]).tobytes(), k
    # the smoothed mesh as the target and as the queries of the distance stage, from the device and from the host
    G = DR.icosphere(3, CR.RADIUS)
    d_max = 4 * vol["voxel"]
    sd.set_target(pv, pf, d_max, nv=n, m=m)
    a = sd.query(G[0])
    sd.set_target(r["verts"], lref["faces"], d_max)
    b = sd.query(G[0])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (b[1] >= 0).any()
    sd.set_target(*G, d_max)
    a, b = sd.query(pv, n=n), sd.query(r["verts"])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (b[1] >= 0).any()
    for o in (fu, c, s, sp, sd):
        o.close()


# ---- pipeline --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring6():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    return dict(images=images, K=K, poses=poses, pairs=pairs, vol=CR.RING6_VOL)


def _parse_ply(path):
    lines = open(path).read().split("\n")
    end = lines.index("end_header")
    nv = int([x for x in lines[:end] if x.startswith("element vertex")][0].split()[2])
    nf = int([x for x in lines[:end] if x.startswith("element face")][0].split()[2])
    vert = np.array([x.split() for x in lines[end + 1:end + 1 + nv]], np.float64)
    face = np.array([x.split() for x in lines[end + 1 + nv:end + 1 + nv + nf]], np.int64)
    assert lines[end + 1 + nv + nf:] == [""]
    return lines[:end], vert, face


def test_host_fuse_smooth(ctx, ring6, tmp_path):
    vol = ring6["vol"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain.ply", "false.ply", "on.ply"))
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    m1 = pipe.fuse(*args, num_disparities=64, ply_path=p1, smooth=False)
    assert set(m0) == set(m1) == {"verts", "faces", "views", "warn"} and m0["warn"] == m1["warn"] and m0["views"] == m1["views"]
    assert m0["verts"].tobytes() == m1["verts"].tobytes() and m0["faces"].tobytes() == m1["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read(), "smooth=False is the call without the argument"
    m = pipe.fuse(*args, num_disparities=64, ply_path=p2, smooth=True)
    assert set(m) == {"verts", "faces", "views", "warn", "smooth"} and m["views"] == 6 and m["warn"] is None
    ref = MR.smooth(m0["verts"], m0["faces"], unit=vol["voxel"], origin=vol["origin"])  # the defaults: the voxel, the volume's origin
    assert m["smooth"] == MR.counts(ref) and ref["pinned"] > 0 and (ref["verts"] != m0["verts"]).any(1).sum() > len(m0["verts"]) / 2
    assert m["verts"].tobytes() == ref["verts"].tobytes() and m["faces"].tobytes() == m0["faces"].tobytes()
    head, pv, pf = _parse_ply(p2)
    assert len(pv) == len(ref["verts"]) and (pf[:, 0] == 3).all() and (pf[:, 1:] == m0["faces"]).all()
    assert np.allclose(pv, ref["verts"], rtol=1e-5, atol=1e-9)
    # the manual chain, with other parameters
    h, w = ring6["images"].shape[1:]
    st, fu, s = ctx.stereo(w, h, num_disparities=64), ctx.fusion(**vol), ctx.smooth()
    for a, b in ring6["pairs"]:
        r = pipe.stereo_rectify(ring6["K"], ring6["poses"][a], ring6["poses"][b], w, h)
        il, ir = (ring6["images"][b], ring6["images"][a]) if r["swapped"] else (ring6["images"][a], ring6["images"][b])
        st.disparity(il, ir, r["H_l"], r["H_r"])
        fu.add_stereo_view(r, st)
    v, f = fu.extract()
    assert v.tobytes() == m0["verts"].tobytes()
    okw = dict(iters=3, lam=0.6, mu=-0.3, pin=0, unit=0.37 * vol["voxel"], origin=(0.001, -0.002, 0.003))
    got = s.fusion(fu, **okw)
    chain = s.read()
    for o in (st, fu, s):
        o.close()
    m3 = pipe.fuse(*args, num_disparities=64, smooth=okw)
    ref3 = MR.smooth(m0["verts"], m0["faces"], **okw)
    assert m3["verts"].tobytes() == chain["verts"].tobytes() == ref3["verts"].tobytes() != ref["verts"].tobytes()
    assert m3["smooth"] == got == MR.counts(ref3) and got["pinned"] == 0
    # no pairs, bad parameters
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, smooth=True)
    assert empty["verts"].shape == (0, 3) and empty["smooth"] == dict(edges=0, boundary_edges=0, irregular_edges=0, pinned=0, isolated=0)
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, smooth=dict(cell=1.0))
    for bad in (dict(unit=0.0), dict(lam=0.0), dict(mu=0.5), dict(iters=65), dict(pin=2), dict(origin=(0.0, float("inf"), 0.0))):
        with pytest.raises(capi.SfmxError):
            pipe.fuse(*args, num_disparities=64, smooth=bad)


def test_host_fuse_smooth_with_every_other_stage(ctx, ring6, tmp_path):
    """consistency, clean, appearance, simplify and evaluate together: the final mesh is the restatements' of the cleaned one
    smoothed and then simplified with the normals it had, its grey is the shading of the final vertices, and the evaluation is that
    of the final mesh; without simplify the smoothed vertices keep faces, normals and their order"""
    vol = ring6["vol"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    ply = str(tmp_path / "all.ply")
    G = synth.shell_mesh(3)
    ekw = dict(gt_verts=G[0], gt_faces=G[1], d_max=4 * vol["voxel"], tau=vol["voxel"])
    h, w = ring6["images"].shape[1:]
    sh, st = ctx.shade(), ctx.stereo(w, h, num_disparities=64)
    for a, b in ring6["pairs"]:
        r = pipe.stereo_rectify(ring6["K"], ring6["poses"][a], ring6["poses"][b], w, h)
        il, ir = (ring6["images"][b], ring6["images"][a]) if r["swapped"] else (ring6["images"][a], ring6["images"][b])
        st.disparity(il, ir, r["H_l"], r["H_r"])
        sh.add_stereo_view(r, st)
    for cons, cl, simp in ((True, True, True), (False, True, False), (True, False, False), (False, False, True)):
        m0 = pipe.fuse(*args, num_disparities=64, consistency=cons, appearance=True, clean=cl)
        m = pipe.fuse(*args, num_disparities=64, consistency=cons, appearance=True, clean=cl, simplify=simp, smooth=dict(iters=4),
                      evaluate=ekw, ply_path=ply)
        want = {"verts", "faces", "views", "warn", "normals", "grey", "vertex_views", "smooth", "evaluation"}
        assert set(m) == want | ({"consistency"} if cons else set()) | ({"clean"} if cl else set()) | ({"simplify"} if simp else set())
        sref = MR.smooth(m0["verts"], m0["faces"], unit=vol["voxel"], origin=vol["origin"], iters=4)
        assert m["smooth"] == MR.counts(sref)
        if cons and not cl:
            assert {k: m["smooth"][k] for k in RING_EDGES} == RING_EDGES, "the surface of DESIGN.md 21's table"
        ref = dict(verts=sref["verts"], faces=m0["faces"], normals=m0["normals"])
        if simp:
            ref = PR.simplify(sref["verts"], m0["faces"], m0["normals"], 2.0 * vol["voxel"], vol["origin"])
            assert 0 < ref["n_faces"] < len(m0["faces"])
            assert m["simplify"]["verts_before"] == len(m0["verts"]) and m["simplify"]["faces_before"] == len(m0["faces"])
            assert m["simplify"]["clusters"] == ref["clusters"]
        for k in ("verts", "faces", "normals"):
            assert m[k].tobytes() == np.asarray(ref[k]).tobytes(), k
        if cl:
            assert m["clean"] == m0["clean"]
        if cons:
            assert m["consistency"] == m0["consistency"]
        assert m["evaluation"] == pipe.surface_eval(ctx, m["verts"], m["faces"], *G, d_max=ekw["d_max"], tau=ekw["tau"])
        g1, c1 = sh.shade(m["verts"], m["normals"], FR.resolve(vol["voxel"]))
        assert m["grey"].tobytes() == g1.tobytes() and m["vertex_views"].tobytes() == c1.tobytes()
        assert (c1 > 0).any() and len(np.unique(g1)) > 10
    sh.close()
    st.close()
    head, pv, pf = _parse_ply(ply)
    assert "property uchar red" in head and "property float nx" in head and pv.shape == (len(ref["verts"]), 9)
    assert (pf[:, 1:] == ref["faces"]).all() and (pv[:, 6] == m["grey"]).all()
    # a surface with nothing left: the cleaning removes every component, the smoothing has nothing to do
    none = str(tmp_path / "none.ply")
    m5 = pipe.fuse(*args, num_disparities=64, clean=dict(min_faces=10 ** 8), smooth=True, ply_path=none)
    assert m5["verts"].shape == (0, 3) and m5["faces"].shape == (0, 3) and "no faces" in m5["warn"] and not os.path.exists(none)
    assert m5["smooth"] == dict(edges=0, boundary_edges=0, irregular_edges=0, pinned=0, isolated=0)


def test_pipeline_run_smooth(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    plain, smooth = str(tmp_path / "plain"), str(tmp_path / "smooth")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in PAIR)
    mesh = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][PAIR[0]], r0["kf_poses"][PAIR[1]], **SMALL)
    lo, hi = mesh["verts"].min(0), mesh["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    fz = dict(pairs=[PAIR], origin=tuple(lo), voxel=voxel, dims=dims, **SMALL)
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain, fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, smooth, fusion=dict(fz, smooth=dict(iters=6)))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(smooth, "X")
    assert sorted(os.listdir(smooth)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m1) == {"verts", "faces", "views", "warn"} and set(m) == set(m1) | {"smooth"} and len(m1["faces"]) > 0
    ref = MR.smooth(m1["verts"], m1["faces"], unit=voxel, origin=tuple(lo), iters=6)
    print("run: %s, %d of %d vertices moved" % (MR.counts(ref), int((ref["verts"] != m1["verts"]).any(1).sum()), len(m1["verts"])))
    assert (ref["verts"] != m1["verts"]).any()
    assert m["verts"].tobytes() == ref["verts"].tobytes() and m["faces"].tobytes() == m1["faces"].tobytes()
    assert m["smooth"] == MR.counts(ref)
    assert open(os.path.join(smooth, "templeRing_mesh_fused.ply")).read().startswith(
        "ply\nformat ascii 1.0\nelement vertex %d\n" % len(ref["verts"]))
