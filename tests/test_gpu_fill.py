"""GPU suite: exact filling of a triangle mesh's small holes by centroid fans on the device.  sfmx_fill_* gives the vertices, the
normals, the faces and the eight counts byte for byte against the NumPy restatement (tests/fill_ref.py): hand meshes at four loop
caps, open tubes with rims at, below and above the cap, disjoint triangles and quads at the block and scan-level edges of
vertices, faces and table slots, all of them relabelled as well, a random soup as it is and permuted, every invalid input and
refused parameter set, every way of feeding a mesh, the state rules, ring-6 through fill and smooth into the simplify, shade and
distance stages, and pipeline.fuse / pipeline.run."""
import importlib
import json
import os

import numpy as np
import pytest

import clean_ref as LR
import consist_ref as CR
import fill_ref as R
import fusion_ref as FR
import helpers as H
import simplify_ref as PR
import smooth_ref as MR
from test_fill_cpu import RING_CLEANED, RING_CLEANED_PINNED, RING_INPUT, RING_ROWS, ZERO

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
PAIR = (2, 3)  # e2e_keyframes: the pair with valid disparity
SMALL = dict(num_disparities=32, census=5)
CAPS = (3, 4, 32, 1024)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fl(ctx):
    """one object for the whole module: its buffers grow and shrink with the cases"""
    f = ctx.fill()
    yield f
    f.close()


def _check(fl, got, ref, what):
    """the counts a run returned and everything read() gives, against the restatement"""
    assert got == R.counts(ref), what + ": counts"
    nrm = ref.get("normals") is not None
    n_out, m_out = len(ref["verts"]), len(ref["faces"])
    assert fl.sizes() == (n_out - ref["new_verts"], m_out - ref["new_faces"], n_out, m_out), what
    assert fl.device_mesh()[::3] == (n_out, m_out) and fl.device_surface()[0] == n_out and (fl.device_surface()[2] is not None) == nrm
    r = fl.read(normals=nrm)
    for k in ("verts", "faces") + (("normals",) if nrm else ()):
        want = np.asarray(ref[k])
        assert r[k].dtype == want.dtype and r[k].shape == want.shape, f"{what}: {k} {r[k].shape} {want.shape}"
        assert r[k].tobytes() == want.tobytes(), f"{what}: {k}"
    return r


def _case(fl, v, f, nrm, what, **kw):
    ref = R.fill(v, f, nrm, **kw)
    _check(fl, fl.run(v, f, nrm, **kw), ref, f"{what} {kw}")
    return ref


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


def _relabel(v, f, nrm, seed):
    v2, f2, n2, _ = R.permute_vertices(v, f, nrm, seed)
    return np.ascontiguousarray(v2), np.ascontiguousarray(f2), (None if n2 is None else np.ascontiguousarray(n2))


# ---- hand meshes and refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.hand_cases()))
def test_hand_meshes(fl, name):
    c = dict(R.hand_cases()[name])
    v, f = np.asarray(c.pop("verts"), np.float64).reshape(-1, 3), np.asarray(c.pop("faces"), np.int32).reshape(-1, 3)
    nrm = c.pop("normals", None)
    nrm = None if nrm is None else np.asarray(nrm, np.float64).reshape(-1, 3)
    if nrm is None and len(v):
        nrm = np.random.default_rng(len(v)).standard_normal(v.shape)
    refs = {}
    for cap in CAPS:
        refs[cap] = _case(fl, v, f, nrm, name, **c, max_edges=cap)
        _case(fl, v, f, None, name + " without normals", **c, max_edges=cap)
    if name in ("open-quad", "cube-open", "half-negative"):
        assert refs[3]["filled_loops"] == 0 and refs[4]["filled_loops"] == 1 and refs[1024]["new_faces"] == 4
    if name in ("lone-triangle", "tetrahedron-open"):
        assert refs[3]["new_faces"] == 1 and refs[3]["new_verts"] == 0
    if name == "two-holes-share-a-vertex":
        assert refs[1024]["filled_loops"] == 0 and refs[1024]["complex_vertices"] == 1
    if name == "tetrahedron-closed":
        assert R.counts(refs[32]) == dict(ZERO, edges=6) and refs[32]["faces"].tobytes() == f.tobytes()


def test_every_invalid_input_then_a_good_call(fl):
    bad, good = R.invalid_inputs()
    gn = np.random.default_rng(5).standard_normal(good["verts"].shape)
    gref = R.fill(good["verts"], good["faces"], gn, unit=1.0)
    assert gref["filled_loops"] == 1

    def good_call(what):
        _check(fl, fl.run(good["verts"], good["faces"], gn, unit=1.0), gref, "after " + what)

    for name, c in bad:
        _invalid(lambda: fl.run(c["verts"], c["faces"], unit=c["unit"]))
        _invalid(fl.read)  # the failed run left no result
        with pytest.raises(capi.SfmxError):
            fl.sizes()
        with pytest.raises(capi.SfmxError):
            fl.counts()
        assert fl.device_mesh() == (-1, None, None, 0) and fl.device_surface() == (-1, None, None), name
        good_call(name)
    for p in R.BAD_PARAMS:
        _invalid(lambda: fl.run(good["verts"], good["faces"], **p))
        _invalid(fl.read)
        good_call(str(p))
    _invalid(lambda: fl.run(good["verts"], good["faces"]))  # unit has no default
    good_call("no unit")
    with pytest.raises(TypeError):
        fl.run(good["verts"], good["faces"], unit=1.0, iters=3)
    assert fl.read()["verts"].shape == (6, 3), "refused in Python, before the library: the result stays"
    for p in R.GOOD_PARAMS:
        if p["unit"] == 1.0:  # the others put this mesh beyond 2^18 units
            _case(fl, good["verts"], good["faces"], gn, "accepted", **p)
    fl.run(good["verts"], good["faces"], unit=1.0)
    _invalid(lambda: fl.read(normals=True))  # a run without normals has none to read
    assert fl.read()["faces"].shape == (6, 3), "a refused read leaves the result"
    # the limits themselves are inside
    v = good["verts"].copy()
    v[3] = (2.0 ** 18, -2.0 ** 18, 0.0)
    v[4] = (-2.0 ** 18, 2.0 ** 18, 2.0 ** 18)
    _case(fl, v, good["faces"], gn, "|q| = 2^18", unit=1.0)
    _invalid(lambda: fl.run(v * 2.0, good["faces"], unit=1.0))
    _case(fl, v * 2.0, good["faces"], gn, "|q| = 2^18 of two units", unit=2.0)
    f = good["faces"].copy()
    f[1, 1] = 4
    _case(fl, good["verts"], f, gn, "the last vertex index", unit=1.0)


def test_one_vertex_too_many(ctx):
    """2^24 - 1 vertices and one open quad: the new vertex would be number 2^24 - 1 + 1; one vertex fewer passes, and so does a
    loop of three, which adds none"""
    f = ctx.fill()
    big = np.zeros((2 ** 24 - 1, 3))
    big[:4] = np.asarray(R.hand_cases()["open-quad"]["verts"])
    quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    _invalid(lambda: f.run(big, quad, unit=1.0))
    _invalid(f.read)
    got = f.run(big[:-1], quad, unit=1.0)
    assert got == dict(ZERO, edges=5, boundary_edges=4, filled_loops=1, filled_edges=4, new_verts=1, new_faces=4)
    assert f.sizes() == (2 ** 24 - 2, 2, 2 ** 24 - 1, 6)
    got = f.run(big, quad[:1], unit=1.0)
    assert got == dict(ZERO, edges=3, boundary_edges=3, filled_loops=1, filled_edges=3, new_faces=1) and f.sizes()[2:] == (2 ** 24 - 1, 2)
    f.close()


# ---- loops at the cap --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 4, 31, 32, 33, 1024, 1025])
def test_open_tubes(fl, k):
    """two rims of k edges each, at max_edges 32 and 1 024; as built (each rim's leader is its first vertex) and relabelled"""
    v, f, nrm = R.open_tube(k)
    for cap in (32, 1024):
        for what, (vv, ff, nn) in (("tube", (v, f, nrm)), ("tube relabelled", _relabel(v, f, nrm, k))):
            ref = _case(fl, vv, ff, nn, f"{what} {k}", unit=0.01, origin=(0.5, 0.25, -1.0), max_edges=cap)
            if k <= cap:
                assert ref["filled_loops"] == 2 and ref["filled_edges"] == 2 * k and ref["new_verts"] == (0 if k == 3 else 2)
                assert R.euler(len(ref["verts"]), ref["faces"]) == 2, "closed"
                again = _case(fl, ref["verts"], ref["faces"], ref["normals"], f"{what} {k} again", unit=0.01, origin=(0.5, 0.25, -1.0), max_edges=cap)
                assert again["filled_loops"] == 0 and again["boundary_edges"] == 0
            else:
                assert R.counts(ref) == dict(ZERO, edges=6 * k - 2 * k, boundary_edges=2 * k)
    v, f, nrm = R.open_tube(k, rings=5)
    _case(fl, v, f, None, f"longer tube {k}", unit=0.01)


# ---- block and scan edges --------------------------------------------------------------------------------------------------
SIZES = [255, 256, 257, 65535, 65536, 65537, 1024 * 1024 + 1]


@pytest.mark.parametrize("k", SIZES)
def test_lone_triangles_at_block_and_scan_edges(fl, k):
    big = k > 100000
    v, f, nrm = R.lone_triangles(k)
    ref = _case(fl, v, f, None if big else nrm, f"triangles {k}", unit=0.01, max_edges=3)
    assert R.counts(ref) == dict(ZERO, edges=3 * k, boundary_edges=3 * k, filled_loops=k, filled_edges=3 * k, new_faces=k)
    assert (ref["faces"][k:] == f[:, [0, 2, 1]]).all(), "the back faces, in order"
    v2, f2, n2 = _relabel(v, f, None if big else nrm, k)
    ref = _case(fl, v2, f2, n2, f"triangles {k} relabelled", unit=0.01)
    assert ref["new_faces"] == k and (np.diff(ref["faces"][k:, 0]) > 0).all() and (ref["faces"][k:, 0] != f2[:, 0]).any()


@pytest.mark.parametrize("k", SIZES)
def test_open_quads_at_block_and_scan_edges(fl, k):
    big = k > 100000
    v, f, nrm = R.open_quads(k)
    ref = _case(fl, v, f, None if big else nrm, f"quads {k}", unit=0.01, max_edges=4)
    assert R.counts(ref) == dict(ZERO, edges=5 * k, boundary_edges=4 * k, filled_loops=k, filled_edges=4 * k, new_verts=k, new_faces=4 * k)
    assert (ref["faces"][2 * k::4, 2] == 4 * k + np.arange(k)).all(), "the new vertices, numbered in loop order"
    v2, f2, n2 = _relabel(v, f, nrm, k)
    ref = _case(fl, v2, f2, None if big else n2, f"quads {k} relabelled", unit=0.01)
    lead = ref["faces"][2 * k::4, 0]
    assert ref["new_verts"] == k and (np.diff(lead) > 0).all() and (lead != f2[::2].min(1)).any(), "the leader is the smallest of its loop's own vertices"
    if not big:
        assert _case(fl, v, f, nrm, f"quads {k} below the cap", unit=0.01, max_edges=3)["filled_loops"] == 0


# ---- random soup -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["as-is", "faces-permuted", "faces-rotated", "vertices-permuted"])
def test_random_soup(fl, order):
    v, f, nrm = LR.soup()
    rng = np.random.default_rng(8)
    if order == "faces-permuted":
        f = f[rng.permutation(len(f))]
    elif order == "faces-rotated":
        rot = rng.integers(0, 3, len(f))
        f = np.ascontiguousarray(np.stack([f[np.arange(len(f)), (rot + j) % 3] for j in range(3)], 1))
    elif order == "vertices-permuted":
        v, f, nrm = _relabel(v, f, nrm, 8)
    for cap in (3, 32, 1024):
        ref = _case(fl, v, f, nrm, "soup", unit=0.01, origin=(0.1, -0.2, 0.3), max_edges=cap)
    assert ref["irregular_edges"] >= 1 and ref["complex_vertices"] > 1000
    # a soup with holes that do get filled: quads, triangles and tubes among the random faces' vertices
    parts = [(v, f, nrm), R.open_quads(300), R.lone_triangles(200), R.open_tube(40), R.open_tube(7, rings=3)]
    off = np.cumsum([0] + [len(p[0]) for p in parts[:-1]])
    mv, mn = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
    mf = np.concatenate([p[1] + o for p, o in zip(parts, off)]).astype(np.int32)
    mv, mf, mn = _relabel(mv, mf, mn, 9)
    ref = _case(fl, mv, mf, mn, "soup with holes", unit=0.01, max_edges=32)
    assert ref["filled_loops"] >= 300 + 200 + 2 and ref["new_verts"] >= 302
    assert _case(fl, mv, mf, mn, "soup with holes", unit=0.01, max_edges=64)["filled_loops"] == ref["filled_loops"] + 2


# ---- feeds and state -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ball(ctx):
    """eight small noisy views of the sphere in a volume: a surface with islands and holes"""
    views = CR.sphere8()[:8]
    fu = ctx.fusion(**CR.SPHERE26_VOL)
    for cam, d16 in views:
        fu.add_view(cam, d16)
    yield fu, views
    fu.close()


def _bytes(r):
    return r["verts"].tobytes() + r["faces"].tobytes() + (r["normals"].tobytes() if r.get("normals") is not None else b"")


def test_feeding_paths_same_bytes(ctx, ball):
    import torch
    fu, _ = ball
    vol = CR.SPHERE26_VOL
    kw = dict(unit=vol["voxel"], origin=vol["origin"], max_edges=64)
    v, f, nrm = fu.extract_normals()
    ref = R.fill(v, f, nrm, **kw)
    assert ref["filled_loops"] > 0 and ref["boundary_edges"] > ref["filled_edges"], "precondition: holes, and a rim that stays"
    s, c = ctx.fill(), ctx.clean()
    _check(s, s.fusion(fu, **kw), ref, "sfmx_fill_fusion")
    resident = _bytes(s.read(normals=True))
    _check(s, s.run(v, f, nrm, **kw), ref, "host pointers")
    host = _bytes(s.read(normals=True))
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, f, nrm))
    torch.cuda.synchronize()
    _check(s, s.run(tv.data_ptr(), tf.data_ptr(), tn.data_ptr(), n=len(v), m=len(f), **kw), ref, "device pointers")
    dev = _bytes(s.read(normals=True))
    n2, pv, pf, m2 = s.device_mesh()
    assert pv not in (tv.data_ptr(), None) and pf not in (tf.data_ptr(), None) and s.device_surface()[1] == pv, "the object's own arrays"
    assert resident == host == dev == _bytes(ref)
    # without normals: device pointers, and a plain extract
    ref0 = R.fill(v, f, None, **kw)
    _check(s, s.run(tv.data_ptr(), tf.data_ptr(), n=len(v), m=len(f), **kw), ref0, "device pointers, no normals")
    # the filled mesh from the device into a second object: nothing left to fill
    s2 = ctx.fill()
    _check(s, s.run(v, f, nrm, **kw), ref, "host pointers again")
    n2, pv, pf, m2 = s.device_mesh()
    again = R.fill(ref["verts"], ref["faces"], ref["normals"], **kw)
    _check(s2, s2.run(pv, pf, s.device_surface()[2], n=n2, m=m2, **kw), again, "a second run")
    assert again["filled_loops"] == 0 and _bytes(s2.read(normals=True)) == _bytes(ref)
    s2.close()
    # the cleaned surface, from the clean object
    lref = LR.clean(v, f, nrm)
    assert c.fusion(fu) == LR.counts(lref) and lref["n_faces"] < len(f)
    cref = R.fill(lref["verts"], lref["faces"], lref["normals"], **kw)
    _check(s, s.clean(c, **kw), cref, "sfmx_fill_clean")
    assert _bytes(s.read(normals=True)) != resident
    v2, f2 = fu.extract()
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    _check(s, s.fusion(fu, **kw), ref0, "sfmx_fill_fusion after a plain extract")
    s.close()
    c.close()


def test_one_object_large_small_large(ctx):
    s = ctx.fill()
    big, small = R.open_quads(40000), R.open_tube(5)
    for what, (v, f, nrm) in (("large", big), ("small", small), ("large again", big)):
        _case(s, v, f, nrm, what, unit=0.01)
        assert s.last_us() == 0.0
    ctx.set_timing(True)
    _case(s, *big, "timed", unit=0.01)
    assert s.last_us() > 0.0
    ctx.set_timing(False)
    s.close()


def test_state_rules(ctx, ball):
    _, views = ball
    vol = CR.SPHERE26_VOL
    kw = dict(unit=vol["voxel"], origin=vol["origin"])
    s, c, fu = ctx.fill(), ctx.clean(), ctx.fusion(**vol)
    _invalid(s.read)  # before a run
    for fn in (s.sizes, s.counts):
        with pytest.raises(capi.SfmxError):
            fn()
    assert s.device_surface() == (-1, None, None) and s.device_mesh() == (-1, None, None, 0)
    _invalid(lambda: s.fusion(fu, **kw))  # nothing extracted yet
    _invalid(lambda: s.clean(c, **kw))  # nothing cleaned yet
    fu.add_view(*views[0])
    assert fu.counts()[1] > 0
    _invalid(lambda: s.fusion(fu, **kw))  # counts alone leave no arrays
    v, f = fu.extract()
    _check(s, s.fusion(fu, **kw), R.fill(v, f, **kw), "after extract")
    fu.add_view(*views[1])
    fu.integrate()
    _invalid(lambda: s.fusion(fu, **kw))  # the volume changed
    _invalid(s.read)
    v, f, nrm = fu.extract_normals()
    ref = R.fill(v, f, nrm, **kw)
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
    assert s.fusion(fu, **kw) == ZERO
    r = s.read()
    assert r["verts"].shape == (0, 3) and r["faces"].shape == (0, 3) and s.sizes() == (0, 0, 0, 0)
    for o in (s, c, fu):
        o.close()


# ---- ring-6 and the stages behind the filling --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring6():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    return dict(images=images, K=K, poses=poses, pairs=pairs, vol=CR.RING6_VOL)


def test_ring6_fill_smooth_then_simplify_shade_and_distances(ctx, ring6):
    """ring-6 filtered, fused, cleaned, filled and smoothed on the device: NumPy's bytes and the integers of DESIGN.md 22's
    calibration; then simplify, shade and the distance stage fed from the fill object's device arrays, equal to the host feed"""
    vol = ring6["vol"]
    kw = dict(unit=vol["voxel"], origin=vol["origin"])
    h, w = ring6["images"].shape[1:]
    st, cs, fu, sh = ctx.stereo(w, h, num_disparities=64), ctx.consist(), ctx.fusion(**vol), ctx.shade()
    c, s, sm, sp, sd = ctx.clean(), ctx.fill(), ctx.smooth(), ctx.simplify(), ctx.sdist()
    for a, b in ring6["pairs"]:
        r = pipe.stereo_rectify(ring6["K"], ring6["poses"][a], ring6["poses"][b], w, h)
        il, ir = (ring6["images"][b], ring6["images"][a]) if r["swapped"] else (ring6["images"][a], ring6["images"][b])
        st.disparity(il, ir, r["H_l"], r["H_r"])
        cs.add_stereo_view(r, st)
        sh.add_stereo_view(r, st)
    cs.filter()
    for i in range(len(ring6["pairs"])):
        fu.add_consist_view(cs, i)
    v, f, nrm = fu.extract_normals()
    assert (len(v), len(f)) == (7552, 13622), "the surface of DESIGN.md 15"
    # uncleaned, at the three caps of the calibration
    for cap, row in RING_ROWS.items():
        ref = R.fill(v, f, nrm, max_edges=cap, **kw)
        _check(s, s.fusion(fu, max_edges=cap, **kw), ref, f"ring-6, max_edges {cap}")
        assert R.counts(ref) == dict(RING_INPUT, filled_loops=row[0], filled_edges=row[1], new_verts=row[0], new_faces=row[1])
        n, pv, pf, m = s.device_mesh()
        got = sm.run(pv, pf, n=n, m=m, **kw)
        sref = MR.smooth(ref["verts"], ref["faces"], **kw)
        assert got == MR.counts(sref) and got["pinned"] == row[2] and sm.read()["verts"].tobytes() == sref["verts"].tobytes()
    # cleaned, the pipeline's order
    lref = LR.clean(v, f, nrm)
    assert c.fusion(fu) == LR.counts(lref)
    ref = R.fill(lref["verts"], lref["faces"], lref["normals"], **kw)
    ctx.set_timing(True)
    _check(s, s.clean(c, **kw), ref, "ring-6 cleaned")
    print("ring-6 cleaned: %s; %.1f us" % (R.counts(ref), s.last_us()))
    ctx.set_timing(False)
    assert R.counts(ref) == RING_CLEANED
    n, pv, pf, m = s.device_mesh()
    pn = s.device_surface()[2]
    assert n == len(lref["verts"]) + 26 and n != c.device_surface()[0] and pn not in (None, c.device_surface()[2])
    got = sm.run(pv, pf, n=n, m=m, **kw)
    sref = MR.smooth(ref["verts"], ref["faces"], **kw)
    assert got == MR.counts(sref) and got["pinned"] == RING_CLEANED_PINNED
    host_chain = ctx.smooth()
    assert host_chain.run(ref["verts"], ref["faces"], **kw) == got
    assert sm.read()["verts"].tobytes() == host_chain.read()["verts"].tobytes() == sref["verts"].tobytes()
    host_chain.close()
    # simplify, from the fill object's device arrays and from the host
    cell = 2 * vol["voxel"]
    dev = sp.run(pv, pf, pn, n=n, m=m, cell=cell, origin=vol["origin"])
    rd = sp.read(normals=True)
    host = sp.run(ref["verts"], ref["faces"], ref["normals"], cell=cell, origin=vol["origin"])
    rh = sp.read(normals=True)
    pref = PR.simplify(ref["verts"], ref["faces"], ref["normals"], cell, vol["origin"])
    assert dev == host == PR.counts(pref) and 0 < pref["n_faces"] < m
    for k in PR.ARRAYS + ("normals",):
        assert rd[k].tobytes() == rh[k].tobytes() == np.asarray(pref[k]).tobytes(), k
    # shade: the new vertices have normals of their own and are seen
    tol = FR.resolve(vol["voxel"])
    g_dev, c_dev = sh.shade(pv, pn, tol, n=n)
    g_host, c_host = sh.shade(ref["verts"], ref["normals"], tol)
    assert g_dev.tobytes() == g_host.tobytes() and c_dev.tobytes() == c_host.tobytes() and (c_host[-26:] > 0).any()
    # the filled mesh as the target and as the queries of the distance stage
    G = synth.shell_mesh(3)
    d_max = 4 * vol["voxel"]
    sd.set_target(pv, pf, d_max, nv=n, m=m)
    a = sd.query(G[0])
    sd.set_target(ref["verts"], ref["faces"], d_max)
    b = sd.query(G[0])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (b[1] >= 0).any()
    sd.set_target(*G, d_max)
    a, b = sd.query(pv, n=n), sd.query(ref["verts"])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (b[1] >= 0).any()
    for o in (st, cs, fu, sh, c, s, sm, sp, sd):
        o.close()


# ---- pipeline --------------------------------------------------------------------------------------------------------------
def _parse_ply(path):
    lines = open(path).read().split("\n")
    end = lines.index("end_header")
    nv = int([x for x in lines[:end] if x.startswith("element vertex")][0].split()[2])
    nf = int([x for x in lines[:end] if x.startswith("element face")][0].split()[2])
    vert = np.array([x.split() for x in lines[end + 1:end + 1 + nv]], np.float64)
    face = np.array([x.split() for x in lines[end + 1 + nv:end + 1 + nv + nf]], np.int64)
    assert lines[end + 1 + nv + nf:] == [""]
    return lines[:end], vert, face


def test_host_fuse_fill(ctx, ring6, tmp_path):
    vol = ring6["vol"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain.ply", "false.ply", "on.ply"))
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    m1 = pipe.fuse(*args, num_disparities=64, ply_path=p1, fill=False)
    assert set(m0) == set(m1) == {"verts", "faces", "views", "warn"} and m0["warn"] == m1["warn"] and m0["views"] == m1["views"]
    assert m0["verts"].tobytes() == m1["verts"].tobytes() and m0["faces"].tobytes() == m1["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read(), "fill=False is the call without the argument"
    m = pipe.fuse(*args, num_disparities=64, ply_path=p2, fill=True)
    assert set(m) == {"verts", "faces", "views", "warn", "fill"} and m["views"] == 6 and m["warn"] is None
    ref = R.fill(m0["verts"], m0["faces"], unit=vol["voxel"], origin=vol["origin"])  # the defaults: the voxel, the volume's origin, 32
    assert m["fill"] == R.counts(ref) and ref["new_verts"] > 10
    assert m["verts"].tobytes() == ref["verts"].tobytes() and m["faces"].tobytes() == ref["faces"].tobytes()
    head, pv, pf = _parse_ply(p2)
    assert len(pv) == len(ref["verts"]) and (pf[:, 0] == 3).all() and (pf[:, 1:] == ref["faces"]).all()
    assert np.allclose(pv, ref["verts"], rtol=1e-5, atol=1e-9)
    # the manual chain, with other parameters
    h, w = ring6["images"].shape[1:]
    st, fu, s = ctx.stereo(w, h, num_disparities=64), ctx.fusion(**vol), ctx.fill()
    for a, b in ring6["pairs"]:
        r = pipe.stereo_rectify(ring6["K"], ring6["poses"][a], ring6["poses"][b], w, h)
        il, ir = (ring6["images"][b], ring6["images"][a]) if r["swapped"] else (ring6["images"][a], ring6["images"][b])
        st.disparity(il, ir, r["H_l"], r["H_r"])
        fu.add_stereo_view(r, st)
    v, f = fu.extract()
    assert v.tobytes() == m0["verts"].tobytes()
    okw = dict(max_edges=6, unit=0.37 * vol["voxel"], origin=(0.001, -0.002, 0.003))
    got = s.fusion(fu, **okw)
    chain = s.read()
    for o in (st, fu, s):
        o.close()
    m3 = pipe.fuse(*args, num_disparities=64, fill=okw)
    ref3 = R.fill(m0["verts"], m0["faces"], **okw)
    assert m3["verts"].tobytes() == chain["verts"].tobytes() == ref3["verts"].tobytes() != ref["verts"].tobytes()
    assert m3["faces"].tobytes() == chain["faces"].tobytes() == ref3["faces"].tobytes()
    assert m3["fill"] == got == R.counts(ref3) and 0 < got["filled_loops"] < ref["filled_loops"]
    # no pairs, bad parameters
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, fill=True)
    assert empty["verts"].shape == (0, 3) and empty["fill"] == ZERO
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, fill=dict(cell=1.0))
    for bad in (dict(unit=0.0), dict(max_edges=2), dict(max_edges=1025), dict(origin=(0.0, float("inf"), 0.0))):
        with pytest.raises(capi.SfmxError):
            pipe.fuse(*args, num_disparities=64, fill=bad)


def test_host_fuse_fill_with_every_other_stage(ctx, ring6, tmp_path):
    """consistency, clean, appearance, smooth, simplify and evaluate in four combinations: the final mesh is the restatements' of
    the stage-before mesh filled, then smoothed, then simplified with the fill's normals; its grey is the shading of the final
    vertices and the evaluation that of the final mesh"""
    vol = ring6["vol"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    ply = str(tmp_path / "all.ply")
    G = synth.shell_mesh(3)
    ekw = dict(gt_verts=G[0], gt_faces=G[1], d_max=4 * vol["voxel"], tau=vol["voxel"])
    kw = dict(unit=vol["voxel"], origin=vol["origin"])
    h, w = ring6["images"].shape[1:]
    sh, st = ctx.shade(), ctx.stereo(w, h, num_disparities=64)
    for a, b in ring6["pairs"]:
        r = pipe.stereo_rectify(ring6["K"], ring6["poses"][a], ring6["poses"][b], w, h)
        il, ir = (ring6["images"][b], ring6["images"][a]) if r["swapped"] else (ring6["images"][a], ring6["images"][b])
        st.disparity(il, ir, r["H_l"], r["H_r"])
        sh.add_stereo_view(r, st)
    for cons, cl, smo, simp in ((True, True, True, True), (True, True, True, False), (True, False, False, False), (False, False, False, True)):
        m0 = pipe.fuse(*args, num_disparities=64, consistency=cons, appearance=True, clean=cl)
        m = pipe.fuse(*args, num_disparities=64, consistency=cons, appearance=True, clean=cl, simplify=simp,
                      smooth=dict(iters=4) if smo else False, fill=dict(max_edges=32), evaluate=ekw, ply_path=ply)
        want = {"verts", "faces", "views", "warn", "normals", "grey", "vertex_views", "fill", "evaluation"}
        assert set(m) == want | ({"consistency"} if cons else set()) | ({"clean"} if cl else set()) | ({"simplify"} if simp else set()) | (
            {"smooth"} if smo else set())
        fref = R.fill(m0["verts"], m0["faces"], m0["normals"], **kw)
        assert m["fill"] == R.counts(fref) and fref["new_verts"] > 10
        if cons:
            assert m["fill"] == (RING_CLEANED if cl else dict(RING_INPUT, filled_loops=50, filled_edges=466, new_verts=50, new_faces=466))
        ref = dict(verts=fref["verts"], faces=fref["faces"], normals=fref["normals"])
        if smo:
            sref = MR.smooth(fref["verts"], fref["faces"], iters=4, **kw)
            assert m["smooth"] == MR.counts(sref) and m["smooth"]["boundary_edges"] == fref["boundary_edges"] - fref["filled_edges"]
            if cons and cl:
                assert m["smooth"]["pinned"] == RING_CLEANED_PINNED
            ref["verts"] = sref["verts"]
        if simp:
            nb = (len(ref["verts"]), len(ref["faces"]))
            ref = PR.simplify(ref["verts"], ref["faces"], ref["normals"], 2.0 * vol["voxel"], vol["origin"])
            assert 0 < ref["n_faces"] < nb[1] and (m["simplify"]["verts_before"], m["simplify"]["faces_before"]) == nb
            assert m["simplify"]["clusters"] == ref["clusters"]
        for k in ("verts", "faces", "normals"):
            assert m[k].tobytes() == np.asarray(ref[k]).tobytes(), (k, cons, cl, smo, simp)
        if cl:
            assert m["clean"] == m0["clean"]
        if cons:
            assert m["consistency"] == m0["consistency"]
        assert m["evaluation"] == pipe.surface_eval(ctx, m["verts"], m["faces"], *G, d_max=ekw["d_max"], tau=ekw["tau"])
        g1, c1 = sh.shade(m["verts"], m["normals"], FR.resolve(vol["voxel"]))
        assert m["grey"].tobytes() == g1.tobytes() and m["vertex_views"].tobytes() == c1.tobytes()
        assert (c1 > 0).any() and len(np.unique(g1)) > 10
        if not simp:  # the PLY parsed back: the new vertices carry normals and colours
            head, pv, pf = _parse_ply(ply)
            k = fref["new_verts"]
            assert "property uchar red" in head and "property float nx" in head and pv.shape == (len(ref["verts"]), 9)
            assert (pf[:, 1:] == ref["faces"]).all() and (pv[:, 6] == m["grey"]).all()
            assert np.allclose(pv[-k:, 3:6], fref["normals"][-k:], atol=1e-6) and (np.abs(np.linalg.norm(pv[-k:, 3:6], axis=1) - 1.0) < 1e-5).all()
            assert (pv[-k:, 6] == m["grey"][-k:]).all() and (m["vertex_views"][-k:] > 0).any()
    sh.close()
    st.close()
    # a surface with nothing left: the cleaning removes every component, the filling has nothing to do
    none = str(tmp_path / "none.ply")
    m5 = pipe.fuse(*args, num_disparities=64, clean=dict(min_faces=10 ** 8), fill=True, smooth=True, ply_path=none)
    assert m5["verts"].shape == (0, 3) and m5["faces"].shape == (0, 3) and "no faces" in m5["warn"] and not os.path.exists(none)
    assert m5["fill"] == ZERO and m5["smooth"] == dict(edges=0, boundary_edges=0, irregular_edges=0, pinned=0, isolated=0)


def test_pipeline_run_fill(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    plain, filled = str(tmp_path / "plain"), str(tmp_path / "filled")
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
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, filled, fusion=dict(fz, fill=dict(max_edges=64)))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(filled, "X")
    assert sorted(os.listdir(filled)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m1) == {"verts", "faces", "views", "warn"} and set(m) == set(m1) | {"fill"} and len(m1["faces"]) > 0
    ref = R.fill(m1["verts"], m1["faces"], unit=voxel, origin=tuple(lo), max_edges=64)
    print("run: %s" % R.counts(ref))
    assert m["verts"].tobytes() == ref["verts"].tobytes() and m["faces"].tobytes() == ref["faces"].tobytes()
    assert m["fill"] == R.counts(ref)
    assert open(os.path.join(filled, "templeRing_mesh_fused.ply")).read().startswith(
        "ply\nformat ascii 1.0\nelement vertex %d\n" % len(ref["verts"]))
