"""GPU suite: exact vertex clustering of a triangle mesh on the device.  sfmx_simplify_* gives the output vertices, normals and
faces, vert_dst, face_src, members and the five counts byte for byte against the NumPy restatement (tests/simplify_ref.py): hand
meshes, every invalid input, the block and scan-level edges of cells, clusters and faces, the two hot words, a random soup from
fine to coarse and permuted, every way of feeding a mesh, the state rules, the sphere-26 surfaces with the exact integers of
DESIGN.md 20, the distance stage fed from the device mesh, and pipeline.fuse / pipeline.run."""
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
from test_simplify_cpu import SPHERE_ROWS

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
def sp(ctx):
    """one object for the whole module: its buffers grow and shrink with the cases"""
    s = ctx.simplify()
    yield s
    s.close()


def _keys(normals):
    return PR.ARRAYS + (("normals",) if normals else ())


def _bytes(r, normals):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in _keys(normals))


def _check(sp, got, ref, what, normals=False):
    """the counts a run returned and everything read() gives, against the restatement"""
    assert got == PR.counts(ref), what + ": counts"
    assert sp.sizes()[2:] == (ref["n_verts"], ref["n_faces"])
    r = sp.read(normals=normals)
    for k in _keys(normals):
        want = np.asarray(ref[k])
        assert r[k].dtype == want.dtype and r[k].shape == want.shape, f"{what}: {k} {r[k].shape} {want.shape}"
        assert r[k].tobytes() == want.tobytes(), f"{what}: {k}"
    return r


def _case(sp, v, f, what, normals=None, cell=1.0, origin=(0.0, 0.0, 0.0)):
    ref = PR.simplify(v, f, normals, cell, origin)
    _check(sp, sp.run(v, f, normals, cell=cell, origin=origin), ref, f"{what} cell={cell}", normals is not None)
    return ref


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


# ---- hand meshes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PR.hand_cases()))
def test_hand_meshes(sp, name):
    c = PR.hand_cases()[name]
    v, f = np.asarray(c["verts"], np.float64).reshape(-1, 3), np.asarray(c["faces"], np.int32).reshape(-1, 3)
    origin = c.get("origin", (0.0, 0.0, 0.0))
    ref = _case(sp, v, f, name, None, c["cell"], origin)
    nrm = np.asarray(c["normals"], np.float64) if "normals" in c else PR.unit(v + 0.125) if len(v) else np.zeros((0, 3))
    ref_n = _case(sp, v, f, name + " with normals", nrm, c["cell"], origin)
    assert ref_n["verts"].tobytes() == ref["verts"].tobytes() and ref_n["faces"].tobytes() == ref["faces"].tobytes()
    if name == "same-orientation":
        assert ref["face_src"].tolist() == [0] and ref["duplicates"] == 2
    if name == "inside-one-cell":
        assert ref["n_verts"] == 0 and sp.device_surface()[0] == 0 and sp.device_mesh()[0] == 0


def test_every_invalid_input_then_a_good_call(sp):
    bad, good = PR.invalid_inputs()
    gref = PR.simplify(**good)
    for name, c in bad:
        _invalid(lambda: sp.run(c["verts"], c["faces"], c["normals"], cell=c["cell"]))
        _invalid(sp.read)  # the failed run left no result
        with pytest.raises(capi.SfmxError):
            sp.sizes()
        with pytest.raises(capi.SfmxError):
            sp.counts()
        assert sp.device_surface()[0] == -1 and sp.device_mesh()[0] == -1, name
        _check(sp, sp.run(good["verts"], good["faces"], good["normals"], cell=1.0), gref, "after " + name, normals=True)
    _invalid(lambda: sp.run(np.zeros((0, 3)), np.array([[0, 0, 0]], np.int32), cell=1.0))  # n = 0: every index is out of range
    for p in PR.BAD_PARAMS:
        _invalid(lambda: sp.run(good["verts"], good["faces"], **p))
        _invalid(sp.read)
        _check(sp, sp.run(good["verts"], good["faces"], cell=1.0), PR.simplify(good["verts"], good["faces"], None, 1.0), f"after {p}")
    _invalid(lambda: sp.run(good["verts"], good["faces"]))  # cell has no default
    with pytest.raises(TypeError):
        sp.run(good["verts"], good["faces"], cell=1.0, grid=3)
    sp.run(good["verts"], good["faces"], cell=1.0)
    with pytest.raises(TypeError):
        sp.run(good["verts"], good["faces"], cell=1.0, grid=3)
    assert sp.read()["faces"].shape == (2, 3), "refused in Python, before the library: the result stays"
    # the limits themselves are inside
    v = good["verts"].copy()
    v[1] = (511.5, 511.5, 511.5)  # a box of exactly 2^27 cells
    _case(sp, v, good["faces"], "512^3 cells")
    v[1] = (2.0 ** 30, 0.5, 0.5)  # the largest cell index; the box is then too long
    _invalid(lambda: sp.run(v, good["faces"], cell=1.0))
    _case(sp, np.array([[2.0 ** 30, -2.0 ** 30, 0.5], [2.0 ** 30 - 1, -2.0 ** 30, 1.5], [2.0 ** 30, 1 - 2.0 ** 30, 0.5]]), [[0, 1, 2]],
          "cell indices of +-2^30")
    nr = good["normals"].copy()
    nr[0] = (4.0, -4.0, 0.0)
    _case(sp, good["verts"], good["faces"], "normal components of +-4", nr)


# ---- block and scan edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [255, 256, 257, 1023, 1024, 1025, 1024 * 1024 + 1])
def test_cells_and_clusters_at_block_and_scan_edges(sp, k):
    """a row of k cells, all occupied (k clusters; 1024^2 + 1 is the third scan level), then the same box with 16 of them
    occupied"""
    v, f = PR.line_of_cells(k)
    ref = _case(sp, v, f, f"k={k} full", PR.unit(v))
    assert ref["clusters"] == k and ref["n_faces"] == k // 3 and ref["n_verts"] == 3 * (k // 3)
    v, f = PR.grid_triangles((k, 1, 1), 5, stride=7)
    ref = _case(sp, v, f, f"k={k} sparse")
    assert ref["clusters"] == 16 and ref["n_faces"] == 5
    if k > 2000:
        a, b = (17, 61681) if k == 1024 * 1024 + 1 else (0, 0)
        assert a * b == k
        v, f = PR.grid_triangles((a, b, 1), 1000, stride=1000)
        assert _case(sp, v, f, f"{a} x {b} cells")["n_faces"] == 1000
    elif k in (1024, 1025):
        dims = (32, 8, 4) if k == 1024 else (41, 5, 5)
        v, f = PR.grid_triangles(dims, 100, stride=9, cell=0.25)
        assert _case(sp, v, f, f"{dims} cells", cell=0.25)["n_faces"] == 100


@pytest.mark.parametrize("m", [255, 256, 257, 1023, 1024, 1025, 1024 * 1024 + 1])
def test_disjoint_triangles_at_block_and_scan_edges(sp, m):
    """m triangles with every corner in a cell of its own: nothing degenerate, nothing duplicated, 3 m clusters"""
    v, f = PR.grid_triangles((3 * m + 3, 1, 1) if m < 2000 else (1024, 3 * 1024 + 3, 1), m, stride=3)
    ref = _case(sp, v, f, f"m={m}")
    assert ref["n_faces"] == m and ref["n_verts"] == 3 * m and ref["clusters"] in (3 * m + 1, 3 * m + 2)


# ---- the two hot words -----------------------------------------------------------------------------------------------------
def test_65536_vertices_in_one_cell(sp):
    v, f, nrm = PR.hot_vertex()
    ref = _case(sp, v, f, "hot cell", nrm)
    assert ref["clusters"] == 4 and ref["members"].tolist() == [65536, 1, 1, 1] and ref["n_faces"] == 3 and ref["duplicates"] == 598
    # in fusion order the crowd is one run per wave; scattered between other cells it is not
    v2, f2, n2, _ = PR.permute_vertices(*PR.hot_vertex(4096), 5)
    far = np.random.default_rng(6).random((4099, 3)) + np.array([3.0, 0.0, 0.0])
    v2, n2 = np.stack([v2, far], 1).reshape(-1, 3), np.stack([n2, n2], 1).reshape(-1, 3)  # every other vertex elsewhere
    _case(sp, v2, (2 * f2).astype(np.int32), "hot cell, interleaved", n2)


def test_65536_faces_with_one_triple(sp):
    v, f = PR.hot_triple()
    ref = _case(sp, v, f, "hot triple")
    assert ref["n_faces"] == 1 and ref["face_src"].tolist() == [0] and ref["duplicates"] == 65535 and ref["members"].tolist() == [65536] * 3
    ref = _case(sp, v, f[::-1].copy(), "hot triple, reversed order")
    assert ref["face_src"].tolist() == [0]


# ---- random soup -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soup():
    v, f, nrm = LR.soup()
    return v, f, PR.unit(nrm)


@pytest.mark.parametrize("order", ["as-is", "vertices-permuted", "faces-permuted"])
def test_random_soup_from_fine_to_coarse(sp, soup, order):
    v, f, nrm = soup
    if order == "vertices-permuted":
        v, f, nrm, _ = PR.permute_vertices(v, f, nrm, 8)
    elif order == "faces-permuted":
        f = f[np.random.default_rng(8).permutation(len(f))]
    refs = [_case(sp, v, f, "soup", nrm, cell, (0.1, -0.2, 0.3)) for cell in (0.02, 0.1, 0.3, 1.0)]
    assert refs[0]["clusters"] > 19900 and 100 < refs[3]["clusters"] < 1000 and refs[3]["duplicates"] > 1000
    _case(sp, v, f, "soup without normals", None, 0.3, (0.1, -0.2, 0.3))
    if order == "as-is":
        sv, sf, _ = LR.soup(2000, 1500, 9)
        assert _case(sp, sv, sf, "sparse soup", None, 0.02)["clusters"] == 2000, "every vertex alone"


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


def test_feeding_paths_same_bytes(ctx, ball):
    import torch
    fu, _ = ball
    vol = CR.SPHERE26_VOL
    kw = dict(cell=2 * vol["voxel"], origin=vol["origin"])
    v, f, nrm = fu.extract_normals()
    ref = PR.simplify(v, f, nrm, **kw)
    assert 0 < ref["n_faces"] < len(f) and ref["degenerate"] > 0, "precondition: simplification acts on this surface"
    s, c = ctx.simplify(), ctx.clean()
    _check(s, s.fusion(fu, **kw), ref, "sfmx_simplify_fusion", normals=True)
    resident = _bytes(s.read(normals=True), True)
    n2, pv, pn = s.device_surface()
    assert n2 == ref["n_verts"] and pv and pn and s.device_mesh()[::3] == (ref["n_verts"], ref["n_faces"])
    _check(s, s.run(v, f, nrm, **kw), ref, "host pointers", normals=True)
    host = _bytes(s.read(normals=True), True)
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, f, nrm))
    torch.cuda.synchronize()
    _check(s, s.run(tv.data_ptr(), tf.data_ptr(), tn.data_ptr(), n=len(v), m=len(f), **kw), ref, "device pointers", normals=True)
    dev = _bytes(s.read(normals=True), True)
    assert resident == host == dev == _bytes(ref, True)
    # the cleaned surface, from the clean object
    lref = LR.clean(v, f, nrm)
    assert c.fusion(fu) == LR.counts(lref) and lref["n_faces"] < len(f)
    cref = PR.simplify(lref["verts"], lref["faces"], lref["normals"], **kw)
    _check(s, s.clean(c, **kw), cref, "sfmx_simplify_clean", normals=True)
    assert _bytes(s.read(normals=True), True) != resident, "another input, another mesh"
    # a plain extract leaves the same surface without normals
    v2, f2 = fu.extract()
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    _check(s, s.fusion(fu, **kw), PR.simplify(v, f, None, **kw), "sfmx_simplify_fusion after a plain extract")
    assert s.device_surface()[2] is None
    c.fusion(fu)
    _check(s, s.clean(c, **kw), PR.simplify(lref["verts"], lref["faces"], None, **kw), "sfmx_simplify_clean without normals")
    s.close()
    c.close()


def test_one_object_large_small_large(ctx):
    s = ctx.simplify()
    big, small = PR.grid_triangles((400, 400, 1), 40000, stride=3), PR.grid_triangles((30, 1, 1), 7, stride=3)
    for what, (v, f) in (("large", big), ("small", small), ("large again", big)):
        _case(s, v, f, what, PR.unit(v + 1.0), cell=2.5)
        assert s.last_us() == 0.0
    ctx.set_timing(True)
    _case(s, *big, "timed")
    assert s.last_us() > 0.0
    ctx.set_timing(False)
    s.close()


def test_state_rules(ctx, ball):
    _, views = ball
    vol = CR.SPHERE26_VOL
    kw = dict(cell=3 * vol["voxel"], origin=vol["origin"])
    s, c, fu = ctx.simplify(), ctx.clean(), ctx.fusion(**vol)
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
    ref = PR.simplify(v, f, None, **kw)
    _check(s, s.fusion(fu, **kw), ref, "after extract")
    assert s.sizes() == (len(v), len(f), ref["n_verts"], ref["n_faces"])
    fu.add_view(*views[1])
    fu.integrate()
    _invalid(lambda: s.fusion(fu, **kw))  # the volume changed
    _invalid(s.read)
    v, f, nrm = fu.extract_normals()
    ref = PR.simplify(v, f, nrm, **kw)
    _check(s, s.fusion(fu, **kw), ref, "after extract_normals", normals=True)
    _invalid(lambda: s.fusion(fu, cell=0.0))  # refused for its parameters: no result left
    _invalid(s.read)
    assert s.device_surface()[0] == -1
    _check(s, s.fusion(fu, **kw), ref, "after a refused call", normals=True)
    c.fusion(fu)
    _invalid(lambda: c.fusion(fu, min_permille=1001))  # the clean object lost its result
    _invalid(lambda: s.clean(c, **kw))
    _invalid(s.read)
    fu.reset()
    _invalid(lambda: s.fusion(fu, **kw))  # after a reset
    v0, f0 = fu.extract()  # an empty volume: a current surface without faces
    assert len(f0) == 0
    assert s.fusion(fu, **kw) == dict(clusters=0, degenerate=0, duplicates=0, n_verts=0, n_faces=0)
    r = s.read(normals=True)
    assert r["verts"].shape == (0, 3) and r["vert_dst"].shape == (0,)
    for o in (s, c, fu):
        o.close()


# ---- sphere-26 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True])
def test_sphere26_on_the_device(ctx, noisy):
    """all 26 maps fused, cleaned and simplified on the device: NumPy's bytes; on the clean sphere (which cleaning leaves as it
    is) the exact integers of DESIGN.md 20, and the distance stage fed from the device mesh equals the host-array feed"""
    views, _ = CR.sphere26(noisy)
    vol = CR.SPHERE26_VOL
    fu, c, s, sd = ctx.fusion(**vol), ctx.clean(), ctx.simplify(), ctx.sdist()
    for cam, d16 in views:
        fu.add_view(cam, d16)
    v, f, nrm = fu.extract_normals()
    lref = LR.clean(v, f, nrm)
    assert c.fusion(fu) == LR.counts(lref)
    assert (lref["n_faces"] == len(f)) == (not noisy)
    for (factor, shift), (ints, _) in SPHERE_ROWS.items():
        cell = factor * vol["voxel"]
        origin = tuple(o + shift * cell for o in vol["origin"])
        ref = PR.simplify(lref["verts"], lref["faces"], lref["normals"], cell, origin)
        r = _check(s, s.clean(c, cell=cell, origin=origin), ref, f"sphere-26 {factor} {shift}", normals=True)
        print("sphere-26%s, %d voxels, shift %.2f: %s, max members %d; %.1f us"
              % (" noisy" if noisy else "", factor, shift, PR.counts(ref), PR.max_members(ref), s.last_us()))
        if not noisy:
            assert (*(ref[k] for k in PR.COUNTS), PR.max_members(ref)) == ints
    # the last result (4 voxels) as the target and as the queries of the distance stage, from the device and from the host
    nv, pv, pf, nf = s.device_mesh()
    assert (nv, nf) == (ref["n_verts"], ref["n_faces"])
    G = DR.icosphere(3, CR.RADIUS)
    d_max = 4 * vol["voxel"]
    sd.set_target(pv, pf, d_max, nv=nv, m=nf)
    dev = sd.query(G[0])
    sd.set_target(r["verts"], r["faces"], d_max)
    host = sd.query(G[0])
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes() and (host[1] >= 0).any()
    sd.set_target(*G, d_max)
    dev, host = sd.query(pv, n=nv), sd.query(r["verts"])
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes() and (host[1] >= 0).any()
    for o in (fu, c, s, sd):
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


def test_host_fuse_simplify(ctx, ring6, tmp_path):
    vol = ring6["vol"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain.ply", "false.ply", "on.ply"))
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    m1 = pipe.fuse(*args, num_disparities=64, ply_path=p1, simplify=False)
    assert set(m0) == set(m1) == {"verts", "faces", "views", "warn"} and m0["warn"] == m1["warn"] and m0["views"] == m1["views"]
    assert m0["verts"].tobytes() == m1["verts"].tobytes() and m0["faces"].tobytes() == m1["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read(), "simplify=False is the call without the argument"
    m = pipe.fuse(*args, num_disparities=64, ply_path=p2, simplify=True)
    assert set(m) == {"verts", "faces", "views", "warn", "simplify"} and m["views"] == 6 and m["warn"] is None
    ref = PR.simplify(m0["verts"], m0["faces"], None, 2.0 * vol["voxel"], vol["origin"])  # the default: 2 voxels, the volume's origin
    assert 0 < ref["n_faces"] < len(m0["faces"]) / 4
    assert m["simplify"] == dict(clusters=ref["clusters"], degenerate=ref["degenerate"], duplicates=ref["duplicates"],
                                 verts_before=len(m0["verts"]), faces_before=len(m0["faces"]))
    assert m["verts"].tobytes() == ref["verts"].tobytes() and m["faces"].tobytes() == ref["faces"].tobytes()
    head, pv, pf = _parse_ply(p2)
    assert len(pv) == ref["n_verts"] and (pf[:, 0] == 3).all() and (pf[:, 1:] == ref["faces"]).all()
    assert np.allclose(pv, ref["verts"], rtol=1e-5, atol=1e-9)
    # the manual chain, with other parameters: factor, cell and origin
    h, w = ring6["images"].shape[1:]
    st, fu, s = ctx.stereo(w, h, num_disparities=64), ctx.fusion(**vol), ctx.simplify()
    for a, b in ring6["pairs"]:
        r = pipe.stereo_rectify(ring6["K"], ring6["poses"][a], ring6["poses"][b], w, h)
        il, ir = (ring6["images"][b], ring6["images"][a]) if r["swapped"] else (ring6["images"][a], ring6["images"][b])
        st.disparity(il, ir, r["H_l"], r["H_r"])
        fu.add_stereo_view(r, st)
    v, f = fu.extract()
    assert v.tobytes() == m0["verts"].tobytes()
    org = (0.001, -0.002, 0.003)
    got = s.fusion(fu, cell=3.5 * vol["voxel"], origin=org)
    chain = s.read()
    for o in (st, fu, s):
        o.close()
    m3 = pipe.fuse(*args, num_disparities=64, simplify=dict(factor=3.5, origin=org))
    m4 = pipe.fuse(*args, num_disparities=64, simplify=dict(cell=3.5 * vol["voxel"], origin=org))
    ref3 = PR.simplify(m0["verts"], m0["faces"], None, 3.5 * vol["voxel"], org)
    assert 0 < ref3["n_faces"] < ref["n_faces"], "other parameters, another mesh"
    assert m3["verts"].tobytes() == m4["verts"].tobytes() == chain["verts"].tobytes() == ref3["verts"].tobytes()
    assert m3["faces"].tobytes() == m4["faces"].tobytes() == chain["faces"].tobytes() == ref3["faces"].tobytes()
    assert m3["simplify"] == m4["simplify"] and m3["simplify"]["clusters"] == got["clusters"] and m3["simplify"]["duplicates"] == got["duplicates"]
    # nothing left (one cell holds the whole volume), no pairs, bad parameters
    p4 = str(tmp_path / "none.ply")
    m5 = pipe.fuse(*args, num_disparities=64, ply_path=p4, simplify=dict(factor=100.0))
    assert m5["verts"].shape == (0, 3) and m5["faces"].shape == (0, 3) and "no faces" in m5["warn"] and not os.path.exists(p4)
    assert m5["simplify"] == dict(clusters=1, degenerate=len(m0["faces"]), duplicates=0, verts_before=len(m0["verts"]), faces_before=len(m0["faces"]))
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, simplify=True)
    assert empty["verts"].shape == (0, 3) and empty["simplify"] == dict(clusters=0, degenerate=0, duplicates=0, verts_before=0, faces_before=0)
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, simplify=dict(cells=1.0))
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, simplify=dict(factor=2.0, cell=0.01))
    for bad in (dict(cell=0.0), dict(factor=-1.0), dict(cell=float("nan")), dict(origin=(0.0, float("inf"), 0.0))):
        with pytest.raises(capi.SfmxError):
            pipe.fuse(*args, num_disparities=64, simplify=bad)


def test_host_fuse_simplify_with_every_other_stage(ctx, ring6, tmp_path):
    """clean, appearance, evaluate and consistency together: the simplified mesh is the restatement's of the cleaned one, its
    grey is the shading of the simplified vertices with their own normals, and the evaluation is that of the simplified mesh"""
    vol = ring6["vol"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    ply = str(tmp_path / "all.ply")
    G = synth.shell_mesh(3)
    ekw = dict(gt_verts=G[0], gt_faces=G[1], d_max=4 * vol["voxel"], tau=vol["voxel"])
    h, w = ring6["images"].shape[1:]
    for cons, cl in ((False, True), (True, False)):
        m0 = pipe.fuse(*args, num_disparities=64, consistency=cons, appearance=True, clean=cl)
        m = pipe.fuse(*args, num_disparities=64, consistency=cons, appearance=True, clean=cl, simplify=True, evaluate=ekw, ply_path=ply)
        want = {"verts", "faces", "views", "warn", "normals", "grey", "vertex_views", "simplify", "evaluation"}
        assert set(m) == want | ({"consistency"} if cons else set()) | ({"clean"} if cl else set())
        ref = PR.simplify(m0["verts"], m0["faces"], m0["normals"], 2.0 * vol["voxel"], vol["origin"])
        assert 0 < ref["n_faces"] < len(m0["faces"])
        for k in ("verts", "faces", "normals"):
            assert m[k].tobytes() == ref[k].tobytes(), k
        assert m["simplify"]["verts_before"] == len(m0["verts"]) and m["simplify"]["faces_before"] == len(m0["faces"])
        if cl:
            assert m["clean"] == m0["clean"]
        if cons:
            assert m["consistency"] == m0["consistency"]
        assert m["evaluation"] == pipe.surface_eval(ctx, m["verts"], m["faces"], *G, d_max=ekw["d_max"], tau=ekw["tau"])
        assert m["evaluation"]["n_rec"] == ref["n_verts"]
        # grey: the shade stage over the simplified vertices and normals, from the same unfiltered views
        sh, st = ctx.shade(), ctx.stereo(w, h, num_disparities=64)
        for a, b in ring6["pairs"]:
            r = pipe.stereo_rectify(ring6["K"], ring6["poses"][a], ring6["poses"][b], w, h)
            il, ir = (ring6["images"][b], ring6["images"][a]) if r["swapped"] else (ring6["images"][a], ring6["images"][b])
            st.disparity(il, ir, r["H_l"], r["H_r"])
            sh.add_stereo_view(r, st)
        g1, c1 = sh.shade(m["verts"], m["normals"], FR.resolve(vol["voxel"]))
        sh.close()
        st.close()
        assert m["grey"].tobytes() == g1.tobytes() and m["vertex_views"].tobytes() == c1.tobytes()
        assert (c1 > 0).any() and len(np.unique(g1)) > 10
    head, pv, pf = _parse_ply(ply)
    assert "property uchar red" in head and "property float nx" in head and pv.shape == (ref["n_verts"], 9)
    assert (pf[:, 1:] == ref["faces"]).all() and (pv[:, 6] == m["grey"]).all() and (pv[:, 7] == pv[:, 8]).all()
    assert (pv[:, 3:6].astype(np.float32) == m["normals"].astype(np.float32)).all()


def test_pipeline_run_simplify(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    plain, simple = str(tmp_path / "plain"), str(tmp_path / "simple")
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
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, simple, fusion=dict(fz, simplify=dict(factor=3.0)))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(simple, "X")
    assert sorted(os.listdir(simple)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m1) == {"verts", "faces", "views", "warn"} and set(m) == set(m1) | {"simplify"} and len(m1["faces"]) > 0
    ref = PR.simplify(m1["verts"], m1["faces"], None, 3.0 * voxel, tuple(lo))
    assert 0 < ref["n_faces"] < len(m1["faces"])
    print("run: %d of %d vertices, %d of %d faces" % (ref["n_verts"], len(m1["verts"]), ref["n_faces"], len(m1["faces"])))
    assert m["verts"].tobytes() == ref["verts"].tobytes() and m["faces"].tobytes() == ref["faces"].tobytes()
    assert m["simplify"] == dict(clusters=ref["clusters"], degenerate=ref["degenerate"], duplicates=ref["duplicates"],
                                 verts_before=len(m1["verts"]), faces_before=len(m1["faces"]))
    assert open(os.path.join(simple, "templeRing_mesh_fused.ply")).read().startswith(
        "ply\nformat ascii 1.0\nelement vertex %d\n" % ref["n_verts"])
