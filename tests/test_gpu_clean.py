"""GPU suite: small connected components removed from a triangle mesh on the device.  sfmx_clean_* gives the cleaned vertices,
normals and faces, vert_src / face_src, the labels, the component face counts and the four counts byte for byte against the
NumPy restatement (tests/clean_ref.py): hand meshes, the block and scan-level edges, chain shapes, a random soup over the
parameter range, every way of feeding a mesh, the state rules, the noisy sphere-26 surface with the bound of DESIGN.md 16,
and pipeline.fuse / pipeline.run."""
import importlib
import json
import os

import numpy as np
import pytest

import clean_ref as LR
import consist_ref as CR
import fusion_ref as FR
import helpers as H
from test_clean_cpu import NOISY_OFF_SHELL, NOISY_ON_DROPPED

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
PAIR = (2, 3)  # e2e_keyframes: the pair with valid disparity
SMALL = dict(num_disparities=32, census=5)
ARRAYS = ("verts", "faces", "vert_src", "face_src", "label", "comp_faces")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cl(ctx):
    """one object for the whole module: its buffers grow and shrink with the cases"""
    c = ctx.clean()
    yield c
    c.close()


def _bytes(r, normals):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ARRAYS + (("normals",) if normals else ()))


def _check(cl, got, ref, what, normals=False):
    """the counts a run returned and everything read() gives, against the restatement"""
    assert got == LR.counts(ref), what + ": counts"
    r = cl.read(normals=normals)
    for k in ARRAYS + (("normals",) if normals else ()):
        want = np.asarray(ref[k])
        assert r[k].dtype == want.dtype and r[k].shape == want.shape, f"{what}: {k} {r[k].shape} {want.shape}"
        assert r[k].tobytes() == want.tobytes(), f"{what}: {k}"
    return r


def _case(cl, v, f, what, normals=None, **params):
    ref = LR.clean(v, f, normals, **params)
    _check(cl, cl.run(v, f, normals, **params), ref, f"{what} {params}", normals is not None)
    return ref


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


# ---- hand meshes -----------------------------------------------------------------------------------------------------------
F0 = np.zeros((0, 3), np.int32)
HAND = {
    "empty": (0, F0),
    "vertices-no-face": (5, F0),
    "one-face": (3, [[2, 0, 1]]),
    "two-disjoint-faces": (7, [[0, 1, 2], [4, 5, 6]]),
    "bow-tie": (6, [[5, 4, 2], [0, 1, 2]]),
    "repeated-indices": (6, [[3, 3, 3], [0, 0, 1], [5, 4, 4]]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_meshes(cl, name):
    n, f = HAND[name]
    v, f = LR._verts(n), np.asarray(f, np.int32).reshape(-1, 3)
    for params in (dict(), dict(min_faces=0, min_permille=0), dict(min_faces=2, min_permille=0), dict(min_permille=1000)):
        ref = _case(cl, v, f, name, normals=-v, **params)
    if name == "two-disjoint-faces":
        assert ref["n_faces"] == 2 and ref["components"] == 2, "a tie at 1000 permille: both kept"
    if name == "bow-tie":
        assert ref["components"] == 1 and ref["largest"] == 2 and (ref["label"][[0, 1, 2, 4, 5]] == 0).all() and ref["label"][3] == 3


def test_index_out_of_range_then_a_good_call(cl):
    v = LR._verts(9)
    good = np.array([[0, 1, 2], [6, 7, 8]], np.int32)
    _case(cl, v, good, "before")
    for bad in (9, -1, 2 ** 31 - 1, -2 ** 31):
        for pos in range(3):
            f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
            f[1, pos] = bad
            _invalid(lambda: cl.run(v, f))
            _invalid(cl.read)  # the failed run left no result
            assert cl.device_surface()[0] == -1
    _invalid(lambda: cl.run(np.zeros((0, 3)), np.array([[0, 0, 0]], np.int32)))  # n = 0: every index is out of range
    _case(cl, v, good, "after")
    assert cl.sizes() == (9, 2, 6, 2)
    # a call refused for its parameters leaves no result either: nothing of the good run above can be read
    for bad in (dict(min_permille=1001), dict(min_permille=-1), dict(min_faces=-1)):
        _invalid(lambda: cl.run(v, good, **bad))
        _invalid(cl.read)
        with pytest.raises(capi.SfmxError):
            cl.sizes()
        assert cl.device_surface()[0] == -1
        _case(cl, v, good, "again")
    with pytest.raises(TypeError):
        cl.run(v, good, min_area=1.0)
    assert cl.read()["faces"].shape == (2, 3), "refused in Python, before the library: the result stays"


# ---- block and scan edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [255, 256, 257, 1023, 1024, 1025, 1024 * 1024 + 1])
def test_disjoint_triangles_at_block_and_scan_edges(cl, m):
    """m triangles, every third joined to its neighbour: components of 1 and of 2 faces, split by min_faces 2 / 1000 permille;
    1024^2 + 1 faces is the third scan level"""
    v, f = LR.disjoint_triangles(m, 3)
    ref = _case(cl, v, f, f"m={m}", min_faces=2, min_permille=0)
    pairs = len(range(0, m - 1, 3))
    assert ref["n_faces"] == 2 * pairs and ref["largest"] == 2 and ref["components"] == m - pairs
    ref = _case(cl, v, f, f"m={m}")
    assert ref["n_faces"] == m and ref["n_verts"] == 3 * m - pairs, "10 permille of 2 faces keeps everything"
    if m < 2000:
        _case(cl, v, f, f"m={m}", min_permille=1000)
        _case(cl, v, f, f"m={m}", min_faces=3)


# ---- chain shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_triangle_strip_is_one_component(cl, order):
    v, f = LR.strip(65536, order)
    ref = _case(cl, v, f, "strip " + order, min_permille=1000)
    assert ref["components"] == 1 and ref["largest"] == 65536 and (ref["label"] == 0).all() and ref["n_verts"] == 65538


# ---- random soup -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("permuted", [False, True])
def test_random_soup_over_the_parameter_range(cl, permuted):
    v, f, nrm = LR.soup()
    if permuted:
        f = f[np.random.default_rng(8).permutation(len(f))]
    kept = set()
    for mf in (0, 1, 2, 5, 100):
        for pm in (0, 1, 10, 500, 1000):
            ref = _case(cl, v, f, "soup", normals=nrm, min_faces=mf, min_permille=pm)
            kept.add(ref["n_faces"])
    assert len(kept) >= 2, "the parameters split the soup"
    # a sparser soup: components of 1, 2, 3, 4, 5, 9 and 631 faces
    v, f, nrm = LR.soup(3000, 800)
    sizes = {_case(cl, v, f, "sparse soup", normals=nrm, min_faces=mf, min_permille=0)["n_faces"] for mf in (0, 2, 3, 5, 9, 10, 632)}
    assert len(sizes) == 7


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
    v, f, nrm = fu.extract_normals()
    ref = LR.clean(v, f, nrm)
    assert ref["components"] > 1 and 0 < ref["n_faces"] < len(f), "precondition: cleaning acts on this surface"
    c = ctx.clean()
    _check(c, c.fusion(fu), ref, "sfmx_clean_fusion", normals=True)
    resident = _bytes(c.read(normals=True), True)
    n2, pv, pn = c.device_surface()
    assert n2 == ref["n_verts"] and pv and pn
    _check(c, c.run(v, f, nrm), ref, "host pointers", normals=True)
    host = _bytes(c.read(normals=True), True)
    tv, tf, tn = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (v, f, nrm))
    torch.cuda.synchronize()
    _check(c, c.run(tv.data_ptr(), tf.data_ptr(), tn.data_ptr(), n=len(v), m=len(f)), ref, "device pointers", normals=True)
    dev = _bytes(c.read(normals=True), True)
    assert resident == host == dev == _bytes(ref, True)
    # a plain extract leaves the same surface without normals
    v2, f2 = fu.extract()
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    _check(c, c.fusion(fu), LR.clean(v, f), "sfmx_clean_fusion after a plain extract")
    assert c.device_surface()[2] is None
    c.close()


def test_one_object_large_small_large(ctx):
    c = ctx.clean()
    big, small = LR.disjoint_triangles(40000, 2), LR.disjoint_triangles(7, 2)
    for what, (v, f) in (("large", big), ("small", small), ("large again", big)):
        _case(c, v, f, what, normals=v[::-1].copy(), min_faces=2, min_permille=0)
        assert c.last_us() == 0.0
    ctx.set_timing(True)
    _case(c, *big, "timed")
    assert c.last_us() > 0.0
    ctx.set_timing(False)
    c.close()


def test_state_rules(ctx, ball):
    _, views = ball
    c, fu = ctx.clean(), ctx.fusion(**CR.SPHERE26_VOL)
    _invalid(c.read)  # before a run
    assert c.device_surface()[0] == -1
    _invalid(lambda: c.fusion(fu))  # nothing extracted yet
    fu.add_view(*views[0])
    _invalid(lambda: c.fusion(fu))
    assert fu.counts()[1] > 0
    _invalid(lambda: c.fusion(fu))  # counts alone leave no arrays
    v, f = fu.extract()
    ref = LR.clean(v, f)
    _check(c, c.fusion(fu), ref, "after extract")
    assert fu.counts() == (len(v), len(f))
    _check(c, c.fusion(fu), ref, "counts keep the surface current")
    fu.add_view(*views[1])
    fu.integrate()
    _invalid(lambda: c.fusion(fu))  # the volume changed
    _invalid(c.read)
    v, f, nrm = fu.extract_normals()
    _check(c, c.fusion(fu), LR.clean(v, f, nrm), "after extract_normals", normals=True)
    assert c.sizes()[:2] == (len(v), len(f))
    _invalid(lambda: c.fusion(fu, min_permille=1001))  # refused for its parameters: no result left
    _invalid(c.read)
    assert c.device_surface()[0] == -1
    _check(c, c.fusion(fu), LR.clean(v, f, nrm), "after a refused call", normals=True)
    fu.reset()
    _invalid(lambda: c.fusion(fu))  # after a reset
    v0, f0 = fu.extract()  # an empty volume: a current surface without faces
    assert len(f0) == 0
    assert c.fusion(fu) == dict(n_verts=0, n_faces=0, components=0, largest=0)
    c.close()
    fu.close()


# ---- noisy sphere-26 -------------------------------------------------------------------------------------------------------
def test_noisy_sphere26(ctx):
    """5 % outliers in all 26 maps, fused unfiltered on the device and cleaned there: NumPy's bytes, at most the recorded number
    of vertices off the shell, and the shading of the cleaned vertices is the uncleaned shading gathered by vert_src"""
    noisy, _ = CR.sphere26(True)
    vol = CR.SPHERE26_VOL
    rng = np.random.default_rng(7)
    fu, sh, c = ctx.fusion(**vol), ctx.shade(), ctx.clean()
    for cam, d16 in noisy:
        fu.add_view(cam, d16)
        sh.add_view(cam, d16, rng.integers(0, 256, d16.shape, dtype=np.uint8))
    v, f, nrm = fu.extract_normals()
    tol = FR.resolve(vol["voxel"])
    g0, c0 = sh.shade_fusion(fu, len(v), tol)
    ref = LR.clean(v, f, nrm)
    got = c.fusion(fu)
    r = _check(c, got, ref, "noisy sphere-26", normals=True)
    off = LR.sphere_off_shell(v, vol["voxel"])
    kept = np.zeros(len(v), bool)
    kept[r["vert_src"]] = True
    print("noisy sphere-26 on the device: %d components, %d faces, largest %d; off the shell %d -> %d, on-shell dropped %d; %.1f us"
          % (got["components"], len(f), got["largest"], off.sum(), (off & kept).sum(), (~off & ~kept).sum(), c.last_us()))
    assert (off & kept).sum() <= NOISY_OFF_SHELL and (~off & ~kept).sum() <= NOISY_ON_DROPPED
    assert off.sum() > 10 * NOISY_OFF_SHELL and got["n_faces"] == got["largest"]
    n2, pv, pn = c.device_surface()
    g1, c1 = sh.shade(pv, pn, tol, n=n2)
    assert (c0 > 0).sum() > 1000 and len(np.unique(g0)) > 100, "the shading has something to tell"
    assert g1.tobytes() == g0[r["vert_src"]].tobytes() and c1.tobytes() == c0[r["vert_src"]].tobytes()
    for o in (fu, sh, c):
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


def test_host_fuse_clean(ctx, ring6, tmp_path):
    vol = ring6["vol"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain.ply", "false.ply", "on.ply"))
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    m1 = pipe.fuse(*args, num_disparities=64, ply_path=p1, clean=False)
    assert set(m0) == set(m1) == {"verts", "faces", "views", "warn"} and m0["warn"] == m1["warn"] and m0["views"] == m1["views"]
    assert m0["verts"].tobytes() == m1["verts"].tobytes() and m0["faces"].tobytes() == m1["faces"].tobytes()
    assert open(p0, "rb").read() == open(p1, "rb").read(), "clean=False is the call without the argument"
    m = pipe.fuse(*args, num_disparities=64, ply_path=p2, clean=True)
    assert set(m) == {"verts", "faces", "views", "warn", "clean"} and m["views"] == 6 and m["warn"] is None
    ref = LR.clean(m0["verts"], m0["faces"])
    assert ref["components"] > 1 and ref["n_faces"] < len(m0["faces"])
    assert m["clean"] == dict(components=ref["components"], largest=ref["largest"], verts_removed=len(m0["verts"]) - ref["n_verts"],
                              faces_removed=len(m0["faces"]) - ref["n_faces"])
    assert m["verts"].tobytes() == ref["verts"].tobytes() and m["faces"].tobytes() == ref["faces"].tobytes()
    head, pv, pf = _parse_ply(p2)
    assert len(pv) == ref["n_verts"] and (pf[:, 0] == 3).all() and (pf[:, 1:] == ref["faces"]).all()
    assert np.allclose(pv, ref["verts"], rtol=1e-5, atol=0)
    # the manual chain
    h, w = ring6["images"].shape[1:]
    st, fu, c = ctx.stereo(w, h, num_disparities=64), ctx.fusion(**vol), ctx.clean()
    for a, b in ring6["pairs"]:
        r = pipe.stereo_rectify(ring6["K"], ring6["poses"][a], ring6["poses"][b], w, h)
        il, ir = (ring6["images"][b], ring6["images"][a]) if r["swapped"] else (ring6["images"][a], ring6["images"][b])
        st.disparity(il, ir, r["H_l"], r["H_r"])
        fu.add_stereo_view(r, st)
    v, f = fu.extract()
    kw = dict(min_faces=40, min_permille=2)
    got = c.fusion(fu, **kw)
    chain = c.read()
    for o in (st, fu, c):
        o.close()
    assert v.tobytes() == m0["verts"].tobytes()
    m3 = pipe.fuse(*args, num_disparities=64, clean=kw)
    ref3 = LR.clean(m0["verts"], m0["faces"], **kw)
    assert ref["n_faces"] < ref3["n_faces"] < len(m0["faces"]), "other parameters, another mesh"
    assert m3["verts"].tobytes() == chain["verts"].tobytes() == ref3["verts"].tobytes()
    assert m3["faces"].tobytes() == chain["faces"].tobytes() == ref3["faces"].tobytes()
    assert m3["clean"]["components"] == got["components"] and m3["clean"]["faces_removed"] == len(f) - got["n_faces"]
    # nothing left, no pairs, bad parameters
    p4 = str(tmp_path / "none.ply")
    m4 = pipe.fuse(*args, num_disparities=64, ply_path=p4, clean=dict(min_faces=10 ** 6))
    assert m4["verts"].shape == (0, 3) and m4["faces"].shape == (0, 3) and "no faces" in m4["warn"] and not os.path.exists(p4)
    assert m4["clean"] == dict(components=ref["components"], largest=ref["largest"], verts_removed=len(m0["verts"]),
                               faces_removed=len(m0["faces"]))
    empty = pipe.fuse(*args[:4], [], *args[5:], num_disparities=64, clean=True)
    assert empty["verts"].shape == (0, 3) and empty["clean"] == dict(components=0, largest=0, verts_removed=0, faces_removed=0)
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, clean=dict(min_area=1.0))
    with pytest.raises(capi.SfmxError):
        pipe.fuse(*args, num_disparities=64, clean=dict(min_permille=1001))


def test_host_fuse_clean_with_consistency_and_appearance(ctx, ring6, tmp_path):
    """grey and view counts of the cleaned mesh are the uncleaned shading gathered by vert_src; the PLY parsed back"""
    vol = ring6["vol"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    ply = str(tmp_path / "all.ply")
    for cons in (False, True):
        m0 = pipe.fuse(*args, num_disparities=64, consistency=cons, appearance=True)
        m = pipe.fuse(*args, num_disparities=64, consistency=cons, appearance=True, clean=True, ply_path=ply)
        want = {"verts", "faces", "views", "warn", "normals", "grey", "vertex_views", "clean"} | ({"consistency"} if cons else set())
        assert set(m) == want
        ref = LR.clean(m0["verts"], m0["faces"], m0["normals"])
        src = ref["vert_src"]
        assert ref["components"] > 1 and 0 < ref["n_faces"] < len(m0["faces"])
        assert m["verts"].tobytes() == ref["verts"].tobytes() and m["faces"].tobytes() == ref["faces"].tobytes()
        assert m["normals"].tobytes() == ref["normals"].tobytes()
        assert m["grey"].tobytes() == m0["grey"][src].tobytes() and m["vertex_views"].tobytes() == m0["vertex_views"][src].tobytes()
        assert (m0["vertex_views"] > 0).any() and len(np.unique(m0["grey"])) > 10
        if cons:
            assert m["consistency"] == m0["consistency"]
    head, pv, pf = _parse_ply(ply)
    assert "property uchar red" in head and "property float nx" in head and pv.shape == (ref["n_verts"], 9)
    assert (pf[:, 1:] == ref["faces"]).all() and (pv[:, 6] == m["grey"]).all() and (pv[:, 7] == pv[:, 8]).all()
    assert (pv[:, 3:6].astype(np.float32) == m["normals"].astype(np.float32)).all()


def test_pipeline_run_clean(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    plain, cleaned = str(tmp_path / "plain"), str(tmp_path / "clean")
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
    kw = dict(min_permille=1000)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, cleaned, fusion=dict(fz, clean=kw))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(cleaned, "X")
    assert sorted(os.listdir(cleaned)) == sorted(os.listdir(plain))
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m1) == {"verts", "faces", "views", "warn"} and set(m) == set(m1) | {"clean"} and len(m1["faces"]) > 0
    ref = LR.clean(m1["verts"], m1["faces"], **kw)
    assert ref["components"] > 1 and ref["n_faces"] == ref["largest"] < len(m1["faces"]), "only the largest component stays"
    print("run: %d components, largest %d, %d of %d faces kept" % (ref["components"], ref["largest"], ref["n_faces"], len(m1["faces"])))
    assert m["verts"].tobytes() == ref["verts"].tobytes() and m["faces"].tobytes() == ref["faces"].tobytes()
    assert m["clean"] == dict(components=ref["components"], largest=ref["largest"], verts_removed=len(m1["verts"]) - ref["n_verts"],
                              faces_removed=len(m1["faces"]) - ref["n_faces"])
    assert open(os.path.join(cleaned, "templeRing_mesh_fused.ply")).read().startswith(
        "ply\nformat ascii 1.0\nelement vertex %d\n" % ref["n_verts"])
