"""CPU suite: exact filling of the fused surface's small holes by centroid fans -- properties and hand cases of the NumPy
restatement (tests/fill_ref.py), its calibration on the filtered ring-6 surface of DESIGN.md 15 (fused by tests/fusion_ref.py),
and parameter validation of the device stage (sfmx_fill_check_params needs no device).

Bounds (the rule of DESIGN.md 15): 1.25 x the value the restatement gives on the fixture, rounded up to 0.1 degree (roughness),
or 1.25 x the distance to 100 % rounded up to half a percentage point (shares); DESIGN.md 22 has the table.  The integer columns
are stated exactly: the restatement is deterministic."""
import importlib
import inspect

import numpy as np
import pytest

import clean_ref as LR
import consist_ref as CR
import fill_ref as R
import fusion_ref as FR
import helpers as H
import smooth_ref as MR
import stereo_ref as SR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")

ZERO = dict.fromkeys(R.COUNTS, 0)
# ring-6, filter on (7 552 v / 13 622 f; roughness 26.23 degrees, outward 97.69 %, edges used once in each direction 92.96 %),
# unit = the voxel: the counts of the input, its loops, and per max_edges the filled loops and edges, then the vertices that 10
# Taubin pairs pin afterwards, then bounds on the roughness before and after smoothing (degrees), the outward faces before and
# after it, and the edges used once in each direction
RING_INPUT = dict(edges=21179, boundary_edges=1492, irregular_edges=0, complex_vertices=10)
RING_LOOPS = dict(loops=52, shortest=4, longest=72, on_loops=580)
RING_ROWS = {
    8: (30, 166, 1316, 35.8, 26.8, 0.96, 0.965, 0.92),    # measured 28.58, 21.42 degrees, 96.95 %, 97.53 %, 93.79 %
    32: (50, 466, 1016, 37.6, 27.8, 0.955, 0.96, 0.94),   # measured 30.00, 22.23 degrees, 96.56 %, 97.10 %, 95.26 %
    128: (52, 580, 902, 38.3, 28.3, 0.955, 0.96, 0.945),  # measured 30.62, 22.60 degrees, 96.46 %, 97.02 %, 95.81 %
}
# the same surface cleaned with the default thresholds (7 304 v / 13 378 f), max_edges 32: the fill counts and the vertices
# smoothing pins afterwards (the GPU suite runs this chain on the device)
RING_CLEANED = dict(edges=20712, boundary_edges=1290, irregular_edges=0, complex_vertices=9, filled_loops=26, filled_edges=292,
                    new_verts=26, new_faces=292)
RING_CLEANED_PINNED = 989


@pytest.fixture(scope="module")
def soup():
    return LR.soup()


@pytest.fixture(scope="module")
def ring6():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    views = []
    for a, b in pairs:
        r = SR.rectify(K, poses[a][0], poses[a][1], poses[b][0], poses[b][1])
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        views.append((r, SR.disparity(il, ir, r["H_l"], r["H_r"], dict(num_disparities=64))))
    vol = CR.RING6_VOL
    m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(views, CR.filter_views(views)))
    assert (len(m["verts"]), len(m["faces"])) == (7552, 13622)
    return m["verts"], m["faces"]


def _face_keys(verts, faces):
    """the faces as a sorted list that depends neither on their order, nor on the corner a face starts at, nor on the labels"""
    p = verts[faces]
    return sorted(min((p[i, [j, (j + 1) % 3, (j + 2) % 3]].tobytes() for j in range(3))) for i in range(len(p)))


def _check_properties(v, f, nrm, **kw):
    n, m = len(v), len(f)
    a = R.fill(v, f, nrm, **kw)
    assert a["verts"][:n].tobytes() == v.tobytes() and a["faces"][:m].tobytes() == f.tobytes() and a["normals"][:n].tobytes() == nrm.tobytes()
    assert len(a["verts"]) == n + a["new_verts"] and len(a["faces"]) == m + a["new_faces"]
    # the faces in another order, and each face starting at another corner: the new rows and the counts do not change
    rng = np.random.default_rng(41)
    rot = rng.integers(0, 3, m)
    assert (rot > 0).any()
    for f2 in (f[rng.permutation(m)], np.stack([f[np.arange(m), (rot + j) % 3] for j in range(3)], 1)):
        b = R.fill(v, f2, nrm, **kw)
        assert b["faces"][:m].tobytes() == np.ascontiguousarray(f2).tobytes() and b["faces"][m:].tobytes() == a["faces"][m:].tobytes()
        assert b["verts"].tobytes() == a["verts"].tobytes() and b["normals"].tobytes() == a["normals"].tobytes()
        assert R.counts(a) == R.counts(b)
    # the vertices in another order, the faces relabelled: the same mesh up to the labels and the loop order
    v2, f2, n2, perm = R.permute_vertices(v, f, nrm, 42)
    c = R.fill(v2, f2, n2, **kw)
    assert R.counts(a) == R.counts(c)
    assert sorted(x.tobytes() for x in c["verts"][n:]) == sorted(x.tobytes() for x in a["verts"][n:])
    assert _face_keys(c["verts"], c["faces"]) == _face_keys(a["verts"], a["faces"])
    if a["new_verts"] > 1:
        assert (perm[c["leaders"]] != a["leaders"]).any(), "precondition: the relabelling changes the loop order"
    # every filled rim edge becomes regular; irregular edges and complex vertices stay; a second run returns its input
    s = R.fill(a["verts"], a["faces"], a["normals"], **kw)
    spokes = a["filled_edges"] - 3 * (a["filled_loops"] - a["new_verts"])  # a loop of three adds no edge
    assert R.counts(s) == dict(ZERO, edges=a["edges"] + spokes, boundary_edges=a["boundary_edges"] - a["filled_edges"],
                               irregular_edges=a["irregular_edges"], complex_vertices=a["complex_vertices"])
    R.same(s, dict(a, **R.counts(s)))
    return a


def test_orders_rotations_relabelling_and_a_second_run(soup, ring6):
    v, f, nrm = soup
    a = _check_properties(v, f, nrm, unit=0.01, origin=(0.1, -0.2, 0.3), max_edges=1024)
    assert a["complex_vertices"] > 1000 and a["irregular_edges"] >= 1, "a random soup: hardly a simple vertex"
    rv, rf = ring6
    vol = CR.RING6_VOL
    rn = np.random.default_rng(43).standard_normal(rv.shape)
    a = _check_properties(rv, rf, rn, unit=vol["voxel"], origin=vol["origin"])
    assert a["filled_loops"] == 50


def test_new_edges_are_the_spokes(ring6):
    """a fan of L faces adds its L spokes to the edge table and nothing else; a loop of three adds no edge"""
    v, f = ring6
    a = R.fill(v, f, unit=CR.RING6_VOL["voxel"], origin=CR.RING6_VOL["origin"])
    s = R.fill(a["verts"], a["faces"], unit=CR.RING6_VOL["voxel"], origin=CR.RING6_VOL["origin"])
    long = a["lengths"][a["lengths"] > 3]
    assert s["edges"] == a["edges"] + int(long.sum()) and a["new_faces"] == int(long.sum()) + int((a["lengths"] == 3).sum())


def test_sphere26_is_closed_and_comes_back_byte_equal():
    views, _ = CR.sphere26(False)
    vol = CR.SPHERE26_VOL
    m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], views)
    v, f = m["verts"], m["faces"]
    for me in (3, 32, 1024):
        r = R.fill(v, f, unit=vol["voxel"], origin=vol["origin"], max_edges=me)
        assert R.counts(r) == dict(ZERO, edges=68352) and r["verts"].tobytes() == v.tobytes() and r["faces"].tobytes() == f.tobytes()


# ---- hand cases ------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    C = R.hand_cases()
    out = {k: R.run_case(c) for k, c in C.items()}

    def new(name):
        r, c = out[name], C[name]
        n, m = len(np.asarray(c["verts"]).reshape(-1, 3)), len(np.asarray(c["faces"]).reshape(-1, 3))
        return r["verts"][n:].tolist(), r["faces"][m:].tolist(), (None if r["normals"] is None else r["normals"][n:].tolist())

    assert R.counts(out["empty"]) == ZERO and out["empty"]["verts"].shape == (0, 3) and out["empty"]["faces"].shape == (0, 3)
    assert out["empty"]["faces"].dtype == np.int32
    assert R.counts(out["no-faces"]) == ZERO and out["no-faces"]["normals"].shape == (5, 3)
    tri = dict(ZERO, edges=3, boundary_edges=3, filled_loops=1, filled_edges=3, new_faces=1)
    assert R.counts(out["lone-triangle"]) == tri and new("lone-triangle") == ([], [[0, 2, 1]], []), "the back face"
    assert R.counts(out["tetrahedron-closed"]) == dict(ZERO, edges=6)
    assert R.counts(out["tetrahedron-open"]) == dict(tri, edges=6) and new("tetrahedron-open")[1] == [[0, 3, 2]], "the missing face, rotated"
    closed = R.fill(out["tetrahedron-open"]["verts"], out["tetrahedron-open"]["faces"], unit=0.125)
    assert R.counts(closed) == dict(ZERO, edges=6)
    quad = dict(ZERO, edges=5, boundary_edges=4, filled_loops=1, filled_edges=4, new_verts=1, new_faces=4)
    assert R.counts(out["cube-open"]) == dict(quad, edges=17)
    nv, nf, nn = new("cube-open")
    assert nv == [[0.75, 0.75, 1.25]] and nf == [[4, 5, 8], [5, 7, 8], [7, 6, 8], [6, 4, 8]], "the centre of the top, wound like the rim"
    assert abs(np.linalg.norm(nn[0]) - 1.0) < 1e-15
    assert R.counts(R.fill(out["cube-open"]["verts"], out["cube-open"]["faces"], unit=0.25)) == dict(ZERO, edges=21)
    assert R.counts(out["open-quad"]) == quad
    nv, nf, nn = new("open-quad")
    assert nv == [[0.5, 0.5, 0.0]] and nf == [[0, 3, 4], [3, 2, 4], [2, 1, 4], [1, 0, 4]]
    # relabelled by two: the leader 0 is the old vertex 2, the same fan starting elsewhere
    nv2, nf2, nn2 = new("open-quad-relabelled")
    assert nv2 == nv and nn2 == nn and nf2 == [[0, 3, 4], [3, 2, 4], [2, 1, 4], [1, 0, 4]]
    assert R.counts(out["two-holes-share-a-vertex"]) == dict(ZERO, edges=10, boundary_edges=8, complex_vertices=1)
    assert R.counts(out["irregular-edge-at-the-rim"]) == dict(ZERO, edges=19, boundary_edges=4, irregular_edges=1, complex_vertices=1)
    g = R.gaps(np.asarray(C["irregular-edge-at-the-rim"]["faces"], np.int32), 9)
    assert g["complex"].tolist() == [False] * 4 + [True] + [False] * 4 and g["next"][[5, 7, 6]].tolist() == [7, 6, 4] and g["next"][4] == -1
    assert R.counts(out["face-a-a-b"]) == dict(ZERO, edges=6, boundary_edges=3, irregular_edges=1, complex_vertices=1)
    assert R.counts(out["face-a-a-a"]) == dict(tri, edges=6) and new("face-a-a-a")[1] == [[0, 3, 2]]
    assert R.counts(out["unused-vertex"]) == dict(quad, edges=17)
    assert new("unused-vertex")[1][0] == [4, 5, 9] and out["unused-vertex"]["verts"][8].tolist() == [9.0, 9.0, 9.0]
    r = out["minus-zero"]
    assert np.signbit(r["verts"][0]).tolist() == [True, False, True], "the input rows keep their bytes"
    assert not np.signbit(r["verts"][4]).any() and not np.signbit(r["normals"][4]).any() and not r["normals"][4].any()
    assert R.counts(out["at-the-limit"]) == quad and new("at-the-limit")[0] == [[65536.0, 65536.0, 0.0]]
    step = 2.0 ** -20
    assert new("half-positive")[0] == [[step, step, 0.0]], "S = 2 and 3 over L = 4: 0.5 and 0.75 both round to 1"
    assert new("half-negative")[0] == [[0.0, -2 * step, 0.0]], "S = -2 and -7 over L = 4: -0.5 rounds to 0 and -1.75 to -2, not -1"
    assert new("normals-sum-to-zero")[2] == [[0.0, 0.0, 0.0]] and new("nan-normals")[2] == [[0.0, 0.0, 0.0]]
    # max_edges at and below the loop's length
    for name, ln in (("open-quad", 4), ("lone-triangle", 3), ("cube-open", 4)):
        assert R.run_case(C[name], max_edges=ln)["filled_loops"] == 1
        if ln > 3:
            r = R.run_case(C[name], max_edges=ln - 1)
            assert r["filled_loops"] == 0 and r["verts"].tobytes() == np.asarray(C[name]["verts"], np.float64).tobytes()


def test_tubes_close_with_euler_characteristic_two():
    for k in (3, 4, 31, 32, 33):
        v, f, nrm = R.open_tube(k)
        r = R.fill(v, f, nrm, unit=0.01)
        if k <= 32:
            assert r["filled_loops"] == 2 and r["filled_edges"] == 2 * k and r["new_verts"] == (2 if k > 3 else 0)
            assert R.euler(len(r["verts"]), r["faces"]) == 2
            assert R.counts(R.fill(r["verts"], r["faces"], unit=0.01)) == dict(ZERO, edges=r["edges"] + (2 * k if k > 3 else 0))
        else:
            assert r["filled_loops"] == 0 and r["boundary_edges"] == 2 * k and R.euler(len(v), f) == 0
    v, f, nrm = R.lone_triangles(7)
    assert R.counts(R.fill(v, f, unit=0.01)) == dict(ZERO, edges=21, boundary_edges=21, filled_loops=7, filled_edges=21, new_faces=7)
    v, f, nrm = R.open_quads(7)
    assert R.counts(R.fill(v, f, unit=0.01)) == dict(edges=35, boundary_edges=28, irregular_edges=0, complex_vertices=0, filled_loops=7,
                                                     filled_edges=28, new_verts=7, new_faces=28)


def test_every_invalid_input_raises():
    bad, good = R.invalid_inputs()
    assert R.fill(**good)["edges"] == 5 and len(bad) == 30 + 12 + 1
    for name, case in bad:
        with pytest.raises(ValueError):
            R.fill(**case)
    for p in R.BAD_PARAMS:
        with pytest.raises(ValueError):
            R.fill(good["verts"], good["faces"], **p)
    # the limits themselves are inside: |q| = 2^18 exactly, the last vertex index
    v = good["verts"].copy()
    v[3] = (2.0 ** 18, -2.0 ** 18, 0.0)
    v[4] = (-2.0 ** 18, 2.0 ** 18, 2.0 ** 18)
    assert R.fill(v, good["faces"], unit=1.0)["filled_loops"] == 1
    with pytest.raises(ValueError):
        R.fill(v * 2.0, good["faces"], unit=1.0)
    assert R.fill(v * 2.0, good["faces"], unit=2.0)["filled_loops"] == 1
    f = good["faces"].copy()
    f[1, 1] = 4
    assert R.fill(good["verts"], f, unit=1.0)["edges"] == 5
    # one vertex too many: 2^24 - 1 vertices and one open quad
    big = np.zeros((2 ** 24 - 1, 3))
    big[:4] = np.asarray(R.hand_cases()["open-quad"]["verts"])
    with pytest.raises(ValueError, match="2\\^24"):
        R.fill(big, [[0, 1, 2], [0, 2, 3]], unit=1.0)
    assert R.fill(big[:-1], [[0, 1, 2], [0, 2, 3]], unit=1.0)["new_verts"] == 1
    assert R.fill(big, [[0, 1, 2]], unit=1.0)["new_faces"] == 1, "a loop of three adds no vertex"


# ---- calibration --------------------------------------------------------------------------------------------
def test_ring6_calibration(ring6):
    v, f = ring6
    vol = CR.RING6_VOL
    kw = dict(unit=vol["voxel"], origin=vol["origin"])
    L = R.all_loops(f, len(v))
    print("loops: %s" % sorted(L.tolist()))
    assert dict(loops=len(L), shortest=int(L.min()), longest=int(L.max()), on_loops=int(L.sum())) == RING_LOOPS
    assert [int((L <= k).sum()) for k in (8, 16, 32, 64)] == [30, 45, 50, 51]
    rough0, out0, share0 = MR.roughness(v, f), MR.outward_share(v, f), R.edge_share(f)
    pinned0 = MR.smooth(v, f, **kw)["pinned"]
    print("input: roughness %.2f degrees, outward %.4f, edges %.4f, pinned %d" % (rough0, out0, share0, pinned0))
    assert pinned0 == 1482
    for me, (loops, edges, pinned, b_rough, b_rough_s, b_out, b_out_s, b_share) in RING_ROWS.items():
        r = R.fill(v, f, max_edges=me, **kw)
        assert R.counts(r) == dict(RING_INPUT, filled_loops=loops, filled_edges=edges, new_verts=loops, new_faces=edges), me
        fv, ff = r["verts"], r["faces"]
        s = MR.smooth(fv, ff, **kw)
        rough, out, share = MR.roughness(fv, ff), MR.outward_share(fv, ff), R.edge_share(ff)
        rough_s, out_s = MR.roughness(s["verts"], ff), MR.outward_share(s["verts"], ff)
        print("max_edges %d: %s; roughness %.2f -> %.2f degrees, outward %.4f -> %.4f, edges %.4f, pinned %d"
              % (me, R.counts(r), rough, rough_s, out, out_s, share, s["pinned"]))
        assert s["pinned"] == pinned and s["boundary_edges"] == RING_INPUT["boundary_edges"] - edges and s["irregular_edges"] == 0
        assert rough <= b_rough and rough_s <= b_rough_s and out >= b_out and out_s >= b_out_s and share >= b_share, me
        assert share > share0 and rough_s < rough, me
        # conditions, not measurements
        assert CR.mesh_quality(fv, ff)[1] == 1.0 and CR.mesh_quality(s["verts"], ff)[1] == 1.0, "every vertex stays in the shell"
        again = R.fill(fv, ff, max_edges=me, **kw)
        assert again["filled_loops"] == 0 and again["verts"].tobytes() == fv.tobytes() and again["faces"].tobytes() == ff.tobytes()
        assert again["complex_vertices"] == RING_INPUT["complex_vertices"]
    c = LR.clean(v, f)
    r = R.fill(c["verts"], c["faces"], **kw)
    assert (len(c["verts"]), len(c["faces"])) == (7304, 13378) and R.counts(r) == RING_CLEANED
    assert MR.smooth(r["verts"], r["faces"], **kw)["pinned"] == RING_CLEANED_PINNED


# ---- library and Python layer ----------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.fill_default_params() == dict(unit=0.0, origin=(0.0, 0.0, 0.0), max_edges=32)
    assert capi.FILL_DEFAULTS == R.DEFAULTS and capi.fill_default_params() == dict(unit=0.0, **capi.FILL_DEFAULTS)
    assert capi.FILL_COUNTS == R.COUNTS
    assert not capi.fill_check_params(**capi.fill_default_params()), "unit has no default"
    assert not capi.fill_check_params() and not R.check_params()
    for good in R.GOOD_PARAMS:
        assert capi.fill_check_params(**good) and R.check_params(**good), good
    for bad in R.BAD_PARAMS:
        assert not capi.fill_check_params(**bad) and not R.check_params(**bad), bad
    with pytest.raises(TypeError):
        capi.fill_params(1.0, max_edges=2.5)
    lib = capi.load_library()
    assert lib.sfmx_fill_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_fill_default_params(None)  # tolerated
    for s in capi.SYMBOLS:
        if s.startswith("sfmx_fill_"):
            assert hasattr(lib, s), s
    assert sum(s.startswith("sfmx_fill_") for s in capi.SYMBOLS) == 13
    assert lib.sfmx_fill_sizes(None, None, None, None, None) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_fill_counts(None, *[None] * 8) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_fill_device_mesh(None, None, None, None, None) == -1 and lib.sfmx_fill_device_surface(None, None, None) == -1
    assert lib.sfmx_fill_last_us(None) == 0.0
    header = open(H.ROOT + "/include/sfmx.h").read()
    for s in capi.SYMBOLS:
        if s.startswith("sfmx_fill_"):
            assert s + "(" in header, s


def test_python_layer_key_checks():
    with pytest.raises(TypeError):
        capi.fill_params(1.0, max_edge=8)
    assert pipe.FILL_KEYS == ("max_edges", "unit", "origin")
    assert set(pipe.FILL_KEYS) == set(capi.FILL_DEFAULTS) | {"unit"}
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    for bad in (dict(max_edge=8), dict(max_edges=8, iters=2), dict(cell=0.2), dict(max_edges=2.5)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, fill=bad)
    assert inspect.signature(pipe.fuse).parameters["fill"].default is False
    assert hasattr(capi.Context, "fill") and all(hasattr(capi.Fill, k) for k in ("run", "fusion", "clean", "read", "device_mesh", "device_surface"))
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_fl") and hasattr(lib, "sfmx_host_fusion_mesh_sm")
