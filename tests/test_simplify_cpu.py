"""CPU suite: exact vertex clustering of the fused surface -- properties and hand cases of the NumPy restatement
(tests/simplify_ref.py), its calibration on the clean sphere-26 and the filtered ring-6 surfaces of DESIGN.md 13 / 15 (fused by
tests/fusion_ref.py), accuracy and completeness by tests/sdist_ref.py, and parameter validation of the device stage
(sfmx_simplify_check_params needs no device).

Bounds (the rule of DESIGN.md 15): 1.25 x the value the restatement gives on the fixture, rounded up to 0.01 voxel (radius
errors) or to 1e-4 (accuracy), or 1.25 x the distance to 100 % rounded up to half a percentage point (shares); DESIGN.md 20 has
the table.  The integer columns are stated exactly: the restatement is deterministic."""
import importlib
import inspect

import numpy as np
import pytest

import clean_ref as LR
import consist_ref as CR
import fusion_ref as FR
import helpers as H
import sdist_ref as DR
import simplify_ref as PR
import stereo_ref as SR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")

# the clean sphere-26 surface (22 786 v / 45 568 f; radius error 0.104 / 0.427 voxels), grid at the volume's origin:
# cell in voxels, grid shift in cells -> (clusters, degenerate, duplicates, n', m', max members),
#   then measured -> bound: radius error RMS, max (voxels), edges used once in each direction, outward faces
SPHERE_ROWS = {
    (2, 0.0): ((1915, 41716, 0, 1915, 3852, 35), (0.11, 0.52, 0.990, 0.985)),    # 0.0851, 0.4099, 99.34 %, 99.17 %
    (3, 0.0): ((834, 43892, 0, 834, 1676, 80), (0.09, 0.46, 0.990, 0.990)),       # 0.0702, 0.3613, 99.28 %, 99.28 %
    (3, -0.37): ((834, 43896, 1, 834, 1671, 79), (0.10, 0.40, 0.990, 0.990)),     # 0.0731, 0.3159, 99.48 %, 99.52 %
    (4, 0.0): ((482, 44604, 2, 482, 962, 130), (0.09, 0.46, 0.995, 0.995)),       # 0.0712, 0.3613, 99.65 %, 99.79 %
}
# accuracy by sdist_ref (d_max = 4 voxels, tau = 1 voxel, level-5 ground truth): cell in voxels -> (n_rec, acc_within,
# comp_within) and the accuracy bound; completeness is 100 % before and after, so its bound is 100 %
SPHERE_ACC = {
    0: ((22786, 22786, 10242), 0.0012),  # the input: measured 0.000907
    2: ((1915, 1915, 10242), 0.0009),    # measured 0.000717
    4: ((482, 482, 10242), 0.0007),      # measured 0.000541
}
# ring-6, filter on (7 552 v / 13 622 f; edges 92.96 %, outward 97.69 %), 2 voxels
RING_ON_ROW = (772, 12367, 0, 736, 1255, 32)
RING_ON_EDGES, RING_ON_OUTWARD = 0.77, 0.94  # measured 81.66 % and 95.54 %


@pytest.fixture(scope="module")
def soup():
    v, f, nrm = LR.soup()
    return v, f, PR.unit(nrm)


@pytest.fixture(scope="module")
def sphere26():
    views, _ = CR.sphere26(False)
    vol = CR.SPHERE26_VOL
    m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], views)
    return m["verts"], m["faces"]


def _same(a, b, normals=False):
    for k in PR.ARRAYS + PR.COUNTS + (("normals",) if normals else ()):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


# ---- properties ------------------------------------------------------------------------------------------------------------
def _check_permutations(v, f, nrm, cell, origin):
    a = PR.simplify(v, f, nrm, cell, origin)
    # the faces in another order: the same vertices, the same faces in another order
    fp = np.random.default_rng(21).permutation(len(f))
    b = PR.simplify(v, f[fp], nrm, cell, origin)
    for k in ("verts", "normals", "vert_dst", "members"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert PR.counts(a) == PR.counts(b) and PR.face_set(a) == PR.face_set(b)
    assert set(map(tuple, a["faces"].tolist())) == set(map(tuple, b["faces"].tolist()))
    # the vertices in another order, the faces relabelled: cluster numbers come from the cells, so only vert_dst is permuted
    v2, f2, n2, perm = PR.permute_vertices(v, f, nrm, 22)
    c = PR.simplify(v2, f2, n2, cell, origin)
    for k in ("verts", "normals", "faces", "face_src", "members"):
        assert a[k].tobytes() == c[k].tobytes(), k
    assert (c["vert_dst"] == a["vert_dst"][perm]).all() and PR.counts(a) == PR.counts(c)
    return a


def test_permutations_change_only_the_face_order(soup, sphere26):
    v, f, nrm = soup
    for cell in (0.1, 1.0):
        a = _check_permutations(v, f, nrm, cell, (0.1, -0.2, 0.3))
    assert a["duplicates"] > 1000 and 100 < a["clusters"] < 1000, "the coarse soup exercises the duplicate rule"
    sv, sf = sphere26
    _check_permutations(sv, sf, PR.unit(sv), 3 * 0.005, CR.SPHERE26_VOL["origin"])


def test_a_vertex_alone_in_its_cell_is_unchanged(soup, sphere26):
    """The 2^27-cell box keeps the cell above 1 / 512 of the mesh's extent, and both fixtures have vertices closer than that
    (the marching-tetrahedra slivers; the soup's dense middle).  So at the smallest cell they admit the property is held per
    vertex: one that is alone comes back unchanged up to the quantisation, and nearly all are alone.  The whole-mesh form is
    the next test, on a soup sparse enough for it."""
    for v, f, cell, origin, alone in ((*soup[:2], 0.02, (0.0, 0.0, 0.0), 19944), (*sphere26, 0.0004, CR.SPHERE26_VOL["origin"], 21363)):
        r = PR.simplify(v, f, None, cell, origin)
        lin = PR.cells(v, cell, origin)[0]
        _, inv, cnt = np.unique(lin, axis=0, return_inverse=True, return_counts=True)
        single = cnt[inv.reshape(-1)] == 1
        assert single.sum() == alone > 0.9 * len(v)
        kept = single & (r["vert_dst"] >= 0)
        assert kept.sum() > 0.8 * len(v) and (r["members"][r["vert_dst"][kept]] == 1).all()
        assert np.abs(r["verts"][r["vert_dst"][kept]] - v[kept]).max() <= cell * 2.0 ** -30


def test_a_cell_that_isolates_every_vertex_changes_nothing():
    for v, f, cell, origin in ((*LR.soup(2000, 1500, 9)[:2], 0.02, (0.0, 0.0, 0.0)), (*LR.soup(500, 2000, 10)[:2], 0.0125, (0.3, 0.1, -0.2))):
        used = np.zeros(len(v), bool)
        used[f.ravel()] = True
        v, f = v[used], (np.cumsum(used) - 1)[f].astype(np.int32)  # every vertex used
        distinct = np.array([len(set(t)) == 3 for t in f.tolist()])
        r = PR.simplify(v, f, None, cell, origin)
        assert r["clusters"] == len(v) == r["n_verts"] and r["degenerate"] == int((~distinct).sum()) and (r["members"] == 1).all()
        # up to the quantisation (half of 2^-30 of a cell, and the rounding of the double operations) and the order
        assert np.abs(r["verts"][r["vert_dst"]] - v).max() <= cell * 2.0 ** -30
        fd = f[distinct]
        dup = len(fd) - len({tuple(np.roll(t, -int(np.argmin(t)))) for t in r["vert_dst"][fd].tolist()})
        assert r["duplicates"] == dup and r["n_faces"] == len(fd) - dup
        back = r["vert_dst"][f[r["face_src"]]]
        assert (np.sort(back, 1) == np.sort(r["faces"], 1)).all(), "the same faces, rotated"


def test_a_second_run_on_the_same_grid_is_stable(soup, sphere26):
    v, f, nrm = soup
    sv, sf = sphere26
    for vv, ff, nn, cell, origin in ((v, f, nrm, 0.3, (0.1, -0.2, 0.3)), (v, f, nrm, 1.0, (0.0, 0.0, 0.0)),
                                     (sv, sf, None, 0.01, CR.SPHERE26_VOL["origin"]), (sv, sf, None, 0.02, CR.SPHERE26_VOL["origin"])):
        a = PR.simplify(vv, ff, nn, cell, origin)
        b = PR.simplify(a["verts"], a["faces"], a.get("normals"), cell, origin)
        assert b["n_verts"] == a["n_verts"] == b["clusters"] and b["n_faces"] == a["n_faces"] > 0
        assert b["degenerate"] == 0 and b["duplicates"] == 0 and (b["members"] == 1).all()
        assert b["faces"].tobytes() == a["faces"].tobytes() and (b["vert_dst"] == np.arange(a["n_verts"])).all()
        ca, cb = PR.cells(a["verts"], cell, origin)[0], PR.cells(b["verts"], cell, origin)[0]
        assert (ca == cb).all(), "no vertex moves to another cell"


# ---- hand cases ------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    R = {k: PR.run_case(c) for k, c in PR.hand_cases().items()}
    assert PR.counts(R["empty"]) == dict(clusters=0, degenerate=0, duplicates=0, n_verts=0, n_faces=0)
    assert R["empty"]["verts"].shape == (0, 3) and R["empty"]["faces"].shape == (0, 3) and R["empty"]["faces"].dtype == np.int32
    r = R["vertices-no-face"]
    assert r["clusters"] == 5 and r["n_verts"] == 0 and (r["vert_dst"] == -1).all()
    r = R["one-face"]
    assert r["faces"].tolist() == [[0, 1, 2]] and r["face_src"].tolist() == [0], "rotated so that the smallest cluster comes first"
    assert r["normals"].tolist() == np.eye(3).tolist()
    # a vertex on a cell face belongs to the cell above it, with offset 0, and is reproduced exactly
    case = PR.hand_cases()["on-cell-faces"]
    c, Q = PR.cells(case["verts"], case["cell"])
    assert c.tolist() == [[-2, 0, 3], [0, 0, 1], [1, 2, -1], [0, 1, 0]] and (Q == 0).all()
    r = R["on-cell-faces"]
    assert sorted(r["verts"].tolist()) == sorted(np.asarray(case["verts"], np.float64).tolist())
    assert not np.signbit(r["verts"]).any() or (r["verts"][np.signbit(r["verts"])] < 0).all(), "-0.0 comes back as +0.0"
    case = PR.hand_cases()["on-cell-faces-origin"]
    c, Q = PR.cells(case["verts"], case["cell"], case["origin"])
    assert c.tolist() == [[-2, 0, 2], [0, 0, 0], [1, 2, -2]] and (Q == 0).all()
    assert sorted(R["on-cell-faces-origin"]["verts"].tolist()) == sorted(np.asarray(case["verts"]).tolist())
    case = PR.hand_cases()["t-rounds-to-one"]
    c, Q = PR.cells(case["verts"], case["cell"])
    assert (c[0, 0], c[1, 1], c[2, 2]) == (-1, -1, -1) and (Q[0, 0], Q[1, 1], Q[2, 2]) == (2 ** 30,) * 3
    assert sorted(R["t-rounds-to-one"]["verts"].tolist()) == sorted([[0.0, 0.5, 0.5], [1.5, 0.0, 0.5], [0.5, 1.5, 0.0]])
    r = R["same-orientation"]
    assert r["face_src"].tolist() == [0] and r["duplicates"] == 2 and r["faces"].tolist() == [[0, 1, 2]] and r["members"].tolist() == [2, 2, 2]
    r = R["opposite-orientation"]
    assert r["face_src"].tolist() == [0, 1] and r["duplicates"] == 0 and r["faces"].tolist() == [[0, 1, 2], [0, 2, 1]]
    r = R["two-corners-in-one-cell"]
    assert r["degenerate"] == 1 and r["face_src"].tolist() == [1]
    r = R["inside-one-cell"]
    assert r["clusters"] == 1 and r["degenerate"] == 2 and r["n_verts"] == 0 and r["vert_dst"].tolist() == [-1, -1, -1]
    assert r["verts"].shape == (0, 3) and r["normals"].shape == (0, 3) and r["members"].shape == (0,)
    r = R["unused-vertex"]
    assert r["verts"][0].tolist() == [0.375, 0.3125, 0.625] and r["members"].tolist() == [2, 1, 1] and r["vert_dst"].tolist() == [0, 1, 2, 0]
    r = R["zero-normal-sum"]
    assert r["normals"][0].tolist() == [0.0, 0.0, 0.0] and r["normals"][2].tolist() == [0.0, 0.0, 0.0] and not np.signbit(r["normals"]).any()
    assert np.allclose(r["normals"][1], np.array([0.0, 3.0, 1.0]) / np.sqrt(10.0), rtol=1e-15)


def test_every_invalid_input_raises():
    bad, good = PR.invalid_inputs()
    assert PR.simplify(**good)["n_faces"] == 2
    assert len(bad) == 9 + 12 + 6 + 1 + 12
    for name, case in bad:
        with pytest.raises(ValueError):
            PR.simplify(**case)
    for p in PR.BAD_PARAMS:
        with pytest.raises(ValueError):
            PR.simplify(good["verts"], good["faces"], None, **p)
    # the limits themselves are inside: a cell index of +-2^30, a normal component of +-4, a box of exactly 2^27 cells
    v = good["verts"].copy()
    v[1] = (2.0 ** 30, 0.5, 0.5)
    with pytest.raises(ValueError, match="2\\^27"):
        PR.simplify(v, good["faces"], None, 1.0)
    v[1] = (511.5, 511.5, 511.5)
    assert PR.simplify(v, good["faces"], None, 1.0)["clusters"] == 4, "512^3 cells"
    assert PR.cells([[2.0 ** 30, -2.0 ** 30, 0.0]], 1.0)[0].tolist() == [[2 ** 30, -2 ** 30, 0]]
    nr = good["normals"].copy()
    nr[0] = (4.0, -4.0, 0.0)
    assert PR.simplify(good["verts"], good["faces"], nr, 1.0)["n_faces"] == 2
    with pytest.raises(ValueError):
        PR.simplify(np.zeros((0, 3)), [[0, 0, 0]], None, 1.0)  # n = 0: every index is out of range


# ---- calibration --------------------------------------------------------------------------------------------
def test_sphere26_calibration(sphere26):
    v, f = sphere26
    vol = CR.SPHERE26_VOL
    assert (len(v), len(f)) == (22786, 45568)
    rms, mx = PR.radius_error(v, f, vol["voxel"])
    print("input: radius error %.4f / %.4f voxels, edges %.4f, outward %.4f" % (rms, mx, PR.edge_share(f), PR.outward_share(v, f)))
    G = DR.icosphere(5, CR.RADIUS)
    meshes = {0: (v, f)}
    for (factor, shift), (ints, (b_rms, b_max, b_edges, b_out)) in SPHERE_ROWS.items():
        cell = factor * vol["voxel"]
        r = PR.simplify(v, f, None, cell, tuple(o + shift * cell for o in vol["origin"]))
        rms, mx = PR.radius_error(r["verts"], r["faces"], vol["voxel"])
        edges, out = PR.edge_share(r["faces"]), PR.outward_share(r["verts"], r["faces"])
        print("%d voxels, shift %.2f: %s, max members %d; radius error %.4f / %.4f voxels, edges %.4f, outward %.4f"
              % (factor, shift, PR.counts(r), PR.max_members(r), rms, mx, edges, out))
        assert (*(r[k] for k in PR.COUNTS), PR.max_members(r)) == ints, (factor, shift)
        assert r["members"].sum() == len(v) and r["degenerate"] + r["duplicates"] + r["n_faces"] == len(f)
        assert rms <= b_rms and mx <= b_max and edges >= b_edges and out >= b_out, (factor, shift)
        if shift == 0.0:
            meshes[factor] = (r["verts"], r["faces"])
    assert SPHERE_ROWS[(3, -0.37)][0][2] == 1 and SPHERE_ROWS[(4, 0.0)][0][2] == 2, "the fixture itself hits the duplicate rule"
    for factor, (ints, bound) in SPHERE_ACC.items():
        e = DR.evaluate(*meshes[factor], *G, 4 * vol["voxel"], vol["voxel"])
        print("%d voxels: accuracy %.6f (mean %.6f, max %.6f, %d of %d within tau), completeness %.4f (%d of %d)"
              % (factor, e["accuracy"], e["acc_mean"], e["acc_max"], e["acc_within"], e["n_rec"], e["completeness"], e["comp_within"], e["n_gt"]))
        assert (e["n_rec"], e["acc_within"], e["comp_within"]) == ints and e["accuracy"] <= bound and e["completeness"] == 1.0, factor


def test_ring6_calibration():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    views = []
    for a, b in pairs:
        r = SR.rectify(K, poses[a][0], poses[a][1], poses[b][0], poses[b][1])
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        views.append((r, SR.disparity(il, ir, r["H_l"], r["H_r"], dict(num_disparities=64))))
    vol = CR.RING6_VOL
    m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(views, CR.filter_views(views)))
    assert (len(m["verts"]), len(m["faces"])) == (7552, 13622)
    r = PR.simplify(m["verts"], m["faces"], None, 2 * vol["voxel"], vol["origin"])
    edges, out = PR.edge_share(r["faces"]), PR.outward_share(r["verts"], r["faces"])
    print("ring-6, filter on, 2 voxels: %s, max members %d; edges %.4f (before %.4f), outward %.4f (before %.4f)"
          % (PR.counts(r), PR.max_members(r), edges, PR.edge_share(m["faces"]), out, PR.outward_share(m["verts"], m["faces"])))
    assert (*(r[k] for k in PR.COUNTS), PR.max_members(r)) == RING_ON_ROW
    assert edges >= RING_ON_EDGES and out >= RING_ON_OUTWARD
    assert CR.mesh_quality(r["verts"], r["faces"])[1] == 1.0, "a mean of vertices in the shell... stays in the shell here"


# ---- library and Python layer ----------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.simplify_default_params() == dict(cell=0.0, origin=(0.0, 0.0, 0.0))
    assert capi.SIMPLIFY_DEFAULTS == PR.DEFAULTS and capi.simplify_default_params() == dict(cell=0.0, **capi.SIMPLIFY_DEFAULTS)
    assert not capi.simplify_check_params(**capi.simplify_default_params()), "cell has no default"
    assert not capi.simplify_check_params() and not PR.check_params()
    for good in (dict(cell=1.0), dict(cell=5e-324), dict(cell=1.7e308), dict(cell=0.01, origin=(-1.5, 2.0, 1e300))):
        assert capi.simplify_check_params(**good) and PR.check_params(**good), good
    for bad in PR.BAD_PARAMS:
        assert not capi.simplify_check_params(**bad) and not PR.check_params(**bad), bad
    lib = capi.load_library()
    assert lib.sfmx_simplify_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_simplify_default_params(None)  # tolerated
    for s in capi.SYMBOLS:
        if s.startswith("sfmx_simplify_"):
            assert hasattr(lib, s), s
    assert sum(s.startswith("sfmx_simplify_") for s in capi.SYMBOLS) == 13
    assert lib.sfmx_simplify_sizes(None, None, None, None, None) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_simplify_counts(None, None, None, None, None, None) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_simplify_device_surface(None, None, None) == -1 and lib.sfmx_simplify_device_mesh(None, None, None, None) == -1


def test_python_layer_key_checks():
    with pytest.raises(TypeError):
        capi.simplify_params(1.0, grid=2)
    assert set(pipe.SIMPLIFY_KEYS) == {"factor", "cell", "origin"}
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    for bad in (dict(cells=1), dict(factor=2.0, step=1), dict(factor=2.0, cell=0.2)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, simplify=bad)
    assert inspect.signature(pipe.fuse).parameters["simplify"].default is False
    assert hasattr(capi.Context, "simplify") and hasattr(capi.Simplify, "fusion") and hasattr(capi.Simplify, "clean")
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_sp")
