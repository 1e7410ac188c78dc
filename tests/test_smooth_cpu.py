"""CPU suite: exact Taubin lambda|mu smoothing of the fused surface -- properties and hand cases of the NumPy restatement
(tests/smooth_ref.py), its calibration on the clean sphere-26 and the filtered ring-6 surfaces of DESIGN.md 13 / 15 (fused by
tests/fusion_ref.py), and parameter validation of the device stage (sfmx_smooth_check_params needs no device).

Bounds (the rule of DESIGN.md 15): 1.25 x the value the restatement gives on the fixture, rounded up to 0.01 voxel (radius
errors, the largest move) or to 0.1 degree (roughness), or 1.25 x the distance to 100 % rounded up to half a percentage point
(shares); DESIGN.md 21 has the table.  The integer columns are stated exactly: the restatement is deterministic."""
import importlib
import inspect

import numpy as np
import pytest

import clean_ref as LR
import consist_ref as CR
import fusion_ref as FR
import helpers as H
import simplify_ref as PR
import smooth_ref as MR
import stereo_ref as SR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")

# the clean sphere-26 surface (22 786 v / 45 568 f; radius error 0.1045 / 0.4273 voxels, roughness 14.31 degrees, closed:
# 68 352 edges, all regular), lambda 0.5, mu -0.53, unit = the voxel: pairs -> bounds on the radius error RMS and max (voxels),
# the roughness (degrees), the outward faces and the largest move of a vertex (voxels)
SPHERE_COUNTS = dict(edges=68352, boundary_edges=0, irregular_edges=0, pinned=0, isolated=0)
SPHERE_BEFORE = (0.1045, 0.4274, 14.32)
SPHERE_ROWS = {
    5: (0.12, 0.52, 9.3, 0.995, 0.66),   # measured 0.0916, 0.4082, 7.44 degrees, 99.996 %, 0.525
    10: (0.11, 0.46, 6.6, 1.0, 0.85),    # measured 0.0879, 0.3674, 5.24 degrees, 100 %, 0.677
    20: (0.11, 0.41, 4.6, 1.0, 0.99),    # measured 0.0857, 0.3225, 3.65 degrees, 100 %, 0.791
}
# ring-6, filter on (7 552 v / 13 622 f; roughness 26.23 degrees, outward 97.69 %, edges used once in each direction 92.96 %),
# 10 pairs: pin -> the counts, then bounds on the roughness, the outward faces and the largest move
RING_EDGES = dict(edges=21179, boundary_edges=1492, irregular_edges=0, isolated=0)
RING_ROWS = {
    1: (1482, 22.7, 0.975, 1.11),  # measured 18.12 degrees, 98.26 %, 0.883
    0: (0, 18.7, 0.98, 1.11),      # measured 14.96 degrees, 98.49 %, 0.883
}


@pytest.fixture(scope="module")
def soup():
    v, f, _ = LR.soup()
    return v, f


@pytest.fixture(scope="module")
def sphere26():
    views, _ = CR.sphere26(False)
    vol = CR.SPHERE26_VOL
    m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], views)
    return m["verts"], m["faces"]


def _same(a, b):
    assert a["verts"].tobytes() == b["verts"].tobytes() and a["flags"].tobytes() == b["flags"].tobytes() and MR.counts(a) == MR.counts(b)


# ---- properties ------------------------------------------------------------------------------------------------------------
def _check_properties(v, f, **kw):
    a = MR.smooth(v, f, **kw)
    # the faces in another order, and each face starting at another corner: nothing changes
    rng = np.random.default_rng(31)
    _same(a, MR.smooth(v, f[rng.permutation(len(f))], **kw))
    rot = rng.integers(0, 3, len(f))
    fr = np.stack([f[np.arange(len(f)), (rot + j) % 3] for j in range(3)], 1)
    assert (rot > 0).any()
    _same(a, MR.smooth(v, fr, **kw))
    # the vertices in another order, the faces relabelled: the output is permuted the same way
    v2, f2, _, perm = MR.permute_vertices(v, f, None, 32)
    c = MR.smooth(v2, f2, **kw)
    assert c["verts"].tobytes() == a["verts"][perm].tobytes() and c["flags"].tobytes() == a["flags"][perm].tobytes()
    assert MR.counts(a) == MR.counts(c)
    return a


def test_orders_and_rotations_change_nothing(soup, sphere26):
    v, f = soup
    for pin in (1, 0):
        a = _check_properties(v, f, unit=0.01, origin=(0.1, -0.2, 0.3), pin=pin, iters=3)
        moved = (a["verts"] != v).any(1)
        assert moved.sum() > (0 if pin else 15000), "nearly every edge of the soup is a boundary edge: it moves with pin = 0"
    sv, sf = sphere26
    a = _check_properties(sv, sf, unit=CR.SPHERE26_VOL["voxel"], origin=CR.SPHERE26_VOL["origin"], iters=2)
    assert (a["verts"] != sv).any(1).all() and not a["flags"].any()


def test_pinned_and_isolated_vertices_keep_their_bytes(soup):
    v, f = soup
    r = MR.smooth(v, f, unit=0.01, pin=1)
    lo, hi, fwd, bwd = MR.edge_table(f, len(v))
    bad = ~((fwd == 1) & (bwd == 1))
    ends = np.unique(np.concatenate([lo[bad], hi[bad]]))
    assert len(ends) == r["pinned"] > 10000 and (r["flags"][ends] == MR.PINNED).all()
    assert r["verts"][ends].tobytes() == v[ends].tobytes()
    iso = np.nonzero(r["flags"] == MR.ISOLATED)[0]
    assert len(iso) == r["isolated"] > 1000 and r["verts"][iso].tobytes() == v[iso].tobytes()
    assert ((r["flags"] == 0) == (r["verts"] != v).any(1)).mean() > 0.99, "the others move (a few land where they were)"
    assert r["edges"] == len(lo) and r["boundary_edges"] == int((fwd + bwd == 1).sum())
    assert r["irregular_edges"] == int((bad & (fwd + bwd != 1)).sum())
    free = MR.smooth(v, f, unit=0.01, pin=0)
    assert free["pinned"] == 0 and not (free["flags"] & MR.PINNED).any() and free["isolated"] == r["isolated"]
    assert (free["verts"][ends] != v[ends]).any()


def test_only_isolated_vertices_come_back_byte_equal():
    v = np.random.default_rng(33).standard_normal((1000, 3))
    v[::7] = -0.0
    for f in (MR.F0, np.array([[5, 5, 5], [0, 0, 0]], np.int32)):
        r = MR.smooth(v, f, unit=1e-3, iters=64, pin=0)
        assert r["verts"].tobytes() == v.tobytes() and (r["flags"] == MR.ISOLATED).all()
        assert MR.counts(r) == dict(edges=0, boundary_edges=0, irregular_edges=0, pinned=0, isolated=1000)


# ---- hand cases ------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    C = MR.hand_cases()
    R = {k: MR.run_case(c) for k, c in C.items()}
    zero = dict(edges=0, boundary_edges=0, irregular_edges=0, pinned=0, isolated=0)
    assert MR.counts(R["empty"]) == zero and R["empty"]["verts"].shape == (0, 3) and R["empty"]["flags"].shape == (0,)
    assert R["empty"]["flags"].dtype == np.uint8
    assert MR.counts(R["only-isolated"]) == dict(zero, isolated=5)
    r = R["triangle-pinned"]
    assert MR.counts(r) == dict(zero, edges=3, boundary_edges=3, pinned=3) and r["flags"].tolist() == [1, 1, 1]
    assert r["verts"].tobytes() == np.asarray(C["triangle-pinned"]["verts"]).tobytes()
    r = R["triangle-free"]
    assert MR.counts(r) == dict(zero, edges=3, boundary_edges=3) and r["flags"].tolist() == [0, 0, 0]
    v0 = np.asarray(C["triangle-free"]["verts"])
    assert (r["verts"] != v0).any(1).all() and np.abs(r["verts"].mean(0) - v0.mean(0)).max() < 1e-4, "about the centroid"
    assert MR.counts(R["shared-edge-opposite"]) == dict(zero, edges=5, boundary_edges=4)
    assert MR.counts(R["shared-edge-same"]) == dict(zero, edges=5, boundary_edges=4, irregular_edges=1)
    r = R["shared-edge-same-pinned"]
    assert MR.counts(r) == dict(zero, edges=5, boundary_edges=4, irregular_edges=1, pinned=4) and (r["flags"] == 1).all()
    assert R["shared-edge-same"]["verts"].tobytes() == R["shared-edge-opposite"]["verts"].tobytes(), "the same neighbours"
    assert MR.counts(R["tetrahedron"]) == dict(zero, edges=6)
    r = R["edge-used-three-times"]
    assert MR.counts(r) == dict(zero, edges=8, boundary_edges=2, irregular_edges=1, pinned=3) and r["flags"].tolist() == [1, 1, 0, 0, 1]
    r = R["face-a-a-b"]  # 3->3 is ignored, 3->1 counts: edge {1, 3} is used twice as 3->1 (bwd = 2) and once as 1->3
    assert MR.counts(r) == dict(zero, edges=6, irregular_edges=1, pinned=2) and r["flags"].tolist() == [0, 1, 0, 1]
    assert MR.counts(R["face-a-a-a"]) == dict(zero, edges=6)
    assert R["face-a-a-a"]["verts"].tobytes() == R["tetrahedron"]["verts"].tobytes()
    r = R["unused-vertex"]
    assert MR.counts(r) == dict(zero, edges=6, isolated=1) and r["flags"].tolist() == [0, 0, 0, 0, 2]
    assert r["verts"][4].tolist() == [9.0, 9.0, 9.0] and r["verts"][:4].tobytes() == R["tetrahedron"]["verts"].tobytes()
    r = R["minus-zero"]
    assert np.signbit(r["verts"][4]).all(), "an isolated vertex keeps its -0.0"
    assert (MR.quantise(C["minus-zero"]["verts"], 1.0) == MR.quantise(np.abs(C["minus-zero"]["verts"]), 1.0)).all()
    assert r["verts"][:4].tobytes() == MR.smooth(np.abs(C["minus-zero"]["verts"]), C["minus-zero"]["faces"], unit=1.0)["verts"][:4].tobytes()
    for name in ("at-the-limit", "at-the-limit-origin"):
        c = C[name]
        Q = MR.quantise(c["verts"], c["unit"], c.get("origin", (0.0, 0.0, 0.0)))
        assert np.abs(Q).max() == 2 ** 38 and MR.counts(R[name]) == dict(zero, edges=6)
    # mu = 0: the odd steps move nothing, so 3 pairs are 3 lambda steps; lambda = 1: the vertex goes to the mean of its neighbours
    c = C["mu-zero"]
    Q = MR.quantise(c["verts"], c["unit"])
    for _ in range(3):
        S = Q.sum(0)[None, :] - Q  # a tetrahedron: every other vertex is a neighbour
        Q = Q + np.floor(0.5 * (S.astype(np.float64) / 3.0 - Q.astype(np.float64)) + 0.5).astype(np.int64)
    assert R["mu-zero"]["verts"].tobytes() == ((Q.astype(np.float64) * 2.0 ** -20) * c["unit"]).tobytes()
    c = C["lambda-one"]
    Q = MR.quantise(c["verts"], c["unit"])
    S = Q.sum(0)[None, :] - Q
    Q1 = Q + np.floor(1.0 * (S.astype(np.float64) / 3.0 - Q.astype(np.float64)) + 0.5).astype(np.int64)
    assert np.abs(3 * Q1 - S).max() <= 2, "one lambda = 1 step: the rounded mean of the neighbours"
    # halves round up, towards +infinity, for positive and negative moves alike
    assert int(np.floor(0.5 * 1.0 + 0.5)) == 1 and int(np.floor(0.5 * -1.0 + 0.5)) == 0 and int(np.floor(-0.5 * 3.0 + 0.5)) == -1
    assert (R["half-way-rounding"]["verts"] != np.asarray(C["half-way-rounding"]["verts"])).any()


def test_every_invalid_input_raises():
    bad, good = MR.invalid_inputs()
    assert MR.smooth(**good)["edges"] == 5
    assert len(bad) == 30 + 12 + 1
    for name, case in bad:
        with pytest.raises(ValueError):
            MR.smooth(**case)
    for p in MR.BAD_PARAMS:
        with pytest.raises(ValueError):
            MR.smooth(good["verts"], good["faces"], **p)
    # the limits themselves are inside: |q| = 2^18 exactly, the last vertex index
    v = good["verts"].copy()
    v[3] = (2.0 ** 18, -2.0 ** 18, 0.0)
    v[4] = (-2.0 ** 18, 2.0 ** 18, 2.0 ** 18)
    assert np.abs(MR.quantise(v, 1.0)).max() == 2 ** 38
    assert MR.smooth(v, good["faces"], unit=1.0)["isolated"] == 1
    f = good["faces"].copy()
    f[1, 1] = 4
    assert MR.smooth(good["verts"], f, unit=1.0)["isolated"] == 1
    with pytest.raises(ValueError):
        MR.smooth(v * 2.0, good["faces"], unit=1.0)
    assert MR.smooth(v * 2.0, good["faces"], unit=2.0)["edges"] == 5


def test_divergence():
    """lambda = 1, mu = -1 on a free unit triangle: a lambda step maps the offset d from the centroid to -d / 2 and the mu step
    that to -5 d / 4, so the triangle grows by 1.25 per pair: 1.25^32 = 1 262 stays below 2^18 units, 1.25^64 = 1.6 10^6 does
    not"""
    v, f = MR.UNIT_TRIANGLE
    r = MR.smooth(v, f, iters=1, **MR.DIVERGING)
    d0, d1 = v - v.mean(0), r["verts"] - r["verts"].mean(0)
    assert np.abs(d1 + 1.25 * d0).max() < 1e-5 and np.abs(r["verts"].mean(0) - v.mean(0)).max() < 1e-5
    r = MR.smooth(v, f, iters=32, **MR.DIVERGING)
    assert abs(np.abs(r["verts"]).max() - (1.0 / 3.0 + 2.0 / 3.0 * 1.25 ** 32)) < 0.5, "vertex 1 lies 2 / 3 from the centroid"
    with pytest.raises(ValueError, match="diverged"):
        MR.smooth(v, f, iters=64, **MR.DIVERGING)


# ---- calibration --------------------------------------------------------------------------------------------
def test_sphere26_calibration(sphere26):
    v, f = sphere26
    vol = CR.SPHERE26_VOL
    assert (len(v), len(f)) == (22786, 45568)
    rms, mx = MR.radius_error(v, f, vol["voxel"])
    rough = MR.roughness(v, f)
    print("input: radius error %.4f / %.4f voxels, roughness %.2f degrees, outward %.5f" % (rms, mx, rough, MR.outward_share(v, f)))
    assert rms <= SPHERE_BEFORE[0] and mx <= SPHERE_BEFORE[1] and rough <= SPHERE_BEFORE[2]
    last = (rms, mx, rough)
    for iters, (b_rms, b_max, b_rough, b_out, b_move) in SPHERE_ROWS.items():
        r = MR.smooth(v, f, unit=vol["voxel"], origin=vol["origin"], iters=iters)
        rms, mx = MR.radius_error(r["verts"], f, vol["voxel"])
        rough, out, move = MR.roughness(r["verts"], f), MR.outward_share(r["verts"], f), MR.max_move(v, r["verts"], vol["voxel"])
        print("%d pairs: %s; radius error %.4f / %.4f voxels, roughness %.2f degrees, outward %.5f, largest move %.3f voxels"
              % (iters, MR.counts(r), rms, mx, rough, out, move))
        assert MR.counts(r) == SPHERE_COUNTS and not r["flags"].any(), iters
        assert rms <= b_rms and mx <= b_max and rough <= b_rough and out >= b_out and move <= b_move, iters
        assert rms < last[0] and mx < last[1] and rough < last[2], "more pairs, a smoother and a rounder sphere"
        last = (rms, mx, rough)
    assert 1.0 - SPHERE_COUNTS["boundary_edges"] / SPHERE_COUNTS["edges"] == PR.edge_share(f) == 1.0


def test_ring6_calibration():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    views = []
    for a, b in pairs:
        r = SR.rectify(K, poses[a][0], poses[a][1], poses[b][0], poses[b][1])
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        views.append((r, SR.disparity(il, ir, r["H_l"], r["H_r"], dict(num_disparities=64))))
    vol = CR.RING6_VOL
    m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(views, CR.filter_views(views)))
    v, f = m["verts"], m["faces"]
    assert (len(v), len(f)) == (7552, 13622)
    rough0, out0 = MR.roughness(v, f), MR.outward_share(v, f)
    print("input: roughness %.2f degrees, outward %.4f, edges %.4f" % (rough0, out0, PR.edge_share(f)))
    for pin, (pinned, b_rough, b_out, b_move) in RING_ROWS.items():
        r = MR.smooth(v, f, unit=vol["voxel"], origin=vol["origin"], pin=pin)
        rough, out, move = MR.roughness(r["verts"], f), MR.outward_share(r["verts"], f), MR.max_move(v, r["verts"], vol["voxel"])
        print("pin %d: %s; roughness %.2f degrees, outward %.4f, largest move %.3f voxels" % (pin, MR.counts(r), rough, out, move))
        assert MR.counts(r) == dict(RING_EDGES, pinned=pinned), pin
        assert rough <= b_rough and rough < rough0 and out >= b_out and out > out0 and move <= b_move, pin
        assert CR.mesh_quality(r["verts"], f)[1] == 1.0, "every vertex stays in the shell"
        # no irregular edge here, so the regular share is the complement of the boundary share: the figure of DESIGN.md 20
        assert r["irregular_edges"] == 0 and (r["edges"] - r["boundary_edges"]) / r["edges"] == PR.edge_share(f)
    assert abs((1.0 - RING_EDGES["boundary_edges"] / RING_EDGES["edges"]) - 0.9296) < 5e-5


# ---- library and Python layer ----------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.smooth_default_params() == dict(unit=0.0, origin=(0.0, 0.0, 0.0), lam=0.5, mu=-0.53, iters=10, pin=1)
    assert capi.SMOOTH_DEFAULTS == MR.DEFAULTS and capi.smooth_default_params() == dict(unit=0.0, **capi.SMOOTH_DEFAULTS)
    assert capi.SMOOTH_COUNTS == MR.COUNTS
    assert not capi.smooth_check_params(**capi.smooth_default_params()), "unit has no default"
    assert not capi.smooth_check_params() and not MR.check_params()
    for good in MR.GOOD_PARAMS:
        assert capi.smooth_check_params(**good) and MR.check_params(**good), good
    for bad in MR.BAD_PARAMS:
        assert not capi.smooth_check_params(**bad) and not MR.check_params(**bad), bad
    with pytest.raises(TypeError):
        capi.smooth_params(1.0, iters=2.5)
    lib = capi.load_library()
    assert lib.sfmx_smooth_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_smooth_default_params(None)  # tolerated
    for s in capi.SYMBOLS:
        if s.startswith("sfmx_smooth_"):
            assert hasattr(lib, s), s
    assert sum(s.startswith("sfmx_smooth_") for s in capi.SYMBOLS) == 13
    assert lib.sfmx_smooth_sizes(None, None, None) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_smooth_counts(None, None, None, None, None, None) == capi.SFMX_ERR_INVALID
    assert lib.sfmx_smooth_device_mesh(None, None, None, None) == -1 and lib.sfmx_smooth_device_surface(None, None, None) == -1
    assert lib.sfmx_smooth_last_us(None) == 0.0
    header = open(H.ROOT + "/include/sfmx.h").read()
    for s in capi.SYMBOLS:
        if s.startswith("sfmx_smooth_"):
            assert s + "(" in header, s


def test_python_layer_key_checks():
    with pytest.raises(TypeError):
        capi.smooth_params(1.0, lambda_=0.5)
    assert pipe.SMOOTH_KEYS == ("iters", "lam", "mu", "pin", "unit", "origin")
    assert set(pipe.SMOOTH_KEYS) == set(capi.SMOOTH_DEFAULTS) | {"unit"}
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    for bad in (dict(iter=1), dict(iters=2, lamda=0.5), dict(cell=0.2), dict(iters=2.5)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, smooth=bad)
    assert inspect.signature(pipe.fuse).parameters["smooth"].default is False
    assert hasattr(capi.Context, "smooth") and all(hasattr(capi.Smooth, k) for k in ("run", "fusion", "clean", "read", "device_mesh"))
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_sm") and hasattr(lib, "sfmx_host_fusion_mesh_sp")
