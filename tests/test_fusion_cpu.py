"""CPU suite: multi-pair depth fusion -- the NumPy restatement (tests/fusion_ref.py) on analytic sphere views (a closed,
consistently oriented surface at the right radius), its triangle table against the rule, and parameter validation of the
device stage (sfmx_fusion_check_params needs no device)."""
import importlib
import itertools
from collections import Counter

import numpy as np
import pytest

import fusion_ref as FR
import helpers as H

capi = importlib.import_module(H.PKG_NAME + ".capi")

# 26 views around a sphere of radius 0.1 from 0.5 away.  f B = 30: one disparity step (1/16 px) is ~3e-4 in depth at
# Z = 0.4, well under the 5 mm voxel.
SPHERE = dict(radius=0.1, w=320, h=320, f=600.0, n_views=26)
VOL = dict(origin=(-0.15, -0.15, -0.15), voxel=0.005, dims=(61, 61, 61))


def sphere_views(radius=0.1, w=320, h=320, f=600.0, n_views=26):
    out = []
    for d in FR.fibonacci_dirs(n_views):
        cam = FR.look_at_cam(0.5 * d, (0.0, 0.0, 0.0), f, w, h)
        out.append((cam, FR.sphere_disp16(cam, w, h, radius)))
    return out


@pytest.fixture(scope="module")
def sphere():
    views = sphere_views(**SPHERE)
    return views, FR.fuse(VOL["origin"], VOL["voxel"], VOL["dims"], views)


def test_sphere_mesh_closed_and_oriented(sphere):
    _, r = sphere
    v, F = r["verts"], r["faces"]
    assert len(F) > 10000
    E = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    directed = Counter(map(tuple, E.tolist()))
    assert max(directed.values()) == 1, "a directed edge appears twice: inconsistent orientation"
    assert all((b, a) in directed for a, b in directed), "an edge without its reverse: the mesh is open"
    undirected = {tuple(sorted(e)) for e in directed}
    assert len(v) - len(undirected) + len(F) == 2, "Euler characteristic"
    assert len(np.unique(F)) == len(v), "every vertex is used"
    n = np.cross(v[F[:, 1]] - v[F[:, 0]], v[F[:, 2]] - v[F[:, 0]])
    assert ((n * v[F].mean(1)).sum(1) > 0).all(), "normals point outward"


def test_sphere_radius(sphere):
    """RMS 0.10 voxel, max 0.43 (the projective distances of 26 directions averaged on a curved surface)"""
    _, r = sphere
    e = (np.linalg.norm(r["verts"], axis=1) - SPHERE["radius"]) / VOL["voxel"]
    assert np.sqrt((e ** 2).mean()) < 0.25
    assert np.percentile(np.abs(e), 99) < 0.3
    assert np.abs(e).max() < 0.5


def test_batching_does_not_change_bits(sphere):
    views, r = sphere
    s, c = None, None
    for v in views:
        s, c = FR.integrate(VOL["origin"], VOL["voxel"], VOL["dims"], [v], sum_=s, count=c)
    H.assert_bits_equal(s, r["sum"], "one view at a time")
    assert (c == r["count"]).all()


def test_table_matches_rule():
    """all 6 x 16 cases: the triangles cover exactly the crossing edges, in the rule's pattern, oriented outward"""
    tets = FR.tets()
    assert tets == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]
    # the six tets tile the cube: volumes 1/6 each, all positive orientation sign the same magnitude
    vols = [abs(np.linalg.det(np.stack([FR.corner_xyz(c) for c in ch[1:]]))) for ch in tets]
    assert vols == [1.0] * 6
    for t, chain in enumerate(tets):
        P = np.array([FR.corner_xyz(c) for c in chain], np.float64)
        for case in range(16):
            ins = [q for q in range(4) if case >> q & 1]
            outs = [q for q in range(4) if not case >> q & 1]
            n = FR.NTRI[t, case]
            assert n == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[len(ins)]
            crossing = {tuple(sorted((chain[a], chain[b]))) for a in ins for b in outs}
            used = set()
            for k in range(n):
                pts = []
                for lo, slot in FR.TRI[t, case, k]:
                    hi = lo + int(FR.D7[slot] @ [1, 2, 4])
                    assert (lo & hi) == lo and hi != lo and hi < 8, "edge runs from a corner to a superset corner"
                    used.add((int(lo), int(hi)))
                    pts.append((FR.corner_xyz(lo) + FR.corner_xyz(hi)) / 2.0)
                nrm = np.cross(pts[1] - pts[0], pts[2] - pts[0])
                d = P[outs].mean(0) - P[ins].mean(0)
                assert nrm @ d > 0, f"tet {t} case {case} triangle {k} points inward"
            assert used == crossing, f"tet {t} case {case}"
            if len(ins) == 2:  # quad (a,c) (a,d) (b,d) (b,c) split on (a,c)-(b,d)
                a, b = (chain[q] for q in ins)
                c, d = (chain[q] for q in outs)
                diag = {tuple(sorted((a, c))), tuple(sorted((b, d)))}
                for k in range(2):
                    tri = {(int(lo), int(lo + FR.D7[s] @ [1, 2, 4])) for lo, s in FR.TRI[t, case, k]}
                    assert diag <= tri


def test_tiny_volume_and_min_weight():
    """one view, 2x2x2 points: a plane crossing the cell; min_weight above the count leaves it undefined"""
    cam = FR.look_at_cam((0.0, 0.0, -1.0), (0.0, 0.0, 0.0), 100.0, 64, 64, B=0.1)
    d16 = np.full((64, 64), int(round(16 * 100.0 * 0.1 / 1.0)), np.int16)  # Z = 1: the plane z = 0
    s, c = FR.integrate((-0.01, -0.01, -0.01), 0.02, (2, 2, 2), [(cam, d16)])
    assert (c == 1).all()
    v, f = FR.extract(s, c, (-0.01, -0.01, -0.01), 0.02)
    assert len(f) > 0 and np.abs(v[:, 2]).max() < 1e-12
    v2, f2 = FR.extract(s, c, (-0.01, -0.01, -0.01), 0.02, min_weight=2)
    assert len(v2) == 0 and len(f2) == 0


def _ok(**kw):
    return capi.fusion_check_params(**kw)


def test_check_params():
    d = capi.fusion_default_params()
    assert d["voxel"] == 0.0 and d["dims"] == (0, 0, 0) and d["trunc"] == 0.0 and d["disp_min"] == 1.0
    assert d["min_weight"] == 1 and d["max_views"] == 64
    assert not _ok(), "bare defaults have no volume"
    vol = dict(origin=(-1.0, -1.0, -1.0), voxel=0.01, dims=(64, 64, 64))
    assert _ok(**vol)
    for bad in [dict(dims=(1, 64, 64)), dict(dims=(64, 1, 64)), dict(dims=(64, 64, 1)), dict(voxel=0.0), dict(voxel=-0.01),
                dict(trunc=-1e-3), dict(min_weight=0), dict(dims=(512, 512, 513)), dict(voxel=float("nan")), dict(max_views=0)]:
        assert not _ok(**{**vol, **bad}), bad
    assert _ok(**{**vol, "dims": (512, 512, 512)}), "exactly 2^27 points"
    assert _ok(**{**vol, "trunc": 0.05, "min_weight": 3, "max_views": 1})


def test_kuhn_chains_are_the_lexicographic_permutations():
    perms = list(itertools.permutations(range(3)))
    assert [(0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7) for p in perms] == FR.tets()
