"""CPU suite: appearance of the fused surface -- the NumPy restatement (tests/appearance_ref.py) on a textured sphere (normals
against the radial direction, vertex grey against the texture, what the two visibility tests are for), on two spheres that
hide each other (where the depth test decides), the gradient's four branches on a hand-set volume, independence of the view
batching, and parameter validation of the device stage (sfmx_shade_check_params needs no device).

Bounds: 1.25 x the value the restatement gives on the fixture, rounded up to the next 0.5 (DESIGN.md 14 has the table).  The
result is deterministic; the margin only covers an honest difference in how an image fixture is rendered."""
import importlib

import numpy as np
import pytest

import appearance_ref as AR
import fusion_ref as FR
import helpers as H
from test_fusion_cpu import SPHERE, VOL

capi = importlib.import_module(H.PKG_NAME + ".capi")


@pytest.fixture(scope="module")
def sphere():
    views = AR.textured_sphere_views(**SPHERE)
    return views, AR.fuse(VOL["origin"], VOL["voxel"], VOL["dims"], views)


@pytest.fixture(scope="module")
def two():
    views = AR.two_sphere_views()
    return views, AR.fuse(AR.TWO_VOL["origin"], AR.TWO_VOL["voxel"], AR.TWO_VOL["dims"], views)


def _radial(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def _err(grey, v):
    return np.abs(grey.astype(np.float64) - AR.texture(SPHERE["radius"] * _radial(v)))


def test_fixture_images_match_fusion_fixture(sphere):
    """the textured views carry test_fusion_cpu's disparity maps, and an image that is 0 exactly where the map is invalid"""
    views, r = sphere
    assert len(r["verts"]) == 22786
    for (cam, d16, img) in views[:3]:
        assert (d16 == FR.sphere_disp16(cam, SPHERE["w"], SPHERE["h"], SPHERE["radius"])).all()
        assert ((img == 0) == (d16 == -16)).all()
        assert img[d16 != -16].min() >= 28 and img.max() <= 228


def test_sphere_normals(sphere):
    """measured: no zero normal; angle to the radial direction mean 4.58, p99 12.15, max 16.27 degrees"""
    _, r = sphere
    v, n = r["verts"], r["normals"]
    ln = np.linalg.norm(n, axis=1)
    print("zero-length normals", int((ln == 0).sum()))
    assert (ln > 0).all()
    assert np.abs(ln - 1.0).max() < 1e-15 * 4
    dot = (n * _radial(v)).sum(1)
    assert (dot > 0).all(), "a normal points into the sphere"
    ang = np.degrees(np.arccos(np.clip(dot, -1.0, 1.0)))
    print("angle mean %.3f p99 %.3f max %.3f" % (ang.mean(), np.percentile(ang, 99), ang.max()))
    assert ang.mean() <= 6.0 and np.percentile(ang, 99) <= 15.5 and ang.max() <= 20.5


def test_sphere_grey_and_visibility_tests(sphere):
    """measured (depth_tol = trunc 0.02, cull on): views 6..13, mean 9.4; |grey - T| mean 0.41, p99 1.81, max 3.60.
    depth_tol 1.0 and cull off: views 18..26, error mean 18.5 (max 55.2).  depth_tol 1.0, cull on: mean 0.42, max 4.85."""
    views, r = sphere
    v, n, g, c = r["verts"], r["normals"], r["grey"], r["vertex_views"]
    assert g.dtype == np.uint8 and c.dtype == np.int32
    e = _err(g, v)
    print("default: views %d..%d mean %.2f; error mean %.3f p99 %.3f max %.3f" % (c.min(), c.max(), c.mean(), e.mean(),
                                                                                    np.percentile(e, 99), e.max()))
    assert (c >= 1).all(), "an uncoloured vertex"
    assert e.mean() <= 1.0 and np.percentile(e, 99) <= 2.5 and e.max() <= 4.5
    g0, c0 = AR.shade(v, n, views, 1.0, cull=0)
    e0 = _err(g0, v)
    print("no tests: views %d..%d; error mean %.3f max %.3f" % (c0.min(), c0.max(), e0.mean(), e0.max()))
    assert (c0 > c).all(), "without the tests every vertex is also seen from behind"
    assert e0.mean() >= 10.0 * e.mean(), "the visibility tests do nothing"
    g1, c1 = AR.shade(v, n, views, 1.0, cull=1)
    e1 = _err(g1, v)
    print("cull only: error mean %.3f max %.3f" % (e1.mean(), e1.max()))
    assert (c1 >= 1).all()
    assert e1.mean() <= 1.0 and e1.max() <= 6.5


def test_two_spheres_depth_test_decides(two):
    """measured: 26 160 vertices, 22 764 on A, 3 396 on B; with depth_tol = trunc every vertex has its own sphere's grey; with
    depth_tol 1.0, 2 909 A vertices and 1 849 B vertices take the other sphere's pixels too (culling cannot tell)"""
    views, r = two
    v, n, g, c = r["verts"], r["normals"], r["grey"], r["vertex_views"]
    A, B = AR.two_sphere_labels(v)
    print("vertices", len(v), "A", int(A.sum()), "B", int(B.sum()))
    assert A.sum() > 10000 and B.sum() > 1000 and not (A & B).any() and (A | B).all()
    assert (np.linalg.norm(n, axis=1) > 0).all()
    assert (c >= 1).all(), "an uncoloured vertex"
    assert (g[A] == AR.TWO["A"]["grey"]).all() and (g[B] == AR.TWO["B"]["grey"]).all()
    g1, _ = AR.shade(v, n, views, 1.0)
    offA, offB = int((g1[A] != AR.TWO["A"]["grey"]).sum()), int((g1[B] != AR.TWO["B"]["grey"]).sum())
    print("depth_tol 1.0: off A", offA, "max", int(g1[A].max()), "off B", offB, "min", int(g1[B].min()))
    assert offA >= 1 and offB >= 1


def test_view_batching_does_not_change_bytes(sphere):
    views, r = sphere
    for chunk in (1, 7, 26):
        g, c = AR.shade(r["verts"], r["normals"], views, 0.02, chunk=chunk)
        assert g.tobytes() == r["grey"].tobytes() and c.tobytes() == r["vertex_views"].tobytes(), chunk


def test_fill_zero_views_and_no_normals(sphere):
    views, r = sphere
    v = r["verts"][:100]
    g, c = AR.shade(v, None, [], 0.02, cull=0, fill=77)
    assert (g == 77).all() and (c == 0).all()
    g, c = AR.shade(v, np.zeros_like(v), views, 0.02, cull=1, fill=9)
    assert (g == 9).all() and (c == 0).all(), "a zero normal fails the strict test"
    g, c = AR.shade(np.zeros((0, 3)), np.zeros((0, 3)), views, 0.02)
    assert g.shape == (0,) and c.shape == (0,)
    # rounding of the mean: (2 acc + cnt) / (2 cnt) rounds halves up
    cam = FR.look_at_cam((0.0, 0.0, -1.0), (0.0, 0.0, 0.0), 100.0, 8, 8, B=0.1)
    d16 = np.full((8, 8), 160, np.int16)  # Z = 1: the plane z = 0
    X = np.zeros((1, 3))
    two_views = [(cam, d16, np.full((8, 8), 10, np.uint8)), (cam, d16, np.full((8, 8), 11, np.uint8))]
    g, c = AR.shade(X, None, two_views, 0.01, cull=0)
    assert g[0] == 11 and c[0] == 2
    g, c = AR.shade(X + [0.0, 0.0, 0.02], None, two_views, 0.01, cull=0, fill=3)
    assert g[0] == 3 and c[0] == 0, "behind the surface the view sees: the depth test"
    g, c = AR.shade(X, None, two_views, 0.01, cull=0, disp_min=10.5)
    assert c[0] == 0


def test_gradient_branches():
    """3 x 3 x 3 with hand-set counts: central, forward-only, backward-only and neither, per the definition"""
    s = np.arange(27, dtype=np.float64).reshape(3, 3, 3) ** 2 * 0.25  # s(i, j, k) = (i + 3 j + 9 k)^2 / 4
    cnt = np.ones((3, 3, 3), np.int32) * 2
    S = FR.values(s * cnt, cnt, 2)
    G, br = AR.gradient(S)
    assert (br[:, 1, 1, 1] == 3).all()
    assert G[0][1, 1, 1] == (S[1, 1, 2] - S[1, 1, 0]) * 0.5 and G[1][1, 1, 1] == (S[1, 2, 1] - S[1, 0, 1]) * 0.5
    assert G[2][1, 1, 1] == (S[2, 1, 1] - S[0, 1, 1]) * 0.5
    # the grid's border: one-sided
    assert br[0][1, 1, 0] == 2 and G[0][1, 1, 0] == S[1, 1, 1] - S[1, 1, 0]
    assert br[0][1, 1, 2] == 1 and G[0][1, 1, 2] == S[1, 1, 2] - S[1, 1, 1]
    # undefined neighbours: count below min_weight
    cnt2 = cnt.copy()
    cnt2[1, 1, 2] = 1  # g + e_x of the centre
    cnt2[0, 1, 1] = 1  # g - e_z of the centre
    cnt2[1, 0, 1] = cnt2[1, 2, 1] = 0  # both y neighbours
    S2 = FR.values(s * cnt, cnt2, 2)
    G2, br2 = AR.gradient(S2)
    assert list(br2[:, 1, 1, 1]) == [1, 0, 2]
    assert G2[0][1, 1, 1] == S[1, 1, 1] - S[1, 1, 0]
    assert G2[1][1, 1, 1] == 0.0
    assert G2[2][1, 1, 1] == S[2, 1, 1] - S[1, 1, 1]


def test_normals_follow_extract_order():
    """a tilted plane through a small volume: as many normals as vertices, all equal to the plane's normal direction"""
    cam = FR.look_at_cam((0.3, 0.2, -1.0), (0.0, 0.0, 0.0), 400.0, 128, 128, B=0.1)
    d16 = np.full((128, 128), int(round(16 * 400.0 * 0.1 / np.linalg.norm([0.3, 0.2, -1.0]))), np.int16)
    vol = dict(origin=(-0.02, -0.02, -0.02), voxel=0.004, dims=(11, 11, 11))
    r = AR.fuse(vol["origin"], vol["voxel"], vol["dims"], [(cam, d16, np.full((128, 128), 50, np.uint8))])
    assert len(r["verts"]) > 50 and len(r["normals"]) == len(r["verts"])
    z = np.asarray(cam["R_rw"])[2]
    assert ((r["normals"] @ -z) > 0.999).all(), "the gradient of Z - q2 is minus the viewing axis"
    assert (r["grey"] == 50).all() and (r["vertex_views"] == 1).all()


def test_check_params():
    d = capi.shade_default_params()
    assert d == dict(depth_tol=0.0, disp_min=1.0, cull=1, fill=0)
    assert not capi.shade_check_params(), "depth_tol has no default"
    assert capi.shade_check_params(depth_tol=0.02)
    assert capi.shade_check_params(depth_tol=1e-9, disp_min=-3.0, cull=0, fill=255)
    for bad in [dict(depth_tol=0.0), dict(depth_tol=-0.02), dict(depth_tol=float("nan")), dict(disp_min=float("nan")), dict(cull=2),
                dict(cull=-1), dict(fill=-1), dict(fill=256)]:
        assert not capi.shade_check_params(**{"depth_tol": 0.02, **bad}), bad
    with pytest.raises(TypeError):
        capi.shade_params(0.02, colour=1)
