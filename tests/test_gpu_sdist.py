"""GPU suite: squared distance from points to the nearest point of a triangle mesh on the device.  sfmx_sdist_* gives d2 and
the nearest face byte for byte against the brute-force NumPy restatement (tests/sdist_ref.py), for every cell size: hand
cases, the culling of a grid that must never drop the nearest face, block and LDS-chunk edges, the refusals, every way of
feeding a mesh, and the surface evaluation of the whole dense chain through pipeline.fuse / pipeline.run."""
import importlib
import json
import os

import numpy as np
import pytest

import clean_ref as LR
import consist_ref as CR
import helpers as H
import sdist_ref as DR

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
PAIR = (2, 3)  # e2e_keyframes: the pair with valid disparity
SMALL = dict(num_disparities=32, census=5)
F0 = np.zeros((0, 3), np.int32)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sd(ctx):
    """one object for the whole module: its buffers grow and shrink with the cases"""
    s = ctx.sdist()
    yield s
    s.close()


def _invalid(fn):
    with pytest.raises(capi.SfmxError) as e:
        fn()
    assert e.value.status == capi.SFMX_ERR_INVALID


def _same(got, ref, what):
    for g, r, k in zip(got, ref, ("d2", "face")):
        assert g.dtype == r.dtype and g.shape == r.shape, f"{what}: {k} {g.dtype} {g.shape} {r.shape}"
        if g.tobytes() != r.tobytes():
            bad = np.flatnonzero(g != r)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} of {len(g)} queries, first {bad[:5]}: {g[bad[:5]]} vs {r[bad[:5]]}")


def _case(sd, P, V, F, d_max, what, cell=0.0, ref=None):
    sd.set_target(V, F, d_max, cell)
    got = sd.query(P)
    _same(got, DR.brute(P, V, F, d_max) if ref is None else ref, f"{what} d_max={d_max} cell={cell}")
    return got


# ---- hand cases ------------------------------------------------------------------------------------------------------------
TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]], np.int32)
# a query in each of the seven regions, with the squared distance worked out by hand
REGIONS = [((0.25, 0.25, 0.5), 0.25), ((0.5, -1.0, 0.0), 1.0), ((1.0, 1.0, 0.0), 0.5), ((-1.0, 0.5, 0.0), 1.0),
           ((-1.0, -1.0, 0.0), 2.0), ((2.0, -1.0, 0.0), 2.0), ((-1.0, 2.0, 0.0), 2.0)]


def test_no_queries_and_no_faces(sd):
    sd.set_target(TRI_V, TRI_F, 4.0)
    d2, face = sd.query(np.zeros((0, 3)))
    assert d2.shape == (0,) and face.shape == (0,) and d2.dtype == np.float64 and face.dtype == np.int32
    assert sd.stats()["tests"] == 0
    P = np.random.default_rng(0).normal(size=(70, 3))
    for V in (TRI_V, np.zeros((0, 3))):
        d2, face = _case(sd, P, V, F0, 0.5, "no faces")
        assert (d2 == 0.25).all() and (face == -1).all()
        assert sd.stats()["dims"] == (0, 0, 0) and sd.stats()["entries"] == 0


def test_one_triangle_regions(sd):
    P = np.array([p for p, _ in REGIONS])
    for cell in (0.0, 0.7, 100.0):
        d2, face = _case(sd, P, TRI_V, TRI_F, 4.0, "regions", cell)
        assert d2.tolist() == [d for _, d in REGIONS] and (face == 0).all()
    d2, face = _case(sd, P, TRI_V, TRI_F, 1.0, "regions clipped")  # exactly d_max is clipped: !(d2 < dm2)
    assert d2.tolist() == [0.25, 1.0, 0.5, 1.0, 1.0, 1.0, 1.0] and face.tolist() == [0, -1, 0, -1, -1, -1, -1]


def test_on_a_vertex_on_an_edge_and_ties(sd):
    V = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    P = np.array([[0, 0, 0], [1, 1, 0], [0.5, 0, 0], [0.25, 0.25, 0], [0.5, 0.5, 1.0], [0.25, 0.25, 0.5], [1, 0, 0], [0.75, 0.25, 0.0]])
    d2, face = _case(sd, P, V, F, 2.0, "square")
    assert d2.tolist() == [0, 0, 0, 0, 1.0, 0.25, 0, 0]
    assert face.tolist() == [0, 0, 0, 0, 0, 0, 0, 0], "on the shared edge and above it both faces tie: the smaller index"
    assert (DR.tri(P[4], V[0], V[1], V[2]) == DR.tri(P[4], V[0], V[2], V[3])), "the tie is exact"
    d2, face = _case(sd, P, V, F[::-1].copy(), 2.0, "square, faces swapped")
    assert face.tolist() == [0, 0, 1, 0, 0, 0, 1, 1]
    d2, face = _case(sd, P, V, np.array([[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3]], np.int32), 2.0, "duplicated faces")
    assert face.max() <= 1


def test_degenerate_faces(sd):
    V = np.array([[0.0, 0, 0], [1, 0, 0], [3, 0, 0], [0, 2, 0], [0.5, 0.5, 0.5]])
    P = np.array([[0.5, 1.0, 0.0], [2.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [4.0, 3.0, 0.0], [0.5, 0.5, 0.5]])
    for name, f, want in (("point", [4, 4, 4], [0.5, 2.75, 2.75, 18.75, 0.0]), ("segment aab", [0, 0, 1], [1.0, 2.0, 1.0, 18.0, 0.5]),
                          ("segment aba", [0, 1, 0], [1.0, 2.0, 1.0, 18.0, 0.5]), ("collinear", [0, 1, 2], [1.0, 1.0, 1.0, 10.0, 0.5]),
                          ("collinear, middle last", [0, 2, 1], [1.0, 1.0, 1.0, 10.0, 0.5])):
        d2, face = _case(sd, P, V, np.array([f], np.int32), 8.0, name)
        assert d2.tolist() == want and (face == 0).all(), name
    F = np.array([[4, 4, 4], [0, 0, 1], [0, 1, 2], [0, 1, 3]], np.int32)
    d2, face = _case(sd, P, V, F, 8.0, "mixed")
    assert np.isfinite(d2).all() and face.tolist() == [3, 2, 1, 2, 0]


# ---- culling ---------------------------------------------------------------------------------------------------------------
ICO3 = DR.icosphere(3, 0.1)
D_MAXES = (0.002, 0.01, 0.05, 1.0)
_cull = {}


def _cells(d_max):
    """the four cell sizes of a case: auto, half of it, three times, one cell for everything"""
    return dict(auto=0.0, half=d_max, triple=6.0 * d_max, one=64.0 * (0.2 + 2.0 * d_max))


def _cull_case(d_max):
    """queries (shared by the four cell sizes of a d_max) and their brute-force answer, computed once"""
    if d_max not in _cull:
        V, F = ICO3
        rng = np.random.default_rng(11)
        d = rng.normal(size=(2000, 3))
        P = [d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.08, 0.12, (2000, 1))]
        lo, hi = V[F].min(axis=(0, 1)) - d_max * DR.GROW, V[F].max(axis=(0, 1)) + d_max * DR.GROW
        for a in range(3):  # beyond each of the six sides of the grid, and exactly on them
            for side, sgn in ((lo, -1.0), (hi, 1.0)):
                for off in (0.0, 1e-12, 0.5 * d_max, 3.0):
                    p = rng.uniform(-0.05, 0.05, 3)
                    p[a] = side[a] + sgn * off
                    P.append(p[None])
        for cell in (2.0 * d_max, d_max, 6.0 * d_max):  # exactly on cell boundaries lo + k * cell, near the surface
            k = np.arange(0, int((hi[0] - lo[0]) / cell) + 1)
            k = k[:: max(1, len(k) // 12)]
            for a in range(3):
                p = rng.normal(size=(len(k), 3))
                p *= 0.1 / np.linalg.norm(p, axis=1, keepdims=True)
                p[:, a] = lo[a] + k * cell
                P.append(p)
        P.append(np.array([[1e3, 0, 0], [0, -1e6, 0], [1e100, 1e100, -1e100], [0.0, 0.0, 0.0]]))  # far, and the centre
        P = np.concatenate(P)
        _cull[d_max] = (P, DR.brute(P, V, F, d_max))
    return _cull[d_max]


@pytest.mark.parametrize("cell", ["auto", "half", "triple", "one"])
@pytest.mark.parametrize("d_max", D_MAXES)
def test_culling_never_changes_a_bit(sd, d_max, cell):
    V, F = ICO3
    P, ref = _cull_case(d_max)
    _case(sd, P, V, F, d_max, f"icosphere {cell}", _cells(d_max)[cell], ref)
    st = sd.stats()
    hit = (ref[1] >= 0).sum()
    print(f"d_max {d_max} cell {cell}: grid {st['dims']} cell {st['cell']:.4g}, {st['entries']} entries, {st['tests']} tests for "
          f"{len(P)} x {len(F)} = {len(P) * len(F)}; {hit} queries within d_max")
    assert hit > (500 if d_max >= 0.01 else 100), "the case has something to find"
    if cell == "one":
        assert st["dims"] == (1, 1, 1) and st["entries"] == len(F)
    if d_max == 1.0:
        assert st["entries"] == len(F) * st["cells"], "every cell sees every face"
    assert st["tests"] < len(P) * len(F)
    if d_max <= 0.01 and cell != "one":
        assert st["tests"] * 4 < len(P) * len(F), "the grid culls"


def test_box_rule_is_inert_on_a_well_shaped_mesh():
    """the grown-box rule of the definition removes no face that the plain minimum over all faces would choose"""
    V, F = ICO3
    for d_max in D_MAXES:
        P, ref = _cull_case(d_max)
        _same(DR.brute(P, V, F, d_max, box=False), ref, f"plain minimum, d_max={d_max}")


# ---- block and chunk edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 255, 256, 257, 1025])
def test_query_and_face_counts_round_the_block_sizes(sd, m):
    V, F = ICO3
    F = F[:m]
    rng = np.random.default_rng(m)
    d = rng.normal(size=(257, 3))
    P = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.09, 0.11, (257, 1))
    ref = DR.brute(P, V, F, 0.05)
    for n in (1, 63, 64, 65, 255, 256, 257):
        for cell in (0.0, 50.0):  # one cell: every query in one run of work items, 64 each
            _case(sd, P[:n], V, F, 0.05, f"n={n} m={m}", cell, (ref[0][:n], ref[1][:n]))


def test_a_cell_longer_than_one_lds_chunk(sd):
    sd.set_target(TRI_V, TRI_F, 1.0)
    chunk = sd.stats()["chunk"]
    assert chunk == capi.SDIST_CHUNK and chunk >= 1
    k = 2 * chunk + chunk // 2 + 3  # a fan round the origin: every cell that holds the origin lists all k faces
    ang = np.linspace(0.0, 2.0 * np.pi, k, endpoint=False)
    V = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(ang), np.sin(ang), 0.1 * np.cos(3 * ang)], axis=1)])
    F = np.stack([np.zeros(k, np.int32), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], axis=1).astype(np.int32)
    rng = np.random.default_rng(3)
    P = rng.uniform(-0.02, 0.02, (130, 3))
    P[0] = 0.0  # on the shared vertex: all k faces tie at 0
    d2, face = _case(sd, P, V, F, 0.05, "fan")
    assert d2[0] == 0.0 and face[0] == 0 and (face >= 0).all() and len(np.unique(face)) > chunk
    st = sd.stats()
    assert st["tests"] >= k * 64, "a cell's list of more than two chunks and a part of one was walked"
    _case(sd, P, V, F[::-1].copy(), 0.05, "fan reversed")


BIG_V = np.array([[0.0, 0, 0], [1, 0, 1], [0, 1, 1]])


def test_one_triangle_across_the_whole_grid(sd):
    """2 d_max = 0.002 would need 501^3 cells: the automatic size doubles to 0.004 (251^3 <= 2^24); every cell lists the face"""
    rng = np.random.default_rng(5)
    w = rng.dirichlet((1, 1, 1), 60)
    P = w @ BIG_V + rng.normal(scale=4e-4, size=(60, 3))
    d2, face = _case(sd, P, BIG_V, TRI_F, 1e-3, "spanning triangle")
    st = sd.stats()
    assert st["cell"] == 0.004 and st["cells"] <= 2 ** 24 and st["entries"] == st["cells"] and (face == 0).sum() > 20
    _invalid(lambda: sd.set_target(BIG_V, TRI_F, 1e-3, 0.001))  # an explicit size that does not fit: 1001^3 cells
    _invalid(lambda: sd.query(P))  # and no target is left
    _invalid(lambda: sd.set_target(BIG_V, TRI_F, 1e-3, 1e-300))
    # the entry cap: 70 copies of the face make 70 x 251^3 > 2^30 pairs at 0.004; explicit is refused, automatic doubles again
    F70 = np.repeat(TRI_F, 70, axis=0)
    _invalid(lambda: sd.set_target(BIG_V, F70, 1e-3, 0.004))
    got = _case(sd, P, BIG_V, F70, 1e-3, "70 spanning triangles", ref=(d2, face))
    assert sd.stats()["cell"] == 0.008 and sd.stats()["entries"] == 70 * sd.stats()["cells"] <= 2 ** 30
    assert got[1].max() == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_then_a_good_call(ctx):
    s = ctx.sdist()
    V, F = ICO3
    P = V[:100] * 1.01
    ref = DR.brute(P, V, F, 0.01)
    _invalid(lambda: s.query(P))  # before any target
    with pytest.raises(capi.SfmxError):
        s.stats()
    _case(s, P, V, F, 0.01, "before", ref=ref)
    for bad in (len(V), -1, 2 ** 31 - 1, -2 ** 31):
        for pos in range(3):
            f = F.copy()
            f[700, pos] = bad
            _invalid(lambda: s.set_target(V, f, 0.01))
            _invalid(lambda: s.query(P))  # the failed call left no target
            _case(s, P, V, F, 0.01, "after a bad index", ref=ref)
    _invalid(lambda: s.set_target(np.zeros((0, 3)), np.array([[0, 0, 0]], np.int32), 0.01))
    _case(s, P, V, F, 0.01, "after a bad index", ref=ref)
    for bad in (np.nan, np.inf, -np.inf):
        q = P.copy()
        q[57, 1] = bad
        _invalid(lambda: s.query(q))
        _same(s.query(P), ref, "the target outlives a refused query")
        v = V.copy()
        v[F[300, 2], 0] = bad
        _invalid(lambda: s.set_target(v, F, 0.01))
        _invalid(lambda: s.query(P))
        _case(s, P, V, F, 0.01, "after a non-finite vertex", ref=ref)
    v = np.concatenate([V, [[np.nan, np.inf, 0.0]]])  # a vertex no face uses may hold anything
    _case(s, P, v, F, 0.01, "NaN in an unused vertex", ref=ref)
    for bad in (0.0, -1.0, np.nan, np.inf, 2.0 ** 61, 1e-300):
        assert not capi.sdist_check_params(bad)
        _invalid(lambda: s.set_target(V, F, bad))
        _invalid(lambda: s.query(P))
        _case(s, P, V, F, 0.01, "after a bad d_max", ref=ref)
    for bad in (-1.0, np.nan, np.inf):
        _invalid(lambda: s.set_target(V, F, 0.01, bad))
    _invalid(lambda: s.set_target(V * 2.0 ** 41, F, 0.01))  # beyond 2^40 d_max the margin argument does not hold
    _case(s, P, V, F, 0.01, "again", ref=ref)
    G = DR.icosphere(1, 0.1)
    with pytest.raises(ValueError):
        pipe.surface_eval(ctx, V, F, *G, d_max=0.01, tau=0.02)
    with pytest.raises(TypeError):
        pipe.surface_eval(ctx, V, F, *G, d_max=0.01)
    with pytest.raises(capi.SfmxError):
        pipe.surface_eval(ctx, V, F, *G, d_max=0.01, tau=0.01, percentile=0.0)
    f = F.copy()
    f[3, 1] = len(V)
    with pytest.raises(capi.SfmxError):
        pipe.surface_eval(ctx, V, f, *G, d_max=0.01, tau=0.01)
    assert pipe.surface_eval(ctx, V, F, *G, d_max=0.01, tau=0.01) == DR.evaluate(V, F, *G, 0.01, 0.01, dist=DR.brute)
    s.close()


# ---- feeds and reuse -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ball():
    views, _ = CR.sphere26(False)
    return views


def test_every_feed_gives_the_same_bytes(ctx, ball):
    import torch
    fu, c, s = ctx.fusion(**CR.SPHERE26_VOL), ctx.clean(), ctx.sdist()
    for cam, d16 in ball[:6]:
        fu.add_view(cam, d16)
    v, f = fu.extract()
    got = c.fusion(fu, min_permille=0)
    cv, cf = (c.read()[k] for k in ("verts", "faces"))
    assert got["n_verts"] == len(cv) > 1000
    G = DR.icosphere(3, 0.1)
    d_max = 0.02
    # the device surfaces as queries
    s.set_target(*G, d_max)
    host = s.query(v)
    _same(host, DR.pruned(v, *G, d_max), "extracted vertices against the icosphere")
    _same(s.query_fusion(fu, len(v)), host, "query_fusion")
    _same(s.query_fusion(fu), host, "query_fusion sized by the library")
    _invalid(lambda: s.query_fusion(fu, len(v) - 1))  # a stale count: refused, not written past
    _same(s.query_fusion(fu, len(v) + 7), host, "a larger capacity")
    tv = torch.from_numpy(v).cuda()
    _same(s.query(tv.data_ptr(), n=len(v)), host, "device pointer queries")
    _same(s.query_clean(c), s.query(cv), "query_clean")
    # the device surfaces as targets
    P = G[0]
    s.set_target(v, f, d_max)
    host = s.query(P)
    _same(host, DR.pruned(P, v, f, d_max), "the icosphere's vertices against the extracted surface")
    assert (host[1] >= 0).sum() > 100
    s.set_target_fusion(fu, d_max)
    _same(s.query(P), host, "set_target_fusion")
    tf = torch.from_numpy(f).cuda()
    s.set_target(tv.data_ptr(), tf.data_ptr(), d_max, nv=len(v), m=len(f))
    del tv, tf  # the target is a copy
    torch.cuda.synchronize()
    _same(s.query(P), host, "device pointer target")
    s.set_target(cv, cf, d_max)
    host = s.query(P)
    s.set_target_clean(c, d_max)
    _same(s.query(P), host, "set_target_clean")
    fu.add_view(*ball[6])
    fu.integrate()
    _invalid(lambda: s.set_target_fusion(fu, d_max))  # the volume changed: no current surface
    _invalid(lambda: s.query(P))
    s.set_target(*G, d_max)
    _invalid(lambda: s.query_fusion(fu, len(v)))
    _invalid(lambda: s.set_target_clean(ctx.clean(), d_max))  # never ran
    for o in (fu, c, s):
        o.close()


def test_one_object_large_small_large_and_two_query_sets(ctx):
    s = ctx.sdist()
    big, small = DR.icosphere(5, 0.1), DR.icosphere(0, 0.1)
    rng = np.random.default_rng(9)
    P = rng.normal(size=(3000, 3))
    P *= rng.uniform(0.09, 0.11, (3000, 1)) / np.linalg.norm(P, axis=1, keepdims=True)
    refs = dict(large=DR.pruned(P, *big, 0.005), small=DR.brute(P, *small, 0.05))
    for what, (V, F), d_max in (("large", big, 0.005), ("small", small, 0.05), ("large", big, 0.005)):
        _case(s, P, V, F, d_max, what, ref=refs[what])
        assert s.last_us() == 0.0
    Q = P[::-1] * 1.02  # one target, another query set, and the first again
    _same(s.query(Q), DR.pruned(Q, *big, 0.005), "second set")
    _same(s.query(P[:5]), tuple(r[:5] for r in refs["large"]), "a smaller set")
    ctx.set_timing(True)
    s.set_target(*big, 0.005)
    t_build = s.last_us()
    _same(s.query(P), refs["large"], "timed")
    assert t_build > 0.0 and s.last_us() > 0.0
    ctx.set_timing(False)
    s.close()


# ---- the whole chain -------------------------------------------------------------------------------------------------------
FIELDS = ("accuracy", "acc_within", "acc_mean", "acc_max", "n_rec", "completeness", "comp_within", "n_gt")


def _eval_from_d2(d2_rec, used_rec, d2_gt, tau, percentile=90.0):
    d = np.sqrt(d2_rec[used_rec])
    dg = np.sqrt(d2_gt)
    return dict(accuracy=DR.nearest_rank(np.sort(d), percentile), acc_within=int((d <= tau).sum()), acc_mean=float(np.cumsum(d)[-1] / len(d)),
                acc_max=float(d.max()), n_rec=len(d), completeness=int((dg <= tau).sum()) / len(dg), comp_within=int((dg <= tau).sum()),
                n_gt=len(dg))


def test_sphere26_chain_on_the_device(ctx):
    """the noisy sphere-26 fused raw, and fused after the filter and cleaned: both evaluated from where they lie on the device
    against a level-5 icosphere; every figure is NumPy's"""
    noisy, _ = CR.sphere26(True)
    vol = CR.SPHERE26_VOL
    G = DR.icosphere(5, CR.RADIUS)
    d_max, tau = 4 * vol["voxel"], vol["voxel"]
    fu, cs, c, s = ctx.fusion(**vol), ctx.consist(), ctx.clean(), ctx.sdist()
    out = {}
    for name in ("raw", "filtered and cleaned"):
        fu.reset()
        if name == "raw":
            for cam, d16 in noisy:
                fu.add_view(cam, d16)
        else:
            for cam, d16 in noisy:
                cs.add_view(cam, d16)
            cs.filter()
            for i in range(len(noisy)):
                fu.add_consist_view(cs, i)
        v, f = fu.extract()
        s.set_target(*G, d_max)
        if name == "raw":
            d2r, _ = s.query_fusion(fu, len(v))
            s.set_target_fusion(fu, d_max)
        else:
            c.fusion(fu)
            r = c.read()
            v, f = r["verts"], r["faces"]
            d2r, _ = s.query_clean(c)
            s.set_target_clean(c, d_max)
        d2g, _ = s.query(G[0])
        used = np.zeros(len(v), bool)
        used[f.ravel()] = True
        got = _eval_from_d2(d2r, used, d2g, tau)
        ref = DR.evaluate(v, f, *G, d_max, tau)
        print(name, got)
        assert got == ref, name
        assert pipe.surface_eval(ctx, v, f, *G, d_max=d_max, tau=tau) == ref, name + ": surface_eval"
        out[name] = got
    assert out["raw"]["accuracy"] > out["filtered and cleaned"]["accuracy"], "the metric sees what the filter and the cleaning do"
    for o in (fu, cs, c, s):
        o.close()


@pytest.fixture(scope="module")
def ring6():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    return dict(images=images, K=K, poses=poses, pairs=pairs, vol=CR.RING6_VOL)


def test_host_fuse_evaluate(ctx, ring6, tmp_path):
    vol = ring6["vol"]
    args = (ctx, ring6["images"], ring6["K"], ring6["poses"], ring6["pairs"], vol["origin"], vol["voxel"], vol["dims"])
    G = synth.shell_mesh(4)
    ev = dict(gt_verts=G[0], gt_faces=G[1], d_max=4 * vol["voxel"], tau=vol["voxel"])
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain.ply", "none.ply", "ev.ply"))
    m0 = pipe.fuse(*args, num_disparities=64, ply_path=p0)
    m1 = pipe.fuse(*args, num_disparities=64, ply_path=p1, evaluate=None)
    m = pipe.fuse(*args, num_disparities=64, ply_path=p2, evaluate=ev)
    assert set(m0) == set(m1) == {"verts", "faces", "views", "warn"} and set(m) == set(m0) | {"evaluation"}
    for k in ("verts", "faces"):
        assert m0[k].tobytes() == m1[k].tobytes() == m[k].tobytes(), k
    assert open(p0, "rb").read() == open(p1, "rb").read() == open(p2, "rb").read(), "the evaluation changes no output"
    ref = DR.evaluate(m0["verts"], m0["faces"], *G, ev["d_max"], ev["tau"])
    print("ring-6:", m["evaluation"])
    assert tuple(m["evaluation"]) == FIELDS and m["evaluation"] == ref
    assert m["evaluation"] == pipe.surface_eval(ctx, m0["verts"], m0["faces"], *G, d_max=ev["d_max"], tau=ev["tau"])
    # with the filter, the cleaning and the appearance: the cleaned mesh is the one evaluated, at another percentile
    kw = dict(consistency=True, clean=True, appearance=True)
    a0 = pipe.fuse(*args, num_disparities=64, **kw)
    a = pipe.fuse(*args, num_disparities=64, evaluate=dict(ev, percentile=50.0, cell=0.05), **kw)
    assert set(a) == set(a0) | {"evaluation"}
    for k in set(a0) - {"clean", "consistency", "warn", "views"}:
        assert a0[k].tobytes() == a[k].tobytes(), k
    assert a["evaluation"] == DR.evaluate(a0["verts"], a0["faces"], *G, ev["d_max"], ev["tau"], 50.0)
    assert a["evaluation"]["accuracy"] < m["evaluation"]["accuracy"]
    # nothing left to evaluate, and the refusals
    e = pipe.fuse(*args, num_disparities=64, clean=dict(min_faces=10 ** 6), evaluate=ev)["evaluation"]
    assert e["n_rec"] == 0 and np.isnan(e["accuracy"]) and e["comp_within"] == 0 and e["completeness"] == 0.0 and e["n_gt"] == len(G[0])
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, evaluate=dict(ev, radius=1.0))
    with pytest.raises(TypeError):
        pipe.fuse(*args, num_disparities=64, evaluate=dict(gt_verts=G[0], gt_faces=G[1], d_max=0.01))
    with pytest.raises(ValueError):
        pipe.fuse(*args, num_disparities=64, evaluate=dict(ev, tau=1.0))
    with pytest.raises(capi.SfmxError):
        pipe.fuse(*args, num_disparities=64, evaluate=dict(ev, gt_faces=G[1] + len(G[0])))


def test_pipeline_run_evaluate(ctx, tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_keyframes.npz"))
    cfg = H.pipe_cfg_from_json(json.loads(str(g["config"])))
    names = [str(s) for s in g["names"]]
    plain, evald = str(tmp_path / "plain"), str(tmp_path / "ev")
    r0 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, None)
    fa, fb = (int(r0["kf_frames"][k]) for k in PAIR)
    sm = pipe.stereo_mesh(ctx, g["images"][fa], g["images"][fb], g["K"], r0["kf_poses"][PAIR[0]], r0["kf_poses"][PAIR[1]], **SMALL)
    lo, hi = sm["verts"].min(0), sm["verts"].max(0)
    pad = 0.1 * (hi - lo).max()
    lo, hi = lo - pad, hi + pad
    voxel = float((hi - lo).min() / 32.0)
    dims = tuple(int(np.ceil((hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    fz = dict(pairs=[PAIR], origin=tuple(lo), voxel=voxel, dims=dims, **SMALL)
    ev = dict(gt_verts=sm["verts"], gt_faces=sm["faces"], d_max=4 * voxel, tau=voxel)  # the pair's own stereo mesh as the truth
    r1 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, plain, fusion=fz)
    r2 = pipe.run(ctx, g["images"], names, g["K"], g["lat"], g["lon"], cfg, evald, fusion=dict(fz, evaluate=ev))
    assert r1["log"].replace(plain, "X") == r2["log"].replace(evald, "X")
    assert sorted(os.listdir(evald)) == sorted(os.listdir(plain))
    for fn in os.listdir(plain):
        assert open(os.path.join(plain, fn), "rb").read() == open(os.path.join(evald, fn), "rb").read(), fn
    m1, m = r1["fused_mesh"], r2["fused_mesh"]
    assert set(m) == set(m1) | {"evaluation"} and len(m1["faces"]) > 0 and m["verts"].tobytes() == m1["verts"].tobytes()
    ref = DR.evaluate(m1["verts"], m1["faces"], sm["verts"], sm["faces"], ev["d_max"], ev["tau"])
    print("run:", m["evaluation"])
    assert m["evaluation"] == ref and ref["acc_within"] > 0 and ref["comp_within"] > 0
