"""Conditions on the inputs of the BA range suite (tests/ba_inputs.py), checked on the CPU oracle: every kind of point is there, both
Huber branches are taken, the equality and boundary cases are really reached, the NaN cases leave most of S finite.  These are
conditions, not measurements: if one fails, the seed or the shares of the generator change, never the threshold.
No device, no binding of the device library."""
import numpy as np
import pytest

import ba_inputs as B


def _in_front_rn(prob):
    out = []
    for p in range(prob.P):
        n = prob.ptr[p + 1] - prob.ptr[p]
        if n > B.BA_MAX_OBS:
            continue
        for o in range(prob.ptr[p], prob.ptr[p + 1]):
            if B.camera_point(prob.poses[prob.li[o]], prob.X[p])[2] > 1e-6:
                out.append(B.residual_norm(prob.poses[prob.li[o]], prob.K, prob.X[p], prob.uv[o]))
    return np.array(out)


def _claimed(W, flavour):
    kinds = ["empty", "single", "over", "behind"] + (["ordinary"] if W >= 2 else []) + (["dup"] if flavour == "dup" else [])
    return kinds


def _point_alone(prob, p):
    lists = B.unpack(prob)
    return B.pack(prob.poses, prob.K, prob.X[p:p + 1], [lists[p]], prob.kinds[p:p + 1])


def _adjacent_free_dup(prob, p):
    ks = prob.li[prob.ptr[p]:prob.ptr[p + 1]].tolist()
    twins = [(i, j) for i in range(len(ks)) for j in range(i + 1, len(ks)) if ks[i] == ks[j]]
    return len(twins) == 1 and twins[0][1] - twins[0][0] >= 2


ALL_PROBLEMS = [pytest.param(W, P, fl, id=f"W{W}-P{P}-{fl}") for W, P, fl in B.WINDOWS] + \
               [pytest.param(W, P, "big", id=f"W{W}-P{P}-big") for W, P in B.BIG_P if P in (4097, 12289)]


def _get(W, P, fl):
    return B.big(W, P) if fl == "big" else B.window(W, fl)


@pytest.mark.parametrize("W,P,fl", ALL_PROBLEMS)
def test_every_problem_holds_every_kind_and_both_huber_branches(W, P, fl):
    prob = _get(W, P, fl)
    assert prob.W == W and prob.P == P and prob.ptr[-1] == len(prob.li) == len(prob.uv)
    assert prob.li.min() >= 0 and prob.li.max() < W
    flavour = "dup" if fl == "big" else fl
    for kind in _claimed(W, flavour):
        assert int((prob.kinds == kind).sum()) >= 3, kind
    counts = np.diff(prob.ptr)
    assert (counts[prob.kinds == "empty"] == 0).all() and (counts[prob.kinds == "single"] == 1).all()
    assert ((counts[prob.kinds == "over"] >= 17) & (counts[prob.kinds == "over"] <= 20)).all()
    assert (counts[(prob.kinds == "ordinary") | (prob.kinds == "dup") | (prob.kinds == "behind")] <= B.BA_MAX_OBS).all()
    assert (counts[(prob.kinds == "ordinary")] >= 2).all()
    dups = np.flatnonzero(prob.kinds == "dup")
    if flavour == "dup":
        assert B.has_dup(prob) and all(_adjacent_free_dup(prob, p) for p in dups)
    else:
        assert len(dups) == 0 and not B.has_dup(prob)
    rn = _in_front_rn(prob)
    share = float((rn > B.HUBER0).mean())
    assert 0.05 <= share <= 0.5, share


@pytest.mark.parametrize("W,P,fl", [pytest.param(W, P, fl, id=f"W{W}-P{P}-{fl}") for W, P, fl in B.WINDOWS])
def test_undamped_system_fills_its_blocks(W, P, fl):
    prob = B.window(W, fl)
    S, b = B.oracle_build(prob, damp=False)
    assert np.isfinite(S).all() and np.isfinite(b).all()
    blocks = np.abs(S).reshape(W, 6, W, 6).max(axis=(1, 3)) > 0
    assert blocks.mean() >= 0.9, blocks.mean()


def test_single_observation_points_contribute_and_do_not():
    """A one-observation point has a rank-2 Hpp: whether |det| < 1e-15 holds is decided by rounding alone, so such a point detects a
    reordered Hpp chain.  Over the WINDOWS problems both outcomes must occur."""
    yes = no = 0
    for W, P, fl in B.WINDOWS:
        prob = B.window(W, fl)
        for p in np.flatnonzero(prob.kinds == "single"):
            S, _ = B.oracle_build(_point_alone(prob, p), damp=False)
            if np.any(S != 0):
                yes += 1
            else:
                no += 1
    print(f"single-observation points: {yes} contribute, {no} do not")
    assert yes >= 1 and no >= 1, (yes, no)


@pytest.mark.parametrize("fl", ["clean", "dup"])
def test_huber_equality_case_is_reached(fl):
    prob = B.window(6, fl)
    rn, p, o = B.rn_star(prob)
    assert prob.kinds[p] == "ordinary" and 0 < rn < B.HUBER0
    S_at, _ = B.oracle_build(prob, huber=rn, damp=False)
    S_below, _ = B.oracle_build(prob, huber=float(np.nextafter(rn, 0.0)), damp=False)
    assert np.any(S_at != S_below)
    # ... and that one observation alone makes the difference
    one = _point_alone(prob, p)
    a, _ = B.oracle_build(one, huber=rn, damp=False)
    c, _ = B.oracle_build(one, huber=float(np.nextafter(rn, 0.0)), damp=False)
    assert np.any(a != c)


@pytest.mark.parametrize("huber", [0.0, 1e-300])
def test_huber_zero_gives_an_exactly_zero_system(huber):
    for prob in (B.window(6, "clean"), B.window(6, "dup"), B.big(6, 4097)):
        S, b = B.oracle_build(prob, huber=huber, damp=False)
        assert not S.any() and not b.any()


def test_huber_nan_gives_nan():
    for prob in (B.window(6, "clean"), B.window(6, "dup")):
        S, _ = B.oracle_build(prob, huber=float("nan"), damp=False)
        assert np.isnan(S).any()


@pytest.mark.parametrize("name", B.NONFINITE)
@pytest.mark.parametrize("P", [64, 4097])
def test_nonfinite_cases_poison_part_of_the_system_only(name, P):
    prob, want_nan = B.nonfinite_case(name, P)
    assert not B.has_dup(prob)
    for i in B.POISON_AT:  # every poisoned point is seen by at most 3 poses
        assert prob.ptr[i + 1] - prob.ptr[i] <= 3
    S, b = B.oracle_build(prob, damp=False)
    assert bool(np.isnan(S).any() or np.isnan(b).any()) == want_nan
    assert bool(np.isnan(S).any()) == (want_nan and name != "inf_v")  # weight 0: 0 * finite keeps S clean, b = 0 * inf is NaN
    assert np.isfinite(S).mean() >= 0.5
    if not want_nan:
        assert np.isfinite(S).all() and np.isfinite(b).all()


def test_overflow_and_subnormal_residuals_are_reached():
    prob, _ = B.nonfinite_case("res_1e300")
    i = B.POISON_AT[0]
    o = prob.ptr[i] + 1
    assert B.residual_norm(prob.poses[prob.li[o]], prob.K, prob.X[i], prob.uv[o]) > 1e300
    prob, _ = B.nonfinite_case("res_1e-310")
    o = prob.ptr[i] + 1
    rn = B.residual_norm(prob.poses[prob.li[o]], prob.K, prob.X[i], prob.uv[o])
    assert 0 < rn < 2.3e-308  # subnormal
    S, _ = B.oracle_build(_point_alone(prob, i), damp=False)
    assert S[12:18, 12:18].any()


def test_depth_boundary_sits_on_the_threshold():
    """pose 2 is the identity, so Xc.z is X.z: 1e-6 and -0.0 are skipped (`<= 1e-6`), the next double above 1e-6 is not"""
    prob, _ = B.nonfinite_case("z_edge")
    assert (prob.poses[2] == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).all()
    for key, live in (("at", False), ("above", True), ("negzero", False)):
        one = B.z_edge_point_alone(key)
        assert B.camera_point(one.poses[2], one.X[0])[2] == B.Z_POINTS[key][2]
        S, _ = B.oracle_build(one, damp=False)
        blk = S[12:18, 12:18]
        assert np.isfinite(S).all()
        assert bool(blk.any()) == live, key


@pytest.mark.parametrize("W", [6, 7, 10, 11])
def test_zero_system_is_singular(W):
    rc, _ = B.oracle_step(B.window(W, "clean"), huber=0.0, lam=0.0)
    assert rc != 0


def test_half_behind_window_has_zero_slots_among_live_ones():
    for fl in ("clean", "dup"):
        prob = B.window(6, fl, half_behind=3)
        seen = [p for p in range(prob.P) if prob.kinds[p] in ("ordinary", "dup") and 3 in prob.li[prob.ptr[p]:prob.ptr[p + 1]]]
        assert len(seen) >= 20
        assert all(B.camera_point(prob.poses[3], prob.X[p])[2] < 0 for p in seen)
        for p in seen[:20]:  # each alone: nothing for pose 3, something for the others
            S, _ = B.oracle_build(_point_alone(prob, p), damp=False)
            assert np.isfinite(S).all() and not S[18:24, :].any() and not S[:, 18:24].any() and S.any()


def test_tables_hold_the_boundaries():
    for t in (16, 32, 64, 128, 256):
        assert {t - 1, t, t + 1} <= set(B.P_EDGES)
    assert {4096, 4097, 8192, 8193} <= {P for W, P in B.BIG_P if W == 6}
    assert {1, 2, 3, 4, 5} <= set(B.P_EDGES)
    assert sorted({W for W, _, _ in B.WINDOWS}) == [1, 2, 3, 5, 6, 7, 9, 10, 11, 15, 16, 17, 33, 64]
    for P in B.P_EDGES:  # short prefixes stay mixed
        if P >= 6:
            assert len(set(B.edge(6, P, "dup").kinds.tolist())) == 6


def test_dispatch_restatement():
    """the ids of the GPU cases name the kernels: the rules of ba_launch_points / sfmx_ba_step as ba_inputs restates them"""
    assert B.points_kernel(6, 300, False) == "lds" and B.points_kernel(6, 300, True) == "window"
    assert B.points_kernel(6, 4097, False) == "bulk" and B.points_kernel(6, 4096, False) == "lds"
    assert B.points_kernel(15, 300, False, pts=4) == "lds" and B.points_kernel(16, 300, False, pts=4) == "window"
    assert B.points_kernel(64, 200, False, pts=2) == "lds" and B.points_kernel(6, 300, False, points_env="global") == "window"
    assert B.points_kernel(6, 64, False, expand="split") == "bulk" and B.points_kernel(6, 8193, False, expand="merged") == "lds"
    assert [B.solver(W) for W in (1, 5, 6, 7, 9, 10, 11, 64)] == ["wave", "wave", "host", "wave", "wave", "host", "blocked", "blocked"]
    assert B.solver(6, "device") == "fused" and B.solver(6, no_fuse=True) == "regs" and B.solver(10, no_fuse=True) == "regs"
