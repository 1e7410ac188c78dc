"""CPU suite: the oracle restatement against the real reference on every input of the range suites.

The tracking, RANSAC, bundle-adjustment and pose-graph kernels are compared with oracle/sfm_oracle.cpp, never with the reference
itself; tests/test_oracle_golden.py holds the oracle to the reference on a handful of well-behaved vectors only.  Here every case of
tests/oracle_range_cases.py -- the inputs of the range suites, from their own generators -- goes through the oracle and

  (a) the digest of the oracle's result equals the reference's recorded one (tests/golden/range_ref.json);           always
  (b) the digest of the reference's result equals the recorded one, so that the fixture cannot go stale unnoticed;    with oracle/_ref
  (c) the two results are equal bit for bit (any NaN equals any NaN), ints and return codes equal;                    with oracle/_ref

and the set of case ids equals the fixture's.  Cases on which the reference's behaviour is undefined are named in the table
UNDEFINED_IN_REFERENCE (tests/oracle_range_cases.py, next to the cases the fixture maker shares): it is empty.

Two properties of the oracle alone ride on the same runs: the tracker cases replenish, and one iteration of
orc_bundle_adjust_window equals orc_ba_build + orc_solve_gauss (the checker the BA kernels are compared with, which has no
counterpart in the reference) on the points in map-iteration order, applied by the oracle's own pose update."""
import json
import os

import numpy as np
import pytest

import ba_inputs as B
import helpers as H
import oracle_range_cases as C

UNDEFINED_IN_REFERENCE = C.UNDEFINED_IN_REFERENCE   # "family/id" -> reference line; empty

O = H.oracle()
REF = H.ref()
CASES = C.all_cases()
BA = {f"bundle_adjust_window/{c.id}": c for c in C.ba_cases()}

with open(os.path.join(H.GOLDEN, "range_ref.json")) as _f:
    FIXTURE = json.load(_f)


def test_case_ids_equal_the_fixtures():
    ids = [C.key(c) for c in CASES]
    assert len(set(ids)) == len(ids), "duplicate case id"
    missing, extra = sorted(set(ids) - set(FIXTURE)), sorted(set(FIXTURE) - set(ids))
    assert not missing and not extra, (f"{len(missing)} cases without a recorded result", missing[:5],
                                       f"{len(extra)} recorded results without a case", extra[:5])
    assert set(UNDEFINED_IN_REFERENCE) <= set(ids)
    assert {k for k, v in FIXTURE.items() if v.get("source") == "oracle"} == set(UNDEFINED_IN_REFERENCE)


def _eliminate(A, b, skip):
    """dense.hpp:54-93 in Python floats, with or without the |f| < 1e-18 skip -> (x, multipliers with 0 < |f| < 1e-18)"""
    A, b = [[float(v) for v in r] for r in A], [float(v) for v in b]
    n, tiny = len(b), 0
    for k in range(n):
        piv = max(range(k, n), key=lambda i: (abs(A[i][k]), -i))
        assert abs(A[piv][k]) >= 1e-15
        A[k], A[piv], b[k], b[piv] = A[piv], A[k], b[piv], b[k]
        akk = A[k][k]
        A[k][k:] = [v / akk for v in A[k][k:]]
        b[k] /= akk
        for i in range(k + 1, n):
            f = A[i][k]
            tiny += 0.0 < abs(f) < 1e-18
            if skip and abs(f) < 1e-18:
                continue
            A[i][k:] = [v - f * u for v, u in zip(A[i][k:], A[k][k:])]
            b[i] -= f * b[k]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = b[i]
        for j in range(i + 1, n):
            s -= A[i][j] * x[j]
        x[i] = s
    return np.array(x), tiny


@pytest.mark.parametrize("name,A,b", C.SI.skip_cases(), ids=[c[0] for c in C.SI.skip_cases()])
def test_skip_cases_stay_solvable_and_the_skip_decides_bits(name, A, b):
    """what tests/solve_inputs.py claims for its skip cases: the oracle solves them, tiny multipliers occur, and an elimination that
    does not skip them gives another solution; the restatement with the skip is the oracle's, bit for bit"""
    rc, x = H.solve_gauss(O, "orc", A, b)
    with_skip, tiny = _eliminate(A, b, True)
    without, _ = _eliminate(A, b, False)
    assert rc == 0 and tiny >= (len(b) // 2) ** 2 // 2
    H.assert_bits_equal(x, with_skip, f"{name}: the restatement with the skip")
    assert (without.view(np.uint64) != x.view(np.uint64)).any(), "the skip decides nothing"


def ba_one_iteration_from_the_build(c: C.BaCase):
    """the poses one iteration of bundle_adjust must leave: the window's world -> camera poses (orc_ba_world_to_cam), the points
    with two or more observations in map-iteration order up to max_points (T:869-881), ba_inputs.oracle_step's dx on them
    (orc_ba_build + orc_solve_gauss), applied by orc_ba_apply_update; unchanged where bundle_adjust returns early"""
    K, poses, X, ptr, li, uv, W, cap, huber, lam = C.ba_arguments(c)
    prob = c.prob()
    out = H.f64(poses).copy()
    if W < 2:
        return out
    nobs = np.diff(ptr)
    sel = np.array([p for p in H.map_iteration_order(O, "orc", len(X)) if nobs[p] >= 2][:cap], np.int64)
    if sel.size == 0:
        return out
    wc = np.zeros_like(out)
    O.call("orc_ba_world_to_cam", None, out, W, wc)
    rows = np.concatenate([np.arange(ptr[p], ptr[p + 1]) for p in sel])
    sub = B.Problem(wc, prob.K, np.ascontiguousarray(X[sel]), np.concatenate([[0], np.cumsum(nobs[sel])]).astype(np.int32),
                    np.ascontiguousarray(li[rows]), np.ascontiguousarray(uv[rows]), prob.kinds[sel])
    rc, dx = B.oracle_step(sub, huber, lam)
    if rc == 0:
        O.call("orc_ba_apply_update", None, out, W, H.f64(dx))
    return out


@pytest.mark.parametrize("case", CASES, ids=[C.key(c) for c in CASES])
def test_oracle_equals_reference(case):
    k = C.key(case)
    got = case.run(O, "orc")
    failed = []
    if case.family == "tracker":   # T:374-389 must have run: more live tracks after a step than tracks that survived it
        if not any(got[f"f{f}/live"] > got[f"f{f}/survivors"] > 0 for f in range(1, C.TRACKER_FRAMES)):
            failed.append("the tracker did not replenish")
    if case.family == "bundle_adjust_window":
        try:
            H.assert_bits_equal(got["iters1"], ba_one_iteration_from_the_build(BA[k]), "one iteration against orc_ba_build", nan_equal=True)
        except AssertionError as e:
            failed.append(str(e))
    rec = C.record(got)
    exp = {f: v for f, v in FIXTURE[k].items() if f != "source"}
    if rec != exp:
        failed.append(f"(a) the oracle's result is not the recorded one: ints {rec['rc']} recorded {exp['rc']}, shapes "
                      f"{'equal' if rec['shapes'] == exp['shapes'] else (rec['shapes'], exp['shapes'])}, sha256 {rec['sha256'][:12]} recorded {exp['sha256'][:12]}")
    if REF is not None and k not in UNDEFINED_IN_REFERENCE:
        ref = case.run(REF, "ref")
        if C.record(ref) != exp:
            failed.append("(b) the reference's result is not the recorded one: tests/golden/range_ref.json is stale")
        try:
            C.compare(case.family, case.id, got, ref)
        except AssertionError as e:
            failed.append(f"(c) {e}")
    assert not failed, (k, failed)
