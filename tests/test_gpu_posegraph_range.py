"""Range suite of csrc/hip/posegraph.hip (k_pg_scatter, k_chol_panel, k_chol_update on v_mfma_f64_16x16x4_f64, k_tri_forward,
k_tri_backward, the host routine sfmx_posegraph_solve) and of its consumer, the structured branch of posegraph_optimize_centers.

Direct suite, through Context.posegraph_solve: every launch shape from n = 1 to 700 on dense SPD matrices (every update tile and
every MFMA lane carries data), ill-conditioned ones and five kinds of graph Laplacian, each held to two a-priori bounds against a
longdouble reference (tests/posegraph_inputs.py: `bounds`), not to a measured tolerance; the 1e-15 pivot threshold from both sides,
zero rows, negative and NaN entries, argument rejection, run-to-run bits, and what a call leaves behind in the shared arena.
Pipeline suite, through pipeline.posegraph with SFMX_POSEGRAPH_SOLVER=structured: N = 2 ... 129 on every graph kind, with
self-edges and out-of-range indices, against the oracle's dense solve; every graph with a keyframe cut off from node 0 is refused
with the centres untouched, loop edges inside the cut-off part or not.

What the inputs contain is asserted on the CPU by tests/test_posegraph_inputs_cpu.py."""
import importlib
from ctypes import POINTER, c_double, c_int, c_int32

import numpy as np
import pytest

import ba_inputs as B
import helpers as H
import posegraph_inputs as P

pytestmark = pytest.mark.gpu
O = H.oracle()
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")

OK, SINGULAR, INVALID = capi.SFMX_OK, capi.SFMX_ERR_SINGULAR, capi.SFMX_ERR_INVALID


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def solve(ctx, c: P.Case, g=None):
    return ctx.posegraph_solve(c.n, c.ij, c.v, c.g if g is None else g)


# ---- 1. every launch shape, every matrix kind, against the two bounds -----------------------------------------------------------
@pytest.mark.parametrize("kind,n", P.direct_cases())
def test_solve_meets_residual_and_forward_bounds(ctx, kind, n):
    """|g - A x|_i <= 2 gamma_{3n+1} (|R||R^T||x|)_i and |x - x*|_i <= 2 gamma_{3n+1} (|A^-1||R||R^T||x|)_i, R, x* and the residual
    in longdouble.  A plain float64 Cholesky sits at 0.0003 ... 0.11 of them (tests/test_posegraph_inputs_cpu.py); a dropped
    k-step, a swapped lane or a mis-decoded tile is off by ten orders of magnitude."""
    c = P.case(kind, n)
    rc, x = solve(ctx, c)
    assert rc == OK, c.name
    assert np.isfinite(x).all()
    res, fwd = P.ratios(c, x)
    print(f"{c.name}: residual / bound {res:.3g}, error / bound {fwd:.3g}")
    assert res <= 1.0 and fwd <= 1.0, (c.name, res, fwd)


# ---- 2. the pivot threshold and singular input ----------------------------------------------------------------------------------
def _diagonal(n, at, d_at):
    """a diagonal matrix of powers of 4 (sqrt and both divisions exact) except d_at at index `at`"""
    d = 4.0 ** ((np.arange(n) % 7) - 3)
    d[at] = d_at
    rng = np.random.default_rng([3, n, at])
    ij = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    return P.Case(f"diagonal n={n} d[{at}]={d_at!r}", n, ij, d, np.diag(d), rng.normal(size=(n, 3)))


@pytest.mark.parametrize("n,at", [(1, 0), (40, 0), (40, 31), (40, 32), (40, 39), (97, 70)])
def test_pivot_threshold_from_both_sides(ctx, n, at):
    """a pivot of exactly 1e-15 is singular, the next double above it is not.  A row without off-diagonal entries is never
    updated, so the solve is exactly the kernels' three operations on it: s = sqrt(d), y = g / s, x = y / s (IEEE, as
    test_device_arithmetic_matches_host pins) -- g / d itself where d is a power of 4, and within two roundings of it otherwise."""
    rc, _ = solve(ctx, _diagonal(n, at, P.PIVOT_MIN))
    assert rc == SINGULAR
    c = _diagonal(n, at, float(np.nextafter(P.PIVOT_MIN, 1.0)))
    rc, x = solve(ctx, c)
    assert rc == OK
    d = np.diag(c.A)[:, None]
    H.assert_bits_equal(x, c.g / np.sqrt(d) / np.sqrt(d), c.name)
    rest = np.arange(n) != at
    H.assert_bits_equal(x[rest], (c.g / d)[rest], c.name + ": rows with an exact square root")
    assert (np.abs(x[at] - c.g[at] / d[at]) <= 4 * P.U * np.abs(c.g[at] / d[at])).all()


def test_zero_negative_and_nan_entries_are_singular(ctx):
    c97, c300 = P.case("dense", 97), P.case("dense", 300)
    for c, i in [(c97, i) for i in (0, 31, 32, 33, 96)] + [(c300, 200)]:
        z = P.with_zero_row(c, i)
        assert not (z.ij == i).any()
        assert solve(ctx, z)[0] == SINGULAR, z.name
        iz = np.concatenate([z.ij, [[i, i]]]).astype(np.int32)                       # the same with an explicit 0.0 on the diagonal
        assert ctx.posegraph_solve(z.n, iz, np.append(z.v, 0.0), z.g)[0] == SINGULAR, z.name
    diag = np.flatnonzero(c97.ij[:, 0] == c97.ij[:, 1])
    for i in (0, 31, 32, 70, 96):
        for bad in (-1.0, -c97.v[diag[i]], np.nan, -np.inf):
            v = c97.v.copy()
            v[diag[i]] = bad
            assert ctx.posegraph_solve(97, c97.ij, v, c97.g)[0] == SINGULAR, (i, bad)
    for r, col in ((5, 3), (50, 3), (96, 0), (96, 95), (70, 40)):   # inside a block, in a panel, the last row, a trailing tile
        v = c97.v.copy()
        v[np.flatnonzero((c97.ij[:, 0] == r) & (c97.ij[:, 1] == col))[0]] = np.nan
        assert ctx.posegraph_solve(97, c97.ij, v, c97.g)[0] == SINGULAR, (r, col)
    rc, x = solve(ctx, c97)                                          # the status word does not outlive the call
    assert rc == OK and max(P.ratios(c97, x)) <= 1.0


def test_nan_in_g_stays_in_its_column(ctx):
    c = P.case("dense", 97)
    rc, x0 = solve(ctx, c)
    assert rc == OK
    for row, col in ((0, 0), (40, 1), (96, 2)):
        g = c.g.copy()
        g[row, col] = np.nan
        rc, x = solve(ctx, c, g)
        assert rc == OK
        assert np.isnan(x[:, col]).all()          # the matrix is dense: back-substitution carries it to every row
        others = [k for k in range(3) if k != col]
        H.assert_bits_equal(x[:, others], x0[:, others], f"columns beside a NaN at g[{row}][{col}]")


# ---- 3. arguments ---------------------------------------------------------------------------------------------------------------
def _raw(ctx, n, ij, v, g, x):
    dp = POINTER(c_double)
    return ctx.lib.sfmx_posegraph_solve(ctx.h_, c_int(n), ij.ctypes.data_as(POINTER(c_int32)), v.ctypes.data_as(dp), c_int(len(v)),
                                        g.ctypes.data_as(dp), x.ctypes.data_as(dp))


def test_bad_arguments_are_rejected_and_change_nothing(ctx):
    c = P.case("fill", 33)
    rc, x0 = solve(ctx, c)
    assert rc == OK

    def entry(i, j):
        ij = c.ij.copy()
        ij[len(ij) // 2] = (i, j)
        return ij
    none_ij, none_v = np.zeros((0, 2), np.int32), np.zeros(0)
    bad = {"n = 0": (0, c.ij, c.v, np.zeros((0, 3))), "m = 0": (33, none_ij, none_v, c.g), "row == n": (33, entry(33, 2), c.v, c.g),
           "column == n": (33, entry(5, 33), c.v, c.g), "negative row": (33, entry(-1, 0), c.v, c.g),
           "negative column": (33, entry(4, -1), c.v, c.g), "upper triangle": (33, entry(3, 4), c.v, c.g),
           "row far outside": (33, entry(2 ** 31 - 1, 0), c.v, c.g)}
    for what, (n, ij, v, g) in bad.items():
        with pytest.raises(capi.SfmxError) as e:
            ctx.posegraph_solve(n, ij, v, g)
        assert e.value.status == INVALID, what
        x = np.full((34, 3), 7.25)                                   # the output of a rejected call is not written
        ij = np.ascontiguousarray(ij if len(ij) else [[0, 0]], np.int32)   # (m = 0 with valid pointers)
        assert _raw(ctx, n, ij, H.f64(v if len(v) else [1.0])[:len(v)], H.f64(g if g.size else c.g), x) == INVALID, what
        assert (x == 7.25).all(), what
        rc, x1 = solve(ctx, c)                                       # and the context solves as before
        assert rc == OK
        H.assert_bits_equal(x1, x0, f"after a rejected call ({what})")
    x = np.full((33, 3), 7.25)
    assert _raw(ctx, 33, c.ij, c.v, H.f64(c.g), x) == OK
    H.assert_bits_equal(x, x0, "raw call")
    assert ctx.lib.sfmx_posegraph_solve(ctx.h_, c_int(33), None, None, c_int(len(c.v)), None, None) == INVALID


# ---- 4. determinism and the shared arena ----------------------------------------------------------------------------------------
def test_same_call_twice_is_bit_identical(ctx):
    for kind, n in (("dense", 353), ("fill", 289), ("dense", 65)):
        c = P.case(kind, n)
        (ra, xa), (rb, xb) = solve(ctx, c), solve(ctx, c)
        assert ra == rb == OK
        H.assert_bits_equal(xa, xb, c.name + " twice")


def test_sequence_on_one_context_equals_fresh_contexts(ctx):
    """a large n, a small one, a singular call and a mid-sized one: stale Ldiag / Y / X / status of the arena decide nothing"""
    seq = [P.case("dense", 700), P.case("fill", 33), P.with_zero_row(P.case("dense", 97), 40), P.case("dense", 97),
           P.case("dense", 1), P.case("hub", 353)]
    got = [solve(ctx, c) for c in seq]
    for c, (rc, x) in zip(seq, got):
        fresh = capi.Context(0)
        try:
            frc, fx = solve(fresh, c)
        finally:
            fresh.close()
        assert rc == frc == (SINGULAR if "zero row" in c.name else OK), c.name
        if rc == OK:
            H.assert_bits_equal(x, fx, c.name + ": in sequence vs fresh context")


def test_dense_solve_and_ba_step_around_a_posegraph_solve(ctx, golden):
    """sfmx_solve_dense and sfmx_ba_step share the context's arena with the structured solve"""
    prob = B.window(6)
    a = prob.kargs() + (B.HUBER0, B.LAMBDA0)
    q = ctx.ba_problem(prob.W, prob.X, prob.ptr, prob.li, prob.uv)
    try:
        rc, xd0 = ctx.solve_dense(golden["sg_A_36"], golden["sg_b_36"])
        assert rc == OK
        H.assert_bits_equal(xd0, golden["sg_x_36"], "dense solve")
        rc, dx0 = q.step(prob.poses, *a)
        assert rc == OK
        H.assert_bits_equal(dx0, B.oracle_step(prob)[1], "BA step")
        c = P.case("dense", 353)
        rc, x0 = solve(ctx, c)
        assert rc == OK
        rc, dx1 = q.step(prob.poses, *a)
        assert rc == OK
        H.assert_bits_equal(dx1, dx0, "BA step after a pose-graph solve")
        rc, xd1 = ctx.solve_dense(golden["sg_A_36"], golden["sg_b_36"])
        assert rc == OK
        H.assert_bits_equal(xd1, xd0, "dense solve after a pose-graph solve")
        rc, x1 = solve(ctx, c)
        assert rc == OK
        H.assert_bits_equal(x1, x0, "pose-graph solve after a dense solve and a BA step")
    finally:
        q.close()


# ---- 5. through posegraph_optimize_centers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", P.PIPE_SIZES)
def test_structured_branch_vs_dense_oracle_on_every_graph_kind(ctx, N, monkeypatch):
    monkeypatch.setenv("SFMX_POSEGRAPH_SOLVER", "structured")
    for kind in P.PIPE_KINDS:
        Rs, C, ei, ej, eR, et, lp = P.pipe_graph(kind, N)
        ok_o, Co = H.posegraph(O, "orc", Rs, C, ei, ej, eR, et, lp)
        ok_s, Cs = pipe.posegraph(ctx, Rs, C, ei, ej, eR, et, lp)
        assert ok_o == 1 and ok_s == 1, (kind, N)
        scale = np.abs(Co - C).max()
        assert scale > 1e-6, (kind, N)                               # the solve must actually move the centres
        err = np.abs(Cs - Co).max()
        print(f"{kind} N={N}: moved {scale:.3g}, structured - dense {err:.3g}")
        assert err <= 1e-9 * max(scale, np.abs(Co).max()), (kind, N, err)
        H.assert_bits_equal(Cs[0], C[0], "node 0 stays")


def test_cut_off_graphs_are_refused_with_the_centres_untouched(ctx, monkeypatch):
    """whatever the oracle's elimination makes of its last pivot: no loops (an exact zero), 3 ... 15 loops inside the cut-off part
    (rounding noise around the device's threshold; tests/test_posegraph_inputs_cpu.py shows which of them a pivot test lets
    through), a keyframe touched only by a self-edge"""
    monkeypatch.setenv("SFMX_POSEGRAPH_SOLVER", "structured")
    graphs = [(f"cut {c}", P.cut_graph(*c)) for c in P.CUT_CASES]
    graphs += [(f"cut N={N}, no loops", P.cut_graph(N, 0, 0)) for N in (3, 33, 40, 129)]
    graphs += [(f"self-edge only N={N}", P.self_edge_only_graph(N)) for N in (3, 33, 129)]
    let_through = []
    for what, (Rs, C, ei, ej, eR, et, lp) in graphs:
        ok_s, Cs = pipe.posegraph(ctx, Rs, C, ei, ej, eR, et, lp)
        if ok_s != 0 or not np.array_equal(H.bits(Cs), H.bits(C)):
            let_through.append((what, ok_s, float(np.abs(Cs - C).max())))
    assert not let_through, let_through
