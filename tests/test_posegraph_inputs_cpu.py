"""The inputs of the pose-graph range suite are what they claim (CPU: numpy, and libsfmx_host.so for the connectivity check): the
GPU cases of tests/test_gpu_posegraph_range.py rest on these sizes, matrices, bounds and graphs."""
import ctypes
import importlib

import numpy as np
import pytest

import helpers as H
import posegraph_inputs as P

pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
L = H.CLib(pipe.HOST_LIB_PATH)

# the smallest n at which each launch shape of sfmx_posegraph_solve first occurs
FIRST = {
    "single block": 1, "partial block": 1, "update inside a block": 2, "block of 31": 31, "full block": 32,
    "several blocks": 33, "rows below": 33, "one-row panel": 33, "tiles=1": 33, "ragged tile": 33,
    "n == ld - 1": 63, "n == ld": 64, "ld beyond its first step": 65, "lower quadrant of a diagonal tile": 65,
    "full tile": 96, "tiles=2": 97, "off-diagonal tile": 97,
    "tiles=3": 161, "tile beyond the first column of the third row": 161,
    "tiles=4": 225, "tiles=5": 289, "second panel workgroup": 289, "second backward workgroup": 289,
    "second backward workgroup, full block": 320, "tiles=6": 353,
}


def test_size_list_reaches_every_launch_shape():
    reach = {n: P.features(n) for n in range(1, 354)}
    first = {}
    for n in range(353, 0, -1):
        for f in reach[n]:
            first[f] = n
    assert first == FIRST
    listed = set().union(*(reach[n] for n in P.SIZES if n <= 353))
    assert listed == set(FIRST), set(FIRST) - listed                 # tiles=4 by the later steps of 289, 321 and 353
    # every size is the first one of some shape, so none can go: 321 is the first LISTED size whose second backward workgroup
    # meets a full 32-row block (320 runs the same launches for it); 700 is every shape at once on grids of up to 55 tiles
    for n in P.SIZES:
        if n == 321:
            assert min(m for m in P.SIZES if "second backward workgroup, full block" in reach.get(m, ())) == 321
        elif n == 700:
            assert {s.update_wgs for s in P.schedule(700)} >= {1, 3, 6, 10, 15, 21, 55, 66} and P.schedule(700)[0].panel_wgs == 3
        else:
            assert n in first.values(), n
    assert reach[353] >= set(FIRST) - {"single block", "n == ld", "n == ld - 1", "block of 31"}
    assert set(P.KIND_SIZES) <= set(P.SIZES)
    assert [P.tile_of(b) for b in range(7)] == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0)]
    for b in (10 ** 6, 2 ** 31 - 1):                                 # the decode's float start and its integer correction
        bi, bj = P.tile_of(b)
        assert 0 <= bj <= bi and bi * (bi + 1) // 2 + bj == b


@pytest.mark.parametrize("kind", ["dense", "ill"])
def test_dense_cases_fill_every_update_tile(kind):
    """every element every k_chol_update workgroup subtracts carries data, in every step; the model of the schedule is a Cholesky
    factorisation (its tiles cover the trailing triangle exactly once)"""
    off = 0
    for k, n in P.direct_cases():
        if k != kind:
            continue
        c = P.case(kind, n)
        assert (c.A != 0).all() and (c.A == c.A.T).all() and len(c.v) == n * (n + 1) // 2
        Lm, use = P.blocked_model(c.A)
        assert len(use) == sum(s.update_wgs for s in P.schedule(n))
        assert all(u.nonzero == u.elems > 0 for u in use), (n, [u for u in use if u.nonzero != u.elems][:3])
        assert np.abs(Lm @ Lm.T - c.A).max() <= 1e-13 * n * np.abs(c.A).max()
        off += sum(u.bi != u.bj for u in use)
    assert off == (1 + 30 + 55 if kind == "ill" else 1 + 5 + 30 + 40 + 55 + 385)   # off-diagonal launches from n = 97 on


def test_existing_chain_graph_leaves_the_update_tiles_almost_empty():
    """why the dense inputs exist: on the graph of test_posegraph_structured_solver_vs_dense_oracle a handful of the elements
    that off-diagonal k_chol_update tiles subtract are nonzero, one or two per loop edge and step"""
    tk = importlib.import_module("test_gpu_kernels")
    for a, b in zip(P.existing_chain(300), tk._pose_graph(300, max(4, 300 // 40), 2)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for N, tiles, live, elems, nonzero in ((300, 30, 17, 81920, 36), (1000, 1240, 211, 4487680, 842)):
        A = P.laplacian_of(P.existing_chain(N))[2]
        assert P.off_diagonal_occupancy(A) == (tiles, live, elems, nonzero)
        assert nonzero / elems < 5e-4                                # 0.044 % and 0.019 %
    # the chain-like Laplacians of the new suite are as empty; `fill` and `hub` are what loads the tiles on a graph
    for kind in ("chain", "backwards", "dup"):
        t, live, e, nz = P.off_diagonal_occupancy(P.case(kind, 353).A)
        assert nz / e < 5e-4
    for kind in ("fill", "hub"):
        t, live, e, nz = P.off_diagonal_occupancy(P.case(kind, 353).A)
        assert live == t == 55 and nz / e > 0.8


@pytest.mark.parametrize("kind", ("dense", "ill") + P.GRAPH_KINDS)
def test_reference_is_sound_and_plain_float64_meets_both_bounds(kind):
    """the longdouble reference solves its system to its own precision, and an unblocked float64 Cholesky with substitution --
    the arithmetic the bounds are derived for -- meets both with room: at most 0.11 below n = 31 and 0.01 from there on (DESIGN.md
    4.5.1 has the worst ratio per family).  The asserted room (0.5 / 0.05) is a cap on that, not a measurement."""
    for k, n in P.direct_cases():
        if k != kind:
            continue
        c = P.case(kind, n)
        assert P.reference_residual_ratio(c) <= 1.0, (c.name, P.reference_residual_ratio(c))
        res, fwd = P.ratios(c, P.solve_f64(c))
        print(f"{c.name}: residual / bound {res:.3g}, error / bound {fwd:.3g}")
        assert res <= 1.0 and fwd <= 1.0, (c.name, res, fwd)
        assert max(res, fwd) <= (0.5 if n < 31 else 0.05), (c.name, res, fwd)
        # the bounds are tight enough to see a kernel fault: one element of x off by 1e-6 relative misses both by orders
        x = P.solve_f64(c).copy()
        x[n // 2, 1] *= 1.0 + 1e-6
        res, fwd = P.ratios(c, x)
        print(f"{c.name}: one element off by 1e-6: residual / bound {res:.3g}, error / bound {fwd:.3g}")
        assert res > 1e3, (c.name, res, fwd)


def test_cut_off_components_with_loops_split_at_the_pivot_threshold():
    """the exposure the reachability check closes: the last pivot of a component without node 0 is zero only up to rounding once
    the component holds loop edges, so a pivot test lets some of these graphs through"""
    through, caught = [], []
    for N, loops, seed in P.CUT_CASES:
        ij, v, A = P.laplacian_of(P.cut_graph(N, loops, seed))
        assert not P.reachable(N, ij).all() and P.reachable(N, ij)[:N // 2 + 1].all()
        piv = P.pivots_f64(A)
        (through if len(piv) == N and (piv > P.PIVOT_MIN).all() else caught).append((N, loops, seed, float(piv[-1])))
        assert len(piv) == N and abs(piv[-1]) < 1e-14, piv[-1]       # only the component's last pivot is in doubt
    assert len(through) >= 3, through                                # (4: N = 40 and 70)
    assert len(caught) >= 3, caught                                  # (20, most of them slightly negative)
    # without loops every entry and every pivot is a small integer: the last one is exactly 0
    for N in (40, 129):
        piv = P.pivots_f64(P.laplacian_of(P.cut_graph(N, 0, 0))[2])
        assert len(piv) == N and piv[-1] == 0.0
    ij, v, A = P.laplacian_of(P.self_edge_only_graph(33))
    assert A[32, 32] == 0.0 and (32, 32) in set(map(tuple, ij.tolist())) and not P.reachable(33, ij)[32]


def _connected(n, ij):
    ij = H.i32(ij).reshape(-1, 2)
    return L.call("sfmx_host_posegraph_connected", ctypes.c_int, n, ij, len(ij))


def test_connectivity_check_on_every_graph_kind():
    seen = {0: 0, 1: 0}
    graphs = [(f"{k} n={n}", n, P.case(k, n).ij) for k in P.GRAPH_KINDS for n in P.KIND_SIZES]
    for kind in P.PIPE_KINDS:
        for N in P.PIPE_SIZES:
            g = P.pipe_graph(kind, N)
            if kind == "selfedge":
                assert (g[2] == g[3]).sum() == 4
            if kind == "oob":
                assert ((g[2] < 0) | (g[2] >= N) | (g[3] < 0) | (g[3] >= N)).sum() == 5
            graphs.append((f"pipe {kind} N={N}", N, P.laplacian_of(g)[0]))
    graphs += [(f"cut {c}", c[0], P.laplacian_of(P.cut_graph(*c))[0]) for c in P.CUT_CASES]
    graphs += [(f"cut {N}", N, P.laplacian_of(P.cut_graph(N, 0, 0))[0]) for N in (3, 40, 129)]
    graphs += [(f"self-edge only {N}", N, P.laplacian_of(P.self_edge_only_graph(N))[0]) for N in (3, 33, 129)]
    for what, n, ij in graphs:
        expect = int(P.reachable(n, ij).all())
        assert _connected(n, ij) == expect, what
        assert _connected(n, ij[::-1]) == expect, what               # any entry order
        seen[expect] += 1
    assert seen[1] >= 70 and seen[0] >= 30, seen
    assert _connected(1, np.zeros((0, 2), np.int32)) == 1            # node 0 alone
    assert _connected(1, [[0, 0]]) == 1
    assert _connected(2, [[0, 0], [1, 1]]) == 0                      # diagonal entries connect nothing
    assert _connected(2, [[0, 0], [1, 1], [1, 0]]) == 1
    assert _connected(3, [[2, 1], [1, 1]]) == 0                      # a component without node 0
    assert _connected(3, [[2, 1], [2, 0], [7, 0], [1, -1]]) == 1     # entries out of range are ignored
    assert _connected(0, [[0, 0]]) < 0 and L.call("sfmx_host_posegraph_connected", ctypes.c_int, 2, None, 1) < 0


def test_structured_branch_refuses_a_cut_graph_before_any_device_work(monkeypatch):
    """posegraph_optimize_centers on the structured branch with no context at all: an unreachable keyframe returns 0 with the
    centres untouched, and never reaches the solve that would need the device"""
    monkeypatch.setenv("SFMX_POSEGRAPH_SOLVER", "structured")
    for graph in (P.cut_graph(40, 3, 1), P.cut_graph(70, 15, 0), P.cut_graph(129, 0, 0), P.self_edge_only_graph(33)):
        Rs, C, ei, ej, eR, et, lp = graph
        c = C.copy()
        rc = L.call("sfmx_host_posegraph", ctypes.c_int, None, len(c), H.f64(Rs), c, len(ei), ei, ej, H.f64(eR), H.f64(et), lp)
        assert rc == 0
        H.assert_bits_equal(c, C, "centres of a refused graph")
