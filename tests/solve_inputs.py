"""The linear systems of the dense-solve cases of tests/test_gpu_kernels.py (test_solve_dense, test_solve_register_kernels_edge_cases,
test_solve_dense_blocked_sizes, test_solve_skipped_multipliers_decide_bits), generated in one place: the GPU tests compare
sfmx_solve_dense with orc_solve_gauss on them, and tests/test_oracle_vs_reference_range.py compares orc_solve_gauss with the reference's solve_gauss on the very same matrices.
numpy only: no device, no oracle.  Every generator draws from one seeded stream in a fixed order, so a case must not be removed
from the middle of a list without the ones behind it changing."""
from __future__ import annotations

import numpy as np

REGISTER_N = (36, 60)   # k_solve_regs<36 / 60>: the BA windows of 6 and 10 poses


def dense_random_cases():
    """[(name, A, b)]: the random systems of test_solve_dense (n = 1 ... 128, the |f| < 1e-18 skip at n = 33) and its 9 x 9 system
    with a NaN on the diagonal (the last entry)"""
    rng = np.random.default_rng(9)
    out = []
    for n in (1, 2, 33, 96, 128):
        A = rng.normal(size=(n, n))
        b = rng.normal(size=n)
        if n == 33:
            A[5, :] *= 1e-20  # exercises the |f| < 1e-18 skip
        out.append((f"random n={n}", A, b))
    A = rng.normal(size=(9, 9))
    A[4, 4] = np.nan  # NaN propagates instead of throwing, as in the reference
    out.append(("nan solve", A, np.ones(9)))
    return out


def register_cases(n):
    """[(name, A, b)] of test_solve_register_kernels_edge_cases: random systems, pivot ties (first position wins), the |f| < 1e-18
    skip, NaN on and off the diagonal, zero columns / singular systems"""
    rng = np.random.default_rng(100 + n)
    cases = []
    for t in range(6):
        cases.append((f"random {t}", rng.normal(size=(n, n)), rng.normal(size=n)))
    M = rng.normal(size=(n, n))
    cases.append(("spd", M @ M.T + 1e-3 * np.eye(n), rng.normal(size=n)))
    A = rng.integers(-3, 4, size=(n, n)).astype(np.float64)  # many equal |values| per column: ties at most steps
    cases.append(("integer ties", A + 0.0, rng.integers(-5, 6, size=n).astype(np.float64)))
    A = rng.normal(size=(n, n))
    A[:, 0] = np.where(np.arange(n) % 2 == 0, 2.5, -2.5)  # every row ties in the first column, signs differ
    cases.append(("tie column 0", A, rng.normal(size=n)))
    A = rng.normal(size=(n, n))
    A[5, :] *= 1e-20
    A[n - 2, :] *= 1e-19
    cases.append(("tiny multipliers", A, rng.normal(size=n)))
    A = rng.normal(size=(n, n))
    A[7, 3] = np.nan
    cases.append(("nan off the diagonal", A, np.ones(n)))
    A = rng.normal(size=(n, n))
    A[0, 0] = np.nan
    cases.append(("nan on the first diagonal element", A, np.ones(n)))
    A = rng.normal(size=(n, n))
    A[:, 4] = 0.0
    cases.append(("zero column", A, np.ones(n)))
    A = rng.normal(size=(n, n))
    A[n - 1, :] = A[0, :]
    cases.append(("duplicate row", A, np.ones(n)))
    cases.append(("identity with signed zeros", np.eye(n) * -1.0 + 0.0 * rng.normal(size=(n, n)), -np.ones(n)))
    return cases


def blocked_cases():
    """[(name, A, b)] of test_solve_dense_blocked_sizes, in its order: sizes around the block edges (tied pivots, skipped multipliers),
    a pose-graph-shaped system, a NaN and a rank-deficient matrix deep inside"""
    rng = np.random.default_rng(21)
    out = []
    for n in (65, 96, 97, 141, 300, 513):
        A = rng.normal(size=(n, n))
        b = rng.normal(size=n)
        if n == 97:
            A[40, :] *= 1e-20          # |f| < 1e-18 skip in the panel, in the block rows and in the trailing update
            A[:, 70] *= 1e-21
        if n == 141:
            A[100] = A[20]             # duplicate rows: tied pivot candidates, later an exactly singular step
        if n == 300:
            A = np.round(A * 4) / 4    # many exactly equal |a_ik|: first-maximum rule
        out.append((f"blocked n={n}", A, b))
    # pose-graph shape: weighted graph Laplacian (x) I3 plus a gauge term, 100 keyframes -> 300 unknowns
    N = 100
    L = np.zeros((3 * N, 3 * N))
    for a in range(N - 1):
        for c, w in ((a + 1, 400.0 + a), (min(N - 1, a + 7), 90.0)):
            for d in range(3):
                L[3 * a + d, 3 * a + d] += w; L[3 * c + d, 3 * c + d] += w
                L[3 * a + d, 3 * c + d] -= w; L[3 * c + d, 3 * a + d] -= w
    L[:3, :3] += np.eye(3) * 1e9
    out.append(("pose-graph system", L, rng.normal(size=3 * N)))
    A = rng.normal(size=(130, 130))
    A[77, 3] = np.nan
    out.append(("nan blocked", A, np.ones(130)))
    A = rng.normal(size=(200, 200))
    A[:, 150] = A[:, 10] * 2.0     # rank deficient: the pivot of some step deep inside falls below 1e-15 (or rounding keeps it alive -- same verdict either way)
    out.append(("rank-deficient blocked", A, np.ones(200)))
    return out


SKIP_N = (12, 36, 60, 97, 141)   # below the register kernels, the two register kernels, the blocked elimination


def skip_cases():
    """[(name, A, b)]: systems on which the |f| < 1e-18 skip (dense.hpp:80) decides bits of the solution.  The rows and columns scaled
    by 1e-20 in the cases above end in a pivot below 1e-15, so they are singular with or without the skip and only the verdict is
    compared.  Here A = [[B1, C], [1e-19 D, 1e-8 B2]] with B1, B2, C, D of order 1: under the first n / 2 pivots the multipliers of the
    lower rows are about 1e-19, and f * C is a 1e-11 share of the 1e-8 entries it would be subtracted from; the lower pivots are about
    1e-8, far above 1e-15.  tests/test_oracle_vs_reference_range.py asserts both properties on the CPU."""
    out = []
    for n in SKIP_N:
        rng = np.random.default_rng(300 + n)
        m = n // 2
        A = rng.normal(size=(n, n))
        A[:m, :m] += 4.0 * np.eye(m)      # pivots of the upper rows stay in the upper rows
        A[m:, :m] *= 1e-19
        A[m:, m:] = 1e-8 * (A[m:, m:] + 4.0 * np.eye(n - m))
        out.append((f"skip n={n}", A, rng.normal(size=n)))
    return out


def all_cases():
    """[(id, A, b)] of every system above, ids unique"""
    out = [(f"dense/{name}", A, b) for name, A, b in dense_random_cases()]
    for n in REGISTER_N:
        out += [(f"regs{n}/{name}", A, b) for name, A, b in register_cases(n)]
    out += [(f"blocked/{name}", A, b) for name, A, b in blocked_cases()]
    out += [(f"skip/{name}", A, b) for name, A, b in skip_cases()]
    return out
