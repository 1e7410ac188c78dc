"""The linear systems of the dense-solve cases of tests/test_gpu_kernels.py (test_solve_dense, test_solve_register_kernels_edge_cases,
test_solve_dense_blocked_sizes, test_solve_skipped_multipliers_decide_bits), generated in one place: the GPU tests compare
sfmx_solve_dense with orc_solve_gauss on them, and tests/test_oracle_vs_reference_range.py compares orc_solve_gauss with the reference's solve_gauss on the very same matrices.
numpy only: no device, no oracle.  Every generator draws from one seeded stream in a fixed order, so a case must not be removed
from the middle of a list without the ones behind it changing.
The second half holds the range suite of the dense solvers (tests/test_gpu_solve_range.py): every n from 1 to 130, designed pivot
sequences, the global-scratch panel, pivot ties in the lower word, both thresholds from both sides, non-finite and subnormal
input, with the NumPy model of the elimination (pivot_trace) that says which branches a system reaches."""
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
    """[(id, A, b)] of every system above and below, ids unique.  A sweep case holds several systems: A and b are then tuples
    (see `systems`)"""
    out = [(f"dense/{name}", A, b) for name, A, b in dense_random_cases()]
    for n in REGISTER_N:
        out += [(f"regs{n}/{name}", A, b) for name, A, b in register_cases(n)]
    out += [(f"blocked/{name}", A, b) for name, A, b in blocked_cases()]
    out += [(f"skip/{name}", A, b) for name, A, b in skip_cases()]
    out += [(f"sweep/{name}", A, b) for name, A, b in sweep_cases()]
    out += [(f"scratch/{name}", A, b) for name, A, b in panel_scratch_cases()]
    out += [(f"tie/{name}", A, b) for name, A, b in tie_cases()]
    out += [(f"threshold/{c[0]}", c[1], c[2]) for c in threshold_cases()]
    out += [(f"special/{name}", A, b) for name, A, b in special_cases()]
    return out


def systems(cid, A, b):
    """[(id, A, b)] of the single systems of one entry of all_cases()"""
    if isinstance(A, tuple):
        return [(f"{cid} {s}", Ak, bk) for s, Ak, bk in zip(SWEEP_SYSTEMS, A, b)]
    return [(cid, A, b)]


# ---- the range suite of the dense solvers (tests/test_gpu_solve_range.py, tests/test_solve_inputs_cpu.py) ----------------------------
# Everything below draws from streams of its own (one per case), so the generators above are untouched.
LU_NB = 32                  # columns per panel of the blocked elimination (csrc/hip/ba.hip)
PANEL_LDS_ROWS = 624        # k_lu_panel<true> while (n - k0) * LU_NB * 8 <= 156 KiB; from 625 rows on the panel copy is in global scratch
MUTANTS = ("high word only", "last of full ties", "skip on <=", "singular on <=", "nan below wins", "b not swapped at n=64 k=0", "fma")


def _fma(a, f, r):
    """a - f * r rounded once (finite operands): math.fma where Python has it, otherwise exact rational arithmetic"""
    import math
    if hasattr(math, "fma"):
        return math.fma(-f, r, a)
    from fractions import Fraction
    return float(Fraction(a) - Fraction(f) * Fraction(r))


def pivot_trace(A, b, mutant=None):
    """dense.hpp:54-93 on whole rows -> (rc, x, pivots, tiny): the first maximum of |a_ik| over i >= k (a NaN never wins unless it
    sits on the diagonal), rc = 1 at a pivot < 1e-15 (x is then None), swap, division of row k, a_i -= f_i * a_k with separate
    multiply and subtract for every row with |f_i| >= 1e-18, the ascending-j subtraction chain of the back substitution.
    pivots[k] is the position chosen at step k (of the steps that ran), tiny the number of non-zero multipliers that were skipped.
    It says which branches an input reaches; `mutant` (one of MUTANTS) changes one rule, for tests/test_solve_inputs_cpu.py."""
    assert mutant is None or mutant in MUTANTS
    n = len(b)
    W = np.empty((n, n + 1))
    W[:, :n], W[:, n] = A, b
    pivots, tiny = [], 0
    with np.errstate(all="ignore"):
        for k in range(n):
            col = np.abs(W[k:, k])
            piv = k
            if mutant == "nan below wins" and np.isnan(col).any():
                piv = k + int(np.argmax(np.isnan(col)))
            elif col[0] == col[0]:
                c = np.where(np.isnan(col), -1.0, col)
                if mutant == "high word only":
                    c = (c.view(np.uint64) >> np.uint64(32)).astype(np.int64)
                    c[np.isnan(col)] = -1
                piv = k + (int(np.flatnonzero(c == c.max())[-1]) if mutant == "last of full ties" else int(np.argmax(c)))
            best = abs(W[piv, k])
            if best <= 1e-15 if mutant == "singular on <=" else best < 1e-15:
                return 1, None, pivots, tiny
            pivots.append(piv)
            if piv != k:
                lim = n if (mutant == "b not swapped at n=64 k=0" and n == 64 and k == 0) else n + 1
                W[[k, piv], k:lim] = W[[piv, k], k:lim]
            W[k, k:] = W[k, k:] / W[k, k]
            f = W[k + 1:, k].copy()
            skip = np.abs(f) <= 1e-18 if mutant == "skip on <=" else np.abs(f) < 1e-18
            tiny += int((skip & (f != 0.0)).sum())
            rows = k + 1 + np.flatnonzero(~skip)
            if mutant == "fma":
                for i in rows:
                    W[i, k:] = [_fma(a, W[i, k], r) for a, r in zip(W[i, k:].tolist(), W[k, k:].tolist())]
            else:
                prod = f[~skip, None] * W[k, k:][None, :]
                W[rows, k:] = W[rows, k:] - prod
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            x[i] = np.subtract.reduce(np.concatenate((W[i, n:], W[i, i + 1:n] * x[i + 1:])))   # ((b_i - p_i+1) - p_i+2) - ...
    return 0, x, pivots, tiny


def urow_rows(pivots, n):
    """the bookkeeping of k_lu_urow, per panel of LU_NB columns: (tracked rows = block rows + distinct rows below the block that a
    step picks, steps that pick a row below the block which is tracked already, swaps inside the block).  The kernel's pos[] / cur[]
    hold 2 * LU_NB tracked rows, out_row[] / out_src[] LU_NB."""
    out = []
    for k0 in range(0, len(pivots), LU_NB):
        k1 = min(k0 + LU_NB, n)
        below, again, inside = set(), 0, 0
        for k in range(k0, min(k1, len(pivots))):
            p = pivots[k]
            if p >= k1:
                again += p in below
                below.add(p)
            elif p != k:
                inside += 1
        out.append((k1 - k0 + len(below), again, inside))
    return out


PATTERNS = ("reverse", "far", "last", "next")


def designed_pivots(n, pattern):
    """the position that `designed` makes win at every step"""
    t = {"reverse": lambda k: max(k, n - 1 - k), "far": lambda k: k + LU_NB if k + LU_NB < n else k,
         "last": lambda k: n - 1, "next": lambda k: min(k + 1, n - 1)}[pattern]
    return [t(k) for k in range(n)]


def designed(n, pattern, seed=0):
    """(A, b): 1e-3 * N(0,1) noise, and for every step k the value +-(8 + k / n) in column k of the row that sits at the pattern's
    target position when step k begins (the swaps of the steps before are followed), so that the elimination picks exactly
    designed_pivots(n, pattern)"""
    rng = np.random.default_rng([700 + seed, n, PATTERNS.index(pattern)])
    A = 1e-3 * rng.normal(size=(n, n))
    at = list(range(n))   # at[position] = original row sitting there
    for k, t in enumerate(designed_pivots(n, pattern)):
        A[at[t], k] = (8.0 + k / n) * (-1.0 if k % 2 else 1.0)
        at[k], at[t] = at[t], at[k]
    return A, rng.normal(size=n)


SWEEP_N = tuple(range(1, 131))
SWEEP_SYSTEMS = ("random",) + PATTERNS


def sweep_systems(n):
    """[(name, A, b)]: one random Gaussian system and the four designed ones of size n"""
    rng = np.random.default_rng([710, n])
    return [("random", rng.normal(size=(n, n)), rng.normal(size=n))] + [(p,) + designed(n, p) for p in PATTERNS]


def sweep_cases():
    """[(name, (A, ...), (b, ...))]: one case per n = 1 ... 130 holding the five systems of sweep_systems(n)"""
    out = []
    for n in SWEEP_N:
        s = sweep_systems(n)
        out.append((f"n={n}", tuple(A for _, A, _ in s), tuple(b for _, _, b in s)))
    return out


SCRATCH_N = (624, 625, 657)   # the last size that is all LDS, the first panel in scratch, the first two panels in scratch
SCRATCH_SINGULAR = "n=657 duplicate column 650"


def panel_scratch_cases():
    """[(name, A, b)]: systems whose pivots move rows inside k_lu_panel<false> (the global-scratch panel copy), the same at the last
    size without it, a random system, and one that turns singular in a late (LDS) panel after both scratch panels"""
    out = []
    for n in SCRATCH_N:
        for p in ("reverse", "far", "last"):
            out.append((f"n={n} {p}",) + designed(n, p))
    rng = np.random.default_rng(720)
    out.append(("n=657 random", rng.normal(size=(657, 657)), rng.normal(size=657)))
    A = rng.normal(size=(657, 657))
    A[:, 650] = A[:, 645]
    out.append((SCRATCH_SINGULAR, A, rng.normal(size=657)))
    return out


TIE_N_KS = ((12, 3), (36, 0), (36, 17), (60, 53), (64, 31), (97, 40), (130, 64))
TIE_HI = 1.5 + 2.0 ** -30   # same upper 32 bits as 1.5, bit 22 of the lower word set


def tie_cases():
    """[(name, A, b)]: A = blockdiag(D, T), D diagonal ks x ks with entries about 3 (steps below ks leave T alone), T = 0.25 * N(0,1)
    with the first column 0.1 except 1.5 at local row 1, the double below TIE_HI at row 2, -TIE_HI at row m / 2 and +TIE_HI at row
    m - 1: all four share the upper word, the lower word decides, and of the two full ties the first (row m / 2) must win step ks"""
    out = []
    for n, ks in TIE_N_KS:
        rng = np.random.default_rng([730, n, ks])
        m = n - ks
        A = np.zeros((n, n))
        A[np.arange(ks), np.arange(ks)] = 3.0 + 0.25 * rng.uniform(-1.0, 1.0, size=ks)
        T = 0.25 * rng.normal(size=(m, m))
        T[:, 0] = 0.1
        T[1, 0], T[2, 0], T[m // 2, 0], T[m - 1, 0] = 1.5, np.nextafter(TIE_HI, 0.0), -TIE_HI, TIE_HI
        A[ks:, ks:] = T
        out.append((f"n={n} ks={ks}", A, rng.normal(size=n)))
    return out


THRESHOLD_N = (12, 36, 60, 64, 97)
PIVOT_EDGE = (1e-15, float(np.nextafter(1e-15, 0.0)))                      # solvable, singular (dense.hpp:67: best < 1e-15)
MULT_EDGE = (1e-18, -1e-18, float(np.nextafter(1e-18, 0.0)), float(-np.nextafter(1e-18, 0.0)))   # applied, applied, skipped, skipped


def multiplier_positions(n):
    """[(tag, k, i)]: the multiplier sits at A[i, k]; at n = 97 once with k and i in different panels, once in the same one"""
    return [("far", n // 8, 3 * n // 4)] + ([("near", 5, 20)] if n == 97 else [])


def threshold_cases():
    """[(name, A, b, rc, tiny)] with the designed verdict and number of skipped non-zero multipliers.
    Pivots: upper-triangular A (every pivot is the diagonal element as it stands) with one diagonal element at exactly 1e-15
    (solvable) or the double below (singular), at the first, a middle and the last step.
    Multipliers: identity plus A[i, k] = f at |f| = 1e-18 (applied) or the double below (skipped), with A[k, i] = 3e17: applying
    f takes 0.3 off A[i, i] = 1, so the two sides differ in every bit pattern that depends on x[i]."""
    out = []
    for n in THRESHOLD_N:
        rng = np.random.default_rng([740, n])
        U = np.triu(rng.normal(size=(n, n)), 1)
        U[np.arange(n), np.arange(n)] = 2.0 + rng.uniform(size=n)
        b = rng.normal(size=n)
        for step in (0, n // 2, n - 1):
            for d in PIVOT_EDGE:
                A = U.copy()
                A[step, step] = d
                out.append((f"pivot n={n} step {step} {d!r}", A, b, int(d < 1e-15), 0))
        for tag, k, i in multiplier_positions(n):
            for f in MULT_EDGE:
                A = np.eye(n)
                A[i, k], A[k, i] = f, 3e17
                out.append((f"multiplier n={n} {tag} {f!r}", A, b, 0, int(abs(f) < 1e-18)))
    return out


SPECIAL_N = (36, 64, 97)
NAN_LATE = "n=97 nan on diagonal element 40"


def special_cases():
    """[(name, A, b)]: an infinite entry below the diagonal (it wins its step, inf / inf follows), two subnormal columns and a column
    of signed zeros (both end singular), a NaN below the diagonal of a column that is zero otherwise (singular: a NaN never wins,
    and the rule that lets it win would solve on) and, at n = 97, a NaN on a diagonal element that is reached in the second panel"""
    out = []
    for n in SPECIAL_N:
        rng = np.random.default_rng([750, n])
        for v in (np.inf, -np.inf):
            A = rng.normal(size=(n, n))
            A[n - 3, n // 3] = v
            out.append((f"n={n} {v!r} below the diagonal", A, rng.normal(size=n)))
        A = rng.normal(size=(n, n))
        A[:, n // 2] *= 1e-310
        A[:, n - 2] *= 1e-320
        out.append((f"n={n} subnormal columns", A, rng.normal(size=n)))
        A = rng.normal(size=(n, n))
        A[:, n // 2] = np.where(np.arange(n) % 2 == 0, -0.0, 0.0)
        out.append((f"n={n} column of signed zeros", A, rng.normal(size=n)))
        A = rng.normal(size=(n, n)) + 40.0 * np.eye(n)   # dominant diagonal: no row moves before step n / 2, the NaN stays in its row
        A[:, n // 2] = 0.0
        A[n - 2, n // 2] = np.nan
        out.append((f"n={n} nan below the diagonal of a zero column", A, rng.normal(size=n)))
    rng = np.random.default_rng(751)
    A = rng.normal(size=(97, 97)) + 40.0 * np.eye(97)   # dominant diagonal: no row moves, the NaN waits at (40, 40)
    A[40, 40] = np.nan
    out.append((NAN_LATE, A, rng.normal(size=97)))
    return out


def non_finite(A):
    """nan_equal applies to a case only where its input holds a NaN or an infinity"""
    return not np.isfinite(A).all()


def banded_6600():
    """the n = 6600 system of test_solve_dense_has_no_size_cliff (tests/test_gpu_kernels.py) as its diagonals {d: values}, from the
    same draws in the same order, without the dense matrix"""
    rng = np.random.default_rng(31)
    for n in (97, 300, 513):
        rng.normal(size=(n, n)), rng.normal(size=n)
    n, bw = 6600, 24
    diags = {d: rng.normal(size=n - abs(d)) for d in range(-bw, bw + 1)}
    diags[0] = diags[0] + 3.0 * bw ** 0.5
    return n, bw, diags


def banded_swaps(n, bw, diags):
    """the number of row swaps of dense.hpp:54-93 on a banded matrix, by elimination inside the band; valid as long as no swap
    happens (a swap widens the band), so it returns at the first one: 0 means none at all"""
    B = np.zeros((n, 2 * bw + 1))   # B[i, bw + d] = A[i, i + d]
    for d, v in diags.items():
        B[max(0, -d):max(0, -d) + len(v), bw + d] = v
    for k in range(n):
        h = min(bw, n - 1 - k)
        col = np.abs(B[np.arange(k, k + h + 1), bw - np.arange(h + 1)])   # A[k + r, k]
        if int(np.argmax(col)) != 0:
            return 1
        assert col[0] >= 1e-15
        B[k, bw:] = B[k, bw:] / B[k, bw]
        for r in range(1, h + 1):
            f = B[k + r, bw - r]
            if abs(f) < 1e-18:
                continue
            B[k + r, bw - r:2 * bw + 1 - r] = B[k + r, bw - r:2 * bw + 1 - r] - f * B[k, bw:]
    return 0
