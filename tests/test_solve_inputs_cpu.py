"""The inputs of the dense-solve range suite are what they claim, so that no GPU case of tests/test_gpu_solve_range.py can pass
vacuously (CPU: numpy, the oracle, and csrc/hip/solve_host.cpp compiled alone).

* solve_inputs.pivot_trace, the NumPy model that says which branches a system reaches, equals orc_solve_gauss bit for bit on every
  system of solve_inputs.all_cases(), verdict included.
* The designed systems realise their designed pivot sequences; from n = 65 on `reverse` and `far` fill the 64 tracked rows of
  k_lu_urow, `last` re-picks one row below the block at every step, `next` swaps inside the block and leaves it at its last step.
* The scratch cases swap rows inside the global-scratch panel; the n = 6600 system of tests/test_gpu_kernels.py never swaps.
* Ties are decided by the lower word and then by position; both thresholds are met from both sides with the designed outcome.
* Seven wrong rules (solve_inputs.MUTANTS), each applied to the model, are each told from the oracle by the group built for it.
* sfmx_host_solve_window, the solver of the product's default BA path, equals the oracle on every system and stays inside its
  work buffer of n * (n + 1) doubles."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import solve_inputs as SI

O = H.oracle()
CASES = SI.all_cases()
GROUPS = ("dense", "regs36", "regs60", "blocked", "skip", "sweep", "scratch", "tie", "threshold", "special")
SYSTEMS = {sid: (A, b) for cid, Ac, bc in CASES for sid, A, b in SI.systems(cid, Ac, bc)}
_trace, _oracle = {}, {}


def group(g):
    return [sid for sid in SYSTEMS if sid.split("/")[0] == g]


def trace(sid):
    if sid not in _trace:
        _trace[sid] = SI.pivot_trace(*SYSTEMS[sid])
    return _trace[sid]


def oracle(sid):
    if sid not in _oracle:
        _oracle[sid] = H.solve_gauss(O, "orc", *SYSTEMS[sid])
    return _oracle[sid]


def differs(sid, rc, x):
    """a result that is not the oracle's: another verdict, or other bits (any NaN equals any NaN)"""
    erc, ex = oracle(sid)
    if rc != erc:
        return True
    if rc != 0:
        return False
    ne = x.view(np.uint64) != ex.view(np.uint64)
    return bool((ne & ~(np.isnan(x) & np.isnan(ex))).any())


def test_groups_are_complete():
    assert {sid.split("/")[0] for sid in SYSTEMS} == set(GROUPS)
    assert len(SYSTEMS) == sum(len(SI.systems(*c)) for c in CASES), "duplicate system id"
    assert [len(group(g)) for g in ("sweep", "scratch", "tie", "threshold", "special")] == [650, 11, 7, 54, 16]


@pytest.mark.parametrize("g", GROUPS)
def test_model_equals_the_oracle(g):
    for sid in group(g):
        rc, x, pivots, tiny = trace(sid)
        erc, ex = oracle(sid)
        assert rc == erc, sid
        if rc == 0:
            H.assert_bits_equal(x, ex, sid, nan_equal=True)
            assert len(pivots) == len(ex)


# ---- designed pivot sequences -------------------------------------------------------------------------------------------------------
def test_designed_systems_realise_their_pivots():
    most = 0
    for n in SI.SWEEP_N:
        for p in SI.PATTERNS:
            rc, x, pivots, tiny = trace(f"sweep/n={n} {p}")
            assert rc == 0 and pivots == SI.designed_pivots(n, p), (n, p)
            panels = SI.urow_rows(pivots, n)
            most = max(most, max(t for t, _, _ in panels))
            if n < 65:
                continue
            nb0 = SI.LU_NB   # the first panel is a full block at these sizes
            if p in ("reverse", "far"):
                assert panels[0] == (2 * nb0, 0, 0), (n, p, panels)       # capacity of pos[] / cur[], out_row[] / out_src[] full
            if p == "last":
                assert panels[0] == (nb0 + 1, nb0 - 1, 0), (n, panels)    # one row below the block, picked at every step
            if p == "next":
                assert panels[0] == (nb0 + 1, 0, nb0 - 1), (n, panels)    # 31 swaps inside the block, then row k1 at kk = 31
                assert pivots[nb0 - 1] == nb0
    assert most == 2 * SI.LU_NB


def test_n64_reverse_reaches_the_lane_0_branch_and_every_dpp_row():
    """k_solve_wave at n = 64, k = 0: b is swapped by lane 0, which happens only where the first pivot is not row 0.  The maxima of
    wave_max_f64 come from each of its four rows of 16 lanes: `reverse` picks max(k, 63 - k), which is every lane of rows 2 and 3
    and by its definition none below 32; `next` (k + 1) supplies rows 0 and 1 at the same size."""
    pivots = trace("sweep/n=64 reverse")[2]
    assert pivots[0] == 63
    assert {p // 16 for p in pivots} == {2, 3} and set(pivots) == set(range(32, 64))
    assert {p // 16 for p in trace("sweep/n=64 next")[2]} == {0, 1, 2, 3} and trace("sweep/n=64 next")[2][0] == 1
    for n in range(34, 65):   # sizes the older cases never ran in this kernel: pivots in lanes 32 ... 63 at every one
        assert max(trace(f"sweep/n={n} reverse")[2]) == n - 1 >= 33


# ---- the global-scratch panel -------------------------------------------------------------------------------------------------------
def scratch_panels(n):
    """the panels (by their first column) whose column-major copy does not fit in LDS"""
    return [k0 for k0 in range(0, n, SI.LU_NB) if n - k0 > SI.PANEL_LDS_ROWS]


def test_scratch_cases_swap_rows_inside_scratch_panels():
    assert SI.PANEL_LDS_ROWS * SI.LU_NB * 8 <= 156 * 1024 < (SI.PANEL_LDS_ROWS + 1) * SI.LU_NB * 8
    assert [scratch_panels(n) for n in SI.SCRATCH_N] == [[], [0], [0, 32]]
    total = 0
    for name, A, b in SI.panel_scratch_cases():
        n = len(b)
        rc, x, pivots, tiny = trace(f"scratch/{name}")
        swaps = sum(pivots[k] != k for k0 in scratch_panels(n) for k in range(k0, k0 + SI.LU_NB))
        total += swaps
        if name == SI.SCRATCH_SINGULAR:
            assert rc == 1 and 640 <= len(pivots) <= 650, len(pivots)   # singular in the panel of columns 640 ... 656, in LDS
        else:
            assert rc == 0
        if n > SI.PANEL_LDS_ROWS:
            assert swaps >= 28 * len(scratch_panels(n)), (name, swaps)
        else:
            assert swaps == 0
        for p in ("reverse", "far", "last"):
            if name.endswith(p):
                assert pivots == SI.designed_pivots(n, p), name
                assert SI.urow_rows(pivots, n)[0] == ((64, 0, 0) if p != "last" else (33, 31, 0))
    print("row swaps inside scratch panels over the scratch cases:", total)
    assert total >= 8 * 32


def test_the_n6600_system_never_swaps():
    """why the scratch cases exist: the only system of the older tests that reaches k_lu_panel<false> (n = 6600, banded, dominant
    diagonal) performs no row swap at all, so pivot search, swap and write-back of that layout ran on trivial pivots only"""
    n, bw, diags = SI.banded_6600()
    assert n - SI.PANEL_LDS_ROWS > 0 and SI.banded_swaps(n, bw, diags) == 0
    # the banded model counts what the dense one counts
    rng = np.random.default_rng(5)
    small = {d: rng.normal(size=60 - abs(d)) for d in range(-3, 4)}
    A = sum(np.diag(v, d) for d, v in small.items())
    assert SI.banded_swaps(60, 3, small) == 1 and any(p != k for k, p in enumerate(SI.pivot_trace(A, np.ones(60))[2]))
    small[0] = small[0] + 9.0
    A = sum(np.diag(v, d) for d, v in small.items())
    assert SI.banded_swaps(60, 3, small) == 0 and SI.pivot_trace(A, np.ones(60))[2] == list(range(60))


# ---- ties and thresholds ------------------------------------------------------------------------------------------------------------
def test_tie_cases_are_decided_by_the_lower_word_then_the_position():
    for (n, ks), (name, A, b) in zip(SI.TIE_N_KS, SI.tie_cases()):
        m = n - ks
        col = np.abs(A[ks:, ks])
        hi, lo = col.view(np.uint64) >> np.uint64(32), col.view(np.uint64) & np.uint64(0xFFFFFFFF)
        top = np.flatnonzero(hi == hi.max())
        assert top.tolist() == [1, 2, m // 2, m - 1], name                      # four candidates share the upper word
        assert len(set(lo[top].tolist())) == 3 and lo[m // 2] == lo[m - 1] == lo[top].max()   # the lower word decides; two tie fully
        rc, x, pivots, tiny = trace(f"tie/{name}")
        assert rc == 0 and pivots[:ks] == list(range(ks)) and pivots[ks] == ks + m // 2, (name, pivots[:ks + 1])


def test_threshold_cases_have_the_designed_outcome():
    cases = SI.threshold_cases()
    for name, A, b, rc, tiny in cases:
        t = trace(f"threshold/{name}")
        assert (t[0], t[3]) == (rc, tiny), (name, t[0], t[3])
        if t[0] == 0:
            assert t[2] == list(range(len(b))), name   # pivots stay on the diagonal
    by = {name: trace(f"threshold/{name}") for name, *_ in cases}
    for n in SI.THRESHOLD_N:
        for tag, k, i in SI.multiplier_positions(n):
            for f in SI.MULT_EDGE[:2]:
                below = float(np.copysign(np.nextafter(abs(f), 0.0), f))
                xa, xs = by[f"multiplier n={n} {tag} {f!r}"][1], by[f"multiplier n={n} {tag} {below!r}"][1]
                assert xa.view(np.uint64)[i] != xs.view(np.uint64)[i] and abs(xa[i] / xs[i] - 1) > 0.1, (n, tag, f)
        assert n <= 64 or (SI.multiplier_positions(n)[0][1] // SI.LU_NB != SI.multiplier_positions(n)[0][2] // SI.LU_NB)


def test_special_cases_reach_their_branches():
    by = {name: (A, trace(f"special/{name}")) for name, A, b in SI.special_cases()}
    for n in SI.SPECIAL_N:
        for v in (np.inf, -np.inf):
            A, (rc, x, pivots, tiny) = by[f"n={n} {v!r} below the diagonal"]
            assert rc == 0 and A[n - 3, n // 3] == v and n - 3 > n // 3
        for name, step in (("subnormal columns", n // 2), ("column of signed zeros", n // 2), ("nan below the diagonal of a zero column", n // 2)):
            A, (rc, x, pivots, tiny) = by[f"n={n} {name}"]
            assert rc == 1 and len(pivots) == step, (n, name, rc, len(pivots))
        A = by[f"n={n} subnormal columns"][0]
        assert (np.abs(A[:, n // 2]) < 2.3e-308).all() and (A[:, n // 2] != 0).all()
        A = by[f"n={n} column of signed zeros"][0]
        assert (A[:, n // 2] == 0).all() and np.signbit(A[:, n // 2]).sum() == (n + 1) // 2
    A, (rc, x, pivots, tiny) = by[SI.NAN_LATE]
    assert rc == 0 and pivots == list(range(97)) and np.isnan(x).all() and 40 // SI.LU_NB == 1


# ---- mutants: one rule changed, and the group built for that rule notices --------------------------------------------------------------
def killers(mutant, sids):
    out = []
    for sid in sids:
        rc, x, _, _ = SI.pivot_trace(*SYSTEMS[sid], mutant=mutant)
        if differs(sid, rc, x):
            out.append(sid)
    return out


MUTANT_GROUP = {
    "high word only": lambda: group("tie"),
    "last of full ties": lambda: group("tie"),
    "skip on <=": lambda: [s for s in group("threshold") if "multiplier" in s],
    "singular on <=": lambda: [s for s in group("threshold") if "pivot" in s],
    "nan below wins": lambda: group("special"),
    "b not swapped at n=64 k=0": lambda: [f"sweep/n=64 {p}" for p in SI.SWEEP_SYSTEMS],
    "fma": lambda: [f"sweep/n={n} {p}" for n in range(2, 13) for p in SI.SWEEP_SYSTEMS],   # exact rational arithmetic where math.fma is missing: small n
}


@pytest.mark.parametrize("mutant", SI.MUTANTS)
def test_mutant_differs_from_the_oracle_on_its_group(mutant):
    sids = MUTANT_GROUP[mutant]()
    k = killers(mutant, sids)
    print(f"{mutant}: told from the oracle by {len(k)} of {len(sids)}:", k[:8])
    assert k, mutant
    if mutant in ("high word only", "last of full ties"):
        assert len(k) == len(sids)   # every tie case on its own: one per kernel and panel position
    if mutant == "skip on <=":
        assert len(k) == len(sids) // 2      # the two cases at exactly +-1e-18 of every size and position
    if mutant == "singular on <=":
        assert len(k) == len(sids) // 2      # the case at exactly 1e-15 of every size and step
    if mutant == "b not swapped at n=64 k=0":
        assert "sweep/n=64 reverse" in k


# ---- the host solver of the default BA path ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_solver(tmp_path_factory):
    """csrc/hip/solve_host.cpp alone, compiled by the product's own recipe for that object into a temporary directory"""
    out = str(tmp_path_factory.mktemp("solve_host"))
    csrc = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
    obj = os.path.join(out, "hiphost_solve_host.o")
    p = subprocess.run(["make", "-C", csrc, f"OUT={out}", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert "-ffp-contract=off" in p.stdout and "solve_host.cpp" in p.stdout, p.stdout
    so = os.path.join(out, "libsolve_host.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-shared", "-o", so, obj])
    fn = ctypes.CDLL(so).sfmx_host_solve_window
    fn.restype = ctypes.c_int
    return fn


GUARD = 64


@pytest.mark.parametrize("g", GROUPS)
def test_host_solver_equals_the_oracle_inside_its_work_buffer(host_solver, g):
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    mark = np.float64(-1.2345e300)
    for sid in group(g):
        A, b = (H.f64(v) for v in SYSTEMS[sid])
        n = len(b)
        work = np.full(GUARD + n * (n + 1) + GUARD, mark)
        x = np.full(GUARD + n + GUARD, mark)
        rc = host_solver(ptr(A), ptr(b), ctypes.c_int(n), ptr(x[GUARD:]), ptr(work[GUARD:]))
        for buf, used in ((work, n * (n + 1)), (x, n)):
            guard = np.concatenate((buf[:GUARD], buf[GUARD + used:]))
            assert len(guard) == 2 * GUARD and (guard.view(np.uint64) == mark.view(np.uint64)).all(), f"{sid}: wrote outside its buffer"
        erc, ex = oracle(sid)
        assert rc == erc, sid
        if rc == 0:
            H.assert_bits_equal(x[GUARD:GUARD + n], ex, sid, nan_equal=SI.non_finite(A))
