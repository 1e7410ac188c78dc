"""Range suite of the dense solve sfmx_solve_dense (csrc/hip/ba.hip): k_solve_wave (n <= 64), k_solve_regs<36 / 60> and the blocked
k_lu_init / k_lu_panel<true / false> / k_lu_urow / k_lu_update / k_lu_backsub<true / false> (n > 64).

Every comparison is with orc_solve_gauss, on bits: the verdicts are equal, and where the system is solvable so is every bit of x;
any NaN equals any NaN only in cases whose input holds a NaN or an infinity.  The systems come from tests/solve_inputs.py:

* every n from 1 to 130 with a random system and four designed pivot sequences (`reverse`, `far`, `last`, `next`): the n = 64
  branch of k_solve_wave, every lanes-per-row schedule, pivots in every DPP row, every panel and update-tile edge of the blocked
  path, and the 64 + 32 entries of k_lu_urow's permutation tables filled to the last one;
* n = 624, 625 and 657 with pivots that swap rows inside the global-scratch panel (and, run again with
  SFMX_BACKSUB_LDS_MAX_N=64, together with the global-scratch back substitution), a verdict of singular in a late panel;
* pivot ties in the upper 32 bits that the lower word decides, and full ties that the position decides, in every kernel;
* a pivot of exactly 1e-15 and the double below, a multiplier of exactly +-1e-18 and the double below;
* infinities, subnormal columns, signed zeros, NaN below the diagonal and on a diagonal element of a later panel;
* what a singular verdict and a large system leave behind in the context for the next call.

That these inputs reach what they claim -- the designed pivots, 64 tracked rows, swaps inside scratch panels, the outcome of
every threshold case, and that a solver with one rule changed is told from the oracle -- is asserted on the CPU by
tests/test_solve_inputs_cpu.py, which also holds the host solver of the default BA path (csrc/hip/solve_host.cpp) to the oracle.

Not covered, because the C API cannot hand them an arbitrary matrix: the copy of solve_regs_wave fused into k_ba_reduce
(SFMX_BA_SOLVE=device), which only ever sees the reduced camera system its own launch has summed, and the fall-back of n = 36 / 60
to k_solve_wave for a matrix that is not 16-byte aligned (the context's buffers always are)."""
import importlib

import numpy as np
import pytest

import helpers as H
import solve_inputs as SI

pytestmark = pytest.mark.gpu
O = H.oracle()
capi = importlib.import_module(H.PKG_NAME + ".capi")

_expected = {}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def expected(sid, A, b):
    if sid not in _expected:
        _expected[sid] = H.solve_gauss(O, "orc", A, b)
    return _expected[sid]


def mismatch(ctx, sid, A, b):
    """None, or what differs between sfmx_solve_dense and the oracle on one system"""
    rc, x = ctx.solve_dense(A, b)
    erc, ex = expected(sid, A, b)
    if rc != (capi.SFMX_ERR_SINGULAR if erc else capi.SFMX_OK):
        return f"{sid}: verdict {rc}, the oracle's {erc}"
    if erc == 0:
        try:
            H.assert_bits_equal(x, ex, sid, nan_equal=SI.non_finite(A))
        except AssertionError as e:
            return str(e)
    return None


def run_all(ctx, systems):
    bad = [m for m in (mismatch(ctx, sid, A, b) for sid, A, b in systems) if m]
    assert not bad, (f"{len(bad)} of {len(systems)} systems differ", bad[:12])


# ---- every n, designed pivots -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(1, 35), (36, 64), (65, 96), (97, 130)])
def test_sweep(ctx, lo, hi):
    systems = [(f"n={n} {name}", A, b) for n in range(lo, hi + 1) for name, A, b in SI.sweep_systems(n)]
    assert len(systems) == 5 * (hi - lo + 1)
    run_all(ctx, systems)


# ---- the global-scratch panel -------------------------------------------------------------------------------------------------------
SCRATCH = SI.panel_scratch_cases()


@pytest.mark.parametrize("backsub", ["lds", "global"])
@pytest.mark.parametrize("name,A,b", SCRATCH, ids=[c[0] for c in SCRATCH])
def test_panel_scratch(ctx, monkeypatch, name, A, b, backsub):
    if backsub == "global":   # k_lu_panel<false> and k_lu_backsub<false> in one solve
        monkeypatch.setenv("SFMX_BACKSUB_LDS_MAX_N", "64")
    run_all(ctx, [(f"scratch/{name}", A, b)])


# ---- ties, thresholds, special values -----------------------------------------------------------------------------------------------
TIES = SI.tie_cases()
THRESHOLDS = SI.threshold_cases()
SPECIAL = SI.special_cases()


@pytest.mark.parametrize("name,A,b", TIES, ids=[c[0] for c in TIES])
def test_ties_in_the_upper_word(ctx, name, A, b):
    run_all(ctx, [(f"tie/{name}", A, b)])


@pytest.mark.parametrize("n", SI.THRESHOLD_N)
def test_thresholds_from_both_sides(ctx, n):
    systems = [(f"threshold/{name}", A, b) for name, A, b, rc, tiny in THRESHOLDS if len(b) == n]
    assert len(systems) == (14 if n == 97 else 10)
    for (sid, A, b), (name, _, _, rc, tiny) in zip(systems, [c for c in THRESHOLDS if len(c[2]) == n]):
        assert expected(sid, A, b)[0] == rc, sid   # the designed verdict is the oracle's
    run_all(ctx, systems)


@pytest.mark.parametrize("name,A,b", SPECIAL, ids=[c[0] for c in SPECIAL])
def test_special_values(ctx, name, A, b):
    run_all(ctx, [(f"special/{name}", A, b)])


# ---- state --------------------------------------------------------------------------------------------------------------------------
def test_a_singular_verdict_and_a_large_system_leave_nothing_behind(ctx):
    """singular then good in each kernel family, then large -> small -> large on the working copy of the blocked path, all on one
    context of its own: every good result equals the one the same system gave as the first call of its kind on another context (and
    the oracle's), so neither a stale status word nor a stale x nor the working copy of the call before shows"""
    sweep = lambda n, name: next((f"n={n} {s}", A, b) for s, A, b in SI.sweep_systems(n) if s == name)
    special = {name: (f"special/{name}", A, b) for name, A, b in SPECIAL}
    scratch = {name: (f"scratch/{name}", A, b) for name, A, b in SCRATCH}
    good36, good64, good657 = sweep(36, "random"), sweep(64, "reverse"), scratch["n=657 random"]
    good65, good7 = sweep(65, "far"), sweep(7, "random")
    sing36, sing64, sing657 = special["n=36 column of signed zeros"], special["n=64 subnormal columns"], scratch[SI.SCRATCH_SINGULAR]
    first = {}
    for sid, A, b in (good36, good64, good657, good65, good7):
        rc, x = ctx.solve_dense(A, b)
        assert rc == capi.SFMX_OK
        first[sid] = x
    c = capi.Context(0)
    try:
        for step, (sid, A, b) in enumerate((sing36, good36, sing64, good64, sing657, good657, good65, good7, good657)):
            rc, x = c.solve_dense(A, b)
            erc, ex = expected(sid, A, b)
            assert rc == (capi.SFMX_ERR_SINGULAR if erc else capi.SFMX_OK), (step, sid, rc)
            if sid in first:
                assert erc == 0
                H.assert_bits_equal(x, first[sid], f"step {step}, {sid}: against the first-time result")
                H.assert_bits_equal(x, ex, f"step {step}, {sid}: against the oracle")
            else:
                assert erc == 1, sid
    finally:
        c.close()
