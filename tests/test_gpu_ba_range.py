"""The bundle-adjustment kernels over their whole range: ragged observation lists with every kind of point (tests/ba_inputs.py),
every points kernel / reduction tile / solver the dispatch rules of csrc/hip/ba.hip can select, W from 1 to 64, P on every tile,
workgroup and chunk boundary, the extremes of huber and lambda, non-finite and boundary data, and re-use of one problem object.
The contract is the one of the rest of the BA tests: S, b and dx equal orc_ba_build / orc_solve_gauss bit for bit, and the status
is SFMX_ERR_SINGULAR exactly where the oracle's solve fails.  tests/test_ba_inputs_cpu.py proves on the CPU that the inputs reach
what they are meant to reach."""
import importlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import ba_inputs as B
import helpers as H

pytestmark = pytest.mark.gpu

capi = importlib.import_module(H.PKG_NAME + ".capi")

SWITCHES = ("SFMX_BA_POINTS", "SFMX_BA_PTS", "SFMX_BA_TILE", "SFMX_BA_SOLVE", "SFMX_BA_PUBLISH", "SFMX_BA_RESIDENT", "SFMX_VIRTUAL_WORLD",
            "SFMX_VIRTUAL_WORLD_ORDER")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _setenv(monkeypatch, **env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


_oracle_cache: dict = {}


def _expected(prob, huber, lam):
    """(S damped, b damped, S raw, b raw, solve status, dx) of the oracle, computed once per problem and parameter set"""
    key = (id(prob), repr(float(huber)), repr(float(lam)))
    if key not in _oracle_cache:
        S1, b1 = B.oracle_build(prob, huber, lam, True)
        S0, b0 = B.oracle_build(prob, huber, lam, False)
        erc, ex = H.solve_gauss(H.oracle(), "orc", S1, b1)
        _oracle_cache[key] = (prob, S1, b1, S0, b0, erc, ex)
    return _oracle_cache[key][1:]


def _compare(got, prob, huber, lam, what, nan=False):
    """got = (S1, b1, S0, b0, rc, dx) of the device against the oracle"""
    S1, b1, S0, b0, erc, ex = _expected(prob, huber, lam)
    if nan:  # NaN by construction: it must really be there, or nan_equal would be a tolerance
        assert np.isnan(S1).any() or np.isnan(b1).any(), what
    H.assert_bits_equal(got[0], S1, f"{what}: S damped", nan_equal=nan)
    H.assert_bits_equal(got[1], b1, f"{what}: b damped", nan_equal=nan)
    H.assert_bits_equal(got[2], S0, f"{what}: S undamped", nan_equal=nan)
    H.assert_bits_equal(got[3], b0, f"{what}: b undamped", nan_equal=nan)
    assert int(got[4]) == (capi.SFMX_OK if erc == 0 else capi.SFMX_ERR_SINGULAR), (what, int(got[4]), erc)
    if erc == 0:
        H.assert_bits_equal(got[5], ex, f"{what}: dx", nan_equal=nan)


def _check(ctx, prob, params, what, nan=False, q=None):
    """build (damped and undamped) against orc_ba_build, step against orc_solve_gauss on the oracle's damped system, the status"""
    huber, lam = params.get("huber", B.HUBER0), params.get("lam", B.LAMBDA0)
    own = q is None
    if own:
        q = ctx.ba_problem(prob.W, prob.X, prob.ptr, prob.li, prob.uv)
    try:
        a = prob.kargs() + (huber, lam)
        S1, b1 = q.build(prob.poses, *a, True)
        S0, b0 = q.build(prob.poses, *a, False)
        rc, dx = q.step(prob.poses, *a)
        _compare((S1, b1, S0, b0, rc, dx), prob, huber, lam, what, nan)
    finally:
        if own:
            q.close()


def _window_id(W, P, fl, **kw):
    return f"W{W}-P{P}-{fl}-{B.points_kernel(W, P, fl == 'dup', **kw)}-{B.solver(W)}"


# ---- a. ragged windows, W = 1 .. 64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,P,fl", [pytest.param(W, P, fl, id=_window_id(W, P, fl)) for W, P, fl in B.WINDOWS])
@pytest.mark.parametrize("K", ["temple", "skewed"])
def test_ragged_window(ctx, W, P, fl, K):
    prob = B.window(W, fl, K=K)
    assert B.has_dup(prob) == (fl == "dup")
    _check(ctx, prob, {}, f"W={W} P={P} {fl} K={K}")


@pytest.mark.parametrize("fl", ["clean", "dup"])
def test_window_with_a_camera_that_looks_away(ctx, fl, monkeypatch):
    """a zero slot among live ones (G of that slot is 0 * iH, which can be -0.0), in the LDS kernel and in the general one"""
    prob = B.window(6, fl, half_behind=3)
    for pts_env in (None, "global"):
        _setenv(monkeypatch, SFMX_BA_POINTS=pts_env)
        _check(ctx, prob, {}, f"half-behind {fl} points={pts_env}")


# ---- b. launch shapes (switches that are read per call) -------------------------------------------------------------------------
GRID = list(itertools.product((None, "global"), (1, 2, 4), (16, 32, 64), (None, "device"), (None, "last")))


@pytest.mark.parametrize("W,fl", [(6, "clean"), (6, "dup"), (10, "clean"), (16, "clean")])
def test_launch_shapes(ctx, W, fl, monkeypatch):
    prob = B.window(W, fl)
    for points, pts, tile, solve, publish in GRID:
        _setenv(monkeypatch, SFMX_BA_POINTS=points, SFMX_BA_PTS=pts, SFMX_BA_TILE=tile, SFMX_BA_SOLVE=solve, SFMX_BA_PUBLISH=publish)
        _check(ctx, prob, {}, f"W={W} {fl} points={points} pts={pts} tile={tile} solve={solve} publish={publish}")


@pytest.mark.parametrize("W", [pytest.param(15, id="W15-lds"), pytest.param(16, id="W16-window")])
def test_lds_budget_either_side(ctx, W, monkeypatch):
    """SFMX_BA_PTS=4: 4 x 15 slot records fit the 40 KB of the LDS kernel, 4 x 16 do not"""
    _setenv(monkeypatch, SFMX_BA_PTS=4)
    assert B.points_kernel(W, 300, False, pts=4) == ("lds" if W == 15 else "window")
    _check(ctx, B.window(W, "clean"), {}, f"W={W} pts=4")


@pytest.mark.parametrize("W,fl", [(6, "clean"), (6, "dup"), (10, "clean"), (7, "dup"), (11, "clean")])
def test_timed_context_takes_the_synchronous_path(ctx, W, fl):
    """with kernel timing on, a step does not poll pinned memory: it synchronises the stream and copies dx | status back"""
    ctx.set_timing(True)
    try:
        _check(ctx, B.window(W, fl), {}, f"timing on, W={W} {fl}")
    finally:
        ctx.set_timing(False)


# ---- c. P on every boundary -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl", ["clean", "dup"])
@pytest.mark.parametrize("P", B.P_EDGES)
@pytest.mark.parametrize("W", B.P_EDGE_W)
def test_point_count_boundaries(ctx, W, P, fl, monkeypatch):
    prob = B.edge(W, P, fl)
    for pts in (1, 2, 4):
        for tile in ((16, 32, 64) if W == 6 else (None,)):  # the switch only selects among the fused W = 6 reductions
            _setenv(monkeypatch, SFMX_BA_PTS=pts, SFMX_BA_TILE=tile)
            _check(ctx, prob, {}, f"W={W} P={P} {fl} pts={pts} tile={tile}")


@pytest.mark.parametrize("W,P", [pytest.param(W, P, id=f"W{W}-P{P}-{B.points_kernel(W, P, True)}") for W, P in B.BIG_P])
def test_big_point_counts(ctx, W, P, monkeypatch):
    """either side of BA_MERGED_EXPAND_MAX_P and of the chunk ends of the two-slot ring (a last chunk of one row)"""
    prob = B.big(W, P)
    _check(ctx, prob, {}, f"W={W} P={P}")
    if P in (4097, 8193) and W == 6:
        erc, ex = _expected(prob, B.HUBER0, B.LAMBDA0)[4:]
        assert erc == 0
        q = ctx.ba_problem(prob.W, prob.X, prob.ptr, prob.li, prob.uv)
        for world in (2, 8):
            _setenv(monkeypatch, SFMX_VIRTUAL_WORLD=world)
            rc, dx = q.step_sharded_elements(None, prob.poses, *prob.kargs(), B.HUBER0, B.LAMBDA0)
            assert rc == 0
            H.assert_bits_equal(dx, ex, f"element-sharded, virtual world {world}, P={P}")
            # point shards handed on in relay order continue each other's running sums (init = S): the reference's sequence again,
            # with shard boundaries that fall inside the chunks of the row ring
            _setenv(monkeypatch, SFMX_VIRTUAL_WORLD_ORDER="relay")
            rc, dx = q.step_sharded(None, prob.poses, *prob.kargs(), B.HUBER0, B.LAMBDA0)
            assert rc == 0
            H.assert_bits_equal(dx, ex, f"point-sharded relay, virtual world {world}, P={P}")
            _setenv(monkeypatch, SFMX_VIRTUAL_WORLD_ORDER=None)
        q.close()


# ---- d. switches that are read once per process: fresh children ----------------------------------------------------------------
_child_fault = []


@pytest.mark.parametrize("which", ["split", "merged", "chunk128", "nofuse", "nopoll"])
def test_process_wide_switches(which, tmp_path):
    if _child_fault:
        pytest.skip(f"nothing more is started on the device after a fault ({_child_fault[0]})")
    out = str(tmp_path / f"{which}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("SFMX_")}
    env.update(B.CHILD_ENV[which])
    env["SFMX_NO_TORCH_PRELOAD"] = "1"  # nothing in the child uses torch: the library binds the system HIP runtime, as the CLI does
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ba_child.py")
    try:
        p = subprocess.run([sys.executable, child, which, out], env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        _child_fault.append(f"{which}: timeout")
        raise
    if p.returncode < 0 or p.returncode in (134, 139):
        _child_fault.append(f"{which}: exit status {p.returncode}")
    assert p.returncode == 0, p.stdout[-3000:]
    got = np.load(out)
    cases = B.child_cases(which)
    assert list(got["names"]) == list(cases)
    for i, (name, prob) in enumerate(cases.items()):
        for tag, rc, dx in (("", "rc", "dx"), (" (second step)", "rc2", "dx2")):
            _compare((got[f"{i}:S1"], got[f"{i}:b1"], got[f"{i}:S0"], got[f"{i}:b0"], got[f"{i}:{rc}"], got[f"{i}:{dx}"]), prob, B.HUBER0, B.LAMBDA0,
                     f"{which}: {name}{tag}")


# ---- e. parameters --------------------------------------------------------------------------------------------------------------
PARAM_PROBLEMS = {"W6-clean": lambda: B.window(6, "clean"), "W6-dup": lambda: B.window(6, "dup"), "W6-P4097": lambda: B.big(6, 4097)}


@pytest.mark.parametrize("huber", B.HUBER, ids=[str(h) for h in B.HUBER])
@pytest.mark.parametrize("name", list(PARAM_PROBLEMS))
def test_huber_range(ctx, name, huber):
    prob = PARAM_PROBLEMS[name]()
    h = B.huber_value(prob, huber)
    _check(ctx, prob, {"huber": h}, f"{name} huber={huber}", nan=(h != h))


@pytest.mark.parametrize("lam", B.LAMBDA)
@pytest.mark.parametrize("name", list(PARAM_PROBLEMS))
def test_lambda_range(ctx, name, lam):
    _check(ctx, PARAM_PROBLEMS[name](), {"lam": lam}, f"{name} lambda={lam}")


@pytest.mark.parametrize("W,solve", [(6, None), (6, "device"), (10, None), (10, "device"), (7, None), (11, None)],
                         ids=["W6-host", "W6-fused", "W10-host", "W10-fused", "W7-wave", "W11-blocked"])
def test_zero_system_is_singular_in_every_solver(ctx, W, solve, monkeypatch):
    _setenv(monkeypatch, SFMX_BA_SOLVE=solve)
    prob = B.window(W, "clean")
    assert _expected(prob, 0.0, 0.0)[4] != 0
    _check(ctx, prob, {"huber": 0.0, "lam": 0.0}, f"W={W} solve={solve} huber=0 lambda=0")


# ---- f. non-finite and boundary data --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.NONFINITE)
@pytest.mark.parametrize("shape", ["lds", "global", "P4097"])
def test_nonfinite_and_boundary_data(ctx, name, shape, monkeypatch):
    prob, nan = B.nonfinite_case(name, 4097 if shape == "P4097" else 64)
    _setenv(monkeypatch, SFMX_BA_POINTS="global" if shape == "global" else None)
    _check(ctx, prob, {}, f"{name} {shape}", nan=nan)


# ---- g. object reuse ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True], ids=["plain", "resident"])
def test_one_object_through_many_windows(ctx, resident, monkeypatch):
    """sfmx_ba_reset on one grow-only object, as the pipeline uses it: stale records and slot tables of a larger problem, lds_points and
    chunk flipping both ways, two resets in a row (the staging slab still in flight).  resident: the W = 6 windows also run a job
    (a step inside it, a step with other parameters than the job was started with, an end after 2 of 5, a reset while it is active)."""
    if resident:
        _setenv(monkeypatch, SFMX_BA_RESIDENT=1)
    seq = B.reset_sequence()
    first = seq[0][1]
    q = ctx.ba_problem(first.W, first.X, first.ptr, first.li, first.uv)

    def job(prob, what):
        a = prob.kargs() + (B.HUBER0, B.LAMBDA0)
        ex = _expected(prob, B.HUBER0, B.LAMBDA0)[5]
        q.begin(5, *a)
        for k in range(2):
            rc, dx = q.step(prob.poses, *a)
            assert rc == 0
            H.assert_bits_equal(dx, ex, f"{what}: step {k} of a job")
        rc, dx = q.step(prob.poses, *prob.kargs(), 0.5, B.LAMBDA0)  # other parameters: the job is released, the plain path runs
        assert rc == 0
        H.assert_bits_equal(dx, _expected(prob, 0.5, B.LAMBDA0)[5], f"{what}: step with another huber inside a job")
        q.begin(5, *a)
        for k in range(2):
            rc, dx = q.step(prob.poses, *a)
            assert rc == 0
            H.assert_bits_equal(dx, ex, f"{what}: step {k} of a job ended early")
        q.end()

    _check(ctx, first, {}, "created: " + seq[0][0], q=q)
    for name, prob in seq[1:]:
        q.reset(prob.W, prob.X, prob.ptr, prob.li, prob.uv)
        assert (q.W, q.P) == (prob.W, prob.P)
        if resident and prob.W == 6:
            job(prob, name)
        _check(ctx, prob, {}, "reset to " + name, q=q)
        if resident and prob.W == 6:  # leave a job active: the next reset has to release it
            q.begin(5, *prob.kargs(), B.HUBER0, B.LAMBDA0)
            rc, dx = q.step(prob.poses, *prob.kargs(), B.HUBER0, B.LAMBDA0)
            assert rc == 0
    a, b = seq[0][1], seq[2][1]
    q.reset(a.W, a.X, a.ptr, a.li, a.uv)  # two resets in a row, no step between them
    q.reset(b.W, b.X, b.ptr, b.li, b.uv)
    _check(ctx, b, {}, "two resets in a row", q=q)
    q.reset(a.W, a.X, a.ptr, a.li, a.uv)
    _check(ctx, a, {}, "back to the largest", q=q)
    q.close()


# ---- h. resident job on ragged data ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [300, 1, 3, 17, 257])
def test_resident_job_on_ragged_data(ctx, P, monkeypatch):
    """the chain of test_ba_resident_job_equals_plain_steps (poses fed back from dx) on windows with every kind of point"""
    W = 6
    prob = B.window(6, "dup") if P == 300 else B.edge(6, P, "dup")
    a = prob.kargs() + (B.HUBER0, B.LAMBDA0)
    q = ctx.ba_problem(W, prob.X, prob.ptr, prob.li, prob.uv)

    def chain(n, resident, iters=None, end_after=None):
        poses = prob.poses.copy()
        out = []
        if resident:
            q.begin(iters if iters is not None else n, *a)
        for k in range(n):
            if end_after is not None and k == end_after:
                q.end()
            rc, dx = q.step(poses, *a)
            assert rc == 0
            out.append(dx.copy())
            poses[1:, 9:] += 1e-3 * dx.reshape(W, 6)[1:, 3:]
        if resident:
            q.end()
        return out

    _setenv(monkeypatch, SFMX_BA_RESIDENT=0)
    ref = chain(5, False)
    H.assert_bits_equal(ref[0], _expected(prob, B.HUBER0, B.LAMBDA0)[5], "plain step 0 vs oracle")
    _setenv(monkeypatch, SFMX_BA_RESIDENT=1)
    for tag, got in (("5 of 5", chain(5, True)), ("ended after 2", chain(5, True, end_after=2)), ("5 steps on a 3-iteration job", chain(5, True, iters=3)),
                     ("again", chain(5, True))):
        for k in range(5):
            H.assert_bits_equal(got[k], ref[k], f"resident job ({tag}) step {k}, P={P}")
    q.close()
