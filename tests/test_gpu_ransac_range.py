"""Range suite of csrc/hip/ransac.hip (k_hypotheses, k_score, k_patch_E, k_sampson_mask, the host logic of sfmx_ransac_score_ex)
and of its consumer ransac_local / ransac_merge: every launch shape, degenerate scenes (planar, rotation-only, duplicated points,
wide-angle and pixel-scale coordinates, NaN points), points a few ulp either side of the threshold, the threshold's own range, the
20-bit counters at their limit, argument rejection, the find_E_ransac seam on 1 ... 403 virtual ranks, and the second ("redo")
round in fresh processes.  The inputs, the oracle tables and the contract checker are tests/ransac_inputs.py; what the inputs
contain is asserted on the CPU by tests/test_ransac_inputs_cpu.py."""
import importlib
import os
import subprocess
import sys
from ctypes import POINTER, byref, c_double, c_int, c_int32, c_uint8

import numpy as np
import pytest

import helpers as H
import ransac_child as C
import ransac_inputs as R

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")

THRESHOLDS = (-1.0, 0.0, 1e-12, 5e-6, 1e-3, 1e9)
WORLDS = (1, 2, 3, 8, 403)
N_MAX = (1 << 20) - 1


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


_scored: dict = {}


def scored(ctx, name):
    """ransac_score_ex of a scene class at n = 600, H = 400 with the default switches, once"""
    if name not in _scored:
        s, T = R.scene(name), R.tables(name)
        _scored[name] = ctx.ransac_score_ex(s.xi, s.xj, T.idx8, s.thr)
    return _scored[name]


def resident_mask(ctx, n, E, thr):
    """sfmx_sampson_mask with xi = xj = NULL: the correspondences the preceding score call left on the device"""
    mask = np.full(n + 8, 7, np.uint8)
    cnt = c_int32()
    E = H.f64(E)
    ctx._chk(ctx.lib.sfmx_sampson_mask(ctx.h_, None, None, c_int(n), E.ctypes.data_as(POINTER(c_double)), c_double(thr),
                                       mask.ctypes.data_as(POINTER(c_uint8)), byref(cnt)))
    assert (mask[n:] == 7).all(), "written past n"
    return mask[:n], cnt.value


# ---- 1. every launch shape ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.N_SIZES)
def test_every_launch_shape(ctx, n):
    """N_SIZES x H_SIZES on `general`: one to seventeen trips of k_score's stride loop, full and ragged groups of k_hypotheses (4 per
    wave) and of k_score (8 per workgroup)"""
    xi, xj = R.points("general", n)
    T = R.tables("general", n)
    cref = R.ref_counts("general", n, R.THR)
    for h in R.H_SIZES:
        what = f"general n={n} H={h}"
        res = ctx.ransac_score_ex(xi, xj, T.idx8[:h], R.THR)
        R.check_contract(res, T.E[:h], cref[:h], what, T.idx8[:h])
        rep = R.repeated(T.idx8[:h])
        assert res["flags"].astype(bool)[rep].all(), (what, "repeated-index octets are scored with the exact host hypothesis")
        counts, bi, bc, _ = ctx.ransac_score(xi, xj, T.idx8[:h], R.THR)
        assert np.array_equal(counts, res["counts"]) and (bi, bc) == (res["best_iter"], res["best_count"]), what
    if n <= 9:
        assert R.repeated(T.idx8).sum() > 0.9 * R.ITERS


# ---- 2. every scene class -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CLASSES)
def test_every_scene_class(ctx, name, monkeypatch):
    s, T = R.scene(name), R.tables(name)
    cref = R.ref_counts(name, R.N0, s.thr)
    res = scored(ctx, name)
    got = R.check_contract(res, T.E, cref, name, T.idx8, nan_equal=name == "nan")
    ex = res["flags"].astype(bool)
    assert ex[R.repeated(T.idx8)].all(), name
    monkeypatch.setenv("SFMX_RANSAC_HYP", "legacy")
    leg = ctx.ransac_score_ex(s.xi, s.xj, T.idx8, s.thr)
    for k in R.KEYS6:
        H.assert_bits_equal(np.ascontiguousarray(leg[k], np.float64), np.ascontiguousarray(res[k], np.float64), f"{name}: legacy vs lean {k}", nan_equal=name == "nan")
    assert (leg["best_iter"], leg["best_count"]) == (res["best_iter"], res["best_count"])
    # populations that keep the case from passing vacuously
    if name == "edge":
        assert ex[T.win] or res["lo"][T.win] < res["hi"][T.win], "the winner's planted points must fall inside its band"
        assert ((res["lo"] < res["hi"]) & ~ex).sum() >= 1
    if name == "rot4":
        assert (~ex & (res["cond"] < 1e-8)).sum() >= 10
    if name in ("dup", "planar0", "rot0"):
        assert got.n_exact_clean >= 10, got
    if name == "dup":
        twin = np.array([len(set((o % (s.n // 2)).tolist())) < 8 for o in T.idx8])
        assert ex[twin].all(), "octets that hold a point and its copy reach the host through the conditioning estimate"
    if name == "nan":
        a, b = s.special
        assert ex[(T.idx8 == a).any(axis=1)].all(), "octets that drew the NaN point"
        for h in (T.win, 0, R.ITERS - 1):
            mask, _ = ctx.sampson_mask(s.xi, s.xj, res["E"][h], s.thr)
            assert mask[a] == 0 and mask[b] == 0
        assert (res["hi"] <= s.n - 2).all()   # no iteration counts a NaN point, drawn or not


# ---- 3. thresholds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general", "edge"])
def test_thresholds(ctx, name):
    s, T = R.scene(name), R.tables(name)
    for thr in THRESHOLDS:
        what = f"{name} thr={thr:g}"
        res = ctx.ransac_score_ex(s.xi, s.xj, T.idx8, thr)
        R.check_contract(res, T.E, R.ref_counts(name, R.N0, thr), what, T.idx8)
        if thr <= 0:
            assert not res["counts"].any() and not res["lo"].any() and not res["hi"].any(), what
            assert (res["best_iter"], res["best_count"]) == (0, 0), what
        if thr == 1e9:
            assert (res["lo"] == s.n).all() and (res["hi"] == s.n).all() and (res["counts"] == s.n).all(), what


# ---- 4. the packed 20-bit counters at their limit -------------------------------------------------------------------------------
def test_counter_limit(ctx):
    rng = np.random.default_rng(4)
    xi, xj = rng.uniform(-0.45, 0.45, (N_MAX + 1, 2)), rng.uniform(-0.45, 0.45, (N_MAX + 1, 2))
    idx8 = R.draws(N_MAX, 8)
    E = R.hypotheses(xi[:N_MAX], xj[:N_MAX], idx8)
    for thr, want in ((1e9, N_MAX), (0.0, 0)):
        res = ctx.ransac_score_ex(xi[:N_MAX], xj[:N_MAX], idx8, thr)
        R.check_contract(res, E, R.counts(xi[:N_MAX], xj[:N_MAX], E, thr), f"n = 2^20 - 1, thr={thr:g}", idx8)
        for k in ("counts", "lo", "hi"):
            assert (res[k] == want).all(), (thr, k, res[k])
    with pytest.raises(capi.SfmxError):
        ctx.ransac_score_ex(xi, xj, idx8, 1e-3)


# ---- 5. k_sampson_mask ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.N_SIZES)
def test_sampson_mask_sizes(ctx, n):
    xi, xj = R.points("general", n)
    T = R.tables("general", n)
    assert T.win != T.runner_up
    for h in (T.win, T.runner_up):
        exp = R.sampson_all(T.E[h], xi, xj) < R.THR
        mask, cnt = ctx.sampson_mask(xi, xj, T.E[h], R.THR)
        assert np.array_equal(mask.astype(bool), exp) and cnt == exp.sum(), (n, h)


def test_sampson_mask_edge_points_and_resident_path(ctx):
    s, T = R.scene("edge"), R.tables("edge")
    for h in (T.win, T.runner_up):
        exp = R.sampson_all(T.E[h], s.xi, s.xj) < s.thr
        mask, cnt = ctx.sampson_mask(s.xi, s.xj, T.E[h], s.thr)
        assert np.array_equal(mask.astype(bool), exp) and cnt == exp.sum() == R.ref_counts("edge", R.N0, s.thr)[h], h
    # resident path: the points of the preceding score call
    g, Tg = R.scene("general"), R.tables("general")
    ctx.ransac_score(g.xi, g.xj, Tg.idx8[:9], g.thr)
    exp = R.sampson_all(Tg.E[Tg.win], g.xi, g.xj) < g.thr
    mask, cnt = resident_mask(ctx, g.n, Tg.E[Tg.win], g.thr)
    assert np.array_equal(mask.astype(bool), exp) and cnt == exp.sum()
    for n in (g.n - 1, g.n + 1):
        with pytest.raises(capi.SfmxError):
            resident_mask(ctx, n, Tg.E[Tg.win], g.thr)
    mask, cnt = resident_mask(ctx, g.n, Tg.E[0], g.thr)   # the rejected calls left the resident set alone
    assert np.array_equal(mask.astype(bool), R.sampson_all(Tg.E[0], g.xi, g.xj) < g.thr)


# ---- 6. argument rejection without a launch -------------------------------------------------------------------------------------
def test_argument_rejection(ctx):
    s, T = R.scene("general"), R.tables("general")
    bad_hi, bad_lo = T.idx8[:17].copy(), T.idx8[:17].copy()
    bad_hi[16, 7], bad_lo[3, 0] = s.n, -1
    for xi, xj, idx8 in ((s.xi[:7], s.xj[:7], np.zeros((4, 8), np.int32)), (s.xi, s.xj, T.idx8[:0]), (s.xi, s.xj, bad_hi), (s.xi, s.xj, bad_lo)):
        with pytest.raises(capi.SfmxError):
            ctx.ransac_score_ex(xi, xj, idx8, s.thr)
        res = ctx.ransac_score_ex(s.xi, s.xj, T.idx8[:17], s.thr)
        R.check_contract(res, T.E[:17], R.ref_counts("general", R.N0, s.thr)[:17], "after a rejected call", T.idx8[:17])


# ---- 7. the seam ----------------------------------------------------------------------------------------------------------------
def _same_pose(got, exp, what):
    assert got["ok"] == exp["ok"] == 1 and got["best_iter"] == exp["best_iter"], (what, got["ok"], got.get("best_iter"), exp["best_iter"])
    assert np.array_equal(got["inliers"], exp["inliers"]), what
    H.assert_bits_equal(got["R"], exp["R"], f"{what}: R")
    H.assert_bits_equal(got["t"], exp["t"], f"{what}: t")


@pytest.mark.parametrize("name", R.CLASSES)
def test_seam_on_every_class_and_world(ctx, name):
    """find_E_ransac and find_E_ransac_world (ranks 0, world - 1 and the one that holds the winner; world 403 > iters leaves ranks
    with an empty range) against orc_find_E_ransac: ok, winner, inliers, R and t bit for bit"""
    s, T = R.scene(name), R.tables(name)
    exp = H.find_E_ransac(H.oracle(), "orc", R.K_ID, s.xi, s.xj, R.ITERS, s.thr, R.MIN_INLIERS)
    assert exp["ok"] == 1 and exp["best_iter"] == T.win
    _same_pose(pipe.find_E_ransac(ctx, R.K_ID, s.xi, s.xj, R.ITERS, s.thr, R.MIN_INLIERS), exp, name)
    for world in WORLDS:
        for as_rank in sorted({0, world - 1, R.rank_of(T.win, R.ITERS, world)}):
            got = pipe.find_E_ransac_world(ctx, R.K_ID, s.xi, s.xj, R.ITERS, s.thr, R.MIN_INLIERS, world, as_rank)
            _same_pose(got, exp, f"{name} world={world} rank={as_rank}")
    over = len(exp["inliers"]) + 1   # one more than the winner has: no pose (T:678)
    assert pipe.find_E_ransac(ctx, R.K_ID, s.xi, s.xj, R.ITERS, s.thr, over)["ok"] == 0
    assert pipe.find_E_ransac_world(ctx, R.K_ID, s.xi, s.xj, R.ITERS, s.thr, over, 3, 1)["ok"] == 0
    assert pipe.find_E_ransac(ctx, R.K_ID, s.xi, s.xj, R.ITERS, s.thr, over - 1)["ok"] == 1


# ---- 8. the redo round, in fresh processes --------------------------------------------------------------------------------------
_child_fault = []


def _run_child(min_cond, tmp_path):
    if _child_fault:
        pytest.fail(f"nothing more is started on the device after a fault ({_child_fault[0]})")
    out = str(tmp_path / "ransac.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("SFMX_")}
    env.update({"SFMX_RANSAC_MIN_COND": min_cond, "SFMX_NO_TORCH_PRELOAD": "1"})
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ransac_child.py")
    try:
        p = subprocess.run([sys.executable, child, "run", out], env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        _child_fault.append(f"MIN_COND={min_cond}: timeout")
        raise
    if p.returncode < 0 or p.returncode in (124, 134, 139):
        _child_fault.append(f"MIN_COND={min_cond}: exit status {p.returncode}")
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(out)


def test_redo_round_every_row_exact(tmp_path):
    """SFMX_RANSAC_MIN_COND=1e300: every hypothesis goes through upload_exact -> k_patch_E -> the compact k_score, so E is the
    oracle's bit for bit and counts = lo = hi = the oracle's on all rows: k_score's arithmetic and reduction at n = 600 (three
    trips of the stride loop), independent of any hypothesis uncertainty"""
    z = _run_child("1e300", tmp_path)
    for i, (name, h) in enumerate(C.CHILD_CASES):
        s, T = R.scene(name), R.tables(name)
        res = C.load(z, i)
        cref = R.ref_counts(name, R.N0, s.thr)[:h]
        what = f"MIN_COND=1e300 {name} H={h}"
        assert res["flags"].all(), what
        H.assert_bits_equal(res["E"], T.E[:h], what)
        for k in ("counts", "lo", "hi"):
            assert np.array_equal(res[k], cref), (what, k)
        R.check_contract(res, T.E[:h], cref, what, T.idx8[:h], min_cond=1e300)


def test_redo_round_mixed_batch(ctx, tmp_path):
    """SFMX_RANSAC_MIN_COND = the median conditioning estimate of rot4's device rows: about half of the rows are patched, in a
    compact batch whose size is no multiple of 8"""
    base = scored(ctx, "rot4")
    dev = ~base["flags"].astype(bool)
    med = float(np.median(base["cond"][dev]))
    z = _run_child(repr(med), tmp_path)
    batch = []
    for i, (name, h) in enumerate(C.CHILD_CASES):
        s, T = R.scene(name), R.tables(name)
        res = C.load(z, i)
        what = f"MIN_COND={med!r} {name} H={h}"
        got = R.check_contract(res, T.E[:h], R.ref_counts(name, R.N0, s.thr)[:h], what, T.idx8[:h], min_cond=med)
        batch.append(got.n_exact_clean)   # size of the compact second-round batch
        if name == "rot4" and h == R.ITERS:
            ex = res["flags"].astype(bool)
            assert np.array_equal(ex, ~dev | (base["cond"] < med)), "exactly the rows below the floor are redone"
            assert 0.3 * R.ITERS < got.n_exact_clean < 0.7 * R.ITERS, got
            # the rows that stayed on the device are untouched by the patching around them
            H.assert_bits_equal(res["E"][~ex], base["E"][~ex], what)
            for k in ("counts", "lo", "hi"):
                assert np.array_equal(res[k][~ex], base[k][~ex]), (what, k)
    # some compact batch spans several workgroups of 8 AND ends in a ragged one (the same m), and some is smaller than one workgroup
    assert any(m > 8 and m % 8 for m in batch) and any(0 < m < 8 for m in batch), batch
