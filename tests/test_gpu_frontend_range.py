"""The tracking front end over its whole range: both KLT kernels of csrc/hip/klt.hip in every variant (one track per wavefront with the
ordered sums on the matrix core or the VALU, pipelined or not; K = 1, 2, 4 tracks per wavefront) for every radius, on interleaved
populations that put NaN, border, outside and interior tracks into one wavefront, on pyramids smaller than the staged window, with
every level count, ragged track counts and the extremes of iters and fb_thresh; the pyramid, score, compaction and corner-fixpoint
kernels of csrc/hip/image.hip on ragged and tiny sizes, tie-heavy score maps, every schedule, min_dist and cap.
Every comparison is bit for bit against the CPU oracle; there is no tolerance anywhere.  The step count and the off-grid step count
of a KLT call equal the totals of the Python restatement of track_point (tests/frontend_inputs.py), which tests/
test_frontend_inputs_cpu.py proves equal to orc_klt_track, and which the same file proves to reach every branch."""
import importlib
import os
import subprocess
import sys
from ctypes import POINTER, byref, c_double, c_int, c_uint32

import numpy as np
import pytest

import frontend_child as C
import frontend_inputs as F
import helpers as H

pytestmark = pytest.mark.gpu

capi = importlib.import_module(H.PKG_NAME + ".capi")
O = H.oracle()

SWITCHES = ("SFMX_KLT_K", "SFMX_KLT_SUMS", "SFMX_KLT_PIPE", "SFMX_KLT_WAVE_PRIO", "SFMX_KLT_LDS_PAD", "SFMX_KLT_STAMPS", "SFMX_KLT_K2_MIN",
            "SFMX_SHI_MODE", "SFMX_SHI_SWEEPS", "SFMX_SHI_INNER")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("SFMX_KLT_") or k.startswith("SFMX_SHI_"):
            monkeypatch.delenv(k, raising=False)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _setenv(monkeypatch, env):
    for k in ("SFMX_KLT_K", "SFMX_KLT_SUMS", "SFMX_KLT_PIPE", "SFMX_SHI_MODE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


_pyr: dict = {}


@pytest.fixture(scope="module")
def pyramids(ctx):
    """(pair name, levels) -> the two device pyramids, built once"""
    def get(name, levels):
        if (name, levels) not in _pyr:
            p = F.pair(name)
            _pyr[(name, levels)] = (ctx.pyramid(p.a, levels), ctx.pyramid(p.b, levels))
        return _pyr[(name, levels)]
    yield get
    for pa, pb in _pyr.values():
        pa.close()
        pb.close()
    _pyr.clear()


# ---- KLT ------------------------------------------------------------------------------------------------------------------------
ONE_TRACK = [(f"one-{sums}-pipe{pipe}", {"SFMX_KLT_SUMS": sums, "SFMX_KLT_PIPE": pipe}) for sums in ("mfma", "valu") for pipe in ("0", "1")]
MULTI = [(f"multi-K{k}", {"SFMX_KLT_K": k}) for k in (1, 2, 4)]
SHORT = [("default", {}), ("multi-K2", {"SFMX_KLT_K": 2}), ("multi-K4", {"SFMX_KLT_K": 4})]


VARIANTS = [("default", {})] + ONE_TRACK + MULTI   # at radius 7 a request for the multi-track kernel takes the one-track kernel


def _bits_or_nan(got, exp, what):
    """bit for bit; where the oracle's value is NaN the device's must be a NaN (x86 and gfx950 generate different NaN bits)"""
    got, exp = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(exp, np.float64)
    assert got.shape == exp.shape, what
    nan = np.isnan(exp)
    assert np.isnan(got[nan]).all(), f"{what}: the oracle has NaN where the device has a number"
    ne = (got.view(np.uint64) != exp.view(np.uint64)) & ~nan
    if ne.any():
        i = np.argwhere(ne)[0]
        raise AssertionError(f"{what}: {int(ne.sum())}/{ne.size} values differ bitwise; first at {i.tolist()} got={got[tuple(i)]!r} expected={exp[tuple(i)]!r}")


def _klt_check(ctx, pyr, xy, levels, r, iters, fb, expected, stats, what):
    efwd, eback, ekeep = expected
    fwd, back, keep, steps = ctx.klt_track(pyr[0], pyr[1], xy, levels, r, iters, fb)
    slow = ctx.klt_slow_steps()
    _bits_or_nan(fwd, efwd, f"{what}: fwd")
    _bits_or_nan(back, eback, f"{what}: back")
    assert np.array_equal(keep, ekeep), (what, "keep", np.flatnonzero(keep != ekeep)[:8].tolist())
    esteps, eslow = sum(s.steps for s in stats), sum(s.slow for s in stats)
    assert steps == esteps, (what, "steps", steps, esteps)
    assert slow == eslow, (what, "off-grid steps", slow, eslow)
    return fwd, back, keep, slow


@pytest.mark.parametrize("r", range(1, F.KLT_MAX_R + 1))
@pytest.mark.parametrize("name", list(F.PAIRS))
def test_klt_every_variant(ctx, pyramids, name, r, monkeypatch):
    """fwd, back and keep equal orc_klt_track; the step count and the off-grid step count equal the restatement's"""
    p = F.pair(name)
    xy, labels = F.pair_population(name, r)
    expected = F.oracle_tracks(name, r, iters=F.VARIANT_ITERS)
    stats = F.restated(name, r, iters=F.VARIANT_ITERS)[3]
    assert np.isnan(expected[1]).any() and 0 < expected[2].sum() < len(xy)
    pyr = pyramids(name, p.levels)
    results = {}
    for vname, env in VARIANTS:
        _setenv(monkeypatch, env)
        got = _klt_check(ctx, pyr, xy, p.levels, r, F.VARIANT_ITERS, 1.0, expected, stats, f"{name} r={r} {vname}")
        assert got[3] > 0, (vname, "no off-grid step")
        results[vname] = got
    if r == 5:  # follows from the above; stated directly
        ref = results["default"]
        for vname, got in results.items():
            for k, what in enumerate(("fwd", "back")):
                H.assert_bits_equal(got[k], ref[k], f"{name} r=5 {vname} against default: {what}", nan_equal=True)
            assert np.array_equal(got[2], ref[2]) and got[3] == ref[3], vname


@pytest.mark.parametrize("r", [2, 5, 6])
@pytest.mark.parametrize("K", [2, 4])
def test_klt_ragged_track_counts(ctx, pyramids, K, r, monkeypatch):
    """the last wave of the multi-track kernel with n % K != 0, after a large call that has filled the pinned result slab"""
    name = "small"
    p = F.pair(name)
    xy, _ = F.pair_population(name, r)
    efwd, eback, ekeep = F.oracle_tracks(name, r, iters=F.VARIANT_ITERS)
    stats = F.restated(name, r, iters=F.VARIANT_ITERS)[3]
    pyr = pyramids(name, p.levels)
    _setenv(monkeypatch, {"SFMX_KLT_K": K})
    for n in F.RAGGED_N:
        _klt_check(ctx, pyr, xy, p.levels, r, F.VARIANT_ITERS, 1.0, (efwd, eback, ekeep), stats, f"K={K} r={r} n={len(xy)}")
        _klt_check(ctx, pyr, np.ascontiguousarray(xy[:n]), p.levels, r, F.VARIANT_ITERS, 1.0, (efwd[:n], eback[:n], ekeep[:n]), stats[:n],
                   f"K={K} r={r} n={n}")


@pytest.mark.parametrize("name", list(F.PAIRS))
def test_klt_every_level_count(ctx, pyramids, name, monkeypatch):
    """levels from 1 to the most the pair allows (8 for the VGA pair, 6 for the small one, whose levels from 2 on are smaller than
    the staged window), plus the level of 1 x 1 pixel that orc_klt_track defines"""
    p = F.pair(name)
    counts = list(range(1, p.max_levels + 1)) + ([F.BELOW_2X2[1]] if name == F.BELOW_2X2[0] else [])
    for levels in counts:
        xy, _ = F.pair_population(name, 5, levels)
        expected = F.oracle_tracks(name, 5, levels, 4)
        stats = F.restated(name, 5, levels, 4)[3]
        pyr = pyramids(name, levels)
        for vname, env in SHORT:
            _setenv(monkeypatch, env)
            _klt_check(ctx, pyr, xy, levels, 5, 4, 1.0, expected, stats, f"{name} levels={levels} {vname}")


def test_klt_coarser_levels_of_a_deeper_pyramid(ctx, pyramids):
    """fewer levels than the pyramid holds use its first levels; more levels than it holds is an error, as radius 8 is"""
    xy, _ = F.pair_population("small", 5, 3)
    deep = pyramids("small", 6)
    _klt_check(ctx, deep, xy, 3, 5, F.VARIANT_ITERS, 1.0, F.oracle_tracks("small", 5, 3, F.VARIANT_ITERS), F.restated("small", 5, 3, F.VARIANT_ITERS)[3],
               "3 levels of a 6-level pyramid")
    pyr = pyramids("small", 3)
    for levels, r in ((4, 5), (9, 5), (0, 5), (3, 8), (3, 0)):
        with pytest.raises(capi.SfmxError):
            ctx.klt_track(pyr[0], pyr[1], xy[:8], levels, r, 3, 1.0)
    with pytest.raises(capi.SfmxError):
        ctx.klt_track(pyr[0], pyr[1], xy[:8], 3, 5, -1, 1.0)


@pytest.mark.parametrize("vname,env", SHORT + [("one-valu-pipe1", {"SFMX_KLT_SUMS": "valu", "SFMX_KLT_PIPE": "1"})])
def test_klt_parameters(ctx, pyramids, vname, env, monkeypatch):
    name, r, levels = "small", 5, 3
    xy, _ = F.pair_population(name, r, levels)
    pyr = pyramids(name, levels)
    _setenv(monkeypatch, env)
    # iters = 0: nothing moves, keep from hypot(0, 0) against fb
    for fb in (1.0, 0.0):
        fwd, back, keep, steps = ctx.klt_track(pyr[0], pyr[1], xy, levels, r, 0, fb)
        _bits_or_nan(fwd, xy, "iters = 0: fwd")
        _bits_or_nan(back, xy, "iters = 0: back")
        assert steps == 0 and ctx.klt_slow_steps() == 0
        assert np.array_equal(keep, F.oracle_tracks(name, r, levels, 0, fb)[2]), fb
    # fb_thresh: 0 keeps only NaN, inf and NaN keep everything, the smallest denormal and 1e-3 sit on the comparison's edge
    stats = F.restated(name, r, levels, F.VARIANT_ITERS)[3]
    e = F.fb_edge(name, r, levels, F.VARIANT_ITERS)[1]
    for fb in F.FB + (e, float(np.nextafter(e, 2.0))):
        _klt_check(ctx, pyr, xy, levels, r, F.VARIANT_ITERS, fb, F.oracle_tracks(name, r, levels, F.VARIANT_ITERS, fb), stats, f"{vname} fb={fb}")
    # xy_back = NULL
    efwd, _, ekeep = F.oracle_tracks(name, r, levels, F.VARIANT_ITERS)
    fwd, back, keep, steps = ctx.klt_track(pyr[0], pyr[1], xy, levels, r, F.VARIANT_ITERS, 1.0, want_back=False)
    assert back is None and steps == sum(s.steps for s in stats)
    _bits_or_nan(fwd, efwd, f"{vname} without xy_back: fwd")
    assert np.array_equal(keep, ekeep)


# ---- pyramid and score ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", F.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_all_levels(ctx, size):
    w, h = size
    img = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)
    pyr = ctx.pyramid(img, F.MAX_LEVELS)
    cur = img
    assert np.array_equal(pyr.level(0), img)
    for l in range(1, F.MAX_LEVELS):
        if min(cur.shape) < 2:
            break
        cur = H.downsample2(O, "orc", cur)
        got = pyr.level(l)
        assert got.shape == cur.shape and np.array_equal(got, cur), (size, l)
    pyr.close()
    with pytest.raises(capi.SfmxError):
        ctx.pyramid(img, F.MAX_LEVELS + 1)


@pytest.mark.parametrize("size", F.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_score_and_candidates(ctx, size):
    """score map and maximum against orc_shi_score (an empty interior band gives a zero map); the ordered compaction against
    np.nonzero(score >= max * quality) for quality 0 (every pixel), 0.01, 1 (the maxima) and 1.5 (nothing, unless the map is zero);
    with a cap, n_out is still the total and exactly min(n, cap) entries are written"""
    w, h = size
    for kind in F.SCORE_KINDS:
        img = F.score_image(kind, w, h)
        pyr = ctx.pyramid(img, 1)
        exp = F.oracle_score(img)
        score, mx = ctx.shi_score(pyr)
        H.assert_bits_equal(score, exp, f"{kind} {size}: score map")
        assert mx == exp.max()
        if min(w, h) < 5 or kind == "constant":
            assert mx == 0.0
        for quality in F.QUALITY:
            yy, xx = np.nonzero(exp >= exp.max() * quality)
            n = len(xx)
            assert n == (w * h if quality == 0.0 or mx == 0.0 else n) and (n >= 1 or quality > 1.0)
            caps = [None] + (sorted({c for c in (1, n - 1, n, n + 1) if c >= 1}) if quality in (0.0, 0.01) or n < 64 else [])
            for cap in caps:
                what = f"{kind} {size} quality={quality} cap={cap}"
                ccap = cap or w * h
                axy = np.full(ccap + C.PAD, C.XY_FILL, np.uint32)
                asc = np.full(ccap + C.PAD, np.nan)
                cn, cmx = c_int(), c_double()
                ctx._chk(ctx.lib.sfmx_shi_tomasi_candidates(ctx.h_, pyr.h_, c_double(quality), c_int(ccap), axy.ctypes.data_as(POINTER(c_uint32)),
                                                            asc.ctypes.data_as(POINTER(c_double)), byref(cn), byref(cmx)))
                assert cn.value == n and cmx.value == exp.max(), (what, cn.value, n)
                m = min(n, ccap)
                assert np.array_equal(axy[:m] & 0xFFFF, xx[:m]) and np.array_equal(axy[:m] >> 16, yy[:m]), what
                H.assert_bits_equal(asc[:m], exp[yy[:m], xx[:m]], f"{what}: scores")
                assert (axy[m:] == C.XY_FILL).all() and np.isnan(asc[m:]).all(), (what, "written past min(n, cap)")
        pyr.close()


# ---- the corner fixpoint ----------------------------------------------------------------------------------------------------------
def _pruned_kinds(size):
    """every kind up to 129 x 65; above that the kinds whose pick the oracle's quadratic walk finishes in about a second"""
    return F.SCORE_KINDS if size[0] * size[1] <= 129 * 65 else ("noisy", "quant4", "checker", "lattice")


@pytest.mark.parametrize("mode", F.SHI_MODES, ids=lambda m: m or "default")
@pytest.mark.parametrize("size", F.PRUNED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pruned_candidates(ctx, size, mode, monkeypatch):
    """the contract of sfmx_shi_tomasi_candidates_pruned (include/sfmx.h) against orc_shi_tomasi without a cap on the corners"""
    w, h = size
    _setenv(monkeypatch, {"SFMX_SHI_MODE": mode} if mode else {})
    for kind in _pruned_kinds(size):
        img = F.score_image(kind, w, h)
        pyr = ctx.pyramid(img, 1)
        for md in F.MIN_DIST:
            res = C.pruned_raw(ctx, pyr, 0.01, md)
            C.check_pruned(res, (kind, size), img, 0.01, md, w * h, f"{kind} {size} min_dist={md} mode={mode}")
        pyr.close()


def test_pruned_survivor_counts_lie_on_both_sides_of_the_speculative_download(ctx):
    img = F.score_image("noisy", 333, 251)
    pyr = ctx.pyramid(img, 1)
    above, below = C.pruned_raw(ctx, pyr, 0.01, 2), C.pruned_raw(ctx, pyr, 0.01, 8)
    assert above.n > F.SHI_SPEC >= below.n > 0, (above.n, below.n)
    # a cap on either side of the speculative download, and of the survivor count: n_out stays, the first cap survivors are written
    for full, md in ((above, 2), (below, 8)):
        for cap in (1, F.SHI_SPEC - 1, F.SHI_SPEC, F.SHI_SPEC + 1, full.n - 1, full.n, full.n + 1):
            res = C.pruned_raw(ctx, pyr, 0.01, md, cap)
            what = f"min_dist={md} cap={cap}"
            C.check_pruned(res, ("noisy", (333, 251)), img, 0.01, md, cap, what)
            m = min(full.n, cap)
            assert res.n == full.n and res.ntot == full.ntot, what
            assert np.array_equal(res.xy[:m], full.xy[:m]) and np.array_equal(res.full[:m], full.full[:m]), what
    pyr.close()


def test_pruned_parameter_limits(ctx):
    pyr = ctx.pyramid(F.score_image("noisy", 65, 33), 1)
    for md in (0, 17, -1):
        with pytest.raises(capi.SfmxError):
            C.pruned_raw(ctx, pyr, 0.01, md)
    C.check_pruned(C.pruned_raw(ctx, pyr, 0.01, 16), ("noisy", (65, 33)), F.score_image("noisy", 65, 33), 0.01, 16, 65 * 33, "after the errors")
    pyr.close()


_child_fault = []


@pytest.mark.parametrize("sweeps", C.CHILD_SWEEPS)
def test_pruned_candidates_sweep_schedules(sweeps, tmp_path):
    """SFMX_SHI_SWEEPS is read once per process: each schedule of the sweep kernels (dense only, dense + work list + tail) in a
    process of its own.  Any schedule is exact: what it leaves undecided travels unflagged."""
    if _child_fault:
        pytest.fail(f"nothing more is started on the device after a fault ({_child_fault[0]})")
    out = str(tmp_path / "pruned.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("SFMX_")}
    env.update({"SFMX_SHI_MODE": "sweeps", "SFMX_SHI_SWEEPS": sweeps, "SFMX_NO_TORCH_PRELOAD": "1"})
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "frontend_child.py")
    try:
        p = subprocess.run([sys.executable, child, out], env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        _child_fault.append(f"{sweeps}: timeout")
        raise
    if p.returncode < 0 or p.returncode in (134, 139):
        _child_fault.append(f"{sweeps}: exit status {p.returncode}")
    assert p.returncode == 0, p.stdout[-3000:]
    z = np.load(out)
    for i, (kind, (w, h), md) in enumerate(C.CHILD_CASES):
        res = C.Pruned(z[f"{i}:xy"], z[f"{i}:sc"], z[f"{i}:full"], int(z[f"{i}:n"][0]), int(z[f"{i}:n"][1]), float(z[f"{i}:mx"]))
        C.check_pruned(res, (kind, (w, h)), F.score_image(kind, w, h), 0.01, md, w * h, f"sweeps={sweeps} {kind} {w}x{h} min_dist={md}")


# ---- the corner pick through the tracker seam -----------------------------------------------------------------------------------
@pytest.mark.parametrize("min_distance", [2, 16])
@pytest.mark.parametrize("kind", ["noisy", "quant4", "checker", "lattice"])
@pytest.mark.parametrize("size", F.TRACKER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_corner_pick_on_ragged_sizes_and_tied_scores(ctx, size, kind, min_distance):
    """reset (frame 0) and one tracked frame with replenishment (frame 1, the image moved by one pixel), tracks bit-equal to the
    oracle's Tracker: the host resolver finishes what the fixpoint leaves undecided in libstdc++'s tie order (T:286-300)"""
    pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
    w, h = size
    img = F.score_image(kind, w + 1, h)
    frames = [np.ascontiguousarray(img[:, :w]), np.ascontiguousarray(img[:, 1:])]
    kw = dict(max_tracks=4000, min_tracks=3900, quality=0.01, min_distance=min_distance, levels=3, radius=5, iters=10, fb=1.0)
    Tg = pipe.Tracker(ctx, w, h, **kw)
    To = H.Tracker(O, "orc", **kw)
    try:
        for f in range(2):
            gp, gc, gi = Tg.step(frames[f])
            op, oc, oi = To.step(frames[f])
            assert np.array_equal(gi, oi), (size, kind, min_distance, f)
            H.assert_bits_equal(gp, op, f"prev {f}")
            H.assert_bits_equal(gc, oc, f"cur {f}")
            gxy, gid = Tg.tracks()
            oxy, oid = To.tracks()
            assert np.array_equal(gid, oid), (size, kind, min_distance, f)
            H.assert_bits_equal(gxy, oxy, f"tracks {kind} {size} min_distance={min_distance} frame {f}")
        assert len(gid) > 0
    finally:
        Tg.close()
        To.close()
