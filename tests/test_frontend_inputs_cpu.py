"""Conditions on the inputs of the front-end range suite (tests/frontend_inputs.py), checked on the CPU oracle: the Python restatement
of track_point IS orc_klt_track (so its step, off-grid and staging counts can be trusted), every class of track is there, every
off-grid branch of the sample grid is taken on both axes, windows are re-staged, levels are left early and exhausted, the tracks of
a wave differ, the tie-heavy score maps really hold ties and the survivor counts lie on both sides of the speculative download.
These are conditions, not measurements: if one fails, the generator or the seed changes, never the threshold.
No device, no binding of the device library.  Run with -s to see the counts."""
import numpy as np
import pytest

import frontend_inputs as F
import helpers as H

RADII = tuple(range(1, F.KLT_MAX_R + 1))
CELLS = [pytest.param(name, r, id=f"{name}-r{r}") for name in F.PAIRS for r in RADII]


def _same_as_oracle(name, r, levels, iters, fb=1.0):
    fwd, back, keep, stats = F.restated(name, r, levels, iters, fb)
    ofwd, oback, okeep = F.oracle_tracks(name, r, levels, iters, fb)
    H.assert_bits_equal(fwd, ofwd, f"{name} r={r} levels={levels} iters={iters}: fwd")
    H.assert_bits_equal(back, oback, f"{name} r={r} levels={levels} iters={iters}: back")
    assert np.array_equal(keep, okeep), (name, r, levels, iters, fb)
    return fwd, back, keep, stats


@pytest.mark.parametrize("name,r", CELLS)
def test_restatement_is_the_oracle_and_every_branch_is_taken(name, r):
    p = F.pair(name)
    xy, labels = F.pair_population(name, r)
    fwd, back, keep, stats = _same_as_oracle(name, r, p.levels, F.VARIANT_ITERS)
    # classes
    classes = ["interior", "dup", "nonfinite", "outside", "border", "pow2"] + [f"{s}{l}" for s in ("left", "top") for l in range(p.levels)]
    counts = {c: int((labels == c).sum()) for c in classes}
    assert set(labels) == set(classes) and min(counts.values()) >= 8, counts
    nf = xy[labels == "nonfinite"]
    assert np.isnan(nf).any() and np.isposinf(nf).any() and np.isneginf(nf).any() and (nf == 1e12).any()
    assert (np.isnan(nf[:, 0]) & ~np.isnan(nf[:, 1])).any() and (~np.isnan(nf[:, 0]) & np.isnan(nf[:, 1])).any() and np.isnan(nf).all(1).any()
    for i in np.flatnonzero(labels == "dup"):
        assert (H.bits(xy[:i]) == H.bits(xy[i])).all(1).any(), i
    for l in range(p.levels):
        for s, ax in (("left", 0), ("top", 1)):
            v = xy[labels == f"{s}{l}", ax] / (1 << l)
            assert ((v > -(r + 3.001)) & (v < 4.001)).all(), (s, l)
    assert np.isnan(back).any()  # the GPU cases compare NaN with NaN: it must be there
    # off-grid steps of every kind on both axes (radius 1 has no slot with two inner neighbours apart from d = 0, whose coordinate
    # is v itself, exact: the both-on-one-slot kind cannot occur there)
    kinds = np.array([s.kinds for s in stats]).sum(0)
    slow = sum(s.slow for s in stats)
    for k, what in enumerate(("x plus", "x minus", "x both", "y plus", "y minus", "y both")):
        if r == 1 and k % 3 == 2:
            assert kinds[k] == 0, what
        else:
            assert kinds[k] >= 8, (what, kinds.tolist())
    assert 0 < slow <= sum(s.steps for s in stats)
    # levels left early and exhausted; both values of keep
    early, exhausted = sum(s.early > 0 for s in stats), sum(s.exhausted > 0 for s in stats)
    assert early >= 8 and exhausted >= 8, (early, exhausted)
    assert 8 <= int(keep.sum()) <= len(keep) - 8
    # the tracks of one wave: groups of four consecutive tracks
    cs = np.array([s.coarse_steps for s in stats]).reshape(-1, 4)
    uneven = float((cs.max(1) != cs.min(1)).mean())
    lab4 = labels.reshape(-1, 4)
    mixed = float((np.isin(lab4, ("nonfinite", "outside")).any(1) & (lab4 == "interior").any(1)).mean())
    assert uneven >= 0.5 and mixed >= 0.25, (uneven, mixed)
    restaged = sum(s.max_stagings > 1 for s in stats)
    if name == "flow":
        assert restaged >= 8
    print(f"\n{name} r={r}: classes {counts}; steps {sum(s.steps for s in stats)}, off-grid {slow}, kinds x(+,-,both) y(+,-,both) {kinds.tolist()}; "
          f"restaged {restaged}, early {early}, exhausted {exhausted}, keep {int(keep.sum())}/{len(keep)}; groups uneven {uneven:.2f}, mixed {mixed:.2f}")


def test_off_grid_neighbours_where_they_are_expected():
    """interior coordinates (v >= 8) have an off-grid neighbour in the minus direction only; the plus direction and the both-on-one-slot
    case need a coordinate near the origin.  The shares are computed here, on the CPU, over full-mantissa coordinates."""
    for r in (1, 2, 5, 7):
        p, m, b = F.off_grid_shares(r, 8.0, 600.0, 4000)
        assert p == 0.0 and b == 0.0 and 0.002 < m < 0.2, (r, p, m, b)
    p, m, b = F.off_grid_shares(5, -1.0, 1.0, 4000)
    assert 0.85 < p < 0.97 and 0.85 < m < 0.97 and 0.05 < b < 0.2, (p, m, b)
    p, m, b = F.off_grid_shares(5, 0.0, 4.0, 4000)
    assert 0.3 < p < 0.42 and 0.68 < m < 0.78, (p, m, b)
    for v in (0.5, 0.25, 17.0, 100.125):   # exact binary fractions never round: what the hand-written edge points of the older tests were
        assert not np.any(F.off_grid(v, 5))


@pytest.mark.parametrize("name", list(F.PAIRS))
def test_restatement_is_the_oracle_at_every_level_count(name):
    p = F.pair(name)
    sizes = [(p.w >> l, p.h >> l) for l in range(p.max_levels)]
    assert min(sizes[-1]) >= 2 and (p.max_levels == F.MAX_LEVELS or min(p.w >> p.max_levels, p.h >> p.max_levels) < 2)
    for levels in range(1, p.max_levels + 1):
        _same_as_oracle(name, 5, levels, 4)
    if name == "small":
        assert max(sizes[2]) < F.KLT_P and p.max_levels >= 6
    if name == "strip":
        assert p.h < F.KLT_P <= sizes[-1][0]


def test_oracle_defines_a_level_below_2x2():
    name, levels = F.BELOW_2X2
    p = F.pair(name)
    assert (p.w >> (levels - 1), p.h >> (levels - 1)) == (1, 1)
    _same_as_oracle(name, 5, levels, 4)


def test_parameter_cases():
    kept = []
    for fb in F.FB:
        _, _, keep, _ = _same_as_oracle("small", 5, 3, F.VARIANT_ITERS, fb)
        kept.append(int(keep.sum()))
    # fb = 0 keeps only NaN, the smallest denormal also what did not move at all, inf and NaN keep everything
    assert 0 < kept[0] < kept[1] <= kept[2] < kept[3] < kept[4] == kept[5] == len(keep), kept
    print(f"\nkept at fb {F.FB}: {kept}")
    t, e = F.fb_edge("small", 5, 3, F.VARIANT_ITERS)   # the comparison's edge: fb >= thresh drops the track (T:362)
    assert _same_as_oracle("small", 5, 3, F.VARIANT_ITERS, e)[2][t] == 0
    assert _same_as_oracle("small", 5, 3, F.VARIANT_ITERS, float(np.nextafter(e, 2.0)))[2][t] == 1
    _, back0, keep0, _ = F.restated("small", 5, 3, F.VARIANT_ITERS, 0.0)
    with np.errstate(invalid="ignore"):
        nan = np.isnan(back0 - F.pair_population("small", 5, 3)[0]).any(1)   # NaN >= fb is false: such a track is kept at every fb (T:362)
    assert nan.any() and keep0[nan].all() and not keep0[~nan].any()
    assert F.restated("small", 5, 3, F.VARIANT_ITERS, float("nan"))[2].all()
    fwd, back, keep, stats = _same_as_oracle("small", 5, 3, 0)
    xy, _ = F.pair_population("small", 5, 3)
    H.assert_bits_equal(fwd, xy, "iters = 0: fwd is the input")
    H.assert_bits_equal(back, xy, "iters = 0: back is the input")
    assert sum(s.steps for s in stats) == 0


# ---- score maps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", F.TIE_HEAVY)
def test_tie_heavy_images_hold_ties(kind):
    for w, h in ((65, 33), (127, 95)):
        for md in (2, 8, 16):
            share = F.tie_share(F.score_image(kind, w, h), 0.01, md)
            print(f"\n{kind} {w}x{h} min_dist {md}: tie share {share:.2f}")
            assert share >= 0.2, (kind, w, h, md, share)
    assert F.tie_share(F.score_image("noisy", 127, 95), 0.01, 8) == 0.0


def test_constant_image_and_empty_band():
    for w, h in F.SMALL_SIZES:
        exp, yy, xx = F.oracle_candidates(F.score_image("constant", w, h), 0.01)
        assert exp.max() == 0.0 and len(yy) == w * h
    for w, h in F.SIZES:
        if min(w, h) < 5:
            assert F.oracle_score(F.score_image("noisy", w, h)).max() == 0.0


def test_survivor_counts_on_both_sides_of_the_speculative_download():
    img = F.score_image("noisy", 333, 251)
    above, below = len(F.oracle_pick(img, 0.01, 2)), len(F.oracle_pick(img, 0.01, 8))
    print(f"\nnoisy 333x251: {above} picks at min_dist 2, {below} at min_dist 8")
    assert above > F.SHI_SPEC > below > 0
