"""The inputs of the RANSAC range suite are what they claim (CPU, oracle only): the GPU cases of tests/test_gpu_ransac_range.py
rest on these populations.  The minima are caps far below what the generators give (in brackets), not measurements."""
import numpy as np
import pytest

import helpers as H
import ransac_inputs as R

O = H.oracle()


def _cond(name):
    s, T = R.scene(name), R.tables(name)
    return R.ref_cond(s.xi, s.xj, T.idx8), ~R.repeated(T.idx8)


def test_tables_are_the_streams_find_E_ransac_draws():
    assert R.N_SIZES == (8, 9, 255, 256, 257, 513, 1000, 4097) and R.H_SIZES == (1, 3, 4, 5, 8, 9, 17, 400)
    assert R.tables("general").idx8.shape == (R.ITERS, 8)
    rep = R.repeated(R.tables("general").idx8)
    assert 5 <= rep.sum() <= 40                       # sampling with replacement: 4.6 % expected at n = 600
    assert R.repeated(R.tables("general", 8).idx8).mean() > 0.9 and R.repeated(R.tables("general", 9).idx8).mean() > 0.9
    for n in R.N_SIZES:
        xi, xj = R.points("general", n)
        assert xi.shape == (n, 2) and xj.shape == (n, 2) and R.tables("general", n).idx8.max() < n


@pytest.mark.parametrize("name", ["planar0", "rot0"])
def test_noise_free_degenerate_scenes_are_rank_deficient(name):
    rc, clean = _cond(name)
    assert (rc[clean] < 1e-13).mean() >= 0.15, (rc[clean] < 1e-13).mean()    # (0.25: octets with at most one outlier)


def test_rotation_with_noise_fills_the_low_conditioning_band():
    rc, clean = _cond("rot4")
    assert ((rc[clean] >= 1e-13) & (rc[clean] < 1e-8)).mean() >= 0.10        # (0.26)


def test_general_scene_is_well_conditioned():
    rc, clean = _cond("general")
    assert ((rc[clean] >= 1e-13) & (rc[clean] < 1e-8)).mean() <= 0.01        # (0.003)


def test_duplicated_points_under_distinct_indices():
    s, T = R.scene("dup"), R.tables("dup")
    h = s.n // 2
    H.assert_bits_equal(s.xi[h:], s.xi[:h], "dup xi")
    H.assert_bits_equal(s.xj[h:], s.xj[:h], "dup xj")
    rc, clean = _cond("dup")
    twin = np.array([len(set((o % h).tolist())) < 8 for o in T.idx8]) & clean   # holds some i and i + 300, no repeated index
    assert twin.sum() >= 10, twin.sum()                                       # (16)
    assert (rc[twin] < 1e-13).all(), rc[twin].max()                           # (2e-16)


def test_noise_free_scene_ties_at_the_maximal_count():
    c = R.ref_counts("general0", R.N0, R.THR)
    assert (c == c.max()).sum() >= 5, (c.max(), (c == c.max()).sum())         # (29 all-inlier octets at 420)


def test_wide_and_pixel_coordinate_ranges():
    w, p = R.scene("wide"), R.scene("pixel")
    assert 2.5 < np.abs(w.xi).max() <= 3.0 and np.abs(w.xj).max() <= 5.0   # the second image is shifted by the baseline
    assert 800 < np.abs(p.xi).max() <= 1000 and np.abs(p.xj).max() <= 2000 and p.thr == R.THR * R.PIXEL_SCALE ** 2


def test_edge_points_sit_within_1e13_of_the_threshold():
    s, T = R.scene("edge"), R.tables("edge")
    for h, least in ((T.win, 8), (T.runner_up, 4)):
        e = R.sampson_all(T.E[h], s.xi, s.xj) / s.thr
        below, above = 1.0 - e, e - 1.0
        assert ((below > 0) & (below <= 1e-13)).sum() >= least, h             # (16 / 8, within 4e-15)
        assert ((above >= 0) & (above <= 1e-13)).sum() >= least, h
    assert len(s.special) == 2 * sum(R.N_EDGE) + sum(R.N_SUPPORT) and s.outlier[s.special].all()
    r = H.find_E_ransac(O, "orc", R.K_ID, s.xi, s.xj, R.ITERS, s.thr, R.MIN_INLIERS)
    assert r["ok"] == 1 and r["best_iter"] == T.win


def test_nan_points_one_drawn_one_never():
    s, T = R.scene("nan"), R.tables("nan")
    a, b = s.special
    assert np.isnan(s.xi[s.special]).all() and np.isnan(s.xj[s.special]).all() and np.isfinite(np.delete(s.xi, s.special, 0)).all()
    assert (T.idx8 == a).any() and not (T.idx8 == b).any()
    hit = (T.idx8 == a).any(axis=1)
    # the reference's Jacobi never picks a NaN pivot (strict '>'), so a NaN octet still yields a finite hypothesis with a count
    assert hit.sum() >= 1 and np.isfinite(T.E).all()
    for h in np.nonzero(hit)[0][:2]:
        e = R.sampson_all(T.E[h], s.xi, s.xj)
        assert np.isnan(e[s.special]).all() and (e < s.thr).sum() == R.ref_counts("nan", R.N0, s.thr)[h]


@pytest.mark.parametrize("name", R.CLASSES)
def test_every_class_has_a_pose_and_an_untouched_winner(name):
    s, T = R.scene(name), R.tables(name)
    c = R.ref_counts(name, R.N0, s.thr)
    r = H.find_E_ransac(O, "orc", R.K_ID, s.xi, s.xj, R.ITERS, s.thr, R.MIN_INLIERS)
    assert r["ok"] == 1 and r["best_iter"] == T.win == int(np.argmax(c)) and len(r["inliers"]) == c[T.win]
    assert T.runner_up != T.win and c[T.runner_up] == np.delete(c, T.win).max()
    assert not np.isin(T.idx8[[T.win, T.runner_up]], s.special).any()
    assert name == "dup" or s.outlier.sum() == round(R.OUTLIER_SHARE * s.n)   # dup: the share of its first half, twice
    again = H.find_E_ransac(O, "orc", R.K_ID, s.xi, s.xj, R.ITERS, s.thr, int(c[T.win]) + 1)
    assert again["ok"] == 0


def test_shard_ranges_cover_every_iteration_once():
    for world in (1, 2, 3, 8, 403):
        edges = [R.shard_range(R.ITERS, r, world) for r in range(world)]
        assert edges[0][0] == 0 and edges[-1][1] == R.ITERS and all(a[1] == b[0] for a, b in zip(edges, edges[1:]))
        assert R.shard_range(R.ITERS, R.rank_of(137, R.ITERS, world), world)[0] <= 137
    assert any(lo == hi for lo, hi in (R.shard_range(R.ITERS, r, 403) for r in range(403)))   # world 403: empty ranges exist
