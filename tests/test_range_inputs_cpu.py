"""CPU suite: the input generators of the parameter-range GPU suites (tests/range_inputs.py).  Each test runs the NumPy
restatement (tests/stereo_ref.py, tests/fusion_ref.py) on a generator and asserts what the GPU cases rely on: true winners in
every disparity band (so in every lane group of the path and select kernels), exact ties that resolve to d = 0, rejections
that carry the noise pair, every row of the triangle table, grid sizes on the scan's block boundaries, and non-empty
surfaces.  These are conditions on the inputs, not on the code under test."""
import numpy as np
import pytest

import fusion_ref as FR
import range_inputs as RI
import stereo_ref as SR

I3 = RI.IDENTITY


def _check_bands(d16, bands, radius, need_valid=None):
    hits = RI.band_hits(d16, bands, radius)
    print("valid %.3f" % (d16 != -16).mean(), [(b, c, round(s, 3)) for b, (c, s) in zip(bands, hits)])
    for b, (cols, share) in zip(bands, hits):
        if cols >= 64:
            assert share >= 0.3, f"band {b}: {share:.3f} of its pixels within one pixel of the truth"
    if need_valid is not None:
        assert (d16 != -16).mean() >= need_valid


@pytest.mark.parametrize("D,census", RI.SWEEP)
def test_sweep_has_winners_in_every_band(D, census):
    il, ir, bands = RI.sweep_pair(D)
    assert {b // 64 for b in bands} == set(range((D + 63) // 64)), "a band in every group of 64 disparities"
    assert 1 in bands and D - 2 in bands and all(m - 1 in bands and m + 1 in bands for m in range(64, D, 64))
    d16 = SR.disparity(il, ir, I3, I3, dict(num_disparities=D, census=census))
    _check_bands(d16, bands, census // 2, need_valid=0.4)


def test_sweep_meets_every_census_at_every_K():
    seen = {((D + 63) // 64, c) for D, c in RI.SWEEP}
    assert seen == {(K, c) for K in (1, 2, 3, 4) for c in (3, 5, 7)}
    assert {D for D, _ in RI.SWEEP} == {16, 48, 64, 80, 128, 144, 176, 192, 208, 256}


@pytest.mark.parametrize("name", list(RI.SHAPES))
def test_shapes_have_winners(name):
    h, w, bands, p = RI.SHAPES[name]
    il, ir = RI.shifted_band_pair(h, w, bands, seed=h)
    assert il.shape == (h, w) and ir.shape == (h, w)
    d16 = SR.disparity(il, ir, I3, I3, p)
    _check_bands(d16, bands, {**SR.DEFAULTS, **p}["census"] // 2, need_valid=0.3)


@pytest.mark.parametrize("name", list(RI.NO_WINDOW))
def test_no_census_window_means_no_disparity(name):
    h, w, p = RI.NO_WINDOW[name]
    il, ir = RI.shifted_band_pair(h, w, (1,), seed=h)
    r = SR.disparity(il, ir, I3, I3, p, want=True)
    assert (r["disp16"] == -16).all()
    nbits = p["census"] ** 2 - 1
    assert (r["S"][:, 0, :] == 4 * nbits).all(), "every cost is nbits: the sums are still defined"


def test_flat_vga_is_one_large_component():
    h, w, bands = RI.FLAT_VGA
    il, ir = RI.shifted_band_pair(h, w, bands, seed=h)
    d16 = SR.disparity(il, ir, I3, I3)
    _check_bands(d16, bands, 2)
    near = np.abs(d16.astype(np.int64) - 16 * bands[0]) <= 16 * SR.DEFAULTS["speckle_range"]
    assert near.sum() >= 250000
    # one component: the speckle filter with a window just below that size keeps them
    assert (SR.speckle(d16, 250000, SR.DEFAULTS["speckle_range"]) != -16).sum() >= 250000


def _min_ties(S):
    return (S == S.min(2, keepdims=True)).sum(2)


def test_adversarial_images():
    h, w = RI.SWEEP_SHAPE
    cases = RI.adversarial_cases(h, w)
    out = {k: SR.disparity(*c[:4], c[4], want=True) for k, c in cases.items()}
    for name in list(RI.TIE_IMAGES) + ["blank_right"]:
        d16 = out[name]["disp16"]
        assert set(np.unique(d16).tolist()) == {-16, 0} and (d16 == 0).mean() >= 0.9, name
    for name in RI.TIE_IMAGES:  # matches at every multiple of 8 (or everywhere): three of the four paths cannot tell them apart
        il, ir = cases[name][:2]
        assert (il[:, 8:] == il[:, :-8]).all() and (il == ir).all(), name
    S = out["blank_right"]["S"]
    assert (S == S[:, :, :1]).all() and (_min_ties(S) == S.shape[2]).all(), "the exact tie: every disparity of every pixel"
    # the noise pair: the rejections carry it; with them off, winners everywhere and exact ties between some of them
    loose, d16 = out["noise_loose"]["disp16"], out["noise"]["disp16"]
    tests_on = SR.disparity(*cases["noise"][:4], dict(speckle_window=0))
    assert (loose != -16).mean() > 0.8 and (tests_on != -16).mean() < 0.5
    assert 0.0 < (d16 != -16).mean() < 0.1
    assert (loose[loose != -16] // 16 >= 64).sum() > 1000, "winners in the upper disparities too"
    assert ((_min_ties(out["noise_loose"]["S"]) > 1) & (loose != -16)).sum() >= 20, "ties between a few lanes"


def test_homographies_cover_the_remap_edges():
    h, w = RI.SWEEP_SHAPE
    il, ir, _ = RI.sweep_pair(128)
    Hs = RI.homographies(w, h)
    share = {}
    for name, Hm in Hs.items():
        rect, valid = SR.remap(il, Hm)
        assert not rect[~valid].any(), "invalid pixels are zero"
        share[name] = valid.mean()
        if name == "identity":
            assert valid.all() and (rect == il).all(), "the last column and row sample exactly on the border"
        if name == "flip":
            assert valid.all() and (rect == il[::-1, ::-1]).all()
        if name == "pole":
            assert valid[:20].any() and not valid[29:].any(), "nothing valid from the pole's row on"
        assert (SR.disparity(il, ir, Hm, Hm) != -16).mean() > 0.05, name
    assert 0.95 < share["translation"] < 1.0 and 0.95 < share["perspective"] < 1.0
    assert 0.05 < share["zoom"] < 0.15 and 0.05 < share["pole"] < 0.5


def test_parameter_cases_change_the_result():
    """every one-parameter case gives a map different from the defaults' (so its case compares something of its own), except
    speckle_window 1 and speckle_range 16, which may coincide with a neighbour; speckle_window 10^6 leaves nothing"""
    il, ir, _ = RI.sweep_pair(128)
    base = SR.disparity(il, ir, I3, I3)
    seen = {}
    for p in RI.PARAMS:
        d16 = SR.disparity(il, ir, I3, I3, p)
        seen[str(p)] = d16
        if p == dict(speckle_window=10 ** 6):
            assert (d16 == -16).all()
        elif p not in (dict(speckle_window=1), dict(speckle_range=16)):
            assert (d16 != base).any(), p
            assert (d16 != -16).any() or p == dict(uniqueness=100), p
    assert (seen[str(dict(speckle_window=1))] == seen[str(dict(speckle_window=0))]).all(), "no component is smaller than one pixel"


# ---- fusion -------------------------------------------------------------------------------------------------------------
_fuse = RI.fuse_ref


def test_slab_covers_the_triangle_table():
    r = _fuse(RI.SLAB_VOL, [RI.slab_view(**RI.SLAB_VOL)], trunc=RI.SLAB_TRUNC)
    configs, pairs = RI.table_coverage(r["sum"], r["count"])
    print(len(configs), len(pairs), len(r["faces"]), (r["count"] == 0).mean())
    assert len(pairs) == 96 and len(configs) >= 250
    assert len(r["faces"]) > 20000 and 0.02 < (r["count"] == 0).mean() < 0.15
    F = r["faces"]
    assert len(np.unique(F)) == len(r["verts"]) and np.bincount(F.ravel()).max() > 1, "vertices are shared between cells"


@pytest.mark.parametrize("name", list(RI.BLOCK_SHAPES) + list(RI.BIG_SHAPES))
def test_volume_shapes_give_faces(name):
    spec = {**RI.BLOCK_SHAPES, **RI.BIG_SHAPES}[name]
    vol, views, trunc = RI.shape_case(*spec)
    r = _fuse(vol, views, trunc=trunc)
    print(name, len(r["verts"]), len(r["faces"]))
    assert len(r["faces"]) > (10 ** 6 if name in RI.BIG_SHAPES else 500)
    assert np.isfinite(r["verts"]).all()


def test_volume_shapes_sit_on_the_block_boundaries():
    n = {k: int(np.prod(v[0])) for k, v in {**RI.BLOCK_SHAPES, **RI.BIG_SHAPES}.items()}
    assert n["s32x16x2"] == 1024 and n["s41x5x5"] == 1025 and n["s41x25x2"] == 2050
    assert n["s128x128x64"] == 1024 ** 2 and n["s128x128x65"] == 1024 ** 2 + 128 * 128
    dims = [v[0] for v in RI.BLOCK_SHAPES.values()]
    assert {(65, 5, 3), (63, 3, 2), (64, 4, 2), (130, 9, 2), (2, 3, 129), (129, 2, 2)} <= set(dims)


def test_slab_parameters():
    vol = RI.SLAB_VOL
    views = RI.slab_views3(extra=(-1, -32768, 32767))
    for v in (-16, 0, -1, -32768, 32767):
        assert all((d16 == v).any() for _, d16 in views), v
    faces = {mw: len(_fuse(vol, views, trunc=RI.SLAB_TRUNC, min_weight=mw)["faces"]) for mw in (1, 2, 3, 4)}
    print(faces)
    assert faces[1] > faces[2] > faces[3] > 0 and faces[4] == 0
    by_min = {dm: _fuse(vol, views, trunc=RI.SLAB_TRUNC, disp_min=dm) for dm in (-5.0, 0.0, 1.0, 40.0, 57.0, float("inf"))}
    for dm, r in by_min.items():
        assert np.isfinite(r["sum"]).all() and np.isfinite(r["verts"]).all(), dm
    assert by_min[0.0]["count"].sum() > by_min[1.0]["count"].sum(), "a disparity of 0 contributes under disp_min <= 0"
    assert by_min[1.0]["count"].sum() > by_min[57.0]["count"].sum() > 0 and len(by_min[57.0]["faces"]) > 0
    assert not by_min[float("inf")]["count"].any()
    for trunc in (0.0, 0.5 * vol["voxel"], RI.SLAB_TRUNC):
        assert len(_fuse(vol, views, trunc=trunc)["faces"]) > 1000, trunc


def test_mixed_size_views():
    views = RI.mixed_size_views()
    assert [d16.shape for _, d16 in views] == [(30, 40), (480, 640), (240, 320)]
    for order in (views, views[::-1]):
        r = _fuse(RI.SLAB_VOL, order, trunc=RI.SLAB_TRUNC)
        assert len(r["faces"]) > 10000 and (r["count"] == 3).mean() > 0.5


def test_special_cameras():
    vol = RI.SLAB_VOL
    one = lambda v: FR.integrate(vol["origin"], vol["voxel"], vol["dims"], [v], trunc=RI.SLAB_TRUNC)[1]
    c = one(RI.inside_view())
    assert not c[:6].any() and c[7:].any(), "only the half of the volume in front of the camera"
    assert not one(RI.away_view()).any()
    c = one(RI.border_view())
    assert c[:, 2:-2, 4:-4].any() and not c[:, :, 0].any() and not c[:, :, -1].any() and not c[:, 0].any() and not c[:, -1].any()
