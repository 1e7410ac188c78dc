"""GPU suite: the fusion kernels over their whole parameter range (sfmx_fusion_check_params), sum bits, count, vertex bits and
faces against the NumPy restatement (tests/fusion_ref.py): a noise slab that reaches every (tetrahedron, case) row of the
triangle table and shares vertices between cells, volume shapes around the 64 x 4 blocks of the integration and the 1 024-element
blocks of the scans (up to 1 024^2 grid points and one slice more), trunc / disp_min / min_weight away from their defaults, maps
holding 0, -1, -32768 and 32767, views of different sizes in one volume (the stack regrown after use), and cameras inside,
behind and partly beside the volume, and the views that fusion, shade and consist must all refuse.  The inputs come from tests/range_inputs.py; tests/test_range_inputs_cpu.py asserts that
they hold what these cases rely on."""
import importlib

import numpy as np
import pytest

import appearance_ref as AR
import consist_ref as CR
import helpers as H
import range_inputs as RI
from test_gpu_fusion import _check

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
VOL, TRUNC = RI.SLAB_VOL, RI.SLAB_TRUNC


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _case(ctx, vol, views, what, **params):
    """all views into one volume, then every output against the reference on the same order of views"""
    ref_kw = {k: v for k, v in params.items() if k != "max_views"}
    ref = RI.fuse_ref(vol, views, **ref_kw)
    fu = ctx.fusion(**vol, **params)
    for cam, d16 in views:
        fu.add_view(cam, d16)
    _check(fu, ref, what)
    n = (len(ref["verts"]), len(ref["faces"]))
    assert fu.counts() == n
    fu.close()
    return ref


def test_slab_reaches_every_table_row(ctx):
    views = [RI.slab_view(**VOL)]
    ref = RI.fuse_ref(VOL, views, trunc=TRUNC)
    configs, pairs = RI.table_coverage(ref["sum"], ref["count"])
    assert len(pairs) == 96 and len(configs) >= 250, (len(pairs), len(configs))  # a property of the input, before the device
    _case(ctx, VOL, views, "noise slab", trunc=TRUNC)


@pytest.mark.parametrize("name", list(RI.BLOCK_SHAPES))
def test_volume_shapes_at_block_boundaries(ctx, name):
    vol, views, trunc = RI.shape_case(*RI.BLOCK_SHAPES[name])
    ref = _case(ctx, vol, views, name, trunc=trunc)
    assert len(ref["faces"]) > 500


@pytest.mark.parametrize("name", list(RI.BIG_SHAPES))
def test_volume_shapes_at_scan_level_boundary(ctx, name):
    """1 024^2 grid points (the second scan level exactly full) and one slice more; millions of vertices and faces"""
    vol, views, trunc = RI.shape_case(*RI.BIG_SHAPES[name])
    ref = _case(ctx, vol, views, name, trunc=trunc)
    assert len(ref["faces"]) > 10 ** 6


@pytest.fixture(scope="module")
def views3():
    return RI.slab_views3(extra=(-1, -32768, 32767))


@pytest.mark.parametrize("trunc", [0.0, 0.5 * VOL["voxel"], TRUNC])
def test_trunc(ctx, views3, trunc):
    ref = _case(ctx, VOL, views3, f"trunc {trunc}", trunc=trunc)
    assert len(ref["faces"]) > 1000


@pytest.mark.parametrize("disp_min", [-5.0, 0.0, 1.0, 40.0, 57.0, float("inf")])
def test_disp_min(ctx, views3, disp_min):
    """disp_min <= 0 lets a disparity of 0 through: Z = +inf, a contribution of exactly 1.0 and no non-finite value anywhere"""
    ref = _case(ctx, VOL, views3, f"disp_min {disp_min}", trunc=TRUNC, disp_min=disp_min)
    assert np.isfinite(ref["sum"]).all() and np.isfinite(ref["verts"]).all()
    assert (len(ref["faces"]) == 0) == (disp_min == float("inf"))


@pytest.mark.parametrize("min_weight", [1, 2, 3, 4])
def test_min_weight(ctx, views3, min_weight):
    """three views: min_weight 4 = views + 1 is the empty surface, (0, 3) shaped outputs and counts (0, 0)"""
    ref = _case(ctx, VOL, views3, f"min_weight {min_weight}", trunc=TRUNC, min_weight=min_weight)
    assert (len(ref["faces"]) == 0) == (min_weight == 4)


@pytest.mark.parametrize("max_views", [1, 2, 64])
@pytest.mark.parametrize("order", ["small_first", "reversed"])
def test_views_of_different_sizes(ctx, order, max_views):
    """40 x 30, 640 x 480, 320 x 240 and the reverse: a larger map arrives after smaller ones have used the stack"""
    views = RI.mixed_size_views()
    if order == "reversed":
        views = views[::-1]
    ref = _case(ctx, VOL, views, f"{order}, max_views {max_views}", trunc=TRUNC, max_views=max_views)
    assert len(ref["faces"]) > 10000


def test_cameras_inside_behind_and_beside(ctx):
    """q2 <= 0 for half of the grid points (camera inside), for all of them (camera looking away), and an image whose four
    borders cut through the volume (the floor(u + 0.5) bounds on both sides); each alone, then all with a plain slab view"""
    special = dict(inside=RI.inside_view(), away=RI.away_view(), border=RI.border_view())
    for name, view in special.items():
        ref = _case(ctx, VOL, [view], name, trunc=TRUNC)
        assert ref["count"].any() == (name != "away")
    ref = _case(ctx, VOL, [RI.slab_view(**VOL, seed=1)] + list(special.values()), "all four", trunc=TRUNC)
    assert len(ref["faces"]) > 10000


def _bad_views(cam, d16):
    """(what, cam, map): NaN and inf in each camera field of one good view, and a 1 x 4097 map (w = 4097, one past the limit)"""
    out = []
    for bad in (float("nan"), float("inf")):
        R = np.array(cam["R_rw"], np.float64)
        R.flat[0] = bad
        c = np.array(cam["c_left"], np.float64)
        c[2] = bad
        out += [(f"R_rw[0] = {bad}", dict(cam, R_rw=R), d16), (f"c_left[2] = {bad}", dict(cam, c_left=c), d16)]
        out += [(f"{k} = {bad}", dict(cam, **{k: bad}), d16) for k in ("f", "cx", "cy", "B")]
    return out + [("w = 4097", cam, np.full((1, 4097), 320, np.int16))]


def test_view_refusals_agree(ctx):
    """fusion, shade and consist refuse the same views with SFMX_ERR_INVALID and keep nothing of them: three good 64 x 64
    sphere views fed afterwards give the reference's bytes in all three (a 9^3 volume, its shaded surface, the filtered maps)"""
    good = CR.sphere_views(3, 64, 64, 120.0)
    textured = [(cam, d16, RI.texture(64, 64, k)) for k, (cam, d16) in enumerate(good)]
    vol = dict(origin=(-0.16, -0.16, -0.16), voxel=0.04, dims=(9, 9, 9))
    ref = AR.fuse(vol["origin"], vol["voxel"], vol["dims"], textured)
    cref = CR.filter_views(good, min_support=1)  # three views far apart: few pixels have one supporter, none has two
    # properties of the input, before the device: a surface, vertices some view sees, pixels kept and pixels dropped
    assert len(ref["faces"]) > 0 and (ref["vertex_views"] > 0).any() and 0 < cref["kept"].sum() < cref["valid"].sum()
    fu, sh, cs = ctx.fusion(**vol), ctx.shade(), ctx.consist()
    for what, cam, d16 in _bad_views(*good[0]):
        img = np.zeros(d16.shape, np.uint8)
        for stage, add in (("fusion", lambda: fu.add_view(cam, d16)), ("shade", lambda: sh.add_view(cam, d16, img)),
                           ("consist", lambda: cs.add_view(cam, d16))):
            with pytest.raises(capi.SfmxError) as e:
                add()
            assert e.value.status == capi.SFMX_ERR_INVALID, f"{stage}: {what}"
        assert sh.view_count() == 0 and cs.view_count() == 0, what
    for cam, d16, img in textured:
        fu.add_view(cam, d16)
        sh.add_view(cam, d16, img)
        cs.add_view(cam, d16)
    assert sh.view_count() == 3 and cs.view_count() == 3
    _check(fu, ref, "after the refusals")
    v, f, n = fu.extract_normals()
    H.assert_bits_equal(v, ref["verts"], "after the refusals: verts")
    H.assert_bits_equal(n, ref["normals"], "after the refusals: normals")
    g, c = sh.shade_fusion(fu, len(v), 4.0 * vol["voxel"])
    assert c.tobytes() == ref["vertex_views"].tobytes() and g.tobytes() == ref["grey"].tobytes(), "after the refusals: shade"
    cs.filter(min_support=1)
    valid, kept = cs.counts()
    assert valid.tobytes() == cref["valid"].tobytes() and kept.tobytes() == cref["kept"].tobytes(), "after the refusals: counters"
    for i in range(3):
        d16, sup = cs.read(i)
        assert d16.tobytes() == cref["disp16"][i].tobytes() and sup.tobytes() == cref["support"][i].tobytes(), f"consist view {i}"
    for o in (fu, sh, cs):
        o.close()
