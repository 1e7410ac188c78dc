"""GPU suite: the stereo kernels over their whole parameter range (sfmx_stereo_check_params), bit for bit against the NumPy
restatement (tests/stereo_ref.py) stage by stage: every K = ceil(D / 64) of k_st_path / k_st_select with full and partly
filled last lanes, the three census windows, every parameter away from its default, image shapes from smaller than the census
window to the maximum width, homographies that reach the remap's edges, exact ties, and one object reused across pairs.
The inputs come from tests/range_inputs.py; tests/test_range_inputs_cpu.py asserts that they hold what these cases rely on.
The small cases run first and the VGA one last."""
import importlib

import numpy as np
import pytest

import helpers as H
import range_inputs as RI
import stereo_ref as SR
from test_gpu_stereo import _mismatch

pytestmark = pytest.mark.gpu
capi = importlib.import_module(H.PKG_NAME + ".capi")
I3 = RI.IDENTITY


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _compare(out, ref, what):
    """stage by stage, so that a mismatch names its stage"""
    if out["rect"] is not None:
        for v, side in enumerate(("left", "right")):
            assert (out["rect"][v] == ref["rect"][v]).all(), f"{what}: rectified {side}: " + _mismatch(out["rect"][v], ref["rect"][v])
    if out["S"] is not None:
        assert (out["S"] == ref["S"]).all(), f"{what}: aggregation: " + _mismatch(out["S"], ref["S"])
    assert (out["disp16"] == ref["disp16"]).all(), f"{what}: disp16: " + _mismatch(out["disp16"], ref["disp16"])


def _case(ctx, il, ir, H_l, H_r, p, what, want_rect=False):
    h, w = il.shape
    ref = SR.disparity(il, ir, H_l, H_r, p, want=True)
    st = ctx.stereo(w, h, **p)
    out = st.disparity(il, ir, H_l, H_r, want_rect=want_rect, want_sum=True)
    st.close()
    _compare(out, ref, what)
    return ref


@pytest.mark.parametrize("D,census", RI.SWEEP)
def test_disparity_range_and_census(ctx, D, census):
    """bands at 1, around every multiple of 64 below D and at D - 2: winners in every lane group and in the last lane"""
    il, ir, bands = RI.sweep_pair(D)
    ref = _case(ctx, il, ir, I3, I3, dict(num_disparities=D, census=census), f"D {D} census {census}")
    assert (ref["disp16"] != -16).mean() >= 0.4


@pytest.mark.parametrize("p", RI.PARAMS, ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
def test_one_parameter_from_defaults(ctx, p):
    il, ir, _ = RI.sweep_pair(128)
    ref = _case(ctx, il, ir, I3, I3, p, str(p))
    if p == dict(speckle_window=10 ** 6):
        assert (ref["disp16"] == -16).all()


@pytest.mark.parametrize("name", list(RI.SHAPES))
def test_shapes(ctx, name):
    h, w, bands, p = RI.SHAPES[name]
    il, ir = RI.shifted_band_pair(h, w, bands, seed=h)
    ref = _case(ctx, il, ir, I3, I3, p, name, want_rect=True)
    assert (ref["disp16"] != -16).mean() >= 0.3


@pytest.mark.parametrize("name", list(RI.NO_WINDOW))
def test_image_smaller_than_census_window(ctx, name):
    h, w, p = RI.NO_WINDOW[name]
    il, ir = RI.shifted_band_pair(h, w, (1,), seed=h)
    ref = _case(ctx, il, ir, I3, I3, p, name, want_rect=True)
    assert (ref["disp16"] == -16).all()


def test_width_above_maximum_refused(ctx):
    assert capi.stereo_check_params(4096, 16, num_disparities=16) and not capi.stereo_check_params(4097, 16, num_disparities=16)
    with pytest.raises(capi.SfmxError) as e:
        ctx.stereo(4097, 16, num_disparities=16)
    assert e.value.status == capi.SFMX_ERR_INVALID


@pytest.mark.parametrize("name", ["constant", "stripes", "checker", "blank_right", "noise", "noise_loose"])
def test_adversarial_images(ctx, name):
    """matches at many disparities, the exact tie of every disparity at every pixel (the smallest-d rule of the packed minimum
    and of the right view's atomicMin), and a pair that the uniqueness and left-right tests decide"""
    il, ir, H_l, H_r, p = RI.adversarial_cases(*RI.SWEEP_SHAPE)[name]
    ref = _case(ctx, il, ir, H_l, H_r, p, name, want_rect=True)
    if name not in ("noise", "noise_loose"):
        assert (ref["disp16"] == 0).mean() >= 0.9


@pytest.mark.parametrize("name", ["identity", "translation", "perspective", "pole", "flip", "zoom"])
def test_homographies(ctx, name):
    h, w = RI.SWEEP_SHAPE
    il, ir, _ = RI.sweep_pair(128)
    Hm = RI.homographies(w, h)[name]
    ref = _case(ctx, il, ir, Hm, Hm, {}, name, want_rect=True)
    assert (ref["disp16"] != -16).mean() > 0.05


def test_object_reuse_carries_no_state(ctx):
    """pair A, pair B, pair A again on one object: A's bytes are those of a fresh object (S, labels, LDS keys), also through
    device-resident inputs"""
    import torch
    h, w = RI.SWEEP_SHAPE
    al, ar, _ = RI.sweep_pair(128)
    bl, br = RI.noise_pair(h, w)
    ref_a, ref_b = SR.disparity(al, ar, I3, I3, want=True), SR.disparity(bl, br, I3, I3, want=True)
    fresh = ctx.stereo(w, h)
    _compare(fresh.disparity(al, ar, I3, I3, want_rect=True, want_sum=True), ref_a, "fresh A")
    fresh.close()
    st = ctx.stereo(w, h)
    run = lambda l, r: st.disparity(l, r, I3, I3, want_rect=True, want_sum=True)
    _compare(run(al, ar), ref_a, "A")
    _compare(run(bl, br), ref_b, "B after A")
    _compare(run(al, ar), ref_a, "A after B")
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (al, ar, bl, br)]
    torch.cuda.synchronize()
    pa, pb = (dev[0].data_ptr(), dev[1].data_ptr()), (dev[2].data_ptr(), dev[3].data_ptr())
    _compare(run(*pb), ref_b, "device B")
    _compare(run(*pa), ref_a, "device A after B")
    st.close()


def test_flat_vga_scene(ctx):
    """a fronto-parallel wall: one constant disparity over the whole image, one speckle component of about 300 000 pixels"""
    h, w, bands = RI.FLAT_VGA
    il, ir = RI.shifted_band_pair(h, w, bands, seed=h)
    ref = _case(ctx, il, ir, I3, I3, {}, "flat VGA")
    assert (np.abs(ref["disp16"].astype(np.int64) - 16 * bands[0]) <= 32).sum() >= 250000
