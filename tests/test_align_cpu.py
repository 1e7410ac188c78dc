"""CPU suite: direct TSDF pose alignment -- the NumPy restatement (tests/align_ref.py) on the four-sphere fixture (the
calibration of DESIGN.md 19), its ordered sum against a plain Python restatement of the same tree, the end states of the loop
(TOO_FEW, DEGENERATE), the single sphere as the rotation-degenerate case it is, and the parts of the library that need no
device: the parameter check and the CPU stand-in, which must report that the stage is not there."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import align_ref as AL
import fusion_ref as FR
import helpers as H
import raycast_ref as RR

capi = importlib.import_module(H.PKG_NAME + ".capi")


# ---- calibration ----------------------------------------------------------------------------------------------
# measured with this file's own code; bounds by the rule of DESIGN.md 14: 1.25 x the measured value, rounded up (errors to 0.05,
# the RMS to 0.01, the spreads to one digit).  The device is held to bit equality, not to these.
CALIB = {
    AL.NOVEL[0]: dict(n=8447, iters=(5, 8, 9), rot=0.20, centre=0.30, rms=0.08, spread_rot=5e-6, spread_centre=7e-6),
    AL.NOVEL[1]: dict(n=7796, iters=(5, 8, 9), rot=0.25, centre=0.30, rms=0.08, spread_rot=1e-5, spread_centre=3e-5),
}
MEASURED = {  # final rotation error (degrees), centre error (voxels), RMS of s; the largest spread over the three starts
    AL.NOVEL[0]: dict(rot=0.13209, centre=0.20556, rms=0.05952, spread_rot=3.82e-6, spread_centre=5.38e-6),
    AL.NOVEL[1]: dict(rot=0.16192, centre=0.21044, rms=0.06240, spread_rot=7.74e-6, spread_centre=2.06e-5),
}


def _up(x, q):
    return math.ceil(1.25 * x / q - 1e-9) * q


def _one_digit(x):
    q = 10.0 ** math.floor(math.log10(1.25 * x))
    return math.ceil(1.25 * x / q - 1e-9) * q


def test_calibration_bounds_follow_the_rule():
    for pos, m in MEASURED.items():
        c = CALIB[pos]
        assert c["rot"] == pytest.approx(_up(m["rot"], 0.05)) and c["centre"] == pytest.approx(_up(m["centre"], 0.05))
        assert c["rms"] == pytest.approx(_up(m["rms"], 0.01))
        assert c["spread_rot"] == pytest.approx(_one_digit(m["spread_rot"])) and c["spread_centre"] == pytest.approx(_one_digit(m["spread_centre"]))


def starts(cam, vol):
    """the three starts of a camera: one default_rng(3) per camera, an axis and a direction drawn per start in STARTS' order"""
    rng = np.random.default_rng(3)
    p = AL.pivot(vol.origin, vol.voxel, vol.n)
    return [AL.perturb(cam, p, deg, vx, vol.voxel, rng) for deg, vx in AL.STARTS]


@pytest.mark.parametrize("pos", AL.NOVEL)
def test_four_spheres_converge_to_one_pose(pos):
    want = CALIB[pos]
    vol = AL.scene_volume()["volume"]
    cam, d16 = AL.novel_view(pos)
    finals = []
    for k, start in enumerate(starts(cam, vol)):
        r = AL.align(vol, start, d16)
        e0, e1 = AL.pose_error(start, cam, vol.voxel), AL.pose_error(r["view"], cam, vol.voxel)
        n, e = r["trace"][-1][0], r["trace"][-1][1]
        rms = math.sqrt(e / n)
        print(pos, AL.STARTS[k], "iterations", r["iterations"], "start", e0, "final", e1, "n", n, "rms", rms)
        assert r["status"] == AL.CONVERGED and r["iterations"] <= AL.DEFAULTS["max_iters"]
        assert r["iterations"] == want["iters"][k] and n == want["n"]
        if k:
            assert e1[0] < e0[0] and e1[1] < e0[1], "the final error is below the start error"
        assert e1[0] <= want["rot"] and e1[1] <= want["centre"] and rms <= want["rms"]
        finals.append(r["view"])
    for i in range(3):
        for j in range(i + 1, 3):
            s = AL.pose_error(finals[i], finals[j], vol.voxel)
            print(pos, "spread", i, j, s)
            assert s[0] <= want["spread_rot"] and s[1] <= want["spread_centre"]


def test_four_spheres_system_is_well_conditioned():
    """condition number of A at the true pose: 600 and 758; every sample is either invalid or used"""
    vol = AL.scene_volume()["volume"]
    for pos, lo, hi in ((AL.NOVEL[0], 550.0, 650.0), (AL.NOVEL[1], 700.0, 820.0)):
        cam, d16 = AL.novel_view(pos)
        sums, n = AL.system(vol, cam, d16)
        A = np.zeros((6, 6))
        for t, (m, k) in enumerate(AL.PAIRS):
            A[m, k] = A[k, m] = sums[t]
        ev = np.linalg.eigvalsh(A)
        assert lo < ev[-1] / ev[0] < hi, ev
        why = AL.rows(vol, cam, d16)[3]
        assert why["used"] == n == CALIB[pos]["n"] and why["outside"] == why["undefined"] == why["far"] == 0


def test_stride_and_damping_reach_the_same_neighbourhood():
    vol = AL.scene_volume()["volume"]
    cam, d16 = AL.novel_view(AL.NOVEL[0])
    start = starts(cam, vol)[2]
    # measured: stride 2 ends 0.1200 degrees / 0.1907 voxels from the true pose in 9 iterations, damping 1000 at 0.1321 / 0.2056
    # in 8; bounds by the same rule
    for kw, iters, rot, centre in ((dict(stride=2), 9, 0.15, 0.25), (dict(damping=1000.0), 8, 0.20, 0.30)):
        r = AL.align(vol, start, d16, **kw)
        e = AL.pose_error(r["view"], cam, vol.voxel)
        print(kw, r["status"], r["iterations"], e)
        assert r["status"] == AL.CONVERGED and r["iterations"] == iters and e[0] <= rot and e[1] <= centre


# ---- the ordered sum ---------------------------------------------------------------------------------------------------------
def _plain_tree(values):
    """the halving tree over a list of 256 Python floats"""
    v = list(values)
    off = 128
    while off >= 1:
        v = [v[t] + v[t + off] for t in range(off)]
        off //= 2
    return v[0]


def _plain_sum(T):
    """align_ref.ordered_sum for one term [nsy][nsx] in plain Python: tiles, tree index t = 4 lane + wave, groups of 256 rows"""
    nsy, nsx = T.shape
    nby, nbx = (nsy + 15) // 16, (nsx + 15) // 16
    part = []
    for by in range(nby):
        for bx in range(nbx):
            slot = [0.0] * 256
            for wave in range(4):
                for lane in range(64):
                    i, j = 16 * bx + 8 * (wave & 1) + (lane & 7), 16 * by + 8 * (wave >> 1) + (lane >> 3)
                    if i < nsx and j < nsy:
                        slot[4 * lane + wave] = float(T[j, i])
            part.append(_plain_tree(slot))
    while len(part) > 1:
        part = [_plain_tree((part[g:g + 256] + [0.0] * 256)[:256]) for g in range(0, len(part), 256)]
    return part[0]


@pytest.mark.parametrize("nsy, nsx", [(1, 1), (16, 16), (17, 16), (7, 9), (40, 300), (272, 272)])
def test_ordered_sum_is_the_written_tree(nsy, nsx):
    rng = np.random.default_rng(nsy * 1000 + nsx)
    T = rng.normal(size=(2, nsy, nsx)) * 10.0 ** rng.integers(-8, 8, size=(2, nsy, nsx))
    T[rng.random(T.shape) < 0.2] = -0.0
    T[1, rng.random((nsy, nsx)) < 0.5] = 0.0
    got = AL.ordered_sum(T)
    for t in range(2):
        want = _plain_sum(T[t])
        assert np.float64(got[t]).tobytes() == np.float64(want).tobytes(), (t, got[t], want)
    if nsy == 272:
        assert ((nsy + 15) // 16) * ((nsx + 15) // 16) > 256, "the second level recurses"


def test_negative_zero_survives_only_a_full_block():
    """-0.0 + +0.0 = +0.0: a sum is -0.0 only when every slot of every block is, and padding makes it +0.0"""
    full = np.full((1, 16, 16), -0.0)
    assert math.copysign(1.0, AL.ordered_sum(full)[0]) == -1.0
    assert math.copysign(1.0, AL.ordered_sum(full[:, :15])[0]) == 1.0
    assert math.copysign(1.0, AL.ordered_sum(np.full((1, 16, 32), -0.0))[0]) == 1.0, "two rows are padded to 256 with +0.0"


# ---- solve and update --------------------------------------------------------------------------------------------------------
def test_solve_and_update_against_numpy():
    rng = np.random.default_rng(5)
    Jm = rng.normal(size=(40, 6))
    A, b = Jm.T @ Jm, Jm.T @ rng.normal(size=40)
    sums = [A[m, n] for m, n in AL.PAIRS] + list(b) + [1.0]
    d = AL.solve(sums)
    assert np.allclose(d, np.linalg.solve(A, -b), rtol=1e-10)
    assert np.allclose(AL.solve(sums, 2.5), np.linalg.solve(A + 2.5 * np.eye(6), -b), rtol=1e-10)
    assert AL.solve([0.0] * 28) is None and AL.solve([float("nan")] * 28) is None and AL.solve([float("inf")] * 28) is None
    D = np.array(AL.cayley([0.3, -0.2, 0.5]))
    assert np.allclose(D @ D.T, np.eye(3), atol=1e-15) and np.linalg.det(D) > 0
    small = np.array(AL.cayley([1e-6, 2e-6, -3e-6]))
    assert np.allclose(small - np.eye(3), [[0, 3e-6, 2e-6], [-3e-6, 0, -1e-6], [-2e-6, 1e-6, 0]], atol=1e-11), "dR = I + [omega]x to first order"
    cam = FR.look_at_cam((0.3, 0.2, -0.3), (0.0, 0.0, 0.0), 300.0, 16, 16)
    out = AL.update(cam, [0.01, 0.02, 0.03], [0.0] * 6)
    # a zero step leaves the values alone (a -0.0 entry may come back as +0.0: 1.0 * -0.0 + 0.0 * x)
    assert np.array_equal(out["R_rw"], cam["R_rw"]) and np.allclose(out["c_left"], cam["c_left"], atol=1e-17)
    assert out["f"] == cam["f"] and out["B"] == cam["B"]


# ---- end states ----------------------------------------------------------------------------------------------------------------
def test_too_few_on_an_all_invalid_map():
    vol = AL.scene_volume()["volume"]
    cam, d16 = AL.novel_view(AL.NOVEL[0])
    sums, n = AL.system(vol, cam, np.full_like(d16, -16))
    assert n == 0 and not sums.any() and not np.signbit(sums).any()
    r = AL.align(vol, cam, np.full_like(d16, -16))
    assert r["status"] == AL.TOO_FEW and r["iterations"] == 1 and r["trace"] == [(0, 0.0, 0.0, 0.0)]
    assert r["view"]["R_rw"] is cam["R_rw"] and r["view"]["c_left"] is cam["c_left"], "the input pose"


def uniform_volume():
    """s = 0.5 everywhere: the gradient is zero, A = 0"""
    return AL.volume(np.full((9, 9, 9), 0.5), np.ones((9, 9, 9), np.int32), (0.0, 0.0, 0.0), 0.01)


def uniform_view():
    cam = RR.axis_camera((0.04, 0.04, -0.2), 100.0, 16, 16, 7.5, 7.5)
    cam["B"] = 0.05
    return cam, np.full((16, 16), int(round(16 * 100.0 * 0.05 / 0.24)), np.int16)


def test_degenerate_on_a_volume_without_gradient():
    vol = uniform_volume()
    cam, d16 = uniform_view()
    sums, n = AL.system(vol, cam, d16)
    assert n == 256 and not sums[:27].any() and sums[27] == 64.0
    r = AL.align(vol, cam, d16)
    assert r["status"] == AL.DEGENERATE and r["iterations"] == 1 and r["view"]["c_left"] is cam["c_left"]
    # with damping the step exists and is exactly zero: the loop converges where it stands
    r = AL.align(vol, cam, d16, damping=1.0)
    assert r["status"] == AL.CONVERGED and r["iterations"] == 1 and r["trace"][0][2:] == (0.0, 0.0)
    assert np.array_equal(r["view"]["R_rw"], cam["R_rw"]) and np.array_equal(r["view"]["c_left"], cam["c_left"])


def test_single_sphere_is_rotation_degenerate():
    """DESIGN.md 13's fixture, one sphere about the pivot: every rotation leaves it unchanged, so three eigenvalues of A are the
    discretisation's alone (measured 1.27e3, 1.96e3, 2.21e3 against 2.20e7 .. 7.33e7, condition 5.8e4) and the pose creeps about
    0.35 degrees per iteration without ever converging.  The case shows one thing only: damping above those eigenvalues keeps
    the step small and finite (0.06 degrees per iteration at 1e4) and leaves the translation alone."""
    sp = RR.sphere_volume()
    vol = AL.volume(sp["sum"], sp["count"], sp["vol"]["origin"], sp["vol"]["voxel"])
    cam = FR.look_at_cam(RR.SPHERE_CAM["pos"], (0.0, 0.0, 0.0), 300.0, 160, 160)
    d16 = FR.sphere_disp16(cam, 160, 160, sp["radius"])
    sums, n = AL.system(vol, cam, d16)
    A = np.zeros((6, 6))
    for t, (m, k) in enumerate(AL.PAIRS):
        A[m, k] = A[k, m] = sums[t]
    ev = np.linalg.eigvalsh(A)
    print("single sphere: n", n, "eigenvalues", ev)
    assert n == 11620 and ev[2] < 3e3 and ev[3] > 2e7
    free, damped = AL.solve(sums, 0.0), AL.solve(sums, 1e4)
    assert all(math.isfinite(x) for x in free + damped)
    assert AL.norm3(damped[:3]) < 0.2 * AL.norm3(free[:3]) and abs(AL.norm3(damped[3:]) / AL.norm3(free[3:]) - 1.0) < 0.01
    r = AL.align(vol, cam, d16, max_iters=4)
    assert r["status"] == AL.MAX_ITERS and all(t[2] > 5e-3 for t in r["trace"]), "it creeps"


# ---- the library without a device ----------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.align_default_params() == capi.ALIGN_DEFAULTS == AL.DEFAULTS
    assert capi.align_check_params()
    assert capi.align_check_params(max_iters=1) and capi.align_check_params(max_iters=64) and capi.ALIGN_ITERS_CAP == 64
    assert capi.align_check_params(stride=5000, disp_min=0.0, min_weight=7, min_pixels=1, damping=1e9, eps_rot=0.0, eps_trans=0.0)
    assert capi.align_check_params(disp_min=-3.0)
    for bad in (dict(max_iters=0), dict(max_iters=65), dict(max_iters=-1), dict(stride=0), dict(stride=-2), dict(disp_min=float("nan")),
                dict(disp_min=float("inf")), dict(min_weight=-1), dict(min_pixels=0), dict(damping=-1e-9), dict(damping=float("nan")),
                dict(damping=float("inf")), dict(eps_rot=-1.0), dict(eps_rot=float("nan")), dict(eps_rot=float("inf")), dict(eps_trans=-1.0),
                dict(eps_trans=float("nan")), dict(eps_trans=float("inf"))):
        assert not capi.align_check_params(**bad), bad
    with pytest.raises(TypeError):
        capi.align_params(iterations=3)
    assert capi.ALIGN_STATUS == ("CONVERGED", "MAX_ITERS", "TOO_FEW", "DEGENERATE")
    assert (capi.ALIGN_CONVERGED, capi.ALIGN_MAX_ITERS, capi.ALIGN_TOO_FEW, capi.ALIGN_DEGENERATE) == (AL.CONVERGED, AL.MAX_ITERS, AL.TOO_FEW, AL.DEGENERATE)


STANDIN_MAIN = r"""
#include <cstdio>
#include "fusion.hpp"
int main() {
  sfmx_ctx* ctx = nullptr;
  if (sfmx_ctx_create(0, &ctx) != SFMX_OK) return 2;
  const double K[9] = {100, 0, 8, 0, 100, 8, 0, 0, 1};
  sfmx_stereo_params sp{};
  sfmx_fusion_params fp{};
  sfmx_fusion_result_ex res{};
  sfmx_align_result out{};
  sfmx_align_request aq{1, sfmx_align_params{10, 1, 1.0, 0, 64, 0.0, 1e-6, 1e-4}, &out};
  const int with = sfmx_host_fusion_mesh_al(ctx, nullptr, 0, 0, 16, 16, K, nullptr, nullptr, 0, &sp, &fp, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, &aq, &res, nullptr, nullptr, 0);
  std::printf("%d\n", with);
  sfmx_ctx_destroy(ctx);
  return 0;
}
"""


def test_stand_in_library_reports_unsupported(tmp_path):
    """the host layer on the CPU stand-in of libsfmx.so (tests/fake_sfmx), which has no device stage: it links, because the
    device entries are weak references, and a request that needs one says SFMX_ERR_UNSUPPORTED"""
    pkg = os.path.join(H.ROOT, H.PKG_NAME)
    host = os.path.join(pkg, "csrc", "host")
    out = str(tmp_path)
    flags = ["-std=c++20", "-O0", "-ffp-contract=off", "-fPIC", "-I" + os.path.join(H.ROOT, "include")]
    with open(os.path.join(out, "main.cpp"), "w") as f:
        f.write(STANDIN_MAIN)
    subprocess.run(["g++", *flags, "-shared", "-o", os.path.join(out, "libsfmx.so"), os.path.join(H.ROOT, "tests", "fake_sfmx", "fake_sfmx.cpp"),
                    os.path.join(H.ROOT, "oracle", "sfm_oracle.cpp"), "-lrt", "-lpthread"], check=True)
    srcs = [os.path.join(host, n) for n in sorted(os.listdir(host)) if n.endswith(".cpp") and n != "main.cpp"]
    subprocess.run(["g++", *flags, "-I" + host, "-o", os.path.join(out, "standin"), os.path.join(out, "main.cpp"), *srcs, "-L" + out, "-lsfmx",
                    "-Wl,-rpath," + out, "-lpthread"], check=True)
    p = subprocess.run([os.path.join(out, "standin")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert int(p.stdout.strip()) == capi.SFMX_ERR_UNSUPPORTED
