"""The raw call of sfmx_shi_tomasi_candidates_pruned, its check against the oracle, and the fresh-process runner of the front-end range
suite (tests/test_gpu_frontend_range.py): SFMX_SHI_SWEEPS is read once per process, so every value of it gets a process of its own.

    python tests/frontend_child.py <out.npz>

The parent puts SFMX_SHI_MODE=sweeps and SFMX_SHI_SWEEPS into the environment.  This process runs the cases of CHILD_CASES and writes
the raw outputs per case; the parent checks them with check_pruned."""
import importlib
import os
import sys
from ctypes import POINTER, byref, c_double, c_int, c_int32, c_uint32
from typing import NamedTuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_inputs as F  # noqa: E402
import helpers as H  # noqa: E402

XY_FILL, FULL_FILL = 0xDEADBEEF, -7   # what the output arrays hold before the call; the scores hold NaN
PAD = 8


class Pruned(NamedTuple):
    xy: np.ndarray     # [cap + PAD] raw (x | y << 16 | accepted << 31)
    sc: np.ndarray     # [cap + PAD]
    full: np.ndarray   # [cap + PAD] cand_full_index
    n: int             # survivors
    ntot: int          # candidates before resolution
    mx: float


def pruned_raw(ctx, pyr, quality, min_dist, cap=None) -> Pruned:
    cap = cap or pyr.w * pyr.h
    xy = np.full(cap + PAD, XY_FILL, np.uint32)
    sc = np.full(cap + PAD, np.nan)
    full = np.full(cap + PAD, FULL_FILL, np.int32)
    n, ntot, mx = c_int(), c_int(), c_double()
    ctx._chk(ctx.lib.sfmx_shi_tomasi_candidates_pruned(ctx.h_, pyr.h_, c_double(quality), c_int(min_dist), c_int(cap),
                                                       xy.ctypes.data_as(POINTER(c_uint32)), sc.ctypes.data_as(POINTER(c_double)),
                                                       full.ctypes.data_as(POINTER(c_int32)), byref(n), byref(ntot), byref(mx)))
    return Pruned(xy, sc, full, n.value, ntot.value, mx.value)


_picks: dict = {}


def expected_pick(key, img, quality, min_dist):
    """the oracle's greedy pick with max_corners = w * h, computed once per key.  With min_dist = 1 no two distinct pixels are within
    min_dist (dx^2 + dy^2 < 1 only for the pixel itself), so the pick is every candidate: above 20 000 candidates that is used
    instead of the oracle's quadratic walk."""
    k = (key, quality, min_dist)
    if k not in _picks:
        exp, yy, xx = F.oracle_candidates(img, quality)
        if min_dist == 1 and len(yy) > 20000:
            _picks[k] = set((yy.astype(np.int64) * img.shape[1] + xx).tolist())
        else:
            _picks[k] = F.oracle_pick(img, quality, min_dist)
    return _picks[k]


def check_pruned(res: Pruned, key, img, quality, min_dist, cap, what):
    """the contract of include/sfmx.h against orc_shi_score and orc_shi_tomasi; returns the survivors' linear indices"""
    h, w = img.shape
    exp, yy, xx = F.oracle_candidates(img, quality)
    lin = yy.astype(np.int64) * w + xx
    assert res.ntot == len(lin), (what, "n_total", res.ntot, len(lin))
    assert res.mx == exp.max(), (what, "max")
    assert 0 <= res.n <= res.ntot, (what, res.n, res.ntot)
    m = min(res.n, cap)
    x, y, flag = (res.xy[:m] & 0x7FFF).astype(np.int64), ((res.xy[:m] >> 16) & 0x7FFF).astype(np.int64), (res.xy[:m] >> 31).astype(bool)
    assert (x < w).all() and (y < h).all(), what
    key_lin = y * w + x
    assert (np.diff(key_lin) > 0).all(), (what, "survivors are not in strictly increasing row-major order")
    pos = res.full[:m].astype(np.int64)
    assert ((pos >= 0) & (pos < len(lin))).all() and np.array_equal(lin[pos], key_lin), (what, "cand_full_index")
    H.assert_bits_equal(res.sc[:m], exp[y, x], f"{what}: scores")
    assert (res.xy[m:] == XY_FILL).all() and np.isnan(res.sc[m:]).all() and (res.full[m:] == FULL_FILL).all(), (what, "written past min(n, cap)")
    pick = expected_pick(key, img, quality, min_dist)
    wrong = set(key_lin[flag].tolist()) - pick
    assert not wrong, (what, "flagged as certainly accepted, not picked by the oracle", sorted(wrong)[:5])
    if cap >= res.n:
        lost = pick - set(key_lin.tolist())
        assert not lost, (what, "picked by the oracle, dropped as certainly rejected", sorted(lost)[:5])
    if min_dist == 1:
        assert res.n == res.ntot and flag.all(), (what, "min_dist = 1: every candidate is accepted")
    return key_lin


# (kind, (w, h), min_dist) of the fresh-process runs
CHILD_CASES = [(kind, size, md) for kind in ("noisy", "quant4", "checker", "lattice") for size in ((40, 20), (65, 33), (127, 95), (333, 251))
               for md in F.MIN_DIST if not (size == (333, 251) and md == 1 and kind != "noisy")]
CHILD_SWEEPS = ("1,0,0", "3,8,40", "64,0,0")   # one dense sweep only; dense + work list + one-workgroup tail; dense sweeps only


def main(out_path):
    capi = importlib.import_module(H.PKG_NAME + ".capi")
    ctx = capi.Context(0)
    out = {}
    for i, (kind, (w, h), md) in enumerate(CHILD_CASES):
        pyr = ctx.pyramid(F.score_image(kind, w, h), 1)
        res = pruned_raw(ctx, pyr, 0.01, md)
        pyr.close()
        out[f"{i}:xy"], out[f"{i}:sc"], out[f"{i}:full"] = res.xy, res.sc, res.full
        out[f"{i}:n"] = np.array([res.n, res.ntot])
        out[f"{i}:mx"] = np.array(res.mx)
    np.savez(out_path, **out)
    ctx.close()
    print(f"frontend_child SFMX_SHI_SWEEPS={os.environ.get('SFMX_SHI_SWEEPS')}: {len(CHILD_CASES)} cases")


if __name__ == "__main__":
    main(sys.argv[1])
