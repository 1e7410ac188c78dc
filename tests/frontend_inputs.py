"""Deterministic inputs for the parameter-range suite of the tracking front end (tests/test_gpu_frontend_range.py): image pairs for the
KLT kernels of csrc/hip/klt.hip, track populations with a class label per track, a restatement of the kernels' on-grid test and of
track_point that counts what the kernels count, score-map images and the size table of the corner kernels of csrc/hip/image.hip.
No files, no device, no binding of the device library; the oracle is loaded lazily, only by the functions of the reference side.
tests/test_frontend_inputs_cpu.py asserts on the CPU the properties of these inputs that the GPU cases rely on (every class present,
every off-grid branch taken, windows re-staged, levels left early and exhausted, ties really there), so that no GPU case can pass on
an input that misses its point.
tests/test_oracle_vs_reference_range.py holds the oracle to the real reference on the pairs, populations, score images and size
tables of this module.

Coordinates are (x, y) in level-0 pixels.  A pair is two u8 images of one size; a population is xy [N][2] plus labels [N]."""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import numpy as np

KLT_P = 32           # side of the staged window (csrc/hip/klt.hip)
KLT_MAX_R = 7
KLT_MULTI_MAX_R = 6  # k_klt_track_multi: the grid slots of an axis sit in one 16-lane row
MAX_LEVELS = 8       # SFMX_MAX_LEVELS
NO_WINDOW = 0x7fffff00
FAR = 0x40000000
SHI_SPEC = 4096      # survivors that travel in the speculative pinned download (csrc/hip/image.hip)


# ---- images ---------------------------------------------------------------------------------------------------------------------
def texture(w, h, seed, shift=(0.0, 0.0), noise=1.5, noise_seed=0, lo=5.0, hi=48.0, waves=48):
    """A sum of `waves` plane waves with wavelengths lo..hi pixels, evaluated at (x + shift[0], y + shift[1]): a second call with
    another shift is an exact sub-pixel warp of the first.  Gaussian noise of `noise` grey levels from its own seed."""
    rng = np.random.default_rng(seed)
    lam = np.exp(rng.uniform(np.log(lo), np.log(hi), waves))
    th, ph, amp = rng.uniform(0, 2 * np.pi, waves), rng.uniform(0, 2 * np.pi, waves), rng.uniform(0.5, 1.0, waves)
    kx, ky = 2 * np.pi / lam * np.cos(th), 2 * np.pi / lam * np.sin(th)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x + shift[0], y + shift[1]
    f = np.zeros((h, w))
    for k in range(waves):
        f += amp[k] * np.cos(kx[k] * x + ky[k] * y + ph[k])
    f = 128.0 + 45.0 * f / np.sqrt(0.5 * np.sum(amp ** 2))
    if noise > 0:
        f += noise * np.random.default_rng(100000 + seed * 100 + noise_seed).normal(size=f.shape)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


class Pair(NamedTuple):
    name: str
    a: np.ndarray
    b: np.ndarray
    max_levels: int   # the most levels with every level at least 2 x 2
    levels: int       # the level count of the variant tests

    @property
    def w(self):
        return self.a.shape[1]

    @property
    def h(self):
        return self.a.shape[0]


# name -> (w, h, texture seed, warp, shortest / longest wavelength, noise, max levels, levels of the variant tests)
#   small  every level from 2 on is smaller than the 32 x 32 staged window in both axes: stage_windows takes its border path
#   strip  below 32 in one axis only, at every level
#   vga    the ordinary case
#   flow   smooth texture moved by 11 x 9 pixels: the estimate walks out of the staged window inside one level
PAIRS = {"small": (100, 76, 11, (0.6, -0.4), 5.0, 48.0, 1.5, 6, 3), "strip": (300, 24, 12, (0.5, 0.3), 5.0, 48.0, 1.5, 4, 2),
         "vga": (640, 480, 13, (1.3, -0.9), 5.0, 48.0, 1.5, 8, 3), "flow": (160, 120, 14, (11.0, -9.0), 24.0, 90.0, 0.5, 6, 1)}
BELOW_2X2 = ("small", 7)   # level 6 of the small pair is 1 x 1: orc_klt_track defines it (every sample is 0), see the CPU test

_cache: dict = {}


def pair(name) -> Pair:
    if ("pair", name) not in _cache:
        w, h, seed, shift, lo, hi, noise, max_levels, levels = PAIRS[name]
        a = texture(w, h, seed, (0.0, 0.0), noise, 1, lo, hi)
        b = texture(w, h, seed, shift, noise, 2, lo, hi)
        _cache[("pair", name)] = Pair(name, a, b, max_levels, levels)
    return _cache[("pair", name)]


# ---- track populations ----------------------------------------------------------------------------------------------------------
NONFINITE = (1e12, float("inf"), float("-inf"), float("nan"))


def full_mantissa(rng, v):
    """v * (1 + e1) / (1 + e2) with |e| < 2^-12: the products and quotients round, so the low mantissa bits are populated
    (uniform(lo, hi) alone returns multiples of a coarse power of two, and v + d then never rounds)"""
    v = np.asarray(v, np.float64)
    return v * (1.0 + rng.uniform(-1, 1, v.shape) * 2.0 ** -12) / (1.0 + rng.uniform(-1, 1, v.shape) * 2.0 ** -12)


def population(w, h, levels, r, groups=96, seed=0):
    """4 * groups tracks, interleaved so that every group of four consecutive tracks (one K = 4 wave, two K = 2 waves) mixes classes:
      slot 0  interior; every fifth group an exact duplicate of an earlier interior track (class dup)
      slot 1  left band: x * 2^-l in (-r-3, 4) for l = group % levels, every other one in (-1.5, 1.5); y interior   (left{l})
      slot 2  in turn: non-finite (1e12, +-inf, NaN in x, in y, in both), entirely outside, on or beyond the right / bottom border,
              within r + 2 of a power of two
      slot 3  top band, as slot 1 with the axes swapped   (top{l})
    Returns (xy [N][2], labels [N])."""
    rng = np.random.default_rng(1000 * seed + 10 * r + levels)
    m = r + 10.0
    pows = [p for p in (64, 128, 256, 512) if p + r + 2 < w - 1] or [16]
    pows_y = [p for p in (64, 128, 256, 512) if p + r + 2 < h - 1] or [16]

    def interior(n=None):
        return np.stack([rng.uniform(min(m, w / 3), max(w - m, 2 * w / 3), n), rng.uniform(min(m, h / 3), max(h - m, 2 * h / 3), n)], -1)

    def band(g, l):
        lo, hi = (-1.5, 1.5) if (g // levels) % 2 else (-(r + 3.0), 4.0)
        return rng.uniform(lo, hi) * (1 << l)

    xy, labels, interiors, dup_of, nf = [], [], [], {}, 0
    for g in range(groups):
        l = g % levels
        p = interior()
        if g % 5 == 4 and interiors:
            dup_of[len(xy)] = interiors[int(rng.integers(len(interiors)))]
            xy.append(p)
            labels.append("dup")
        else:
            interiors.append(len(xy))
            xy.append(p)
            labels.append("interior")
        q = interior()
        xy.append(np.array([band(g, l), q[1]]))
        labels.append(f"left{l}")
        kind = g % 4
        q = interior()
        if kind == 0:
            v = NONFINITE[nf % 4]
            where = (nf // 4) % 3
            q = np.array([v if where != 1 else q[0], v if where != 0 else q[1]])
            nf += 1
            labels.append("nonfinite")
        elif kind == 1:
            side = (g // 4) % 4
            far = (r + 4.0) * (1 << (levels - 1)) + rng.uniform(8, 300)  # touches nothing at any level
            q = np.array([[-far, q[1]], [w + far, q[1]], [q[0], -far], [q[0], h + far]][side])
            labels.append("outside")
        elif kind == 2:
            if (g // 4) % 2:
                q = np.array([rng.uniform(w - 2.0, w + r + 2.0), q[1]])
            else:
                q = np.array([q[0], rng.uniform(h - 2.0, h + r + 2.0)])
            labels.append("border")
        else:
            if (g // 4) % 2:
                q = np.array([pows[(g // 8) % len(pows)] + rng.uniform(-(r + 2.0), r + 2.0), q[1]])
            else:
                q = np.array([q[0], pows_y[(g // 8) % len(pows_y)] + rng.uniform(-(r + 2.0), r + 2.0)])
            labels.append("pow2")
        xy.append(q)
        q = interior()
        xy.append(np.array([q[0], band(g, l)]))
        labels.append(f"top{l}")
    xy = np.array(xy, np.float64)
    labels = np.array(labels)
    fin = np.isfinite(xy) & (np.abs(xy) < 1e9)
    xy = np.where(fin, full_mantissa(rng, np.where(fin, xy, 1.0)), xy)
    for i, src in dup_of.items():   # an exact duplicate of an earlier interior track
        xy[i] = xy[src]
    return np.ascontiguousarray(xy), labels


def pair_population(name, r, levels=None, groups=96):
    p = pair(name)
    levels = levels or p.levels
    key = ("pop", name, r, levels, groups)
    if key not in _cache:
        _cache[key] = population(p.w, p.h, levels, r, groups, seed=sorted(PAIRS).index(name) + 1)
    return _cache[key]


# ---- the on-grid test of the sample grid, restated (k_klt_track / k_klt_track_multi, csrc/hip/klt.hip) ----------------------------
def off_grid(v, r):
    """For the step coordinate v of one axis: (plus, minus), two bool arrays over d = -r..r.  plus[d + r]: fl(c_d + 1) is not bitwise
    the neighbouring slot fl(v + (d + 1)), with c_d = fl(v + d); minus likewise with fl(c_d - 1) and fl(v + (d - 1)).  The outermost
    neighbours (plus of d = r, minus of d = -r) have slots of their own and are always on the grid."""
    c = float(v) + np.arange(-r, r + 1, dtype=np.float64)
    plus = np.zeros(2 * r + 1, bool)
    minus = np.zeros(2 * r + 1, bool)
    plus[:-1] = (c[:-1] + 1.0).view(np.uint64) != c[1:].view(np.uint64)
    minus[1:] = (c[1:] - 1.0).view(np.uint64) != c[:-1].view(np.uint64)
    return plus, minus


def off_grid_shares(r, lo, hi, n=20000, seed=5):
    """shares of coordinates in (lo, hi) with at least one plus / minus / both-on-one-slot off-grid neighbour"""
    rng = np.random.default_rng(seed)
    v = full_mantissa(rng, rng.uniform(lo, hi, n))
    pm = [off_grid(x, r) for x in v]
    return (float(np.mean([p.any() for p, _ in pm])), float(np.mean([m.any() for _, m in pm])),
            float(np.mean([(p & m).any() for p, m in pm])))


def book_floor(v):
    if not (v > -1.0e9 and v < 1.0e9):
        return FAR
    return math.floor(v)


# ---- the reference side (imported lazily) ----------------------------------------------------------------------------------------
def cpu_pyramid(img, levels):
    """levels of orc_downsample2"""
    import helpers as H
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(1, levels):
        out.append(H.downsample2(H.oracle(), "orc", out[-1]))
    return out


class TrackStats(NamedTuple):
    steps: int
    slow: int            # steps with an off-grid neighbour on either axis (what the kernels count in slow_steps)
    kinds: tuple         # steps with a (plus, minus, both-on-one-slot) neighbour on the x axis, then the same three on the y axis
    max_stagings: int    # the most stagings of the window inside one level
    early: int           # levels left before iters was exhausted
    exhausted: int       # levels that used all iters
    coarse_steps: int    # steps at the coarsest level of the forward pass


def restate_tracks(a, b, levels, r, iters, xy, fb=1.0):
    """track_point forward and backward (T:402-422, 356-362) as a Python loop over orc_lk_step calls -- levels, iterations, the
    hypot(step) < 1e-3 exit, the backward pass from the forward result, keep = !(hypot(back - p0) >= fb) -- with the kernels'
    bookkeeping next to it: the `touches` test, the `covered` rule of the staged window and the on-grid test per step.
    Returns (fwd, back, keep, [TrackStats])."""
    import helpers as H
    lib = H.oracle()
    fn = lib.dll.orc_lk_step
    fn.restype = None
    pa, pb = cpu_pyramid(a, levels), cpu_pyramid(b, levels)
    ptr = [[im.ctypes.data_as(ctypes.c_void_p) for im in pyr] for pyr in (pa, pb)]
    out2 = np.zeros(2)
    out_p = out2.ctypes.data_as(ctypes.c_void_p)
    cr = ctypes.c_int(r)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    n = xy.shape[0]
    fwd, back, keep, stats = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n, np.uint8), []
    with np.errstate(all="ignore"):
        for t in range(n):
            p0x, p0y = float(xy[t, 0]), float(xy[t, 1])
            px, py = p0x, p0y
            steps = slow = max_st = early = exhausted = coarse = 0
            kinds = [0] * 6
            for direction in range(2):
                for l in range(levels - 1, -1, -1):
                    h, w = pa[l].shape
                    cw, ch = ctypes.c_int(w), ctypes.c_int(h)
                    i0, i1 = ptr[direction][l], ptr[1 - direction][l]
                    sc = 1.0 / float(1 << l)
                    plx, ply = px * sc, py * sc
                    dlx = dly = 0.0
                    ox = oy = NO_WINDOW
                    stagings = lsteps = 0
                    left = False
                    for _ in range(iters):
                        x, y = plx + dlx, ply + dly
                        bx, by = book_floor(x), book_floor(y)
                        if (bx + r + 3 >= 0) and (bx - r - 2 < w) and (by + r + 3 >= 0) and (by - r - 2 < h):
                            if not ((bx - r - 2 >= ox) and (bx + r + 3 < ox + KLT_P) and (by - r - 2 >= oy) and (by + r + 3 < oy + KLT_P)):
                                ox, oy = bx - (KLT_P // 2 - 1), by - (KLT_P // 2 - 1)
                                stagings += 1
                            pxm, mxm = off_grid(x, r)
                            pym, mym = off_grid(y, r)
                            k = (pxm.any(), mxm.any(), (pxm & mxm).any(), pym.any(), mym.any(), (pym & mym).any())
                            for i in range(6):
                                kinds[i] += int(k[i])
                            slow += int(any(k))
                        fn(i0, i1, cw, ch, cr, ctypes.c_double(x), ctypes.c_double(y), out_p)
                        sx, sy = float(out2[0]), float(out2[1])
                        dlx += sx
                        dly += sy
                        lsteps += 1
                        if np.hypot(sx, sy) < 1e-3:
                            left = True
                            break
                    steps += lsteps
                    max_st = max(max_st, stagings)
                    if iters > 0:
                        if left and lsteps < iters:
                            early += 1
                        elif lsteps == iters and not left:
                            exhausted += 1
                    if direction == 0 and l == levels - 1:
                        coarse = lsteps
                    px, py = (plx + dlx) * float(1 << l), (ply + dly) * float(1 << l)
                if direction == 0:
                    fwd[t] = px, py
            back[t] = px, py
            keep[t] = 0 if np.hypot(px - p0x, py - p0y) >= fb else 1
            stats.append(TrackStats(steps, slow, tuple(kinds), max_st, early, exhausted, coarse))
    return fwd, back, keep, stats


def restated(name, r, levels=None, iters=6, fb=1.0, groups=96):
    """restate_tracks on the pair's interleaved population, computed once"""
    p = pair(name)
    levels = levels or p.levels
    key = ("restated", name, r, levels, iters, repr(float(fb)), groups)
    if key not in _cache:
        xy, _ = pair_population(name, r, levels, groups)
        _cache[key] = restate_tracks(p.a, p.b, levels, r, iters, xy, fb)
    return _cache[key]


def oracle_tracks(name, r, levels=None, iters=6, fb=1.0, groups=96):
    """orc_klt_track on the pair's interleaved population, computed once"""
    import helpers as H
    p = pair(name)
    levels = levels or p.levels
    key = ("oracle", name, r, levels, iters, repr(float(fb)), groups)
    if key not in _cache:
        xy, _ = pair_population(name, r, levels, groups)
        _cache[key] = H.klt_track(H.oracle(), "orc", p.a, p.b, levels, r, iters, xy, fb)
    return _cache[key]


def fb_edge(name, r, levels=None, iters=6):
    """(track, e): a track whose forward-backward error e = hypot(back - p0) lies in (1e-3, 1): fb_thresh = e drops it (e >= e),
    the next double above e keeps it"""
    xy, _ = pair_population(name, r, levels)
    _, back, _ = oracle_tracks(name, r, levels, iters)
    with np.errstate(invalid="ignore"):
        e = np.hypot(back[:, 0] - xy[:, 0], back[:, 1] - xy[:, 1])
        t = int(np.flatnonzero((e > 1e-3) & (e < 1.0))[0])
    return t, float(e[t])


# the (pair, radius) cells of the variant tests
VARIANT_PAIRS = ("small", "vga")
VARIANT_ITERS = 6
RAGGED_N = (1, 2, 3, 4, 5, 7, 63, 64, 65)
FB = (0.0, 5e-324, 1e-3, 1.0, float("inf"), float("nan"))


# ---- score-map images -----------------------------------------------------------------------------------------------------------
SCORE_KINDS = ("noisy", "clean", "quant4", "checker", "lattice", "constant", "corner")
TIE_HEAVY = ("quant4", "checker", "lattice")


def score_image(kind, w, h, seed=3):
    if kind in ("noisy", "clean"):   # two-level blobs (corners and curved edges between flat regions), with and without noise
        f = np.where(texture(w, h, 20 + seed, noise=0.0, lo=10.0, hi=40.0) > 128, 190.0, 60.0)
        if kind == "noisy":
            f += 2.0 * np.random.default_rng(500 + seed).normal(size=f.shape)
        return np.clip(np.rint(f), 0, 255).astype(np.uint8)
    if kind == "quant4":   # four grey levels: large flat regions (score 0), equal scores along the level lines
        return (texture(w, h, 20 + seed, noise=0.0, lo=8.0, hi=32.0) // 64 * 85).astype(np.uint8)
    if kind == "checker":  # period 8 in x, 6 in y: every corner of the board repeats exactly
        y, x = np.mgrid[0:h, 0:w]
        return np.where(((x // 4) + (y // 3)) % 2 == 0, 200, 40).astype(np.uint8)
    if kind == "lattice":  # one 5 x 5 blob per 9 x 7 cell
        y, x = np.mgrid[0:h, 0:w]
        blob = np.array([[0, 20, 40, 20, 0], [20, 90, 140, 90, 20], [40, 140, 220, 140, 40], [20, 90, 140, 90, 20], [0, 20, 40, 20, 0]])
        cx, cy = x % 9, y % 7
        return np.where((cx < 5) & (cy < 5), blob[np.minimum(cy, 4), np.minimum(cx, 4)], 0).astype(np.uint8) + 10
    if kind == "constant":
        return np.full((h, w), 128, np.uint8)
    if kind == "corner":   # one bright quadrant: a single corner (and the edges it leaves at the border band)
        img = np.full((h, w), 30, np.uint8)
        img[h // 2:, w // 2:] = 220
        return img
    raise KeyError(kind)


# (w, h): below the 5 x 5 support of the score, below / on / above the 64 x 32 tile of k_shi_tile and its half-tile shift, widths on the
# 64- and 256-thread row loops, heights where k_row_scan carries (64, 128)
SIZES = ((1, 1), (3, 7), (4, 4), (5, 5), (7, 5), (40, 20), (63, 31), (64, 32), (65, 33), (31, 200), (127, 95), (128, 64), (129, 65),
         (255, 127), (256, 128), (257, 129), (1, 130), (333, 251))
SMALL_SIZES = tuple(s for s in SIZES if s[0] * s[1] <= 65 * 33)
PRUNED_SIZES = ((5, 5), (40, 20), (63, 31), (64, 32), (65, 33), (96, 48), (97, 49), (127, 95), (129, 65), (333, 251))
MIN_DIST = (1, 2, 8, 16)
QUALITY = (0.0, 0.01, 1.0, 1.5)
SHI_MODES = (None, "tile,2", "tile,5", "sweeps")
TRACKER_SIZES = ((65, 33), (127, 95), (333, 251), (40, 20))


def oracle_score(img):
    import helpers as H
    h, w = img.shape
    exp = np.zeros((h, w))
    H.oracle().call("orc_shi_score", None, H.u8(img), w, h, exp)
    return exp


def oracle_candidates(img, quality):
    """(score map, ys, xs) of the candidates in row-major order: score >= max * quality (T:274-285)"""
    exp = oracle_score(img)
    yy, xx = np.nonzero(exp >= exp.max() * quality)
    return exp, yy, xx


def oracle_pick(img, quality, min_dist):
    """the greedy pick without a cap on the corners, as linear indices y * w + x (a set)"""
    import helpers as H
    h, w = img.shape
    pts = H.shi_tomasi(H.oracle(), "orc", img, w * h, quality, min_dist)
    return set((pts[:, 1].astype(np.int64) * w + pts[:, 0].astype(np.int64)).tolist())


def tie_share(img, quality, min_dist):
    """share of the candidates that have another candidate of exactly their score within min_dist (dx^2 + dy^2 < min_dist^2)"""
    exp, yy, xx = oracle_candidates(img, quality)
    h, w = exp.shape
    cand = np.zeros((h, w), bool)
    cand[yy, xx] = True
    tied = np.zeros((h, w), bool)
    R = min_dist - 1
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if (dx or dy) and dx * dx + dy * dy < min_dist * min_dist:
                ys, yd = slice(max(0, dy), h + min(0, dy)), slice(max(0, -dy), h + min(0, -dy))
                xs, xd = slice(max(0, dx), w + min(0, dx)), slice(max(0, -dx), w + min(0, -dx))
                tied[yd, xd] |= cand[yd, xd] & cand[ys, xs] & (exp[yd, xd] == exp[ys, xs])
    return float(tied[yy, xx].mean()) if len(yy) else 0.0
