"""Deterministic inputs for the parameter-range suites of the stereo and fusion kernels (tests/test_gpu_stereo_range.py,
tests/test_gpu_fusion_range.py) and the tables of their cases.  No files, no device: tests/test_range_inputs_cpu.py runs the
NumPy restatements on every generator and asserts the properties of the inputs that the GPU cases rely on (a winner in every
lane group, exact ties, every triangle-table row), so that no GPU case can pass on an empty result.
"""
from __future__ import annotations

import numpy as np

import fusion_ref as FR

IDENTITY = np.eye(3)


# ---- stereo: images ---------------------------------------------------------------------------------------------------
def texture(h, w, seed):
    """a lightly blurred random texture, u8 [h][w]: uniform noise under a 3 x 3 box filter (integer arithmetic)"""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 256, (h + 2, w + 2)).astype(np.int64)
    acc = sum(n[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((acc + 4) // 9).astype(np.uint8)


def band_rows(h, n, k):
    """rows [y0, y1) of band k of n in an image of h rows"""
    return k * h // n, (k + 1) * h // n


def shifted_band_pair(h, w, bands, seed=0):
    """(left, right): right is the texture, left is the texture shifted right by bands[k] pixels in horizontal band k, so the
    true disparity of band k is bands[k].  The columns a shift uncovers hold more of the same texture."""
    pad = max(bands)
    T = texture(h, w + pad, seed)
    right = np.ascontiguousarray(T[:, pad:pad + w])
    left = np.empty_like(right)
    for k, d in enumerate(bands):
        y0, y1 = band_rows(h, len(bands), k)
        left[y0:y1] = T[y0:y1, pad - d:pad - d + w]
    return left, right


def lane_bands(D):
    """true disparities that put winners into every lane group of k_st_path / k_st_select (lane l holds l K .. l K + K - 1,
    K = ceil(D / 64)): 1, just below and just above every multiple of 64 below D, and D - 2 (in the last, partly filled lane)"""
    b = [1]
    for m in range(64, D, 64):
        b += [m - 1, m + 1]
    return tuple(b + [D - 2])


def band_hits(d16, bands, radius):
    """per band: (columns left of it, share of the band's pixels with x >= band + radius whose disparity is within one pixel)"""
    h, w = d16.shape
    out = []
    for k, d in enumerate(bands):
        y0, y1 = band_rows(h, len(bands), k)
        part = d16[y0:y1, d + radius:].astype(np.int64)
        out.append((w - d, float(((part != -16) & (np.abs(part - 16 * d) < 16)).mean()) if part.size else 0.0))
    return out


def constant_image(h, w):
    return np.full((h, w), 128, np.uint8)


def stripes_image(h, w):
    """vertical stripes of period 8: an exact tie at every disparity that is a multiple of 8"""
    return np.ascontiguousarray(np.broadcast_to(np.where(np.arange(w) % 8 < 4, 60, 200).astype(np.uint8), (h, w)))


def checker_image(h, w):
    """a two-level checkerboard of 4 x 4 cells: exact ties at every multiple of 8"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x // 4) + (y // 4)) % 2 == 0, 60, 200).astype(np.uint8)


def noise_pair(h, w, seed=0):
    """two unrelated noise images: nothing matches, the uniqueness and left-right tests decide every pixel"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w)).astype(np.uint8), rng.integers(0, 256, (h, w)).astype(np.uint8)


TIE_IMAGES = dict(constant=constant_image, stripes=stripes_image, checker=checker_image)
FAR = np.array([[1.0, 0.0, 1e4], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])  # every sample outside the source: an all-invalid view
LOOSE = dict(uniqueness=0, lr_max_diff=-1, speckle_window=0)


def adversarial_cases(h, w):
    """name -> (left, right, H_l, H_r, parameters).  The three periodic images match at many disparities, but the left-to-right
    path carries the border's cost along the whole row (p1 per disparity step), so their minimum of S is unique and d = 0 wins
    outright.  `blank_right` is the exact tie: with no valid right census every cost is nbits, S is the same at every disparity
    of every pixel, and the smallest-d rule alone decides the left winner and the right view's.  The noise pair has no true
    match: with the filters on the rejections decide it, with them off its winners spread over all disparities, with exact
    ties between a few of them at a few hundred pixels."""
    I = IDENTITY
    out = {k: (f(h, w), f(h, w), I, I, {}) for k, f in TIE_IMAGES.items()}
    T = texture(h, w, 7)
    out["blank_right"] = (T, T, I, FAR, dict(uniqueness=0))
    a, b = noise_pair(h, w)
    out["noise"] = (a, b, I, I, {})
    out["noise_loose"] = (a, b, I, I, LOOSE)
    return out


def homographies(w, h):
    """name -> H (rectified pixel -> source pixel), used for both views"""
    return dict(
        identity=np.eye(3),
        translation=np.array([[1.0, 0.0, 0.37], [0.0, 1.0, -0.61], [0.0, 0.0, 1.0]]),
        perspective=np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1e-4, -2e-4, 1.0]]),
        pole=np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0 / 40.0, 1.0]]),  # denominator 0 on row 40, negative below
        flip=np.array([[-1.0, 0.0, w - 1.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]]),
        zoom=np.array([[3.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 1.0]]),  # a ninth of the view lies inside the source
    )


# ---- stereo: case tables ------------------------------------------------------------------------------------------------
SWEEP_SHAPE = (96, 320)  # h, w of the D sweep and of the parameter, homography and adversarial cases
# (D, census): K = 1, 2, 3, 4 each meet census 3, 5 and 7
SWEEP = [(16, 3), (48, 5), (64, 7), (80, 3), (80, 5), (128, 7), (144, 5), (176, 3), (192, 7), (208, 5), (256, 7), (256, 3)]
# one parameter away from the defaults at a time, D 128
PARAMS = ([dict(p1=a, p2=b) for a, b in ((1, 2), (8, 9), (1000, 2048))] + [dict(uniqueness=u) for u in (0, 1, 50, 99, 100)]
          + [dict(lr_max_diff=v) for v in (-1, 0, 5)] + [dict(speckle_window=v) for v in (0, 1, 10 ** 6)]
          + [dict(speckle_range=v) for v in (0, 16)])
# name -> (h, w, bands, parameters)
SHAPES = dict(
    w_equals_D=(40, 64, (0, 20, 62), dict(num_disparities=64)),
    w_below_D=(64, 40, (0, 20, 38), dict(num_disparities=64)),
    tall_narrow=(600, 24, (1, 8, 14), dict(num_disparities=16)),
    odd=(37, 157, (1, 65, 126), dict()),
    wide=(40, 1100, (1, 65, 127, 193, 255), dict(num_disparities=256)),
    max_width=(16, 4096, (1, 15), dict(num_disparities=16)),
)
# smaller than the census window: every pixel invalid, S still defined
NO_WINDOW = dict(tiny=(4, 4, dict(num_disparities=16, census=5)), one_row=(1, 300, dict(census=5)))
FLAT_VGA = (480, 640, (40,))  # one constant disparity: a single speckle component of about 300 000 pixels


def sweep_pair(D):
    h, w = SWEEP_SHAPE
    bands = lane_bands(D)
    return (*shifted_band_pair(h, w, bands, seed=D), bands)


# ---- fusion -------------------------------------------------------------------------------------------------------------
SLAB_VOL = dict(origin=(-0.09, -0.05, -0.03), voxel=0.005, dims=(37, 21, 13))
SLAB_TRUNC = 0.05  # ten voxels: no noise sample is cut off


def vol_centre(origin, voxel, dims):
    return np.asarray(origin, np.float64) + 0.5 * float(voxel) * (np.asarray(dims, np.float64) - 1.0)


def noise_disp16(cam, w, h, z_lo, z_hi, seed, invalid=0.03, zero=0.01, extra=()):
    """a noise map rint(16 f B / Z) with Z uniform per pixel in [z_lo, z_hi); a share `invalid` of the pixels is -16, a share
    `zero` is 0, and every value of `extra` replaces a further 0.5 %"""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(z_lo, z_hi, (h, w))
    d16 = np.rint(16.0 * cam["f"] * cam["B"] / Z).astype(np.int16)
    r = rng.random((h, w))
    lo = 0.0
    for share, val in [(invalid, -16), (zero, 0)] + [(0.005, v) for v in extra]:
        d16[(r >= lo) & (r < lo + share)] = val
        lo += share
    return d16


def slab_view(origin, voxel, dims, axis=2, sign=-1, dist=0.5, w=320, h=240, f=600.0, seed=0, **noise):
    """(cam, disp16): a camera `dist` in front of the volume's face, looking along `axis` (from the `sign` side) at the volume's
    centre, and a noise map over the volume's depth range"""
    depth = float(voxel) * (dims[axis] - 1)
    target = vol_centre(origin, voxel, dims)
    centre = target.copy()
    centre[axis] += sign * (0.5 * depth + dist)
    cam = FR.look_at_cam(centre, target, f, w, h)
    return cam, noise_disp16(cam, w, h, dist, dist + depth, seed, **noise)


def inside_view(vol=SLAB_VOL, w=320, h=240, f=100.0, seed=51):
    """a camera at the volume's centre looking along +z: q2 <= 0 for the half of the volume behind it"""
    c = vol_centre(**vol)
    cam = FR.look_at_cam(c, c + np.array([0.0, 0.0, 1.0]), f, w, h, B=0.002)
    return cam, noise_disp16(cam, w, h, 0.004, 0.5 * vol["voxel"] * (vol["dims"][2] - 1), seed)


def away_view(vol=SLAB_VOL, w=320, h=240, f=600.0, seed=52):
    """the front slab camera turned round: q2 <= 0 for every grid point"""
    cam, d16 = slab_view(**vol, w=w, h=h, f=f, seed=seed)
    return dict(cam, R_rw=-np.asarray(cam["R_rw"])), d16


def border_view(vol=SLAB_VOL, seed=53):
    """a slab camera whose 160 x 100 image is smaller than the volume's projection (216 x 120): all four borders cut through it"""
    return slab_view(**vol, w=160, h=100, seed=seed)


def slab_views3(vol=SLAB_VOL, **kw):
    """three slab views from different seeds and positions (front, back and a side)"""
    return [slab_view(**vol, axis=2, sign=-1, seed=1, **kw), slab_view(**vol, axis=2, sign=1, seed=2, **kw),
            slab_view(**vol, axis=1, sign=-1, seed=3, **kw)]


def mixed_size_views(vol=SLAB_VOL):
    """slab views of 40 x 30, 640 x 480 and 320 x 240 pixels, one focal length each so that every one spans the volume"""
    return [slab_view(**vol, w=40, h=30, f=75.0, seed=11), slab_view(**vol, w=640, h=480, f=1200.0, seed=12, sign=1),
            slab_view(**vol, w=320, h=240, f=600.0, seed=13, axis=1)]


def fuse_ref(vol, views, **kw):
    """fusion_ref.fuse on a volume dict; a disparity of 0 under disp_min <= 0 divides by zero on purpose (Z = +inf)"""
    with np.errstate(divide="ignore"):
        return FR.fuse(vol["origin"], vol["voxel"], vol["dims"], views, **kw)


def table_coverage(sum_, count, min_weight=1):
    """(corner configurations, (tetrahedron, case) pairs) that occur among the meshed cells; 256 and 6 x 16 = 96 at most"""
    S = FR.values(sum_, count, min_weight)
    c = np.stack([S[(b >> 2) & 1:S.shape[0] - 1 + ((b >> 2) & 1), (b >> 1) & 1:S.shape[1] - 1 + ((b >> 1) & 1),
                    (b & 1):S.shape[2] - 1 + (b & 1)].ravel() for b in range(8)], 1)
    c = c[~np.isnan(c).any(1)]
    inside = c < 0
    configs = set(np.unique((inside.astype(np.int64) << np.arange(8)).sum(1)).tolist())
    pairs = set()
    for t, chain in enumerate(FR.tets()):
        case = sum(inside[:, chain[q]].astype(np.int64) << q for q in range(4))
        pairs |= {(t, int(cs)) for cs in np.unique(case)}
    return configs, pairs


# name -> (dims, voxel, list of slab_view keywords, trunc): volume shapes around the 64 x 4 blocks of the integration and
# the 1 024-element blocks of the scans; every camera looks along the volume's shortest axis, or there are several
BLOCK_SHAPES = dict(
    s65x5x3=((65, 5, 3), 0.005, [dict(axis=2, seed=21), dict(axis=1, seed=22)], SLAB_TRUNC),
    s63x3x2=((63, 3, 2), 0.005, [dict(axis=2, seed=23), dict(axis=1, seed=24)], SLAB_TRUNC),
    s64x4x2=((64, 4, 2), 0.005, [dict(axis=2, seed=25), dict(axis=1, seed=26)], SLAB_TRUNC),
    s130x9x2=((130, 9, 2), 0.005, [dict(axis=2, seed=27, f=300.0), dict(axis=2, sign=1, seed=28, f=300.0)], SLAB_TRUNC),
    s2x3x129=((2, 3, 129), 0.005, [dict(axis=0, seed=29, f=300.0), dict(axis=1, seed=30, f=300.0)], SLAB_TRUNC),
    s129x2x2=((129, 2, 2), 0.005, [dict(axis=2, seed=31, f=300.0), dict(axis=1, seed=32, f=300.0)], SLAB_TRUNC),
    s32x16x2=((32, 16, 2), 0.005, [dict(axis=2, seed=33)], SLAB_TRUNC),  # 1 024 points
    s41x25x2=((41, 25, 2), 0.005, [dict(axis=2, seed=34)], SLAB_TRUNC),  # 2 050 points: two scan blocks and two more
    s41x5x5=((41, 5, 5), 0.005, [dict(axis=2, seed=35), dict(axis=1, seed=36)], SLAB_TRUNC),  # 1 025 points
)
# 1 024^2 grid points and one slice more, at 1 mm: one VGA slab view; large outputs
BIG_SHAPES = dict(
    s128x128x64=((128, 128, 64), 0.001, [dict(axis=2, seed=41, w=640, h=480, f=1200.0)], 0.1),
    s128x128x65=((128, 128, 65), 0.001, [dict(axis=2, seed=42, w=640, h=480, f=1200.0)], 0.1),
)


def shape_case(dims, voxel, cams, trunc):
    """(vol, views, trunc) of a BLOCK_SHAPES / BIG_SHAPES entry; the volume is centred on the origin"""
    origin = tuple(-0.5 * voxel * (n - 1) for n in dims)
    vol = dict(origin=origin, voxel=voxel, dims=dims)
    return vol, [slab_view(**vol, **kw) for kw in cams], trunc
