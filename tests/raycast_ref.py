"""NumPy restatement of TSDF ray casting ("Rendering the volume"), written from the definition, not from the
kernel.  The volume, s(g) and "defined" come from fusion_ref, the gradient G from appearance_ref.

Two forms of the same definition:
 * brute()  evaluates every sample k = 0 .. K-1 of every ray and clips nothing;
 * render() finds per ray the run of samples that are inside the grid by bisection on the sample index (the grid coordinate of
   a sample is a monotone function of k in floating point, so that run is one interval) and marches only through it.
All arithmetic is IEEE double in the definition's expression order.  The device results must equal brute() bit for bit.
"""
from __future__ import annotations

import numpy as np

import appearance_ref as AR
import fusion_ref as FR

K_MAX, W_MAX, WH_MAX = 1 << 20, 4096, 1 << 24


def sample_count(z_min, z_max, step):
    return int(np.floor((float(z_max) - float(z_min)) / float(step))) + 1


def resolve_step(voxel, step=0.0):
    return float(voxel) / 2.0 if step == 0.0 else float(step)


def rays(cam, w, h):
    """dw [3] of [h][w]: the depth-1 ray of every pixel in world coordinates"""
    R = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
    f, cx, cy = float(cam["f"]), float(cam["cx"]), float(cam["cy"])
    dc0 = np.broadcast_to(((np.arange(w, dtype=np.float64) - cx) / f)[None, :], (h, w))
    dc1 = np.broadcast_to(((np.arange(h, dtype=np.float64) - cy) / f)[:, None], (h, w))
    return [(R[0, a] * dc0 + R[1, a] * dc1) + R[2, a] * 1.0 for a in range(3)]


class Volume:
    """s(g), defined(g) and G(g) of a sum / count volume"""

    def __init__(self, sum_, count, origin, voxel, min_weight=1):
        self.S = FR.values(np.asarray(sum_, np.float64), np.asarray(count, np.int32), min_weight)
        self.defined = np.asarray(count) >= min_weight
        self.nz, self.ny, self.nx = self.S.shape
        self.n = (self.nx, self.ny, self.nz)
        self.origin = [float(v) for v in origin]
        self.voxel = float(voxel)
        self.inv = 1.0 / self.voxel
        self._G = None

    @property
    def G(self):
        if self._G is None:
            self._G = AR.gradient(np.where(self.defined, self.S, np.nan))[0]
        return self._G

    def grid(self, P):
        """g [3] of the points P [3]"""
        return [(P[a] - self.origin[a]) * self.inv for a in range(3)]

    def inside(self, g):
        ok = np.ones(np.shape(g[0]), bool)
        for a in range(3):
            ok &= (0.0 <= g[a]) & (g[a] < float(self.n[a] - 1))
        return ok

    def interp(self, fields, g):
        """(defined, [value per field]) at grid coordinates g (1-D arrays): inside and all 8 corners defined; the lerp order of
        the definition (x, then y, then z)"""
        ok = self.inside(g)
        idx = np.nonzero(ok)[0]
        i = [np.floor(g[a][idx]).astype(np.int64) for a in range(3)]
        f = [g[a][idx] - i[a].astype(np.float64) for a in range(3)]
        corner_ok = np.ones(len(idx), bool)
        for b in range(8):
            corner_ok &= self.defined[i[2] + ((b >> 2) & 1), i[1] + ((b >> 1) & 1), i[0] + (b & 1)]
        idx, i, f = idx[corner_ok], [v[corner_ok] for v in i], [v[corner_ok] for v in f]
        ok = np.zeros(len(g[0]), bool)
        ok[idx] = True
        out = []
        for F in fields:
            c = {(bx, by, bz): F[i[2] + bz, i[1] + by, i[0] + bx] for bx in (0, 1) for by in (0, 1) for bz in (0, 1)}

            def lerp(p, q, t):
                return p + t * (q - p)
            c00, c10 = lerp(c[0, 0, 0], c[1, 0, 0], f[0]), lerp(c[0, 1, 0], c[1, 1, 0], f[0])
            c01, c11 = lerp(c[0, 0, 1], c[1, 0, 1], f[0]), lerp(c[0, 1, 1], c[1, 1, 1], f[0])
            c0, c1 = lerp(c00, c10, f[1]), lerp(c01, c11, f[1])
            v = np.zeros(len(g[0]))
            v[idx] = lerp(c0, c1, f[2])
            out.append(v)
        return ok, out


def _finish(vol, cam, dw, hit, depth, background):
    """points, normals, shaded and hits from the hit mask and depth (flat arrays)"""
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    n = len(depth)
    points, normals, shaded = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, int(background), np.uint8)
    idx = np.nonzero(hit)[0]
    d = [v[idx] for v in dw]
    P = [c[a] + depth[idx] * d[a] for a in range(3)]
    ok, N = vol.interp([vol.G[0], vol.G[1], vol.G[2]], vol.grid(P))
    N = [np.where(ok, v, 0.0) for v in N]
    ln = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
    with np.errstate(invalid="ignore", divide="ignore"):
        nr = [np.where(ln > 0, N[a] / ln, 0.0) for a in range(3)]
    L = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    lam = -(((nr[0] * d[0] + nr[1] * d[1]) + nr[2] * d[2]) / L)
    sh = np.where(lam > 0, np.minimum(255.0, np.floor(lam * 255.0 + 0.5)), 0.0).astype(np.uint8)
    for a in range(3):
        points[idx, a] = P[a]
        normals[idx, a] = nr[a]
    shaded[idx] = sh
    return points, normals, shaded, ok


def _march(vol, cam, w, h, z_min, z_max, step, background, k_lo, k_hi):
    """the definition over the samples k_lo[ray] <= k < k_hi[ray] of every ray (flat int arrays)"""
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    dw = [v.ravel() for v in rays(cam, w, h)]
    n = w * h
    depth, hit = np.zeros(n), np.zeros(n, bool)
    prev_s, prev_ok = np.zeros(n), np.zeros(n, bool)
    z_min, step = float(z_min), float(step)
    for k in range(int(k_lo.min()) if n else 0, int(k_hi.max()) if n else 0):
        act = np.nonzero((k_lo <= k) & (k < k_hi) & ~hit)[0]
        z = z_min + float(k) * step
        ok, (s,) = vol.interp([vol.S], vol.grid([c[a] + z * dw[a][act] for a in range(3)]))
        if k >= 1:
            cross = ok & prev_ok[act] & (prev_s[act] > 0) & (s <= 0)
            j = act[cross]
            zp = z_min + float(k - 1) * step
            with np.errstate(invalid="ignore", divide="ignore"):
                t = prev_s[j] / (prev_s[j] - s[cross])
            depth[j] = zp + t * (z - zp)
            hit[j] = True
        # a ray that is not active at k has an undefined sample there
        prev_ok[:] = False
        prev_ok[act] = ok
        prev_s[act] = s
    points, normals, shaded, n_ok = _finish(vol, cam, dw, hit, depth, background)
    out = dict(depth=depth.reshape(h, w), normals=normals.reshape(h, w, 3), points=points.reshape(h, w, 3), shaded=shaded.reshape(h, w),
               hits=int(hit.sum()), hit=hit.reshape(h, w))
    out["normal_defined"] = np.zeros(n, bool)
    out["normal_defined"][np.nonzero(hit)[0]] = n_ok
    out["normal_defined"] = out["normal_defined"].reshape(h, w)
    return out


def _args(sum_, count, origin, voxel, cam, w, h, z_min, z_max, step, min_weight):
    step = resolve_step(voxel, step)
    K = sample_count(z_min, z_max, step)
    assert z_min > 0 and z_max > z_min and 1 <= K <= K_MAX and 1 <= w <= W_MAX and h >= 1 and w * h <= WH_MAX
    return Volume(sum_, count, origin, voxel, max(int(min_weight), 1)), step, K


def brute(sum_, count, origin, voxel, cam, w, h, z_min, z_max, step=0.0, min_weight=1, background=0):
    """every k of every ray.  dict(depth [h][w], normals [h][w][3], points [h][w][3], shaded u8 [h][w], hits, hit [h][w] bool,
    normal_defined [h][w] bool (the interpolated gradient exists at the hit point))"""
    vol, step, K = _args(sum_, count, origin, voxel, cam, w, h, z_min, z_max, step, min_weight)
    n = w * h
    return _march(vol, cam, w, h, z_min, z_max, step, background, np.zeros(n, np.int64), np.full(n, K, np.int64))


def inside_run(vol, cam, w, h, z_min, step, K):
    """(k_lo, k_hi) per ray: the samples with k_lo <= k < k_hi are exactly the ones inside the grid.  Per axis the grid
    coordinate of sample k is a monotone function of k (each of its operations rounds monotonically), so "below the lower face"
    and "at or above the upper face" are each a prefix or a suffix of 0 .. K-1, found by bisection."""
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    dw = [v.ravel() for v in rays(cam, w, h)]
    n = w * h
    z_min, step = float(z_min), float(step)

    def g_of(a, k):
        return ((c[a] + (z_min + k.astype(np.float64) * step) * dw[a]) - vol.origin[a]) * vol.inv

    def first_true(pred):
        """smallest k in [0, K] with pred(k), for a predicate that is false then true along k (K if never)"""
        lo, hi = np.zeros(n, np.int64), np.full(n, K, np.int64)
        while (lo < hi).any():
            mid = (lo + hi) // 2
            p = pred(np.minimum(mid, K - 1)) & (mid < K)
            go = lo < hi
            hi = np.where(go & p, mid, hi)
            lo = np.where(go & ~p, mid + 1, lo)
        return lo

    k_lo, k_hi = np.zeros(n, np.int64), np.full(n, K, np.int64)
    for a in range(3):
        top = float(vol.n[a] - 1)
        up, down = dw[a] > 0, dw[a] < 0
        flat = ~up & ~down
        g0 = g_of(a, np.zeros(n, np.int64))
        out_flat = flat & ~((0.0 <= g0) & (g0 < top))
        # rising coordinate: inside from the first k with g >= 0 up to the first k with g >= top; falling: the mirror image
        enter = np.where(up, first_true(lambda k: g_of(a, k) >= 0.0), np.where(down, first_true(lambda k: g_of(a, k) < top), 0))
        leave = np.where(up, first_true(lambda k: g_of(a, k) >= top), np.where(down, first_true(lambda k: g_of(a, k) < 0.0), K))
        k_lo = np.maximum(k_lo, np.where(out_flat, K, enter))
        k_hi = np.minimum(k_hi, np.where(out_flat, 0, leave))
    return k_lo, np.maximum(k_hi, k_lo)


def render(sum_, count, origin, voxel, cam, w, h, z_min, z_max, step=0.0, min_weight=1, background=0):
    """brute()'s result from the samples inside the grid alone"""
    vol, step, K = _args(sum_, count, origin, voxel, cam, w, h, z_min, z_max, step, min_weight)
    k_lo, k_hi = inside_run(vol, cam, w, h, z_min, step, K)
    return _march(vol, cam, w, h, z_min, z_max, step, background, k_lo, k_hi)


def same(a, b):
    """bit equality of two results"""
    return (a["hits"] == b["hits"] and a["shaded"].tobytes() == b["shaded"].tobytes()
            and all(a[k].shape == b[k].shape and a[k].view(np.uint64).tobytes() == b[k].view(np.uint64).tobytes()
                    for k in ("depth", "normals", "points")))


# ---- test scenes -------------------------------------------------------------------------------------------------------------
# the novel camera of the sphere fixture (test_fusion_cpu: 26 views, 61^3 at 5 mm): 341 samples per ray
SPHERE_CAM = dict(pos=(0.31, 0.22, -0.33), f=300.0, w=160, h=160)
SPHERE_MARCH = dict(z_min=0.05, z_max=0.9, step=0.0025)
# the calibration's conditions need a camera none of whose silhouette rays grazes the surface from behind
CALIB_POS = (0.0, 0.0, -0.5)


def camera(pos, target, f, w, h, cx=None, cy=None):
    """fusion_ref.look_at_cam with its image size in the dict, as capi.Raycast.render takes it"""
    cam = FR.look_at_cam(pos, target, f, w, h)
    cam.update(w=int(w), h=int(h))
    if cx is not None:
        cam.update(cx=float(cx), cy=float(cy))
    return cam


def axis_camera(c, f, w, h, cx, cy):
    """R_rw = I: the optical axis is +z of the world"""
    return dict(R_rw=np.eye(3), c_left=np.asarray(c, np.float64), f=float(f), cx=float(cx), cy=float(cy), B=0.0, w=int(w), h=int(h))


_sphere = {}


def sphere_volume():
    """(sum, count, vol) of the sphere fixture, integrated once"""
    if not _sphere:
        from test_fusion_cpu import SPHERE, VOL, sphere_views
        s, c = FR.integrate(VOL["origin"], VOL["voxel"], VOL["dims"], sphere_views(**SPHERE))
        s.setflags(write=False)
        c.setflags(write=False)
        _sphere.update(sum=s, count=c, vol=VOL, radius=SPHERE["radius"])
    return _sphere


def random_volume(dims, seed, undefined=0.3):
    """uniform sum in [-1, 1], `undefined` of the counts 0 and the others 1: defined and undefined cells interleave"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    s = rng.uniform(-1.0, 1.0, (nz, ny, nx))
    c = (rng.random((nz, ny, nx)) >= undefined).astype(np.int32)
    return s, c


RANDOM_VOXEL = 0.01


RANDOM_STEPS = (0.0, 0.0125)  # voxel / 2 and 1.25 voxels
RANDOM_SEEDS = (0, 1)


def random_case(dims, seed, step=0.0, w=64, h=48):
    """a random volume at the origin and a camera outside it that looks along its longest axis, obliquely, zoomed so that most
    rays cross it: (sum, count, origin, voxel, cam, march).  About 6 % of the cells have all 8 corners defined, so a ray meets
    short runs of defined samples between undefined ones."""
    s, c = random_volume(dims, seed)
    ext = (np.asarray(dims, np.float64) - 1.0) * RANDOM_VOXEL
    centre = ext / 2.0
    off = np.array([-(ext[0] / 2.0 + 0.05), 0.02, -0.04])
    cam = camera(centre + off, centre, 0.9 * np.linalg.norm(off) * w / min(ext.max(), 0.16), w, h)
    return s, c, (0.0, 0.0, 0.0), RANDOM_VOXEL, cam, dict(z_min=0.02, z_max=0.9, step=step)
