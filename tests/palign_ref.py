"""NumPy restatement of the direct photometric alignment of a camera to the textured mesh ("Registering a camera
to the textured mesh"), written from the definition, not from the kernels.  The key image and the winners' t and s are
photo_ref's (raster_ref's contest of the whole mesh at cull = 0), the layout texture_ref's, the ordered sum, the 6 x 6 Cholesky
solve and the Cayley update align_ref's.  All arithmetic is IEEE double in the definition's expression order; the only library
function is sqrt.  The device results must equal these bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

import align_ref as AL
import photo_ref as PH
import raster_ref as R

DEFAULTS = dict(max_iters=10, stride=1, margin=4, min_pixels=64, r_max=255.0, damping=0.0, eps_rot=5e-5, eps_trans=1e-6)
CONVERGED, MAX_ITERS, TOO_FEW, DEGENERATE = range(4)
TERMS = 28
MARGIN_CAP = 64
ordered_sum = AL.ordered_sum  # the same function: the tree is the view alignment's


def check_params(z_min=0.0, pivot=(0.0, 0.0, 0.0), max_iters=10, stride=1, margin=4, min_pixels=64, r_max=255.0, damping=0.0, eps_rot=5e-5,
                 eps_trans=1e-6):
    fin = math.isfinite
    return bool(fin(z_min) and z_min > 0 and all(fin(float(v)) for v in pivot) and 1 <= max_iters <= 64 and stride >= 1
                and 1 <= margin <= MARGIN_CAP and min_pixels >= 1 and fin(r_max) and r_max >= 0 and fin(damping) and damping >= 0
                and fin(eps_rot) and eps_rot >= 0 and fin(eps_trans) and eps_trans >= 0)


def model(verts, faces, tex, atlas=None):
    """the model of a run: the mesh, the texture result (texture_ref.run's dict or the device's) and the atlas that is read (tex's,
    or the levelled one); ValueError for sfmx_palign_set_model's refusals"""
    if tex is None:
        raise ValueError("the texture needs a successful run")
    X = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    fview, uvh = np.asarray(tex["face_view"]), np.asarray(tex["uv_half"])
    W, H = int(tex["W"]), int(tex["H"])
    if len(fview) != len(F) or ("n" in tex and int(tex["n"]) != len(X)):
        raise ValueError("the mesh of the texture's run")
    A = np.asarray(tex["atlas"] if atlas is None else atlas, np.uint8)
    if A.shape != (H, W):
        raise ValueError("the levelled atlas has another size")
    if ((F < 0) | (F >= len(X))).any():
        raise ValueError("a face index outside [0, n)")
    return dict(X=X, F=F, fview=fview, uvh=uvh, A=A)


def ok_mask(M, cam, z_min, brute=False):
    """(ok bool [h][w], the winners of the hit pixels as photo_ref._winners gives them, the projection)"""
    w, h = int(cam["w"]), int(cam["h"])
    pr, keys = PH.key_image(M["X"], M["F"], cam, z_min, brute)
    win = PH._winners(M["F"], pr, keys, w)
    px, fw, back = win[0], win[1], win[2]
    ok = np.zeros(w * h, bool)
    ok[px] = ~back & (M["fview"][fw] >= 0) if len(px) else False
    return ok.reshape(h, w), win, pr


def candidates(ok, margin):
    """bool [h][w]: ok at every pixel within `margin` in x and in y; a pixel outside the image is not ok.  Rows, then columns."""
    ok = np.asarray(ok, bool)
    h, w = ok.shape
    m = int(margin)
    P = np.zeros((h, w + 2 * m), bool)
    P[:, m:m + w] = ok
    rows = np.ones((h, w), bool)
    for d in range(2 * m + 1):
        rows &= P[:, d:d + w]
    P = np.zeros((h + 2 * m, w), bool)
    P[m:m + h] = rows
    out = np.ones((h, w), bool)
    for d in range(2 * m + 1):
        out &= P[d:d + h]
    return out


def atlas_g(t, s, uvh, atlas):
    """photo_ref.lookup's g before its rounding: the same expression in the same order"""
    Af = np.asarray(atlas, np.uint8).astype(np.float64)
    H, W = Af.shape
    h = np.asarray(uvh, np.int32).astype(np.float64)
    hx = ((t[0] * h[:, 0, 0] + t[1] * h[:, 1, 0]) + t[2] * h[:, 2, 0]) / s
    hy = ((t[0] * h[:, 0, 1] + t[1] * h[:, 1, 1]) + t[2] * h[:, 2, 1]) / s
    a, b = hx * 0.5 - 0.5, hy * 0.5 - 0.5
    ac, bc = np.minimum(np.maximum(a, 0.0), float(W - 1)), np.minimum(np.maximum(b, 0.0), float(H - 1))
    x0, y0 = np.floor(ac), np.floor(bc)
    fx, fy = ac - x0, bc - y0
    xi0, yi0 = x0.astype(np.int64), y0.astype(np.int64)
    xi1, yi1 = np.minimum(xi0 + 1, W - 1), np.minimum(yi0 + 1, H - 1)
    top = (1.0 - fx) * Af[yi0, xi0] + fx * Af[yi0, xi1]
    bot = (1.0 - fx) * Af[yi1, xi0] + fx * Af[yi1, xi1]
    return (1.0 - fy) * top + fy * bot


def jacobian(Gx, Gy, x, y, z, cam, pivot):
    """(J [6], X [3]) of samples at pixel centres (x, y) (float arrays) with depth z and picture gradient (Gx, Gy)"""
    R_ = np.asarray(cam["R_rw"], np.float64).reshape(3, 3)
    c = np.asarray(cam["c_left"], np.float64).reshape(3)
    f, cx, cy = float(cam["f"]), float(cam["cx"]), float(cam["cy"])
    p = [float(v) for v in pivot]
    dx, dy = (x - cx) / f, (y - cy) / f
    q = [dx * z, dy * z, z]
    iz = 1.0 / z
    a0, a1 = (Gx * f) * iz, (Gy * f) * iz
    a2 = -((a0 * dx) + (a1 * dy))
    gw = [(a0 * R_[0, b] + a1 * R_[1, b]) + a2 * R_[2, b] for b in range(3)]
    X = [c[b] + ((R_[0, b] * q[0] + R_[1, b] * q[1]) + R_[2, b] * q[2]) for b in range(3)]
    Q = [X[b] - p[b] for b in range(3)]
    J = [Q[2] * gw[1] - Q[1] * gw[2], Q[0] * gw[2] - Q[2] * gw[0], Q[1] * gw[0] - Q[0] * gw[1], -gw[0], -gw[1], -gw[2]]
    return J, X


def rows(M, cam, image, z_min, pivot, stride=1, margin=4, r_max=255.0, brute=False):
    """(state u8 [nsy][nsx]: 0 not a candidate, 1 trimmed, 2 used; J [6] of [nsy][nsx]; r [nsy][nsx]): J is 0 where the sample is
    not used, r is 0 where it is not a candidate"""
    I = np.asarray(image, np.uint8)
    h, w = I.shape
    assert (int(cam["w"]), int(cam["h"])) == (w, h)
    ok, (px, fw, back, t, s), pr = ok_mask(M, cam, z_min, brute)
    cand = candidates(ok, margin)
    nsx, nsy = AL.sample_grid(w, h, stride)
    ys, xs = np.meshgrid(np.arange(nsy, dtype=np.int64) * stride, np.arange(nsx, dtype=np.int64) * stride, indexing="ij")
    flat = (ys * w + xs).ravel()
    hit_of = np.full(w * h, -1, np.int64)
    hit_of[px] = np.arange(len(px))
    sel = np.nonzero(cand.ravel()[flat])[0]  # the candidate samples
    k = hit_of[flat[sel]]
    assert (k >= 0).all()
    state = np.zeros(nsy * nsx, np.uint8)
    r = np.zeros(nsy * nsx)
    J = [np.zeros(nsy * nsx) for _ in range(6)]
    if len(sel):
        x, y = xs.ravel()[sel], ys.ravel()[sel]
        f = fw[k]
        _, _, U, V, _ = pr
        Uf, Vf = U[M["F"][f]], V[M["F"][f]]
        A = (Uf[:, 1] - Uf[:, 0]) * (Vf[:, 2] - Vf[:, 0]) - (Vf[:, 1] - Vf[:, 0]) * (Uf[:, 2] - Uf[:, 0])
        If = I.astype(np.float64)
        with np.errstate(all="ignore"):
            g = atlas_g([ti[k] for ti in t], s[k], M["uvh"][f], M["A"])
            z = np.abs(A).astype(np.float64) / s[k]
            rr = If[y, x] - g
            used = np.abs(rr) <= float(r_max)  # false for a NaN
            Gx = 0.5 * (If[y, x + 1] - If[y, x - 1])
            Gy = 0.5 * (If[y + 1, x] - If[y - 1, x])
            Jc, _ = jacobian(Gx, Gy, x.astype(np.float64), y.astype(np.float64), z, cam, pivot)
        state[sel] = np.where(used, 2, 1)
        r[sel] = rr
        for m in range(6):
            J[m][sel] = np.where(used, Jc[m], 0.0)
    return state.reshape(nsy, nsx), [v.reshape(nsy, nsx) for v in J], r.reshape(nsy, nsx)


def terms(state, J, r):
    """[28][nsy][nsx]: A_mn (m <= n, row by row), b_m, e; +0.0 where the sample is not used"""
    used = state == 2
    with np.errstate(all="ignore"):
        out = [J[m] * J[n] for m, n in AL.PAIRS] + [J[m] * r for m in range(6)] + [r * r]
    return np.stack([np.where(used, v, 0.0) for v in out])


def system(M, cam, image, z_min, pivot, stride=1, margin=4, r_max=255.0, brute=False, want_rows=False):
    """(sums f64 [28], n) of one evaluation at cam's pose; with want_rows also (state, r)"""
    state, J, r = rows(M, cam, image, z_min, pivot, stride, margin, r_max, brute)
    sums, n = ordered_sum(terms(state, J, r)), int((state == 2).sum())
    return (sums, n, state, r) if want_rows else (sums, n)


def _finite(cam):
    return bool(np.isfinite(np.asarray(cam["R_rw"], np.float64)).all() and np.isfinite(np.asarray(cam["c_left"], np.float64)).all())


def align(M, cam, image, z_min, pivot, max_iters=10, stride=1, margin=4, min_pixels=64, r_max=255.0, damping=0.0, eps_rot=5e-5,
          eps_trans=1e-6, brute=False):
    """the loop: dict(view, status, iterations, trace=[(n, e, |omega|, |v|), ...])"""
    if not check_params(z_min, pivot, max_iters, stride, margin, min_pixels, r_max, damping, eps_rot, eps_trans):
        raise ValueError("parameters")
    p = [float(v) for v in pivot]
    cur, good = dict(cam), dict(cam)
    status, trace = MAX_ITERS, []
    for _ in range(int(max_iters)):
        sums, n = system(M, cur, image, z_min, p, stride, margin, r_max, brute)
        e = float(sums[27])
        if n < min_pixels:
            trace.append((n, e, 0.0, 0.0))
            status, cur = TOO_FEW, good
            break
        delta = AL.solve(sums, damping)
        nxt = AL.update(cur, p, delta) if delta is not None else None
        if nxt is None or not _finite(nxt):  # a refused pivot, or an update that overflowed: no step
            trace.append((n, e, 0.0, 0.0))
            status, cur = DEGENERATE, good
            break
        good, cur = cur, nxt
        rot, tr = AL.norm3(delta[0:3]), AL.norm3(delta[3:6])
        trace.append((n, e, rot, tr))
        if rot <= eps_rot and tr <= eps_trans:
            status = CONVERGED
            break
    return dict(view=cur, status=status, iterations=len(trace), trace=trace)


same_result = AL.same_result


# ---- the pyramid of pipeline.view_register -------------------------------------------------------------------------------------
def reduce_image(I):
    """(a + b + c + d + 2) >> 2 over 2 x 2 blocks; an odd trailing row or column is dropped"""
    I = np.asarray(I, np.uint8)
    h, w = I.shape[0] // 2, I.shape[1] // 2
    q = I[:2 * h, :2 * w].astype(np.int64)
    return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def reduce_cam(cam):
    """the camera of the reduced picture: pixel (i, j) of it covers the full pixels 2 i, 2 i + 1, so its centre is at 2 i + 0.5"""
    out = dict(cam)
    out.update(f=float(cam["f"]) / 2.0, cx=(float(cam["cx"]) - 0.5) / 2.0, cy=(float(cam["cy"]) - 0.5) / 2.0, w=int(cam["w"]) // 2,
               h=int(cam["h"]) // 2)
    return out


def mesh_box(verts, faces):
    """(centre [3], diagonal) of the bounding box of the vertices a face uses: pipeline.view_register's default pivot and the
    scale of its default eps_trans"""
    X = np.asarray(verts, np.float64).reshape(-1, 3)
    used = np.unique(np.asarray(faces, np.int64).ravel())
    lo, hi = X[used].min(0), X[used].max(0)
    return [float(lo[a]) + 0.5 * (float(hi[a]) - float(lo[a])) for a in range(3)], float(math.sqrt(sum((float(hi[a]) - float(lo[a])) ** 2 for a in range(3))))


def view_register(M, cam, image, z_min, pivot, levels=1, **params):
    """the coarse-to-fine loop as pipeline.view_register runs it: dict(view, status, iterations, n, rms, levels=[align's dict per
    level, coarsest first])"""
    imgs, cams = [np.asarray(image, np.uint8)], [dict(cam)]
    for _ in range(1, int(levels)):
        imgs.append(reduce_image(imgs[-1]))
        cams.append(reduce_cam(cams[-1]))
    view, out = dict(cam), []
    for l in range(int(levels) - 1, -1, -1):
        start = dict(cams[l], R_rw=view["R_rw"], c_left=view["c_left"])
        res = align(M, start, imgs[l], z_min, pivot, **params)
        out.append(res)
        view = res["view"]
    last = out[-1]
    n, e = last["trace"][-1][0], last["trace"][-1][1]
    return dict(view=last["view"], status=last["status"], iterations=sum(r["iterations"] for r in out), n=n,
                rms=math.sqrt(e / n) if n else None, levels=out)


# ---- the calibration scene --------------------------------------------------------------------------------------
# texture_ref.fidelity_scene(): a level-4 icosphere under 26 cameras, textured from the 13 even views; view HELD_OUT is registered.
# A single textured sphere: the case the view alignment to the volume could not constrain.
HELD_OUT = 5
CALIB_PARAMS = dict(stride=2, margin=8, eps_rot=5e-5)  # eps_trans: pipeline.view_register's default, 1e-5 x the box diagonal
STARTS = ((0.0, 0.0, 1), (1.0, 2.5e-3, 1), (2.0, 5e-3, 1), (4.0, 10e-3, 2))  # (degrees about the pivot, metres, levels)
_calib = {}


def calibration():
    """dict(verts, faces, cams, images (the 13 texture views), z_min, depth_tol, patch, tex, M, pivot, diag, cam, image (the
    held-out view at its true pose), starts, params), built once"""
    if not _calib:
        import texture_ref as TR
        v, f, cams, imgs = TR.fidelity_scene()
        ev = list(range(0, len(cams), 2))
        z, tol, patch = TR.FIDELITY["z_min"], TR.FIDELITY["depth_tol"], TR.FIDELITY["patch"]
        tcams, timgs = [cams[i] for i in ev], [imgs[i] for i in ev]
        tex = TR.run(v, f, tcams, timgs, z, tol, patch=patch)
        piv, diag = mesh_box(v, f)
        rng = np.random.default_rng(29)
        starts = [AL.perturb(cams[HELD_OUT], piv, deg, metres, 1.0, rng) for deg, metres, _ in STARTS]
        _calib.update(verts=v, faces=f, cams=tcams, images=timgs, z_min=z, depth_tol=tol, patch=patch, tex=tex, M=model(v, f, tex), pivot=piv,
                      diag=diag, cam=cams[HELD_OUT], image=imgs[HELD_OUT], starts=starts, params=dict(CALIB_PARAMS, eps_trans=1e-5 * diag))
    return _calib


_calib_results = {}


def calibration_result(i):
    """view_register's dict of start i, computed once"""
    if i not in _calib_results:
        c = calibration()
        _calib_results[i] = view_register(c["M"], c["starts"][i], c["image"], c["z_min"], c["pivot"], levels=STARTS[i][2], **c["params"])
    return _calib_results[i]


BAD_PARAMS = (dict(z_min=0.0), dict(z_min=float("nan")), dict(z_min=float("inf")), dict(pivot=(0.0, float("nan"), 0.0)),
              dict(pivot=(float("inf"), 0.0, 0.0)), dict(max_iters=0), dict(max_iters=65), dict(stride=0), dict(margin=0), dict(margin=65),
              dict(min_pixels=0), dict(r_max=-1.0), dict(r_max=float("inf")), dict(r_max=float("nan")), dict(damping=-1e-300),
              dict(damping=float("inf")), dict(eps_rot=-1.0), dict(eps_rot=float("nan")), dict(eps_trans=-1.0), dict(eps_trans=float("inf")))
GOOD_PARAMS = (dict(), dict(max_iters=1), dict(max_iters=64), dict(stride=1 << 30), dict(margin=1), dict(margin=64), dict(min_pixels=1 << 30),
               dict(r_max=0.0), dict(damping=1e300), dict(eps_rot=0.0, eps_trans=0.0), dict(z_min=5e-324), dict(pivot=(1e300, -1e300, 0.0)))
