"""ctypes binding of the C++ host pipeline (libsfmx_host.so: sfmx_pipeline_run) — plumbing only."""
from __future__ import annotations

import ctypes
import os
import struct
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_ubyte, c_ulonglong, c_void_p

import numpy as np

from . import capi

HOST_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build", "libsfmx_host.so")
CLI_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build", "templering_sfm")


class PipelineCfg(ctypes.Structure):
    _fields_ = [("frames", c_int), ("export_pointcloud", c_int), ("max_tracks", c_int), ("min_tracks", c_int),
                ("quality", c_double), ("min_distance", c_int), ("pyr_levels", c_int), ("win_radius", c_int),
                ("klt_iters", c_int), ("fb_thresh", c_double), ("kf_min_gap", c_int), ("kf_min_inliers", c_int),
                ("kf_parallax_px", c_double), ("ba_window", c_int), ("ba_iters", c_int), ("ba_max_points", c_int),
                ("ba_huber", c_double), ("ba_lambda", c_double),
                ("comm_ba", c_void_p), ("comm_ransac", c_void_p)]


class PipelineStats(ctypes.Structure):
    _fields_ = [("n_keyframes", c_int), ("n_points", c_int), ("n_edges", c_int), ("n_frames", c_int),
                ("sec_total", c_double), ("sec_klt", c_double), ("sec_shi", c_double), ("sec_ransac", c_double),
                ("sec_ba", c_double), ("sec_upload", c_double), ("sec_host", c_double),
                ("sec_shi_gpu", c_double), ("sec_shi_replay", c_double), ("sec_desc", c_double), ("sec_bookkeeping", c_double),
                ("sec_r_pre", c_double), ("sec_r_gpu", c_double), ("sec_r_verify", c_double), ("sec_r_decomp", c_double),
                ("sec_tri_iter", c_double), ("sec_tri_solve", c_double), ("sec_tri_insert", c_double),
                ("us_klt_kernel", c_double), ("us_ransac_kernel", c_double), ("us_ba_kernel", c_double),
                ("us_shi_kernel", c_double),
                ("lk_steps", c_ulonglong), ("tracks_in", c_ulonglong), ("klt_calls", c_ulonglong),
                ("ransac_calls", c_ulonglong), ("ransac_points", c_ulonglong), ("ba_calls", c_ulonglong),
                ("ba_iters", c_ulonglong), ("ransac_verified", c_ulonglong), ("shi_fallbacks", c_ulonglong),
                ("shi_calls", c_ulonglong), ("shi_memo_hits", c_ulonglong), ("shi_prefetched", c_ulonglong), ("sec_shi_wait", c_double),
                ("sec_setup", c_double), ("sec_wall", c_double), ("sec_pf_busy", c_double), ("sec_pf_gpu", c_double),
                ("sec_pf_replay", c_double), ("sec_lane_b_busy", c_double), ("sec_lane_c_busy", c_double),
                ("sec_join_wait", c_double), ("sec_ba_gather", c_double), ("sec_m_step", c_double), ("sec_m_ransac", c_double),
                ("sec_m_kf", c_double), ("sec_feed_wait", c_double), ("ransac_cert_misses", c_ulonglong),
                ("us_kernel", c_double * 16), ("calls_kernel", c_ulonglong * 16), ("sec_lane_a_busy", c_double), ("sec_lane_e_busy", c_double)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("us_kernel", "calls_kernel")}
        lib = capi.load_library()
        # per-kernel GPU time (us) and launches over every context of the run; filled only when timing was enabled
        d["kernels"] = {lib.sfmx_kernel_profile_name(c_int(i)).decode(): (float(self.us_kernel[i]), int(self.calls_kernel[i]))
                        for i in range(16) if lib.sfmx_kernel_profile_name(c_int(i))}
        return d


class StereoRect(ctypes.Structure):
    _fields_ = [("R_rw", c_double * 9), ("c_left", c_double * 3), ("c_right", c_double * 3), ("f", c_double), ("cx", c_double),
                ("cy", c_double), ("B", c_double), ("H_l", c_double * 9), ("H_r", c_double * 9), ("swapped", c_int)]

    def asdict(self):
        return dict(R_rw=np.array(self.R_rw[:]).reshape(3, 3), c_left=np.array(self.c_left[:]), c_right=np.array(self.c_right[:]),
                    f=self.f, cx=self.cx, cy=self.cy, B=self.B, H_l=np.array(self.H_l[:]).reshape(3, 3),
                    H_r=np.array(self.H_r[:]).reshape(3, 3), swapped=bool(self.swapped))


class StereoMeshParams(ctypes.Structure):
    _fields_ = [("step", c_int), ("disp_min", c_double), ("disp_jump", c_double), ("z_max_percentile", c_double)]


class StereoRequest(ctypes.Structure):
    _fields_ = [("kf_a", c_int), ("kf_b", c_int), ("params", capi.StereoParams), ("mesh", StereoMeshParams)]


class StereoResult(ctypes.Structure):
    _fields_ = [("verts", POINTER(c_double)), ("verts_cap", c_int), ("faces", POINTER(c_int)), ("faces_cap", c_int),
                ("disp16", c_void_p), ("n_verts", c_int), ("n_faces", c_int), ("rect", StereoRect)]


# the reference's mesh_stereo section (step, disp_min, disp_jump, z_max_percentile); disparity parameters: capi.STEREO_DEFAULTS
STEREO_MESH_DEFAULTS = dict(step=4, disp_min=1.0, disp_jump=3.0, z_max_percentile=98.0)


def _split_stereo_params(params: dict):
    unknown = set(params) - set(capi.STEREO_DEFAULTS) - set(STEREO_MESH_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown stereo parameters {sorted(unknown)}")
    sp = capi.stereo_params(**{k: v for k, v in params.items() if k in capi.STEREO_DEFAULTS})
    mp = StereoMeshParams(**{**STEREO_MESH_DEFAULTS, **{k: v for k, v in params.items() if k in STEREO_MESH_DEFAULTS}})
    return sp, mp


def _pose12(pose):
    """camera->world pose as 12 doubles (R row-major, centre): accepts a 12-array or (R, c)"""
    if isinstance(pose, (tuple, list)) and len(pose) == 2:
        return np.concatenate([np.asarray(pose[0], np.float64).reshape(9), np.asarray(pose[1], np.float64).reshape(3)])
    return np.ascontiguousarray(pose, np.float64).reshape(12)


def stereo_rectify(K, pose_a, pose_b, w: int, h: int) -> dict:
    """Rectification of a posed pair (host, double): dict(R_rw, c_left, c_right, f, cx, cy, B, H_l, H_r, swapped).
    Poses are camera->world (R, centre).  A zero baseline raises."""
    lib = load_host_library()
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    pa, pb = _pose12(pose_a), _pose12(pose_b)
    r = StereoRect()
    dp = POINTER(c_double)
    rc = lib.sfmx_host_stereo_rectify(K.ctypes.data_as(dp), pa.ctypes.data_as(dp), pb.ctypes.data_as(dp), c_int(w), c_int(h), byref(r))
    if rc != capi.SFMX_OK:
        raise capi.SfmxError(rc, "stereo_rectify: zero baseline or degenerate pair")
    return r.asdict()


def _rect_struct(rect: dict) -> StereoRect:
    r = StereoRect()
    for k in ("R_rw", "c_left", "c_right", "H_l", "H_r"):
        getattr(r, k)[:] = [float(v) for v in np.asarray(rect[k], np.float64).ravel()]
    r.f, r.cx, r.cy, r.B, r.swapped = float(rect["f"]), float(rect["cx"]), float(rect["cy"]), float(rect["B"]), int(bool(rect.get("swapped")))
    return r


def _grid_caps(w, h, step):
    step = max(1, int(step))
    n = ((w + step - 1) // step) * ((h + step - 1) // step)
    return n, 2 * n


def stereo_grid_mesh(disp16, rect: dict, step=4, disp_min=1.0, disp_jump=3.0, z_max_percentile=98.0):
    """The host grid mesh of a disparity map (no device): (verts [n][3], faces [m][3] int32, warn or None)."""
    lib = load_host_library()
    d16 = np.ascontiguousarray(disp16, np.int16)
    h, w = d16.shape
    vcap, fcap = _grid_caps(w, h, step)
    verts, faces = np.zeros((vcap, 3)), np.zeros((fcap, 3), np.int32)
    nf = c_int(0)
    warn = ctypes.create_string_buffer(128)
    r = _rect_struct(rect)
    mp = StereoMeshParams(int(step), float(disp_min), float(disp_jump), float(z_max_percentile))
    nv = lib.sfmx_host_stereo_grid_mesh(d16.ctypes.data_as(c_void_p), c_int(w), c_int(h), byref(r), byref(mp), verts.ctypes.data_as(POINTER(c_double)),
                                        c_int(vcap), faces.ctypes.data_as(POINTER(c_int)), c_int(fcap), byref(nf), warn, c_int(len(warn)))
    if nv < 0:
        raise capi.SfmxError(-nv, "stereo_grid_mesh")
    return verts[:nv].copy(), faces[:nf.value].copy(), (warn.value.decode() or None)


def stereo_mesh(ctx: capi.Context, img_a, img_b, K, pose_a, pose_b, shape=None, **params) -> dict:
    """Keyframe-pair stereo mesh: rectify (host) -> disparity (device) -> grid mesh (host).
    img_a / img_b: u8 [h][w] host arrays, or device pointers (ints) with shape=(h, w).  params: capi.STEREO_DEFAULTS keys and
    STEREO_MESH_DEFAULTS keys.  Returns dict(verts, faces, disp16 (left rectified view), swapped, rect, warn)."""
    lib = load_host_library()
    on_dev = isinstance(img_a, int)
    if on_dev:
        h, w = shape
        pa_img, pb_img = c_void_p(img_a), c_void_p(img_b)
    else:
        img_a = np.ascontiguousarray(img_a, np.uint8)
        img_b = np.ascontiguousarray(img_b, np.uint8)
        h, w = img_a.shape
        assert img_b.shape == (h, w)
        pa_img, pb_img = img_a.ctypes.data_as(c_void_p), img_b.ctypes.data_as(c_void_p)
    sp, mp = _split_stereo_params(params)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    pa, pb = _pose12(pose_a), _pose12(pose_b)
    vcap, fcap = _grid_caps(w, h, mp.step)
    verts, faces = np.zeros((vcap, 3)), np.zeros((fcap, 3), np.int32)
    d16 = np.zeros((h, w), np.int16)
    res = StereoResult(verts.ctypes.data_as(POINTER(c_double)), vcap, faces.ctypes.data_as(POINTER(c_int)), fcap, d16.ctypes.data_as(c_void_p))
    warn = ctypes.create_string_buffer(128)
    dp = POINTER(c_double)
    rc = lib.sfmx_host_stereo_mesh(ctx.h_, pa_img, pb_img, c_int(1 if on_dev else 0), c_int(w), c_int(h), K.ctypes.data_as(dp),
                                   pa.ctypes.data_as(dp), pb.ctypes.data_as(dp), byref(sp), byref(mp), byref(res), warn, c_int(len(warn)))
    if rc != capi.SFMX_OK:
        raise capi.SfmxError(rc, (ctx.lib.sfmx_last_error(ctx.h_) or b"").decode() or "stereo_mesh")
    return dict(verts=verts[:res.n_verts].copy(), faces=faces[:res.n_faces].copy(), disp16=d16, swapped=bool(res.rect.swapped),
                rect=res.rect.asdict(), warn=warn.value.decode() or None)


class FusionResult(ctypes.Structure):
    _fields_ = [("verts", POINTER(c_double)), ("faces", POINTER(c_int)), ("n_verts", c_int), ("n_faces", c_int), ("n_views", c_int)]


class FusionResultEx(ctypes.Structure):
    _fields_ = [("verts", POINTER(c_double)), ("faces", POINTER(c_int)), ("n_verts", c_int), ("n_faces", c_int), ("n_views", c_int),
                ("normals", POINTER(c_double)), ("grey", POINTER(c_ubyte)), ("views", POINTER(c_int))]


APPEARANCE_KEYS = ("depth_tol", "cull", "fill")
CONSISTENCY_KEYS = ("rel_tol", "reproj_px", "min_support")
CLEAN_KEYS = ("min_faces", "min_permille")
SIMPLIFY_KEYS = ("factor", "cell", "origin")
SMOOTH_KEYS = ("iters", "lam", "mu", "pin", "unit", "origin")
FILL_KEYS = ("max_edges", "unit", "origin")
EVALUATE_KEYS = ("gt_verts", "gt_faces", "d_max", "tau", "percentile", "cell")
EVALUATION_FIELDS = ("accuracy", "acc_within", "acc_mean", "acc_max", "n_rec", "completeness", "comp_within", "n_gt")


class SurfaceEvalParams(ctypes.Structure):
    _fields_ = [("d_max", c_double), ("tau", c_double), ("percentile", c_double), ("cell", c_double)]


class SurfaceEvalResult(ctypes.Structure):
    _fields_ = [("accuracy", c_double), ("acc_mean", c_double), ("acc_max", c_double), ("completeness", c_double),
                ("acc_within", c_int), ("n_rec", c_int), ("comp_within", c_int), ("n_gt", c_int)]

    def asdict(self):
        return {k: (float if k in ("accuracy", "acc_mean", "acc_max", "completeness") else int)(getattr(self, k)) for k in EVALUATION_FIELDS}


RENDER_KEYS = ("cameras", "w", "h", "z_min", "z_max", "step", "min_weight", "background", "pgm_prefix")


class RenderOut(ctypes.Structure):
    _fields_ = [("depth", POINTER(c_double)), ("normals", POINTER(c_double)), ("points", POINTER(c_double)), ("shaded", POINTER(c_ubyte)),
                ("grey", POINTER(c_ubyte)), ("views", POINTER(c_int)), ("hits", c_int)]


class RenderRequest(ctypes.Structure):
    _fields_ = [("cameras", POINTER(capi.FusionView)), ("n_cameras", c_int), ("params", capi.RaycastParams), ("out", POINTER(RenderOut))]


RASTER_KEYS = ("cameras", "w", "h", "z_min", "cull", "background", "pgm_prefix")


class RasterOut(ctypes.Structure):
    _fields_ = [("depth", POINTER(c_double)), ("face", POINTER(c_int)), ("points", POINTER(c_double)), ("normals", POINTER(c_double)),
                ("shaded", POINTER(c_ubyte)), ("grey", POINTER(c_ubyte)), ("counts", c_int * 8), ("fragments", ctypes.c_uint64)]


class RasterRequest(ctypes.Structure):
    _fields_ = [("cameras", POINTER(capi.FusionView)), ("n_cameras", c_int), ("params", capi.RasterParams), ("out", POINTER(RasterOut))]


VISIBILITY_KEYS = ("z_min", "depth_tol", "min_views", "colour", "cull", "fill")


class VisibRequest(ctypes.Structure):
    _fields_ = [("params", capi.VisibParams), ("colour", c_int), ("counts", c_int * 5), ("pairs", ctypes.c_uint64 * 3), ("n_in", c_int),
                ("m_in", c_int), ("face_views", POINTER(c_int)), ("face_back_views", POINTER(c_int)), ("vert_views", POINTER(c_int))]


TEXTURE_KEYS = ("z_min", "depth_tol", "patch", "cells_per_row", "fill", "obj_path")


class TextureRequest(ctypes.Structure):
    _fields_ = [("params", capi.TextureParams), ("counts", c_int * 6), ("n_faces", c_int), ("n_views", c_int), ("atlas", POINTER(c_ubyte)),
                ("face_view", POINTER(c_int)), ("face_area", POINTER(ctypes.c_int64)), ("uv_half", POINTER(c_int)),
                ("view_faces", POINTER(c_int))]


LEVEL_KEYS = ("iterations",)


class LevelRequest(ctypes.Structure):
    _fields_ = [("params", capi.LevelParams), ("counts", c_int * 6), ("n_faces", c_int), ("n_verts", c_int), ("atlas", POINTER(c_ubyte)),
                ("corner_adj", POINTER(c_int)), ("corner_sample", POINTER(c_int)), ("vertex_views", POINTER(c_int))]


ALIGN_KEYS = ("seed", "max_iters", "stride", "min_pixels", "damping", "eps_rot", "eps_trans", "min_weight")


class AlignRequest(ctypes.Structure):
    _fields_ = [("seed", c_int), ("params", capi.AlignParams), ("out", POINTER(capi.AlignResult))]


PHOTO_KEYS = ("background", "pgm_prefix")
PALIGN_KEYS = ("cameras", "images", "levels", "z_min", "pivot") + tuple(capi.PALIGN_DEFAULTS)


class PhotoRequest(ctypes.Structure):
    _fields_ = [("params", capi.PhotoParams), ("n_views", c_int), ("w", c_int), ("h", c_int), ("rendered", POINTER(c_ubyte)),
                ("cls", POINTER(c_ubyte)), ("face", POINTER(c_int)), ("classes", POINTER(ctypes.c_int64)), ("stats", POINTER(ctypes.c_int64)),
                ("hist", POINTER(ctypes.c_int64))]


CARVE_KEYS = ("threshold", "cap", "margin", "mode", "min_views", "hull_only")


class CarveRequest(ctypes.Structure):
    _fields_ = [("params", capi.CarveParams), ("threshold", c_int), ("hull_only", c_int), ("counts", c_int * 3), ("n_views", c_int),
                ("inside_pixels", POINTER(c_int))]


def write_pgm(path: str, image) -> None:
    """a u8 [h][w] image as a binary PGM (P5)"""
    image = np.ascontiguousarray(image, np.uint8)
    h, w = image.shape
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h))
        f.write(image.tobytes())


def write_bmp(path: str, image) -> None:
    """a u8 [h][w] image as an uncompressed 8-bit BMP with a grey palette (rows bottom-up, padded to four bytes)"""
    image = np.ascontiguousarray(image, np.uint8)
    h, w = image.shape
    stride = (w + 3) & ~3
    rows = np.zeros((h, stride), np.uint8)
    rows[:, :w] = image[::-1]
    offset = 14 + 40 + 1024
    with open(path, "wb") as f:
        f.write(struct.pack("<2sIHHI", b"BM", offset + stride * h, 0, 0, offset))
        f.write(struct.pack("<IiiHHIIiiII", 40, w, h, 1, 8, 0, stride * h, 2835, 2835, 256, 0))
        f.write(b"".join(bytes((g, g, g, 0)) for g in range(256)))
        f.write(rows.tobytes())


def write_textured_obj(path: str, verts, faces, uv, atlas) -> None:
    """NAME.obj (v with %.17g, three vt per face, f a/ta b/tb c/tc), NAME.mtl, NAME_atlas.pgm and NAME_atlas.bmp from path =
    NAME.obj (or NAME); uv float64 [m][3][2], atlas u8 [H][W]"""
    stem = path[:-4] if path.lower().endswith(".obj") else path
    name = os.path.basename(stem)
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    atlas = np.ascontiguousarray(atlas, np.uint8)
    if atlas.size == 0:
        atlas = np.zeros((1, 1), np.uint8)  # neither format has an empty image
    write_pgm(stem + "_atlas.pgm", atlas)
    write_bmp(stem + "_atlas.bmp", atlas)
    with open(stem + ".mtl", "w") as f:
        f.write(f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {name}_atlas.bmp\n")
    with open(stem + ".obj", "w") as f:
        f.write(f"mtllib {name}.mtl\nusemtl atlas\n")
        f.write("".join("v %.17g %.17g %.17g\n" % tuple(v) for v in verts))
        f.write("".join("vt %.17g %.17g\n" % tuple(t) for t in uv))
        f.write("".join("f %d/%d %d/%d %d/%d\n" % (a + 1, 3 * i + 1, b + 1, 3 * i + 2, c + 1, 3 * i + 3) for i, (a, b, c) in enumerate(faces)))


class SurfaceGt(ctypes.Structure):
    _fields_ = [("verts", POINTER(c_double)), ("n_verts", c_int), ("faces", POINTER(c_int)), ("n_faces", c_int),
                ("params", SurfaceEvalParams)]


def _eval_params(d_max, tau, percentile, cell) -> SurfaceEvalParams:
    if d_max is None or tau is None:
        raise TypeError("surface evaluation needs d_max and tau (lengths in the mesh's units; there is no default)")
    if not float(tau) <= float(d_max):
        raise ValueError(f"tau = {tau} must not exceed d_max = {d_max}")
    return SurfaceEvalParams(float(d_max), float(tau), float(percentile), float(cell))


REGISTER_KEYS = ("d_max", "init") + tuple(capi.REGISTER_DEFAULTS)


def _register_request(register, d_max) -> dict | None:
    """the keyword arguments of surface_register for a `register` request (None / False, True or a dict); d_max defaults to the
    evaluation's"""
    if register is None or register is False:
        return None
    rkw = {} if register is True else dict(register)
    unknown = set(rkw) - set(REGISTER_KEYS)
    if unknown:
        raise TypeError(f"unknown register parameters {sorted(unknown)}")
    rkw.setdefault("d_max", d_max)
    return rkw


def surface_register(ctx: capi.Context, verts, faces, gt_verts, gt_faces, d_max=None, init=None, **params) -> dict:
    """Registers the reconstruction (verts, faces) to the ground truth (gt_verts, gt_faces) by Sim(3) point-to-plane
    Gauss-Newton on the device (capi.Register): the source points are the vertices a face uses, the target is the
    ground-truth mesh, d_max (required, in the ground truth's units) is the trimming distance, init (dict(s, R, t), default the
    identity) the start.  params: capi.REGISTER_DEFAULTS keys.  Returns dict(T=dict(s, R, t), status, iterations, n (samples
    used by the last evaluation), rms_plane, rms_point (of that evaluation; nan when n = 0), trace, verts (all vertices moved by
    T, float64 [nv][3]))."""
    if d_max is None:
        raise TypeError("surface registration needs d_max (a length in the ground truth's units; there is no default)")
    unknown = set(params) - set(capi.REGISTER_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown register parameters {sorted(unknown)}")
    rv = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    rf = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    if len(rf) and (rf.min() < 0 or rf.max() >= len(rv)):
        raise ValueError("a face index is outside the vertices")
    mask = np.zeros(len(rv), bool)
    mask[rf.ravel()] = True
    cell = params.pop("cell", 0.0)
    rg = ctx.register()
    try:
        rg.set_target(gt_verts, gt_faces, d_max, cell)
        res = rg.run(rv[mask], init=init, **params)
        moved = rg.apply(res["T"], rv)
    finally:
        rg.close()
    n, e, c = res["trace"][-1][:3]
    nan = float("nan")
    res.update(n=n, rms_plane=float(np.sqrt(e / n)) if n > 0 else nan, rms_point=float(np.sqrt(c / n)) if n > 0 else nan, verts=moved)
    return res


def reduce_image(image) -> np.ndarray:
    """one level of view_register's pyramid: (a + b + c + d + 2) >> 2 over 2 x 2 blocks of a u8 picture; an odd trailing row or
    column is dropped"""
    I = np.ascontiguousarray(image, np.uint8)
    h, w = I.shape[0] // 2, I.shape[1] // 2
    q = I[:2 * h, :2 * w].astype(np.int64)
    return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def reduce_camera(cam: dict) -> dict:
    """the camera of reduce_image's picture: f / 2, (cx - 0.5) / 2, (cy - 0.5) / 2, w // 2, h // 2 (pixel i of the reduced picture
    is centred at 2 i + 0.5 of the full one)"""
    out = dict(cam)
    out.update(f=float(cam["f"]) / 2.0, cx=(float(cam["cx"]) - 0.5) / 2.0, cy=(float(cam["cy"]) - 0.5) / 2.0, w=int(cam["w"]) // 2,
               h=int(cam["h"]) // 2)
    return out


def view_register(ctx: capi.Context, tx: "capi.Texture", verts, faces, cam: dict, image, z_min=None, lv: "capi.Level" = None, levels=1,
                  init=None, pivot=None, **params) -> dict:
    """Registers a camera to the textured mesh by direct photometric Gauss-Newton alignment on the device (DESIGN.md 29;
    capi.PAlign).  tx: the Texture whose last run was on (verts, faces); lv: a Level run on tx, then its atlas is read (or both
    as results on the host: dict(face_view, uv_half, atlas) and dict(atlas), as fuse returns them).  cam:
    dict(R_rw, c_left, f, cx, cy) of the picture `image` u8 [h][w] at a rough pose; init: dict(R_rw, c_left) replaces cam's pose
    as the start.  z_min (required) is the z-buffer's.  pivot defaults to the centre of the bounding box of the vertices a face
    uses, eps_trans to 1e-5 x that box's diagonal.  levels > 1 runs coarse to fine on the host: level l uses the picture reduced l
    times (reduce_image) under the camera reduced as often (reduce_camera), starts at the view the coarser level returned and
    keeps margin in pixels.  params: capi.PALIGN_DEFAULTS keys.
    Returns dict(view, status, iterations (over all levels), n and rms = sqrt(e / n) of the last evaluation (rms nan when n = 0),
    levels = [dict(view, status, iterations, trace) per level, coarsest first])."""
    if z_min is None:
        raise TypeError("view registration needs z_min (a depth in the mesh's units; there is no default)")
    unknown = set(params) - set(capi.PALIGN_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown palign parameters {sorted(unknown)}")
    levels = int(levels)
    if levels < 1:
        raise ValueError("levels >= 1")
    rv = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    rf = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    if len(rf) and (rf.min() < 0 or rf.max() >= len(rv)):
        raise ValueError("a face index is outside the vertices")
    if pivot is None or "eps_trans" not in params:
        if not len(rf):
            raise ValueError("a mesh without faces has no bounding box: give pivot and eps_trans")
        used = rv[np.unique(rf.ravel())]
        lo, hi = used.min(0), used.max(0)
        if pivot is None:
            pivot = [float(lo[a]) + 0.5 * (float(hi[a]) - float(lo[a])) for a in range(3)]
        if "eps_trans" not in params:
            params["eps_trans"] = 1e-5 * float(np.sqrt(sum((float(hi[a]) - float(lo[a])) ** 2 for a in range(3))))
    img = np.ascontiguousarray(image, np.uint8)
    if img.ndim != 2:
        raise TypeError("the picture is uint8 [h][w]")
    cams, imgs = [dict(cam, w=img.shape[1], h=img.shape[0])], [img]
    if init is not None:
        cams[0].update(R_rw=init["R_rw"], c_left=init["c_left"])
    for _ in range(1, levels):
        imgs.append(reduce_image(imgs[-1]))
        cams.append(reduce_camera(cams[-1]))
        if min(imgs[-1].shape) < 1:
            raise ValueError("the picture is too small for that many levels")
    pa = ctx.palign()
    try:
        pa.set_model(tx, rv, rf, lv=lv)
        view, per = cams[0], []
        for l in range(levels - 1, -1, -1):
            pa.set_image(imgs[l])
            res = pa.view(dict(cams[l], R_rw=view["R_rw"], c_left=view["c_left"]), z_min, pivot, **params)
            per.append(res)
            view = res["view"]
    finally:
        pa.close()
    last = per[-1]
    n, e = last["trace"][-1][0], last["trace"][-1][1]
    return dict(view=last["view"], status=last["status"], iterations=sum(r["iterations"] for r in per), n=n,
                rms=float(np.sqrt(e / n)) if n > 0 else float("nan"), levels=per)


def surface_eval(ctx: capi.Context, verts, faces, gt_verts, gt_faces, d_max=None, tau=None, percentile=90.0, cell=0.0,
                 register=None) -> dict:
    """Accuracy and completeness of the reconstruction (verts, faces) against the ground truth (gt_verts, gt_faces), sampled at
    the vertices a face uses; the distances come from the device (capi.Sdist).  accuracy: the distance within
    which `percentile` % of the reconstruction lies of the ground truth (nearest rank; distances are clipped at d_max);
    acc_within / comp_within: vertices within tau; completeness = comp_within / n_gt.  d_max and tau are required, tau <= d_max.
    Returns dict(accuracy, acc_within, acc_mean, acc_max, n_rec, completeness, comp_within, n_gt).
    register: None (default), True or dict(d_max=, init=, capi.REGISTER_DEFAULTS keys) -- the reconstruction is first registered
    to the ground truth (surface_register; its d_max defaults to the evaluation's) and the moved vertices are evaluated; the
    result gains registration = surface_register's dict without the vertices.  d_max and tau are in the ground truth's units."""
    lib = load_host_library()
    p = _eval_params(d_max, tau, percentile, cell)
    rkw = _register_request(register, d_max)
    if rkw is not None:
        reg = surface_register(ctx, verts, faces, gt_verts, gt_faces, **rkw)
        out = surface_eval(ctx, reg.pop("verts"), faces, gt_verts, gt_faces, d_max=d_max, tau=tau, percentile=percentile, cell=cell)
        out["registration"] = reg
        return out
    rv = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    rf = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    gv = np.ascontiguousarray(gt_verts, np.float64).reshape(-1, 3)
    gf = np.ascontiguousarray(gt_faces, np.int32).reshape(-1, 3)
    out = SurfaceEvalResult()
    dp, ip = POINTER(c_double), POINTER(c_int)
    rc = lib.sfmx_host_surface_eval(ctx.h_, rv.ctypes.data_as(dp), c_int(len(rv)), rf.ctypes.data_as(ip), c_int(len(rf)),
                                    gv.ctypes.data_as(dp), c_int(len(gv)), gf.ctypes.data_as(ip), c_int(len(gf)), byref(p), byref(out))
    if rc != capi.SFMX_OK:
        raise capi.SfmxError(rc, (ctx.lib.sfmx_last_error(ctx.h_) or b"").decode() or "surface_eval")
    return out.asdict()


def _split_fusion_params(params: dict):
    unknown = set(params) - set(capi.STEREO_DEFAULTS) - set(capi.FUSION_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown fusion parameters {sorted(unknown)}")
    sp = capi.stereo_params(**{k: v for k, v in params.items() if k in capi.STEREO_DEFAULTS})
    return sp, {k: v for k, v in params.items() if k in capi.FUSION_DEFAULTS}


def fuse(ctx: capi.Context, images, K, poses, pairs, origin, voxel, dims, shape=None, ply_path: str | None = None, appearance=False,
         consistency=False, clean=False, evaluate=None, render=None, align=False, simplify=False, smooth=False, fill=False, raster=None,
         visibility=False, texture=False, level=False, photo=False, palign=False, carve=False, **params) -> dict:
    """Multi-pair depth fusion: per pair rectify (host) -> disparity (device) -> one TSDF view; then integrate and extract
    the surface (device).  images: u8 [n][h][w] host array, or a list of device pointers (ints) with shape=(h, w).
    poses: [n] camera->world poses (12 doubles or (R, c)); pairs: [(a, b), ...] indices into images.  The volume is
    explicit: dims = (nx, ny, nz) grid points at origin + (i, j, k) * voxel.  params: capi.STEREO_DEFAULTS and
    capi.FUSION_DEFAULTS keys.  Returns dict(verts, faces, views (pairs integrated), warn (WARN lines or None)).
    appearance: True, or dict(depth_tol=, cull=, fill=) (depth_tol defaults to the volume's trunc) -- vertex normals from the
    volume's gradient and vertex grey from the views that see each vertex: the dict gains normals [n][3] f64,
    grey [n] u8 and vertex_views [n] i32 (views that saw the vertex), and the PLY gains nx ny nz and red green blue.
    consistency: True, or dict(rel_tol=, reproj_px=, min_support=) (disp_min is the fusion's) -- every pair's disparity map is
    filtered against the other pairs' before it enters the volume: the dict gains consistency =
    dict(valid=[...], kept=[...]), the valid and the kept pixels of each integrated pair.  The shade views of appearance keep
    the unfiltered maps.
    clean: True, or dict(min_faces=, min_permille=) -- the small connected components of the extracted surface are removed on
    the device before the arrays and the PLY are made; with appearance the cleaned vertices are shaded.  The dict
    gains clean = dict(components=, largest=, verts_removed=, faces_removed=).
    evaluate: dict(gt_verts=, gt_faces=, d_max=, tau=, percentile=90, cell=0) -- the final mesh (the cleaned one with clean) is
    evaluated against the ground-truth mesh from where it lies on the device: the dict gains evaluation =
    surface_eval()'s dict.  d_max and tau are required.  With register= (True or a dict, as surface_eval takes it) the final mesh
    is, after the chain has returned, registered to the ground truth first and evaluation is that of the moved
    vertices, with registration inside it; verts, faces and the PLY stay in the reconstruction's own frame.
    render: dict(cameras=[dict(R_rw, c_left, f, cx, cy), ...], w=, h=, z_min=, z_max=, step=0, min_weight=0, background=0,
    pgm_prefix=None) -- the integrated volume is ray cast from each camera at w x h (z_min and z_max are required):
    the dict gains renders = [dict(depth, normals, points, shaded, hits), ...]; with appearance each also carries grey and
    pixel_views, the shade stage over the render's points and normals from the retained views.  pgm_prefix writes
    <prefix>_<i>_shaded.pgm (and _grey.pgm with appearance).  The mesh and the PLY are what they are without render.
    align: True, or dict(seed=1, max_iters=, stride=, min_pixels=, damping=, eps_rot=, eps_trans=, min_weight=) (disp_min is the
    fusion's) -- the pairs are processed in list order: the first `seed` integrated pairs enter the volume at their given poses,
    every later pair's view is first registered to the volume integrated so far and enters it, and the shade views
    of appearance, at its refined view.  The dict gains alignment = [dict(pair, status, iterations, n, rms, view), ...], one per
    aligned pair: status as capi.ALIGN_STATUS, n and rms = sqrt(e / n) of the last evaluation, view the refined camera.  A pair
    whose alignment ends TOO_FEW or DEGENERATE keeps its given view (one WARN line).  Not together with consistency.
    simplify: True, or dict(factor=2.0, cell=, origin=) -- the surface (the cleaned one with clean) is simplified on the device by
    exact vertex clustering on a grid of `factor` voxels, or of `cell` in the volume's units (not both), whose
    corner `origin` defaults to the volume's; with appearance the simplified vertices are shaded with their own normals, and
    evaluate measures the simplified mesh.  The dict gains simplify = dict(clusters=, degenerate=, duplicates=, verts_before=,
    faces_before=).
    smooth: True, or dict(iters=10, lam=0.5, mu=-0.53, pin=1, unit=, origin=) -- the surface (the cleaned one with clean) is smoothed
    on the device by the exact Taubin lambda|mu filter before it is simplified, shaded, evaluated and written: `iters`
    pairs of a lambda and a mu step over each vertex's distinct neighbours, with the vertices of every edge that is not used once in
    each direction held in place (pin=1).  unit (the length 2^20 fixed-point steps stand for) defaults to the voxel and origin to
    the volume's.  Normals stay with their vertices.  The dict gains smooth = dict(edges=, boundary_edges=, irregular_edges=,
    pinned=, isolated=).
    fill: True, or dict(max_edges=32, unit=, origin=) -- the small holes of the surface (the cleaned one with clean) are filled on the
    device by exact centroid fans before it is smoothed, simplified, shaded, evaluated and written: every closed loop
    of at most `max_edges` boundary edges through simple vertices gets one new vertex at its rounded centroid (none for a loop of
    three) and a fan of faces; the surface's outer rim and longer loops stay open.  unit and origin default as for smooth.  With
    appearance a new vertex carries the normalised sum of its loop's normals and is shaded like any other.  The dict gains fill =
    dict(edges=, boundary_edges=, irregular_edges=, complex_vertices=, filled_loops=, filled_edges=, new_verts=, new_faces=).
    raster: dict(cameras=[dict(R_rw, c_left, f, cx, cy), ...], w=, h=, z_min=, cull=0, background=0, pgm_prefix=None) -- the final
    mesh, the one in the arrays and the PLY, is rendered from each camera at w x h by the exact z-buffer (z_min is
    required): the dict gains rasters = [dict(depth, face, points, normals, shaded, the capi.RASTER_COUNTS, fragments), ...]; with
    appearance the vertex normals and grey are interpolated and each also carries grey.  pgm_prefix writes
    <prefix>_<i>_mesh_shaded.pgm (and _mesh_grey.pgm with appearance).  Everything else is what it is without raster.
    visibility: dict(z_min=, depth_tol=, min_views=1, colour=False, cull=1, fill=0) -- the faces of the final mesh (after simplify)
    that fewer than min_views of the integrated pairs' left rectified cameras (the refined ones with align) see from the front are
    removed on the device (z_min is required, depth_tol defaults to the voxel) before the mesh is shaded, evaluated,
    rendered by raster and written.  The dict gains visibility = dict(face_views, face_back_views, vert_views (per element of the
    mesh that entered the stage), the capi.VISIB_COUNTS, verts_removed, faces_removed).  colour=True (needs appearance) replaces
    grey / vertex_views and the PLY colour by this stage's, from the pairs' left rectified images (cull and fill are its).
    texture: dict(z_min=, depth_tol=, patch=8, cells_per_row=0, fill=0, obj_path=None) -- the final mesh (after the visibility
    culling) gets a texture atlas on the device (z_min is required, depth_tol defaults to the voxel): every face takes
    the integrated pair's left rectified camera that sees it from the front with the largest image area, its patch of the atlas is
    sampled bilinearly from that pair's left rectified image.  The dict gains texture = dict(atlas u8 [H][W], uv f64 [m][3][2],
    uv_half, face_view, face_area, view_faces, the capi.TEXTURE_COUNTS).  obj_path = NAME.obj writes NAME.obj, NAME.mtl,
    NAME_atlas.pgm and NAME_atlas.bmp.  Everything else is what it is without texture.
    level: True, or dict(iterations=64) (needs texture) -- the atlas's seams are levelled on the device: every (vertex,
    view) of a textured face gets an offset in 1/256 grey level, pinned on the vertices where views meet to the mean of the views'
    samples and relaxed elsewhere by `iterations` Jacobi sweeps, and every texel gets the blend of its face's three offsets before
    its rounding.  The dict gains level = dict(atlas u8 [H][W], corner_adj i32 [m][3], corner_sample i32 [m][3], vertex_views i32
    [n], the capi.LEVEL_COUNTS); texture is unchanged, and with obj_path the written atlas files are the levelled atlas.
    photo: True, or dict(background=0, pgm_prefix=None) (needs texture) -- the textured final mesh is rendered back into the texture's
    own views on the device (z_min is the texture's), from the levelled atlas with level, and compared with their
    images.  The dict gains photo = dict(rendered u8 / cls u8 / face i32 [V][h][w], classes i64 [V][5], stats i64 [V][2][3], hist
    i64 [V][2][256], summary = capi.photo_summary's dict).  pgm_prefix writes <prefix>_<q>_photo.pgm.  Everything else is what it
    is without photo.
    palign: dict(cameras=[dict(R_rw, c_left, f, cx, cy), ...], images=[u8 [h][w], ...], levels=1, z_min=the texture's, pivot=None,
    capi.PALIGN_DEFAULTS keys) (needs texture) -- after the chain has returned, each listed camera is registered to the final
    textured mesh by direct photometric alignment on the device (view_register, on the levelled atlas with level).
    The dict gains palign = [view_register's dict per camera] ([] for a mesh without faces).  Everything else is what it is
    without palign.
    carve: True, or dict(threshold=1, cap=16, margin=0.5, mode="intersect" | "clear", min_views=1, hull_only=False) -- shape from
    silhouette: the silhouette of each integrated pair is its left rectified picture at `threshold` (1 .. 255) under
    the pair's left rectified camera (the refined one with align); after the last integration and before the extraction, the normals
    and render, every grid point that some camera sees more than `margin` (in units of the volume's trunc) outside its silhouette
    is made undefined (clear) or given the hull's value where the volume holds none or a smaller one (intersect).  The dict gains
    carve = dict(defined, outside, changed, inside_pixels=[per view]).  A trunc given to the fusion is the hull's too.
    hull_only=True skips the disparities and the integration,
    stores the hull itself in the volume and lets the rest of the chain run on it (views, the pairs integrated, is then 0, mode is
    not used and changed is 0); it raises ValueError together with consistency,
    align and appearance.  The object must lie inside every picture (a rectified picture is 0 where its source has no pixel)."""
    kq = None
    if carve is not False and carve is not None:  # carve={} is the defaults
        kkw = {} if carve is True else dict(carve)
        unknown = set(kkw) - set(CARVE_KEYS)
        if unknown:
            raise TypeError(f"unknown carve parameters {sorted(unknown)}")
        k_thr, k_hull = kkw.pop("threshold", 1), kkw.pop("hull_only", False)
        if isinstance(k_thr, bool) or not isinstance(k_thr, (int, np.integer)) or not isinstance(k_hull, (bool, np.bool_)):
            raise TypeError("carve: threshold is an int, hull_only a bool")
        kp = capi.carve_params(**kkw)
        if not 1 <= int(k_thr) <= 255 or not capi.carve_check_params(**kkw):
            raise ValueError("carve parameters outside their range")
        if k_hull and (consistency or align or appearance):
            raise ValueError("carve hull_only has no disparity maps: not together with consistency, align or appearance")
        kq = CarveRequest(kp, int(k_thr), int(bool(k_hull)))
    lib = load_host_library()
    if isinstance(images, (list, tuple)) and images and isinstance(images[0], int):
        h, w = shape
        n = len(images)
        ptrs = (c_void_p * max(n, 1))(*images)
        on_dev, keep = 1, None
    else:
        keep = np.ascontiguousarray(images, np.uint8)
        n, h, w = keep.shape
        ptrs = (c_void_p * max(n, 1))(*[keep[i].ctypes.data for i in range(n)])
        on_dev = 0
    poses12 = np.ascontiguousarray(np.stack([_pose12(p) for p in poses]) if len(poses) else np.zeros((0, 12)), np.float64)
    if len(poses12) != n:
        raise ValueError(f"{n} images but {len(poses12)} poses")
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    sp, fkw = _split_fusion_params(params)
    fp = capi.fusion_params(origin, voxel, dims, **fkw)
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    warn = ctypes.create_string_buffer(1 << 16)
    dp = POINTER(c_double)
    ap = cp = counts = lp = None
    if appearance:
        akw = {} if appearance is True else dict(appearance)
        unknown = set(akw) - set(APPEARANCE_KEYS)
        if unknown:
            raise TypeError(f"unknown appearance parameters {sorted(unknown)}")
        ap = capi.shade_params(akw.pop("depth_tol", 0.0), disp_min=fp.disp_min, **akw)  # 0 = the volume's trunc
    if consistency:
        ckw = {} if consistency is True else dict(consistency)
        unknown = set(ckw) - set(CONSISTENCY_KEYS)
        if unknown:
            raise TypeError(f"unknown consistency parameters {sorted(unknown)}")
        cp = capi.consist_params(disp_min=fp.disp_min, **ckw)
        counts = np.full((max(len(pr), 1), 2), -1, np.int32)
    if clean:
        lkw = {} if clean is True else dict(clean)
        unknown = set(lkw) - set(CLEAN_KEYS)
        if unknown:
            raise TypeError(f"unknown clean parameters {sorted(unknown)}")
        lp = capi.clean_params(**lkw)
        lcounts = np.zeros(4, np.int32)
    mp = None
    if simplify:
        mkw = {} if simplify is True else dict(simplify)
        unknown = set(mkw) - set(SIMPLIFY_KEYS)
        if unknown:
            raise TypeError(f"unknown simplify parameters {sorted(unknown)}")
        if "factor" in mkw and "cell" in mkw:
            raise TypeError("simplify takes factor (voxels) or cell (a length), not both")
        mcell = float(mkw["cell"]) if "cell" in mkw else float(mkw.get("factor", 2.0)) * float(voxel)
        mp = capi.simplify_params(mcell, origin=mkw.get("origin", origin))
        mcounts = np.zeros(5, np.int32)
    tp = None
    if smooth:
        tkw = {} if smooth is True else dict(smooth)
        unknown = set(tkw) - set(SMOOTH_KEYS)
        if unknown:
            raise TypeError(f"unknown smooth parameters {sorted(unknown)}")
        tp = capi.smooth_params(float(tkw.pop("unit", voxel)), origin=tkw.pop("origin", origin), **tkw)
        tcounts = np.zeros(5, np.int32)
    hp = None
    if fill:
        hkw = {} if fill is True else dict(fill)
        unknown = set(hkw) - set(FILL_KEYS)
        if unknown:
            raise TypeError(f"unknown fill parameters {sorted(unknown)}")
        hp = capi.fill_params(float(hkw.pop("unit", voxel)), origin=hkw.pop("origin", origin), **hkw)
        hcounts = np.zeros(8, np.int32)
    gt = None
    if evaluate is not None:
        ekw = dict(evaluate)
        ereg = _register_request(ekw.pop("register", None), ekw.get("d_max"))  # applied to the final mesh, after the chain
        unknown = set(ekw) - set(EVALUATE_KEYS)
        if unknown:
            raise TypeError(f"unknown evaluate parameters {sorted(unknown)}")
        if "gt_verts" not in ekw or "gt_faces" not in ekw:
            raise TypeError("evaluate needs gt_verts and gt_faces")
        gv = np.ascontiguousarray(ekw["gt_verts"], np.float64).reshape(-1, 3)
        gf = np.ascontiguousarray(ekw["gt_faces"], np.int32).reshape(-1, 3)
        gt = SurfaceGt(gv.ctypes.data_as(dp), len(gv), gf.ctypes.data_as(POINTER(c_int)), len(gf),
                       _eval_params(ekw.get("d_max"), ekw.get("tau"), ekw.get("percentile", 90.0), ekw.get("cell", 0.0)))
        ev = SurfaceEvalResult()
    rq = None
    if render is not None:
        rkw = dict(render)
        unknown = set(rkw) - set(RENDER_KEYS)
        if unknown:
            raise TypeError(f"unknown render parameters {sorted(unknown)}")
        missing = [k for k in ("cameras", "w", "h", "z_min", "z_max") if k not in rkw]
        if missing:
            raise TypeError(f"render needs {missing}")
        rw, rh = int(rkw["w"]), int(rkw["h"])
        if rw < 1 or rh < 1 or rw > 4096 or rw * rh > capi.RAYCAST_MAX_PIXELS:
            raise ValueError(f"render size {rw} x {rh} is outside 1 <= w <= 4096, w * h <= 2^24")
        rcams = list(rkw["cameras"])
        rviews = (capi.FusionView * max(len(rcams), 1))(*[capi.fusion_view({**c, "B": c.get("B", 0.0)}, rw, rh) for c in rcams])
        rarr = [dict(depth=np.zeros((rh, rw)), normals=np.zeros((rh, rw, 3)), points=np.zeros((rh, rw, 3)), shaded=np.zeros((rh, rw), np.uint8))
                for _ in rcams]
        if ap is not None:
            for a in rarr:
                a.update(grey=np.zeros((rh, rw), np.uint8), pixel_views=np.zeros((rh, rw), np.int32))
        ub, ip = POINTER(c_ubyte), POINTER(c_int)
        routs = (RenderOut * max(len(rcams), 1))(*[
            RenderOut(a["depth"].ctypes.data_as(dp), a["normals"].ctypes.data_as(dp), a["points"].ctypes.data_as(dp), a["shaded"].ctypes.data_as(ub),
                      a["grey"].ctypes.data_as(ub) if ap is not None else None, a["pixel_views"].ctypes.data_as(ip) if ap is not None else None, 0)
            for a in rarr])
        rq = RenderRequest(rviews, len(rcams), capi.raycast_params(rkw["z_min"], rkw["z_max"], rkw.get("step", 0.0), rkw.get("min_weight", 0),
                                                                   rkw.get("background", 0)), routs)
    zq = None
    if raster is not None:
        zkw = dict(raster)
        unknown = set(zkw) - set(RASTER_KEYS)
        if unknown:
            raise TypeError(f"unknown raster parameters {sorted(unknown)}")
        missing = [k for k in ("cameras", "w", "h", "z_min") if k not in zkw]
        if missing:
            raise TypeError(f"raster needs {missing}")
        zw, zh = int(zkw["w"]), int(zkw["h"])
        if zw < 1 or zh < 1 or zw > 4096 or zw * zh > capi.RASTER_MAX_PIXELS:
            raise ValueError(f"raster size {zw} x {zh} is outside 1 <= w <= 4096, w * h <= 2^24")
        zcams = list(zkw["cameras"])
        zviews = (capi.FusionView * max(len(zcams), 1))(*[capi.fusion_view({**c, "B": c.get("B", 0.0)}, zw, zh) for c in zcams])
        zarr = [dict(depth=np.zeros((zh, zw)), face=np.zeros((zh, zw), np.int32), points=np.zeros((zh, zw, 3)), normals=np.zeros((zh, zw, 3)),
                     shaded=np.zeros((zh, zw), np.uint8)) for _ in zcams]
        if ap is not None:
            for a in zarr:
                a.update(grey=np.zeros((zh, zw), np.uint8))
        zouts = (RasterOut * max(len(zcams), 1))(*[
            RasterOut(a["depth"].ctypes.data_as(dp), a["face"].ctypes.data_as(POINTER(c_int)), a["points"].ctypes.data_as(dp),
                      a["normals"].ctypes.data_as(dp), a["shaded"].ctypes.data_as(POINTER(c_ubyte)),
                      a["grey"].ctypes.data_as(POINTER(c_ubyte)) if ap is not None else None) for a in zarr])
        zq = RasterRequest(zviews, len(zcams), capi.raster_params(zkw["z_min"], cull=zkw.get("cull", 0), background=zkw.get("background", 0)),
                           zouts)
    vq = None
    if visibility:
        vkw = {} if visibility is True else dict(visibility)
        unknown = set(vkw) - set(VISIBILITY_KEYS)
        if unknown:
            raise TypeError(f"unknown visibility parameters {sorted(unknown)}")
        if "z_min" not in vkw:
            raise TypeError("visibility needs z_min")
        vcolour = bool(vkw.pop("colour", False))
        if vcolour and ap is None:
            raise TypeError("visibility colour=True needs appearance")
        vq = VisibRequest(capi.visib_params(vkw.pop("z_min"), vkw.pop("depth_tol", 0.0), **vkw), int(vcolour))  # 0 = the voxel
    xq = None
    if texture:
        xkw = {} if texture is True else dict(texture)
        unknown = set(xkw) - set(TEXTURE_KEYS)
        if unknown:
            raise TypeError(f"unknown texture parameters {sorted(unknown)}")
        if "z_min" not in xkw:
            raise TypeError("texture needs z_min")
        obj_path = xkw.pop("obj_path", None)
        xq = TextureRequest(capi.texture_params(xkw.pop("z_min"), xkw.pop("depth_tol", 0.0), **xkw))  # 0 = the voxel
    lq = None
    if level:
        lkw = {} if level is True else dict(level)
        unknown = set(lkw) - set(LEVEL_KEYS)
        if unknown:
            raise TypeError(f"unknown level parameters {sorted(unknown)}")
        if xq is None:
            raise TypeError("level needs texture")
        lq = LevelRequest(capi.level_params(**lkw))
    pq = None
    if photo:
        pkw = {} if photo is True else dict(photo)
        unknown = set(pkw) - set(PHOTO_KEYS)
        if unknown:
            raise TypeError(f"unknown photo parameters {sorted(unknown)}")
        if xq is None:
            raise TypeError("photo needs texture")
        photo_prefix = pkw.pop("pgm_prefix", None)
        pq = PhotoRequest(capi.photo_params(xq.params.z_min, **pkw))  # the texture's z_min
    gq = None
    if palign:
        if not isinstance(palign, dict):
            raise TypeError("palign is a dict with cameras and images")
        gq = dict(palign)
        unknown = set(gq) - set(PALIGN_KEYS)
        if unknown:
            raise TypeError(f"unknown palign parameters {sorted(unknown)}")
        if xq is None:
            raise TypeError("palign needs texture")
        if "cameras" not in gq or "images" not in gq or len(gq["cameras"]) != len(gq["images"]):
            raise TypeError("palign needs cameras and images, one picture per camera")
        gcams, gimgs = list(gq.pop("cameras")), list(gq.pop("images"))
        glevels, gz, gpivot = int(gq.pop("levels", 1)), float(gq.pop("z_min", xq.params.z_min)), gq.pop("pivot", None)
        if glevels < 1 or not capi.palign_check_params(gz, (0.0, 0.0, 0.0) if gpivot is None else gpivot, **gq):
            raise ValueError("palign parameters outside their range")
    aq = None
    if align:
        gkw = {} if align is True else dict(align)
        unknown = set(gkw) - set(ALIGN_KEYS)
        if unknown:
            raise TypeError(f"unknown align parameters {sorted(unknown)}")
        seed = int(gkw.pop("seed", 1))
        aouts = (capi.AlignResult * max(len(pr), 1))()
        aq = AlignRequest(seed, capi.align_params(disp_min=fp.disp_min, **gkw), aouts)
    if ap is not None or cp is not None or lp is not None or gt is not None or rq is not None or aq is not None or mp is not None or tp is not None or hp is not None or zq is not None or vq is not None or xq is not None or kq is not None:
        rex = FusionResultEx()
        head = (ctx.h_, ptrs, c_int(on_dev), c_int(n), c_int(w), c_int(h), K.ctypes.data_as(dp), poses12.ctypes.data_as(dp),
                pr.ctypes.data_as(POINTER(c_int)), c_int(len(pr)), byref(sp), byref(fp), byref(ap) if ap is not None else None)
        tail = (byref(rex), ply_path.encode() if ply_path else None, warn, c_int(len(warn)))
        if kq is not None:
            rc = lib.sfmx_host_fusion_mesh_cv(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq) if aq is not None else None,
                                              byref(mp) if mp is not None else None,
                                              mcounts.ctypes.data_as(POINTER(c_int)) if mp is not None else None,
                                              byref(tp) if tp is not None else None,
                                              tcounts.ctypes.data_as(POINTER(c_int)) if tp is not None else None,
                                              byref(hp) if hp is not None else None,
                                              hcounts.ctypes.data_as(POINTER(c_int)) if hp is not None else None,
                                              byref(zq) if zq is not None else None, byref(vq) if vq is not None else None,
                                              byref(xq) if xq is not None else None, byref(lq) if lq is not None else None,
                                              byref(pq) if pq is not None else None, byref(kq), *tail)
        elif pq is not None:
            rc = lib.sfmx_host_fusion_mesh_ph(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq) if aq is not None else None,
                                              byref(mp) if mp is not None else None,
                                              mcounts.ctypes.data_as(POINTER(c_int)) if mp is not None else None,
                                              byref(tp) if tp is not None else None,
                                              tcounts.ctypes.data_as(POINTER(c_int)) if tp is not None else None,
                                              byref(hp) if hp is not None else None,
                                              hcounts.ctypes.data_as(POINTER(c_int)) if hp is not None else None,
                                              byref(zq) if zq is not None else None, byref(vq) if vq is not None else None, byref(xq),
                                              byref(lq) if lq is not None else None, byref(pq), *tail)
        elif lq is not None:
            rc = lib.sfmx_host_fusion_mesh_lv(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq) if aq is not None else None,
                                              byref(mp) if mp is not None else None,
                                              mcounts.ctypes.data_as(POINTER(c_int)) if mp is not None else None,
                                              byref(tp) if tp is not None else None,
                                              tcounts.ctypes.data_as(POINTER(c_int)) if tp is not None else None,
                                              byref(hp) if hp is not None else None,
                                              hcounts.ctypes.data_as(POINTER(c_int)) if hp is not None else None,
                                              byref(zq) if zq is not None else None, byref(vq) if vq is not None else None, byref(xq), byref(lq), *tail)
        elif xq is not None:
            rc = lib.sfmx_host_fusion_mesh_tx(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq) if aq is not None else None,
                                              byref(mp) if mp is not None else None,
                                              mcounts.ctypes.data_as(POINTER(c_int)) if mp is not None else None,
                                              byref(tp) if tp is not None else None,
                                              tcounts.ctypes.data_as(POINTER(c_int)) if tp is not None else None,
                                              byref(hp) if hp is not None else None,
                                              hcounts.ctypes.data_as(POINTER(c_int)) if hp is not None else None,
                                              byref(zq) if zq is not None else None, byref(vq) if vq is not None else None, byref(xq), *tail)
        elif vq is not None:
            rc = lib.sfmx_host_fusion_mesh_vs(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq) if aq is not None else None,
                                              byref(mp) if mp is not None else None,
                                              mcounts.ctypes.data_as(POINTER(c_int)) if mp is not None else None,
                                              byref(tp) if tp is not None else None,
                                              tcounts.ctypes.data_as(POINTER(c_int)) if tp is not None else None,
                                              byref(hp) if hp is not None else None,
                                              hcounts.ctypes.data_as(POINTER(c_int)) if hp is not None else None,
                                              byref(zq) if zq is not None else None, byref(vq), *tail)
        elif zq is not None:
            rc = lib.sfmx_host_fusion_mesh_rs(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq) if aq is not None else None,
                                              byref(mp) if mp is not None else None,
                                              mcounts.ctypes.data_as(POINTER(c_int)) if mp is not None else None,
                                              byref(tp) if tp is not None else None,
                                              tcounts.ctypes.data_as(POINTER(c_int)) if tp is not None else None,
                                              byref(hp) if hp is not None else None,
                                              hcounts.ctypes.data_as(POINTER(c_int)) if hp is not None else None, byref(zq), *tail)
        elif hp is not None:
            rc = lib.sfmx_host_fusion_mesh_fl(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq) if aq is not None else None,
                                              byref(mp) if mp is not None else None,
                                              mcounts.ctypes.data_as(POINTER(c_int)) if mp is not None else None,
                                              byref(tp) if tp is not None else None,
                                              tcounts.ctypes.data_as(POINTER(c_int)) if tp is not None else None,
                                              byref(hp), hcounts.ctypes.data_as(POINTER(c_int)), *tail)
        elif tp is not None:
            rc = lib.sfmx_host_fusion_mesh_sm(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq) if aq is not None else None,
                                              byref(mp) if mp is not None else None,
                                              mcounts.ctypes.data_as(POINTER(c_int)) if mp is not None else None,
                                              byref(tp), tcounts.ctypes.data_as(POINTER(c_int)), *tail)
        elif mp is not None:
            rc = lib.sfmx_host_fusion_mesh_sp(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq) if aq is not None else None,
                                              byref(mp), mcounts.ctypes.data_as(POINTER(c_int)), *tail)
        elif aq is not None:
            rc = lib.sfmx_host_fusion_mesh_al(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None,
                                              byref(rq) if rq is not None else None, byref(aq), *tail)
        elif rq is not None:
            rc = lib.sfmx_host_fusion_mesh_rc(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None,
                                              byref(gt) if gt is not None else None, byref(ev) if gt is not None else None, byref(rq), *tail)
        elif gt is not None:
            rc = lib.sfmx_host_fusion_mesh_ev(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None,
                                              byref(lp) if lp is not None else None,
                                              lcounts.ctypes.data_as(POINTER(c_int)) if lp is not None else None, byref(gt), byref(ev), *tail)
        elif lp is not None:
            rc = lib.sfmx_host_fusion_mesh_cl(*head, byref(cp) if cp is not None else None,
                                              counts.ctypes.data_as(POINTER(c_int)) if cp is not None else None, byref(lp),
                                              lcounts.ctypes.data_as(POINTER(c_int)), *tail)
        elif cp is not None:
            rc = lib.sfmx_host_fusion_mesh_cs(*head, byref(cp), counts.ctypes.data_as(POINTER(c_int)), *tail)
        else:
            rc = lib.sfmx_host_fusion_mesh_ex(*head, *tail)
        if rc != capi.SFMX_OK:
            if kq is not None:
                lib.sfmx_host_carve_free(byref(kq))
            raise capi.SfmxError(rc, (ctx.lib.sfmx_last_error(ctx.h_) or b"").decode() or "fuse")
        try:
            if kq is not None:
                kn = int(kq.n_views)
                car = dict(zip(capi.CARVE_COUNTS, (int(c) for c in kq.counts)),
                           inside_pixels=[int(kq.inside_pixels[i]) for i in range(kn)] if kn else [])
            if vq is not None:
                vn, vm = int(vq.n_in), int(vq.m_in)
                vis = dict(face_views=np.ctypeslib.as_array(vq.face_views, (vm,)).astype(np.int32) if vm else np.zeros(0, np.int32),
                           face_back_views=np.ctypeslib.as_array(vq.face_back_views, (vm,)).astype(np.int32) if vm else np.zeros(0, np.int32),
                           vert_views=np.ctypeslib.as_array(vq.vert_views, (vn,)).astype(np.int32) if vn else np.zeros(0, np.int32),
                           **dict(zip(capi.VISIB_COUNTS, [int(c) for c in vq.counts] + [int(c) for c in vq.pairs])))
                vis.update(verts_removed=vn - vis["verts_kept"], faces_removed=vm - vis["faces_kept"])
            if xq is not None:
                xm, xv = int(xq.n_faces), int(xq.n_views)
                xc = dict(zip(capi.TEXTURE_COUNTS, [int(c) for c in xq.counts]))
                xw, xh = xc["W"], xc["H"]
                tex = dict(atlas=np.ctypeslib.as_array(xq.atlas, (xh, xw)).copy() if xw * xh else np.zeros((0, 0), np.uint8),
                           face_view=np.ctypeslib.as_array(xq.face_view, (xm,)).astype(np.int32) if xm else np.zeros(0, np.int32),
                           face_area=np.ctypeslib.as_array(xq.face_area, (xm,)).astype(np.int64) if xm else np.zeros(0, np.int64),
                           uv_half=np.ctypeslib.as_array(xq.uv_half, (xm, 3, 2)).astype(np.int32) if xm else np.zeros((0, 3, 2), np.int32),
                           view_faces=np.ctypeslib.as_array(xq.view_faces, (xv,)).astype(np.int32) if xm and xv else np.zeros(xv, np.int32), **xc)
                tex["uv"] = capi.texture_uv(tex["uv_half"], xw, xh)
            if lq is not None:
                qm, qn = int(lq.n_faces), int(lq.n_verts)
                lev = dict(atlas=np.ctypeslib.as_array(lq.atlas, (xh, xw)).copy() if qm and xw * xh else np.zeros((xh, xw) if qm else (0, 0), np.uint8),
                           corner_adj=np.ctypeslib.as_array(lq.corner_adj, (qm, 3)).astype(np.int32) if qm else np.zeros((0, 3), np.int32),
                           corner_sample=np.ctypeslib.as_array(lq.corner_sample, (qm, 3)).astype(np.int32) if qm else np.zeros((0, 3), np.int32),
                           vertex_views=np.ctypeslib.as_array(lq.vertex_views, (qn,)).astype(np.int32) if qm and qn else np.zeros(qn, np.int32),
                           **dict(zip(capi.LEVEL_COUNTS, [int(c) for c in lq.counts])))
            if pq is not None:
                pQ, pw, ph_ = int(pq.n_views), int(pq.w), int(pq.h)
                ppx = pQ * pw * ph_
                pho = dict(rendered=np.ctypeslib.as_array(pq.rendered, (pQ, ph_, pw)).copy() if ppx else np.zeros((0, 0, 0), np.uint8),
                           cls=np.ctypeslib.as_array(pq.cls, (pQ, ph_, pw)).copy() if ppx else np.zeros((0, 0, 0), np.uint8),
                           face=np.ctypeslib.as_array(pq.face, (pQ, ph_, pw)).astype(np.int32) if ppx else np.zeros((0, 0, 0), np.int32),
                           classes=np.ctypeslib.as_array(pq.classes, (pQ, 5)).astype(np.int64) if pQ else np.zeros((0, 5), np.int64),
                           stats=np.ctypeslib.as_array(pq.stats, (pQ, 2, 3)).astype(np.int64) if pQ else np.zeros((0, 2, 3), np.int64),
                           hist=np.ctypeslib.as_array(pq.hist, (pQ, 2, 256)).astype(np.int64) if pQ else np.zeros((0, 2, 256), np.int64))
                pho["summary"] = capi.photo_summary(pho["stats"], pho["hist"])
            nv, nf = (rex.n_verts, rex.n_faces) if rex.n_faces else (0, 0)
            verts = np.ctypeslib.as_array(rex.verts, (nv, 3)).copy() if nf else np.zeros((0, 3))
            faces = np.ctypeslib.as_array(rex.faces, (nf, 3)).astype(np.int32) if nf else np.zeros((0, 3), np.int32)
            out = dict(verts=verts, faces=faces, views=int(rex.n_views), warn=warn.value.decode() or None)
            if ap is not None:
                out["normals"] = np.ctypeslib.as_array(rex.normals, (nv, 3)).copy() if nf else np.zeros((0, 3))
                out["grey"] = np.ctypeslib.as_array(rex.grey, (nv,)).copy() if nf else np.zeros(0, np.uint8)
                out["vertex_views"] = np.ctypeslib.as_array(rex.views, (nv,)).astype(np.int32) if nf else np.zeros(0, np.int32)
        finally:
            lib.sfmx_host_fusion_free_ex(byref(rex))
            if kq is not None:
                lib.sfmx_host_carve_free(byref(kq))
            if vq is not None:
                lib.sfmx_host_visib_free(byref(vq))
            if xq is not None:
                lib.sfmx_host_texture_free(byref(xq))
            if lq is not None:
                lib.sfmx_host_level_free(byref(lq))
            if pq is not None:
                lib.sfmx_host_photo_free(byref(pq))
        if kq is not None:
            out["carve"] = car
        if pq is not None:
            out["photo"] = pho
            if photo_prefix:
                for q in range(len(pho["rendered"])):
                    write_pgm(f"{photo_prefix}_{q}_photo.pgm", pho["rendered"][q])
        if vq is not None:
            out["visibility"] = vis
        if xq is not None:
            out["texture"] = tex
            if lq is not None:
                out["level"] = lev
            if obj_path:
                write_textured_obj(obj_path, out["verts"], out["faces"], tex["uv"], lev["atlas"] if lq is not None else tex["atlas"])
        if gq is not None:  # in Python, after the chain: the host library knows nothing of it
            out["palign"] = [view_register(ctx, tex, out["verts"], out["faces"], c, im, z_min=gz, lv=lev if lq is not None else None,
                                           levels=glevels, pivot=gpivot, **gq) for c, im in zip(gcams, gimgs)] if len(out["faces"]) else []
        if cp is not None:
            done = counts[:len(pr)][counts[:len(pr), 0] >= 0]
            out["consistency"] = dict(valid=[int(v) for v in done[:, 0]], kept=[int(v) for v in done[:, 1]])
        if lp is not None:
            out["clean"] = dict(zip(("components", "largest", "verts_removed", "faces_removed"), (int(v) for v in lcounts)))
        if mp is not None:
            out["simplify"] = dict(zip(("clusters", "degenerate", "duplicates", "verts_before", "faces_before"), (int(v) for v in mcounts)))
        if tp is not None:
            out["smooth"] = dict(zip(capi.SMOOTH_COUNTS, (int(v) for v in tcounts)))
        if hp is not None:
            out["fill"] = dict(zip(capi.FILL_COUNTS, (int(v) for v in hcounts)))
        if gt is not None:
            out["evaluation"] = ev.asdict()
            if ereg is not None:
                out["evaluation"] = surface_eval(ctx, out["verts"], out["faces"], gv, gf, d_max=ekw.get("d_max"), tau=ekw.get("tau"),
                                                 percentile=ekw.get("percentile", 90.0), cell=ekw.get("cell", 0.0), register=ereg)
        if rq is not None:
            out["renders"] = [dict(a, hits=int(routs[i].hits)) for i, a in enumerate(rarr)]
            if rkw.get("pgm_prefix"):
                for i, a in enumerate(rarr):
                    write_pgm(f"{rkw['pgm_prefix']}_{i}_shaded.pgm", a["shaded"])
                    if ap is not None:
                        write_pgm(f"{rkw['pgm_prefix']}_{i}_grey.pgm", a["grey"])
        if zq is not None:
            out["rasters"] = [dict(a, **dict(zip(capi.RASTER_COUNTS, (int(c) for c in zouts[i].counts))), fragments=int(zouts[i].fragments))
                              for i, a in enumerate(zarr)]
            if zkw.get("pgm_prefix"):
                for i, a in enumerate(zarr):
                    write_pgm(f"{zkw['pgm_prefix']}_{i}_mesh_shaded.pgm", a["shaded"])
                    if ap is not None:
                        write_pgm(f"{zkw['pgm_prefix']}_{i}_mesh_grey.pgm", a["grey"])
        if aq is not None:
            out["alignment"] = []
            for q in range(len(pr)):
                if aouts[q].status < 0:
                    continue
                r = aouts[q].asdict()
                n_last, e_last = r["trace"][-1][0], r["trace"][-1][1]
                out["alignment"].append(dict(pair=(int(pr[q, 0]), int(pr[q, 1])), status=r["status"], iterations=r["iterations"], n=n_last,
                                             rms=float(np.sqrt(e_last / n_last)) if n_last > 0 else float("nan"), view=r["view"]))
        return out
    res = FusionResult()
    rc = lib.sfmx_host_fusion_mesh(ctx.h_, ptrs, c_int(on_dev), c_int(n), c_int(w), c_int(h), K.ctypes.data_as(dp),
                                   poses12.ctypes.data_as(dp), pr.ctypes.data_as(POINTER(c_int)), c_int(len(pr)), byref(sp), byref(fp),
                                   byref(res), ply_path.encode() if ply_path else None, warn, c_int(len(warn)))
    if rc != capi.SFMX_OK:
        raise capi.SfmxError(rc, (ctx.lib.sfmx_last_error(ctx.h_) or b"").decode() or "fuse")
    try:
        verts = np.ctypeslib.as_array(res.verts, (res.n_verts, 3)).copy() if res.n_faces else np.zeros((0, 3))
        faces = np.ctypeslib.as_array(res.faces, (res.n_faces, 3)).astype(np.int32) if res.n_faces else np.zeros((0, 3), np.int32)
    finally:
        lib.sfmx_host_fusion_free(byref(res))
    return dict(verts=verts, faces=faces, views=int(res.n_views), warn=warn.value.decode() or None)


DEFAULTS = dict(frames=12, export_pointcloud=1, max_tracks=2200, min_tracks=900, quality=0.01, min_distance=8,
                pyr_levels=3, win_radius=5, klt_iters=10, fb_thresh=1.0, kf_min_gap=1, kf_min_inliers=200,
                kf_parallax_px=18.0, ba_window=6, ba_iters=5, ba_max_points=600, ba_huber=3.0, ba_lambda=1e-3)

_host = None


def load_host_library() -> ctypes.CDLL:
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise capi.SfmxError(capi.SFMX_ERR_NO_DEVICE, f"{HOST_LIB_PATH} not built: run __graft_entry__.build()")
        capi.load_library()
        _host = ctypes.CDLL(HOST_LIB_PATH)
        _host.sfmx_host_hypot.restype = c_double
        _host.sfmx_host_hypot.argtypes = [c_double, c_double]
        _host.sfmx_host_lane_plan.restype = ctypes.c_char_p
    return _host


def lane_plan() -> str:
    """The stream creation plan of the last warm-up of the helper contexts in this process ('' before the first run)."""
    return load_host_library().sfmx_host_lane_plan().decode()


def run(ctx: capi.Context, images: np.ndarray | None, names, K, lat=None, lon=None, cfg: dict | None = None,
        out_dir: str | None = None, images_dev: int | None = None, shape=None, timing: bool = False, comms=None, stereo: dict | None = None,
        fusion: dict | None = None):
    """Run the per-frame loop.  images: host [F,h,w] u8, or images_dev: device pointer with shape=(F,h,w).
    Returns dict(log, stats, centres, kf_poses [n][12] (camera->world R row-major + centre), kf_frames [n]).
    stereo (optional): {'kf_pair': (a, b), **params} (capi.STEREO_DEFAULTS and STEREO_MESH_DEFAULTS keys) -- after the run, the
    stereo mesh of keyframes a and b from the run's own frames: the result gains stereo_mesh = dict(verts, faces, disp16, swapped,
    rect), and out_dir gains templeRing_mesh_stereo_kf{a}_kf{b}.ply (a skipped export writes no file and one WARN log line).
    fusion (optional): {'pairs': [(a, b), ...], 'origin', 'voxel', 'dims', **params} (keyframe indices; params as fuse) -- after
    the run, fuse() on the run's own keyframe frames and kf_poses: the result gains fused_mesh = fuse()'s dict, and out_dir
    gains templeRing_mesh_fused.ply; 'appearance' (True or a dict, as fuse) adds normals and vertex grey to both;
    'consistency' (True or a dict, as fuse) filters the pairs' disparity maps against each other first; 'clean' (True or a
    dict, as fuse) removes the surface's small connected components; 'evaluate' (a dict, as fuse) evaluates the final mesh against
    a ground-truth mesh; 'render' (a dict, as fuse) ray casts the volume from further cameras; 'align' (True or a dict, as fuse) registers each later
    pair's view to the volume before it enters it; 'simplify' (True or a dict, as fuse) simplifies the final surface by exact vertex
    clustering; 'smooth' (True or a dict, as fuse) smooths it with the exact Taubin filter first; 'fill' (True or a dict, as fuse) fills its small
    holes before that; 'raster' (a dict, as fuse) renders the final mesh from further cameras; 'visibility' (a dict, as fuse) first removes
    the faces no pair's camera sees from the front; 'texture' (a dict, as fuse) bakes a texture atlas for the final mesh; 'level' (True or a dict, as fuse, with texture) levels its seams; 'photo' (True or a dict, as fuse, with texture) renders the textured mesh back into the texture's views and measures the photometric error; 'palign' (a dict, as fuse, with texture) registers further cameras to the textured mesh; 'carve' (True or a dict, as fuse) carves the volume with the pairs' silhouettes, or with hull_only builds the surface from them alone.  The run itself, its log and every other output are unchanged.
    comms (optional): (ba, ransac) capi.Comm objects -- every rank runs the same sequence, BA points and RANSAC hypotheses
    are sharded over the ranks: `ba` carries the S | b all-reduce of lane B, `ransac` the winner merges the geometry
    thread issues in program order (csrc/host/pipeline.hpp: PipelineConfig)."""
    lib = load_host_library()
    if images is not None:
        images = np.ascontiguousarray(images, np.uint8)
        F, h, w = images.shape
    else:
        F, h, w = shape
    c = PipelineCfg(**{**DEFAULTS, **(cfg or {})})
    if comms is not None:
        if len(comms) != 2:
            raise ValueError("comms = (ba, ransac)")
        c.comm_ba, c.comm_ransac = [m.h_ if m is not None else None for m in comms]
    arr = (c_char_p * F)(*[str(n).encode() for n in names])
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    lat = np.zeros(F) if lat is None else np.ascontiguousarray(lat, np.float64)
    lon = np.zeros(F) if lon is None else np.ascontiguousarray(lon, np.float64)
    has_ang = np.ones(F, np.uint8)
    log = ctypes.create_string_buffer(1 << 20)
    st = PipelineStats()
    centres = np.zeros((F, 3))
    kf_poses = np.zeros((F, 12))
    kf_frames = np.zeros(F, np.int32)
    req = res = None
    if stereo is not None:
        params = dict(stereo)
        a, b = params.pop("kf_pair")
        sp, mp = _split_stereo_params(params)
        req = StereoRequest(int(a), int(b), sp, mp)
        vcap, fcap = _grid_caps(w, h, mp.step)
        sverts, sfaces = np.zeros((vcap, 3)), np.zeros((fcap, 3), np.int32)
        sd16 = np.full((h, w), -16, np.int16)
        res = StereoResult(sverts.ctypes.data_as(POINTER(c_double)), vcap, sfaces.ctypes.data_as(POINTER(c_int)), fcap, sd16.ctypes.data_as(c_void_p))
    ctx.set_timing(timing)
    rc = lib.sfmx_pipeline_run_ex(ctx.h_, images.ctypes.data_as(c_void_p) if images is not None else None,
                                  c_void_p(images_dev) if images_dev else None, c_int(F), c_int(w), c_int(h), arr,
                                  K.ctypes.data_as(POINTER(c_double)), lat.ctypes.data_as(POINTER(c_double)),
                                  lon.ctypes.data_as(POINTER(c_double)), has_ang.ctypes.data_as(POINTER(c_ubyte)), byref(c),
                                  out_dir.encode() if out_dir else None, log, c_int(len(log)), byref(st),
                                  centres.ctypes.data_as(POINTER(c_double)), c_int(F), byref(req) if req is not None else None,
                                  byref(res) if res is not None else None, kf_poses.ctypes.data_as(POINTER(c_double)),
                                  kf_frames.ctypes.data_as(POINTER(c_int)), c_int(F))
    text = log.value.decode()
    if rc != capi.SFMX_OK:
        raise capi.SfmxError(rc, text.strip())
    n = st.n_keyframes
    out = dict(log=text, stats=st.asdict(), centres=centres[:n].copy(), kf_poses=kf_poses[:n].copy(), kf_frames=kf_frames[:n].copy())
    if res is not None:
        out["stereo_mesh"] = dict(verts=sverts[:res.n_verts].copy(), faces=sfaces[:res.n_faces].copy(), disp16=sd16,
                                  swapped=bool(res.rect.swapped), rect=res.rect.asdict())
    if fusion is not None:
        fz = dict(fusion)
        pairs, origin, voxel, dims = fz.pop("pairs"), fz.pop("origin"), fz.pop("voxel"), fz.pop("dims")
        frames = [int(f) for f in out["kf_frames"]]
        if images is not None:
            imgs, fshape = images[frames], None
        else:
            imgs, fshape = [int(images_dev) + f * h * w for f in frames], (h, w)
        ply = os.path.join(out_dir, "templeRing_mesh_fused.ply") if out_dir else None
        appearance = fz.pop("appearance", False)
        consistency = fz.pop("consistency", False)
        clean = fz.pop("clean", False)
        evaluate = fz.pop("evaluate", None)
        render = fz.pop("render", None)
        align = fz.pop("align", False)
        simplify = fz.pop("simplify", False)
        smooth = fz.pop("smooth", False)
        fill = fz.pop("fill", False)
        raster = fz.pop("raster", None)
        visibility = fz.pop("visibility", False)
        texture = fz.pop("texture", False)
        level = fz.pop("level", False)
        photo = fz.pop("photo", False)
        palign = fz.pop("palign", False)
        carve = fz.pop("carve", False)
        out["fused_mesh"] = fuse(ctx, imgs, K, out["kf_poses"], pairs, origin, voxel, dims, shape=fshape, ply_path=ply,
                                 appearance=appearance, consistency=consistency, clean=clean, evaluate=evaluate, render=render, align=align,
                                 simplify=simplify, smooth=smooth, fill=fill, raster=raster, visibility=visibility, texture=texture,
                                 level=level, photo=photo, palign=palign, carve=carve, **fz)
    return out


def find_E_ransac(ctx: capi.Context, K, pi, pj, iters: int, thr: float, min_inliers: int):
    """The find_E_ransac seam (T:646-761) of the host library on its own: dict(ok, R, t, inliers, best_iter)."""
    lib = load_host_library()
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    pi = np.ascontiguousarray(pi, np.float64)
    pj = np.ascontiguousarray(pj, np.float64)
    n = pi.shape[0]
    R, t = np.zeros((3, 3)), np.zeros(3)
    inl = np.zeros(max(n, 1), np.int32)
    n_inl, best = c_int(0), c_int(-1)
    dp = POINTER(c_double)
    rc = lib.sfmx_host_find_E_ransac(ctx.h_, K.ctypes.data_as(dp), pi.ctypes.data_as(dp), pj.ctypes.data_as(dp), c_int(n), c_int(iters),
                                     c_double(thr), c_int(min_inliers), R.ctypes.data_as(dp), t.ctypes.data_as(dp),
                                     inl.ctypes.data_as(POINTER(c_int)), byref(n_inl), byref(best))
    if rc < 0:
        raise capi.SfmxError(-rc, "find_E_ransac")
    return dict(ok=rc, R=R, t=t, inliers=inl[:n_inl.value].copy(), best_iter=best.value)


def find_E_ransac_world(ctx: capi.Context, K, pi, pj, iters: int, thr: float, min_inliers: int, world: int, as_rank: int):
    """find_E_ransac as `world` ranks run it, emulated on one GPU (test hook): each virtual rank's local winner, the merge the
    all-reduces compute, and the result as rank `as_rank` forms it."""
    lib = load_host_library()
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    pi = np.ascontiguousarray(pi, np.float64)
    pj = np.ascontiguousarray(pj, np.float64)
    n = pi.shape[0]
    R, t = np.zeros((3, 3)), np.zeros(3)
    inl = np.zeros(max(n, 1), np.int32)
    n_inl, best = c_int(0), c_int(-1)
    dp = POINTER(c_double)
    rc = lib.sfmx_host_find_E_ransac_world(ctx.h_, K.ctypes.data_as(dp), pi.ctypes.data_as(dp), pj.ctypes.data_as(dp), c_int(n), c_int(iters),
                                           c_double(thr), c_int(min_inliers), c_int(world), c_int(as_rank), R.ctypes.data_as(dp),
                                           t.ctypes.data_as(dp), inl.ctypes.data_as(POINTER(c_int)), byref(n_inl), byref(best))
    if rc < 0:
        raise capi.SfmxError(-rc, "find_E_ransac_world")
    return dict(ok=rc, R=R, t=t, inliers=inl[:n_inl.value].copy(), best_iter=best.value)


class Tracker:
    """The KLTTracker seam (T:307-400) of the host library on its own: step(image) -> (prev, cur, ids); tracks()."""

    def __init__(self, ctx: capi.Context, w: int, h: int, max_tracks=2200, min_tracks=900, quality=0.01, min_distance=8, levels=3,
                 radius=5, iters=10, fb=1.0):
        self.lib = load_host_library()
        self.cap, self.w, self.h = max_tracks, w, h
        self.lib.sfmx_host_tracker_create.restype = c_void_p
        self.h_ = c_void_p(self.lib.sfmx_host_tracker_create(ctx.h_, c_int(w), c_int(h), c_int(max_tracks), c_int(min_tracks),
                                                              c_double(quality), c_int(min_distance), c_int(levels), c_int(radius),
                                                              c_int(iters), c_double(fb)))
        if not self.h_:
            raise capi.SfmxError(capi.SFMX_ERR_INVALID, "tracker_create")

    def step(self, img: np.ndarray):
        img = np.ascontiguousarray(img, np.uint8)
        assert img.shape == (self.h, self.w)
        prev, cur = np.zeros((self.cap, 2)), np.zeros((self.cap, 2))
        ids = np.zeros(self.cap, np.int32)
        dp = POINTER(c_double)
        n = self.lib.sfmx_host_tracker_step(self.h_, img.ctypes.data_as(c_void_p), prev.ctypes.data_as(dp), cur.ctypes.data_as(dp),
                                            ids.ctypes.data_as(POINTER(c_int)), c_int(self.cap))
        if n < 0:
            raise capi.SfmxError(-n, "tracker_step")
        return prev[:n].copy(), cur[:n].copy(), ids[:n].copy()

    def tracks(self):
        xy = np.zeros((self.cap, 2))
        ids = np.zeros(self.cap, np.int32)
        n = self.lib.sfmx_host_tracker_tracks(self.h_, xy.ctypes.data_as(POINTER(c_double)), ids.ctypes.data_as(POINTER(c_int)), c_int(self.cap))
        if n < 0:
            raise capi.SfmxError(-n, "tracker_tracks")
        return xy[:n].copy(), ids[:n].copy()

    def close(self):
        if self.h_:
            self.lib.sfmx_host_tracker_destroy(self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def posegraph(ctx: capi.Context, Rs, centres, ei, ej, eR, et, is_loop):
    """posegraph_optimize_centers (T:1131-1197) of the host library on its own: (ok, centres)"""
    lib = load_host_library()
    Rs = np.ascontiguousarray(Rs, np.float64)
    c = np.ascontiguousarray(centres, np.float64).copy()
    ei, ej = np.ascontiguousarray(ei, np.int32), np.ascontiguousarray(ej, np.int32)
    eR, et = np.ascontiguousarray(eR, np.float64), np.ascontiguousarray(et, np.float64)
    lp = np.ascontiguousarray(is_loop, np.int32)
    dp, ip = POINTER(c_double), POINTER(c_int)
    rc = lib.sfmx_host_posegraph(ctx.h_, c_int(len(c)), Rs.ctypes.data_as(dp), c.ctypes.data_as(dp), c_int(len(ei)), ei.ctypes.data_as(ip),
                                 ej.ctypes.data_as(ip), eR.ctypes.data_as(dp), et.ctypes.data_as(dp), lp.ctypes.data_as(ip))
    if rc < 0:
        raise capi.SfmxError(-rc, "posegraph_optimize_centers")
    return rc, c
