"""ctypes binding of include/sfmx.h (libsfmx.so) — plumbing for tests and bench.py.

There is NO fallback: if the library is missing or no gfx950 device can be opened, every entry
point raises ``SfmxError``.  Nothing here computes anything on the CPU.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_int32, c_uint8, c_uint32, c_uint64, c_void_p

import numpy as np

# the pipeline keeps five streams busy; HIP's default of 4 hardware queues makes lanes share one.
# Only effective if the HIP runtime has not initialised yet (bench.py sets it before importing torch).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_build", "libsfmx.so")

SFMX_OK, SFMX_ERR_INVALID, SFMX_ERR_HIP, SFMX_ERR_NO_DEVICE, SFMX_ERR_SINGULAR, SFMX_ERR_UNSUPPORTED = range(6)

# every symbol include/sfmx.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "sfmx_ctx_create", "sfmx_ctx_create_prio", "sfmx_ctx_destroy", "sfmx_last_error", "sfmx_sync", "sfmx_ctx_device", "sfmx_ctx_make_current", "sfmx_stream", "sfmx_set_timing", "sfmx_get_timing",
    "sfmx_last_kernel_us", "sfmx_kernel_profile", "sfmx_kernel_profile_name", "sfmx_pyramid_create", "sfmx_pyramid_destroy", "sfmx_pyramid_upload",
    "sfmx_pyramid_set_device", "sfmx_pyramid_set_device_async", "sfmx_pyramid_wait", "sfmx_pyramid_fetched_level", "sfmx_pyramid_download_level", "sfmx_pyramid_level_size", "sfmx_shi_tomasi_score",
    "sfmx_shi_tomasi_candidates", "sfmx_shi_tomasi_candidates_pruned", "sfmx_shi_tomasi_fetch_all_keys", "sfmx_klt_track", "sfmx_ransac_score", "sfmx_ransac_score_ex", "sfmx_sampson_mask", "sfmx_ba_create",
    "sfmx_ba_reset", "sfmx_ba_destroy", "sfmx_ba_build", "sfmx_ba_step", "sfmx_ba_begin", "sfmx_ba_end", "sfmx_ba_build_partial", "sfmx_ba_step_sharded", "sfmx_ba_step_sharded_elements", "sfmx_solve_dense", "sfmx_posegraph_solve",
    "sfmx_comm_get_unique_id", "sfmx_comm_create", "sfmx_comm_destroy", "sfmx_comm_rank", "sfmx_comm_world", "sfmx_shard_range",
    "sfmx_comm_allreduce_f64", "sfmx_comm_allreduce_u64_max",
    "sfmx_debug_hypot", "sfmx_debug_divsqrt", "sfmx_debug_klt_slow_steps",
    "sfmx_stereo_default_params", "sfmx_stereo_check_params", "sfmx_stereo_create", "sfmx_stereo_destroy", "sfmx_stereo_disparity",
    "sfmx_stereo_rectify", "sfmx_stereo_last_us",
    "sfmx_fusion_default_params", "sfmx_fusion_check_params", "sfmx_fusion_create", "sfmx_fusion_destroy", "sfmx_fusion_reset",
    "sfmx_fusion_add_view", "sfmx_fusion_add_stereo_view", "sfmx_fusion_integrate", "sfmx_fusion_read", "sfmx_fusion_extract",
    "sfmx_fusion_last_us",
    "sfmx_fusion_extract_normals", "sfmx_fusion_normals_us",
    "sfmx_shade_default_params", "sfmx_shade_check_params", "sfmx_shade_create", "sfmx_shade_destroy", "sfmx_shade_reset",
    "sfmx_shade_add_view", "sfmx_shade_add_stereo_view", "sfmx_shade_view_count", "sfmx_shade_vertices", "sfmx_shade_fusion",
    "sfmx_shade_last_us",
    "sfmx_consist_default_params", "sfmx_consist_check_params", "sfmx_consist_create", "sfmx_consist_destroy", "sfmx_consist_reset",
    "sfmx_consist_add_view", "sfmx_consist_add_stereo_view", "sfmx_consist_view_count", "sfmx_consist_filter", "sfmx_consist_read",
    "sfmx_consist_counts", "sfmx_fusion_add_consist_view", "sfmx_consist_last_us",
    "sfmx_clean_default_params", "sfmx_clean_check_params", "sfmx_clean_create", "sfmx_clean_destroy", "sfmx_clean_run",
    "sfmx_clean_fusion", "sfmx_clean_read", "sfmx_clean_sizes", "sfmx_clean_device_surface", "sfmx_clean_last_us",
    "sfmx_sdist_default_params", "sfmx_sdist_check_params", "sfmx_sdist_create", "sfmx_sdist_destroy", "sfmx_sdist_set_target",
    "sfmx_sdist_set_target_fusion", "sfmx_sdist_set_target_clean", "sfmx_sdist_query", "sfmx_sdist_query_fusion",
    "sfmx_sdist_query_clean", "sfmx_sdist_stats", "sfmx_sdist_last_us",
    "sfmx_raycast_default_params", "sfmx_raycast_check_params", "sfmx_raycast_create", "sfmx_raycast_destroy", "sfmx_raycast_render",
    "sfmx_raycast_render_arrays", "sfmx_raycast_read", "sfmx_raycast_device_surface", "sfmx_raycast_shade", "sfmx_raycast_last_us",
    "sfmx_raycast_last_samples",
    "sfmx_align_default_params", "sfmx_align_check_params", "sfmx_align_create", "sfmx_align_destroy", "sfmx_align_system",
    "sfmx_align_system_arrays", "sfmx_align_view", "sfmx_align_view_arrays", "sfmx_align_stereo_view", "sfmx_align_last_us",
    "sfmx_register_default_params", "sfmx_register_check_params", "sfmx_register_create", "sfmx_register_destroy",
    "sfmx_register_set_target", "sfmx_register_pivot", "sfmx_register_system", "sfmx_register_run", "sfmx_register_apply",
    "sfmx_register_last_us", "sfmx_register_last_query_us",
    "sfmx_simplify_default_params", "sfmx_simplify_check_params", "sfmx_simplify_create", "sfmx_simplify_destroy", "sfmx_simplify_run",
    "sfmx_simplify_fusion", "sfmx_simplify_clean", "sfmx_simplify_read", "sfmx_simplify_sizes", "sfmx_simplify_counts",
    "sfmx_simplify_device_surface", "sfmx_simplify_device_mesh", "sfmx_simplify_last_us",
    "sfmx_smooth_default_params", "sfmx_smooth_check_params", "sfmx_smooth_create", "sfmx_smooth_destroy", "sfmx_smooth_run",
    "sfmx_smooth_fusion", "sfmx_smooth_clean", "sfmx_smooth_read", "sfmx_smooth_sizes", "sfmx_smooth_counts",
    "sfmx_smooth_device_mesh", "sfmx_smooth_device_surface", "sfmx_smooth_last_us",
    "sfmx_fill_default_params", "sfmx_fill_check_params", "sfmx_fill_create", "sfmx_fill_destroy", "sfmx_fill_run",
    "sfmx_fill_fusion", "sfmx_fill_clean", "sfmx_fill_read", "sfmx_fill_sizes", "sfmx_fill_counts",
    "sfmx_fill_device_mesh", "sfmx_fill_device_surface", "sfmx_fill_last_us",
    "sfmx_raster_default_params", "sfmx_raster_check_params", "sfmx_raster_create", "sfmx_raster_destroy", "sfmx_raster_run",
    "sfmx_raster_read", "sfmx_raster_counts", "sfmx_raster_device_surface", "sfmx_raster_last_us", "sfmx_raster_last_big_faces",
    "sfmx_visib_default_params", "sfmx_visib_check_params", "sfmx_visib_create", "sfmx_visib_destroy", "sfmx_visib_reset",
    "sfmx_visib_add_view", "sfmx_visib_add_stereo_view", "sfmx_visib_view_count", "sfmx_visib_set_batch", "sfmx_visib_run", "sfmx_visib_read", "sfmx_visib_sizes",
    "sfmx_visib_counts", "sfmx_visib_device_mesh", "sfmx_visib_device_surface", "sfmx_visib_last_us", "sfmx_visib_last_batch",
    "sfmx_texture_default_params", "sfmx_texture_check_params", "sfmx_texture_create", "sfmx_texture_destroy", "sfmx_texture_reset",
    "sfmx_texture_add_view", "sfmx_texture_add_stereo_view", "sfmx_texture_view_count", "sfmx_texture_set_batch", "sfmx_texture_run",
    "sfmx_texture_read", "sfmx_texture_sizes", "sfmx_texture_counts", "sfmx_texture_device_atlas", "sfmx_texture_last_us",
    "sfmx_texture_last_bake_us", "sfmx_texture_last_batch",
    "sfmx_level_default_params", "sfmx_level_check_params", "sfmx_level_create", "sfmx_level_destroy", "sfmx_level_run",
    "sfmx_level_read", "sfmx_level_counts", "sfmx_level_device_atlas", "sfmx_level_last_us", "sfmx_level_last_sweeps_us",
    "sfmx_level_last_bake_us",
    "sfmx_photo_default_params", "sfmx_photo_check_params", "sfmx_photo_create", "sfmx_photo_destroy", "sfmx_photo_reset",
    "sfmx_photo_add_view", "sfmx_photo_add_texture_views", "sfmx_photo_view_count", "sfmx_photo_set_batch", "sfmx_photo_run",
    "sfmx_photo_read", "sfmx_photo_sizes", "sfmx_photo_device_rendered", "sfmx_photo_last_us", "sfmx_photo_last_resolve_us",
    "sfmx_photo_last_batch",
    "sfmx_palign_default_params", "sfmx_palign_check_params", "sfmx_palign_create", "sfmx_palign_destroy", "sfmx_palign_set_model",
    "sfmx_palign_set_model_arrays", "sfmx_palign_set_image", "sfmx_palign_system", "sfmx_palign_view", "sfmx_palign_read", "sfmx_palign_sizes", "sfmx_palign_last_us",
    "sfmx_palign_last_zbuffer_us", "sfmx_palign_last_system_us",
    "sfmx_carve_default_params", "sfmx_carve_check_params", "sfmx_carve_create", "sfmx_carve_destroy", "sfmx_carve_reset",
    "sfmx_carve_add_view", "sfmx_carve_add_stereo_view", "sfmx_carve_inside_pixels", "sfmx_carve_view_count", "sfmx_carve_read_view", "sfmx_carve_set_batch", "sfmx_carve_run", "sfmx_carve_read",
    "sfmx_carve_apply", "sfmx_carve_count", "sfmx_carve_store", "sfmx_carve_last_us", "sfmx_carve_last_edt_us",
]


class SfmxError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"sfmx status {status}: {msg}")
        self.status = status


class KltCfg(ctypes.Structure):
    _fields_ = [("levels", c_int), ("win_radius", c_int), ("iters", c_int), ("fb_thresh", c_double)]


class StereoParams(ctypes.Structure):
    _fields_ = [("num_disparities", c_int), ("census", c_int), ("p1", c_int), ("p2", c_int), ("uniqueness", c_int),
                ("lr_max_diff", c_int), ("speckle_window", c_int), ("speckle_range", c_int)]


STEREO_DEFAULTS = dict(num_disparities=128, census=5, p1=8, p2=96, uniqueness=10, lr_max_diff=1, speckle_window=100, speckle_range=2)


def stereo_params(**kw) -> StereoParams:
    unknown = set(kw) - set(STEREO_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown stereo parameters {sorted(unknown)}")
    return StereoParams(**{**STEREO_DEFAULTS, **kw})


class FusionParams(ctypes.Structure):
    _fields_ = [("origin", c_double * 3), ("voxel", c_double), ("nx", c_int), ("ny", c_int), ("nz", c_int), ("trunc", c_double),
                ("disp_min", c_double), ("min_weight", c_int), ("max_views", c_int)]


class FusionView(ctypes.Structure):
    _fields_ = [("R_rw", c_double * 9), ("c_left", c_double * 3), ("f", c_double), ("cx", c_double), ("cy", c_double), ("B", c_double),
                ("w", c_int), ("h", c_int)]


# trunc 0 = 4 x voxel (resolved at create); the volume (origin, voxel, dims) has no default
FUSION_DEFAULTS = dict(trunc=0.0, disp_min=1.0, min_weight=1, max_views=64)


def fusion_params(origin=(0.0, 0.0, 0.0), voxel=0.0, dims=(0, 0, 0), **kw) -> FusionParams:
    unknown = set(kw) - set(FUSION_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown fusion parameters {sorted(unknown)}")
    p = FusionParams()
    p.origin[:] = [float(v) for v in origin]
    p.voxel = float(voxel)
    p.nx, p.ny, p.nz = (int(v) for v in dims)
    for k, v in {**FUSION_DEFAULTS, **kw}.items():
        setattr(p, k, v)
    return p


def fusion_default_params() -> dict:
    """sfmx_fusion_default_params as a dict (needs no device)"""
    p = FusionParams()
    load_library().sfmx_fusion_default_params(byref(p))
    return dict(origin=tuple(p.origin), voxel=p.voxel, dims=(p.nx, p.ny, p.nz), trunc=p.trunc, disp_min=p.disp_min,
                min_weight=p.min_weight, max_views=p.max_views)


def fusion_check_params(**kw) -> bool:
    """True if sfmx_fusion_create would accept the volume and parameters; needs no device"""
    return load_library().sfmx_fusion_check_params(byref(fusion_params(**kw))) == SFMX_OK


def fusion_view(cam: dict, w: int, h: int) -> FusionView:
    """cam: a rectified left camera, dict(R_rw, c_left, f, cx, cy, B) (e.g. pipeline.stereo_rectify's result)"""
    v = FusionView()
    v.R_rw[:] = [float(x) for x in np.asarray(cam["R_rw"], np.float64).ravel()]
    v.c_left[:] = [float(x) for x in np.asarray(cam["c_left"], np.float64).ravel()]
    v.f, v.cx, v.cy, v.B = float(cam["f"]), float(cam["cx"]), float(cam["cy"]), float(cam["B"])
    v.w, v.h = int(w), int(h)
    return v


class ShadeParams(ctypes.Structure):
    _fields_ = [("depth_tol", c_double), ("disp_min", c_double), ("cull", c_int), ("fill", c_int)]


# depth_tol has no default at this level (pipeline.fuse uses the volume's trunc)
SHADE_DEFAULTS = dict(disp_min=1.0, cull=1, fill=0)


def shade_params(depth_tol=0.0, **kw) -> ShadeParams:
    unknown = set(kw) - set(SHADE_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown shade parameters {sorted(unknown)}")
    kw = {**SHADE_DEFAULTS, **kw}
    return ShadeParams(float(depth_tol), float(kw["disp_min"]), int(kw["cull"]), int(kw["fill"]))


def shade_default_params() -> dict:
    """sfmx_shade_default_params as a dict (needs no device)"""
    p = ShadeParams()
    load_library().sfmx_shade_default_params(byref(p))
    return dict(depth_tol=p.depth_tol, disp_min=p.disp_min, cull=p.cull, fill=p.fill)


def shade_check_params(**kw) -> bool:
    """True if sfmx_shade_vertices / _fusion would accept the parameters; needs no device"""
    return load_library().sfmx_shade_check_params(byref(shade_params(**kw))) == SFMX_OK


class ConsistParams(ctypes.Structure):
    _fields_ = [("rel_tol", c_double), ("reproj_px", c_double), ("disp_min", c_double), ("min_support", c_int)]


CONSIST_DEFAULTS = dict(rel_tol=0.01, reproj_px=1.0, disp_min=1.0, min_support=2)


def consist_params(**kw) -> ConsistParams:
    unknown = set(kw) - set(CONSIST_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown consist parameters {sorted(unknown)}")
    kw = {**CONSIST_DEFAULTS, **kw}
    return ConsistParams(float(kw["rel_tol"]), float(kw["reproj_px"]), float(kw["disp_min"]), int(kw["min_support"]))


def consist_default_params() -> dict:
    """sfmx_consist_default_params as a dict (needs no device)"""
    p = ConsistParams()
    load_library().sfmx_consist_default_params(byref(p))
    return dict(rel_tol=p.rel_tol, reproj_px=p.reproj_px, disp_min=p.disp_min, min_support=p.min_support)


def consist_check_params(**kw) -> bool:
    """True if sfmx_consist_filter would accept the parameters; needs no device"""
    return load_library().sfmx_consist_check_params(byref(consist_params(**kw))) == SFMX_OK


class CarveParams(ctypes.Structure):
    _fields_ = [("cap", c_int), ("min_views", c_int), ("margin", c_double), ("mode", c_int), ("trunc", c_double)]


class CarveVolume(ctypes.Structure):
    _fields_ = [("origin", c_double * 3), ("voxel", c_double), ("nx", c_int), ("ny", c_int), ("nz", c_int)]


CARVE_MODES = ("intersect", "clear")
CARVE_COUNTS = ("defined", "outside", "changed")
CARVE_DEFAULTS = dict(cap=16, min_views=1, margin=0.5, mode="intersect", trunc=0.0)


def carve_params(**kw) -> CarveParams:
    unknown = set(kw) - set(CARVE_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown carve parameters {sorted(unknown)}")
    kw = {**CARVE_DEFAULTS, **kw}
    for k in ("cap", "min_views"):
        if isinstance(kw[k], (bool, np.bool_)) or not isinstance(kw[k], (int, np.integer)):
            raise TypeError(f"carve {k} is an int")
    mode = kw["mode"]
    if isinstance(mode, str):
        if mode not in CARVE_MODES:
            raise ValueError(f"carve mode is one of {CARVE_MODES}")
        mode = CARVE_MODES.index(mode)
    return CarveParams(int(kw["cap"]), int(kw["min_views"]), float(kw["margin"]), int(mode), float(kw["trunc"]))


def carve_default_params() -> dict:
    """sfmx_carve_default_params as a dict (needs no device)"""
    p = CarveParams()
    load_library().sfmx_carve_default_params(byref(p))
    return dict(cap=p.cap, min_views=p.min_views, margin=p.margin, mode=CARVE_MODES[p.mode], trunc=p.trunc)


def carve_check_params(**kw) -> bool:
    """True if the sfmx_carve entries would accept the parameters; needs no device"""
    return load_library().sfmx_carve_check_params(byref(carve_params(**kw))) == SFMX_OK


class CleanParams(ctypes.Structure):
    _fields_ = [("min_faces", c_int), ("min_permille", c_int)]


CLEAN_DEFAULTS = dict(min_faces=0, min_permille=10)


def clean_params(**kw) -> CleanParams:
    unknown = set(kw) - set(CLEAN_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown clean parameters {sorted(unknown)}")
    kw = {**CLEAN_DEFAULTS, **kw}
    return CleanParams(int(kw["min_faces"]), int(kw["min_permille"]))


def clean_default_params() -> dict:
    """sfmx_clean_default_params as a dict (needs no device)"""
    p = CleanParams()
    load_library().sfmx_clean_default_params(byref(p))
    return dict(min_faces=p.min_faces, min_permille=p.min_permille)


def clean_check_params(**kw) -> bool:
    """True if sfmx_clean_run / _fusion would accept the parameters; needs no device"""
    return load_library().sfmx_clean_check_params(byref(clean_params(**kw))) == SFMX_OK


class SimplifyParams(ctypes.Structure):
    _fields_ = [("cell", c_double), ("origin", c_double * 3)]


# cell has no default (a length in the caller's units)
SIMPLIFY_DEFAULTS = dict(origin=(0.0, 0.0, 0.0))


def simplify_params(cell=0.0, **kw) -> SimplifyParams:
    unknown = set(kw) - set(SIMPLIFY_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown simplify parameters {sorted(unknown)}")
    kw = {**SIMPLIFY_DEFAULTS, **kw}
    p = SimplifyParams()
    p.cell = float(cell)
    p.origin[:] = [float(v) for v in kw["origin"]]
    return p


def simplify_default_params() -> dict:
    """sfmx_simplify_default_params as a dict (needs no device)"""
    p = SimplifyParams()
    load_library().sfmx_simplify_default_params(byref(p))
    return dict(cell=p.cell, origin=tuple(p.origin))


def simplify_check_params(cell=0.0, **kw) -> bool:
    """True if sfmx_simplify_run / _fusion / _clean would accept the parameters; needs no device"""
    return load_library().sfmx_simplify_check_params(byref(simplify_params(cell, **kw))) == SFMX_OK


class SmoothParams(ctypes.Structure):
    _fields_ = [("unit", c_double), ("origin", c_double * 3), ("lam", c_double), ("mu", c_double), ("iters", c_int), ("pin", c_int)]


# unit has no default (a length in the caller's units: the voxel in the pipeline)
SMOOTH_DEFAULTS = dict(origin=(0.0, 0.0, 0.0), lam=0.5, mu=-0.53, iters=10, pin=1)
SMOOTH_COUNTS = ("edges", "boundary_edges", "irregular_edges", "pinned", "isolated")


def smooth_params(unit=0.0, **kw) -> SmoothParams:
    unknown = set(kw) - set(SMOOTH_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown smooth parameters {sorted(unknown)}")
    kw = {**SMOOTH_DEFAULTS, **kw}
    p = SmoothParams()
    p.unit = float(unit)
    p.origin[:] = [float(v) for v in kw["origin"]]
    p.lam, p.mu = float(kw["lam"]), float(kw["mu"])
    if int(kw["iters"]) != kw["iters"] or int(kw["pin"]) != kw["pin"]:
        raise TypeError("smooth parameters iters and pin are integers")
    p.iters, p.pin = int(kw["iters"]), int(kw["pin"])
    return p


def smooth_default_params() -> dict:
    """sfmx_smooth_default_params as a dict (needs no device)"""
    p = SmoothParams()
    load_library().sfmx_smooth_default_params(byref(p))
    return dict(unit=p.unit, origin=tuple(p.origin), lam=p.lam, mu=p.mu, iters=p.iters, pin=p.pin)


def smooth_check_params(unit=0.0, **kw) -> bool:
    """True if sfmx_smooth_run / _fusion / _clean would accept the parameters; needs no device"""
    return load_library().sfmx_smooth_check_params(byref(smooth_params(unit, **kw))) == SFMX_OK


class FillParams(ctypes.Structure):
    _fields_ = [("unit", c_double), ("origin", c_double * 3), ("max_edges", c_int)]


# unit has no default (a length in the caller's units: the voxel in the pipeline)
FILL_DEFAULTS = dict(origin=(0.0, 0.0, 0.0), max_edges=32)
FILL_COUNTS = ("edges", "boundary_edges", "irregular_edges", "complex_vertices", "filled_loops", "filled_edges", "new_verts", "new_faces")


def fill_params(unit=0.0, **kw) -> FillParams:
    unknown = set(kw) - set(FILL_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown fill parameters {sorted(unknown)}")
    kw = {**FILL_DEFAULTS, **kw}
    p = FillParams()
    p.unit = float(unit)
    p.origin[:] = [float(v) for v in kw["origin"]]
    if int(kw["max_edges"]) != kw["max_edges"]:
        raise TypeError("fill parameter max_edges is an integer")
    p.max_edges = int(kw["max_edges"])
    return p


def fill_default_params() -> dict:
    """sfmx_fill_default_params as a dict (needs no device)"""
    p = FillParams()
    load_library().sfmx_fill_default_params(byref(p))
    return dict(unit=p.unit, origin=tuple(p.origin), max_edges=p.max_edges)


def fill_check_params(unit=0.0, **kw) -> bool:
    """True if sfmx_fill_run / _fusion / _clean would accept the parameters; needs no device"""
    return load_library().sfmx_fill_check_params(byref(fill_params(unit, **kw))) == SFMX_OK


class SdistParams(ctypes.Structure):
    _fields_ = [("d_max", c_double), ("cell", c_double)]


SDIST_CHUNK = 64  # SFMX_SDIST_CHUNK: triangles of a cell staged through LDS at a time


def sdist_params(d_max, cell=0.0) -> SdistParams:
    """d_max has no default (a length in the caller's units); cell 0 = auto"""
    return SdistParams(float(d_max), float(cell))


def sdist_default_params() -> dict:
    """sfmx_sdist_default_params as a dict (needs no device)"""
    p = SdistParams()
    load_library().sfmx_sdist_default_params(byref(p))
    return dict(d_max=p.d_max, cell=p.cell)


def sdist_check_params(d_max, cell=0.0) -> bool:
    """True if sfmx_sdist_set_target would accept the parameters; needs no device"""
    return load_library().sfmx_sdist_check_params(byref(sdist_params(d_max, cell))) == SFMX_OK


class RaycastParams(ctypes.Structure):
    _fields_ = [("z_min", c_double), ("z_max", c_double), ("step", c_double), ("min_weight", c_int), ("background", c_uint8)]


RAYCAST_MAX_SAMPLES, RAYCAST_MAX_PIXELS = 1 << 20, 1 << 24  # SFMX_RAYCAST_MAX_SAMPLES / _PIXELS


def raycast_params(z_min=0.0, z_max=0.0, step=0.0, min_weight=0, background=0) -> RaycastParams:
    """z_min and z_max have no default (depths in the volume's units); step 0 = voxel / 2, min_weight 0 = the volume's own"""
    if not 0 <= int(background) <= 255:
        raise ValueError(f"background = {background} is not a byte")
    return RaycastParams(float(z_min), float(z_max), float(step), int(min_weight), int(background))


def raycast_default_params() -> dict:
    """sfmx_raycast_default_params as a dict (needs no device)"""
    p = RaycastParams()
    load_library().sfmx_raycast_default_params(byref(p))
    return dict(z_min=p.z_min, z_max=p.z_max, step=p.step, min_weight=p.min_weight, background=p.background)


def raycast_check_params(**kw) -> bool:
    """True if sfmx_raycast_render would accept the parameters (a step of 0 is checked again against the voxel); needs no device"""
    return load_library().sfmx_raycast_check_params(byref(raycast_params(**kw))) == SFMX_OK


class RasterParams(ctypes.Structure):
    _fields_ = [("z_min", c_double), ("cull", c_int), ("background", c_uint8)]


# z_min has no default (a depth in the mesh's units)
RASTER_DEFAULTS = dict(cull=0, background=0)
RASTER_COUNTS = ("faces_behind", "faces_outside", "faces_degenerate", "faces_back", "faces_culled", "faces_drawn", "hits", "back_pixels")
RASTER_MAX_PIXELS, RASTER_MAX_VERTS, RASTER_MAX_FACES = 1 << 24, 1 << 24, 1 << 30  # SFMX_RASTER_MAX_*


def raster_params(z_min=0.0, **kw) -> RasterParams:
    unknown = set(kw) - set(RASTER_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown raster parameters {sorted(unknown)}")
    kw = {**RASTER_DEFAULTS, **kw}
    if int(kw["cull"]) != kw["cull"]:
        raise TypeError("raster parameter cull is an integer")
    if not 0 <= int(kw["background"]) <= 255:
        raise ValueError(f"background = {kw['background']} is not a byte")
    return RasterParams(float(z_min), int(kw["cull"]), int(kw["background"]))


def raster_default_params() -> dict:
    """sfmx_raster_default_params as a dict (needs no device)"""
    p = RasterParams()
    load_library().sfmx_raster_default_params(byref(p))
    return dict(z_min=p.z_min, cull=p.cull, background=p.background)


def raster_check_params(z_min=0.0, **kw) -> bool:
    """True if sfmx_raster_run would accept the parameters; needs no device"""
    return load_library().sfmx_raster_check_params(byref(raster_params(z_min, **kw))) == SFMX_OK


class VisibParams(ctypes.Structure):
    _fields_ = [("z_min", c_double), ("depth_tol", c_double), ("min_views", c_int), ("cull", c_int), ("fill", c_int)]


# z_min and depth_tol have no default (lengths in the mesh's units)
VISIB_DEFAULTS = dict(min_views=1, cull=1, fill=0)
VISIB_COUNTS = ("faces_seen", "faces_back_only", "faces_unseen", "faces_kept", "verts_kept", "pairs_visible", "pairs_occluded", "pairs_off")
VISIB_MAX_BATCH = 64


def visib_params(z_min=0.0, depth_tol=-1.0, **kw) -> VisibParams:
    unknown = set(kw) - set(VISIB_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown visibility parameters {sorted(unknown)}")
    kw = {**VISIB_DEFAULTS, **kw}
    for k in VISIB_DEFAULTS:
        if int(kw[k]) != kw[k]:
            raise TypeError(f"visibility parameter {k} is an integer")
    return VisibParams(float(z_min), float(depth_tol), int(kw["min_views"]), int(kw["cull"]), int(kw["fill"]))


def visib_default_params() -> dict:
    """sfmx_visib_default_params as a dict (needs no device)"""
    p = VisibParams()
    load_library().sfmx_visib_default_params(byref(p))
    return {k: getattr(p, k) for k, _ in VisibParams._fields_}


def visib_check_params(z_min=0.0, depth_tol=-1.0, **kw) -> bool:
    """True if sfmx_visib_run would accept the parameters; needs no device"""
    return load_library().sfmx_visib_check_params(byref(visib_params(z_min, depth_tol, **kw))) == SFMX_OK


class TextureParams(ctypes.Structure):
    _fields_ = [("z_min", c_double), ("depth_tol", c_double), ("patch", c_int), ("cells_per_row", c_int), ("fill", c_int)]


# z_min and depth_tol have no default (lengths in the mesh's units)
TEXTURE_DEFAULTS = dict(patch=8, cells_per_row=0, fill=0)
TEXTURE_COUNTS = ("faces_textured", "faces_untextured", "cells", "W", "H", "cells_per_row")


def texture_params(z_min=0.0, depth_tol=-1.0, **kw) -> TextureParams:
    unknown = set(kw) - set(TEXTURE_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown texture parameters {sorted(unknown)}")
    kw = {**TEXTURE_DEFAULTS, **kw}
    for k in TEXTURE_DEFAULTS:
        if int(kw[k]) != kw[k]:
            raise TypeError(f"texture parameter {k} is an integer")
    return TextureParams(float(z_min), float(depth_tol), int(kw["patch"]), int(kw["cells_per_row"]), int(kw["fill"]))


def texture_default_params() -> dict:
    """sfmx_texture_default_params as a dict (needs no device)"""
    p = TextureParams()
    load_library().sfmx_texture_default_params(byref(p))
    return {k: getattr(p, k) for k, _ in TextureParams._fields_}


def texture_check_params(z_min=0.0, depth_tol=-1.0, **kw) -> bool:
    """True if sfmx_texture_run would accept the parameters; needs no device"""
    return load_library().sfmx_texture_check_params(byref(texture_params(z_min, depth_tol, **kw))) == SFMX_OK


def texture_uv(uv_half, W, H):
    """float64 [m][3][2] from the corners in half-texels: u = hx / (2 W), v = 1 - hy / (2 H) (zeros for an empty atlas)"""
    uvh = np.asarray(uv_half, np.float64)
    out = np.zeros(uvh.shape)
    if W and H:
        out[..., 0] = uvh[..., 0] / (2.0 * W)
        out[..., 1] = 1.0 - uvh[..., 1] / (2.0 * H)
    return out


class LevelParams(ctypes.Structure):
    _fields_ = [("iterations", c_int)]


LEVEL_DEFAULTS = dict(iterations=64)
LEVEL_COUNTS = ("nodes", "seam_vertices", "pinned_nodes", "free_nodes", "node_edges", "iterations")


def level_params(**kw) -> LevelParams:
    unknown = set(kw) - set(LEVEL_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown level parameters {sorted(unknown)}")
    kw = {**LEVEL_DEFAULTS, **kw}
    if int(kw["iterations"]) != kw["iterations"]:
        raise TypeError("level parameter iterations is an integer")
    return LevelParams(int(kw["iterations"]))


def level_default_params() -> dict:
    """sfmx_level_default_params as a dict (needs no device)"""
    p = LevelParams()
    load_library().sfmx_level_default_params(byref(p))
    return {k: getattr(p, k) for k, _ in LevelParams._fields_}


def level_check_params(**kw) -> bool:
    """True if sfmx_level_run would accept the parameters; needs no device"""
    return load_library().sfmx_level_check_params(byref(level_params(**kw))) == SFMX_OK


class PhotoParams(ctypes.Structure):
    _fields_ = [("z_min", c_double), ("background", c_uint8)]


# z_min has no default (a depth in the mesh's units)
PHOTO_DEFAULTS = dict(background=0)
PHOTO_CLASSES = ("empty", "back", "untextured", "own", "cross")
PHOTO_MAX_PIXELS = 1 << 28  # the sum of w h over the views


def photo_params(z_min=0.0, **kw) -> PhotoParams:
    unknown = set(kw) - set(PHOTO_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown photo parameters {sorted(unknown)}")
    kw = {**PHOTO_DEFAULTS, **kw}
    if int(kw["background"]) != kw["background"]:
        raise TypeError("photo parameter background is an integer")
    if not 0 <= int(kw["background"]) <= 255:
        raise ValueError(f"background = {kw['background']} is not a byte")
    return PhotoParams(float(z_min), int(kw["background"]))


def photo_default_params() -> dict:
    """sfmx_photo_default_params as a dict (needs no device)"""
    p = PhotoParams()
    load_library().sfmx_photo_default_params(byref(p))
    return dict(z_min=p.z_min, background=p.background)


def photo_check_params(z_min=0.0, **kw) -> bool:
    """True if sfmx_photo_run would accept the parameters; needs no device"""
    return load_library().sfmx_photo_check_params(byref(photo_params(z_min, **kw))) == SFMX_OK


def _photo_measures(stats3, hist256) -> dict:
    cnt, sd, sd2 = (int(x) for x in stats3)
    if cnt == 0:
        return dict(count=0, mae=None, rmse=None, psnr=None, p90=None)
    # the 90th percentile: the smallest d with at least 0.9 count pixels at or below it (integers: 10 cum >= 9 count)
    cum, p90 = 0, 255
    for d in range(256):
        cum += int(hist256[d])
        if 10 * cum >= 9 * cnt:
            p90 = d
            break
    import math
    return dict(count=cnt, mae=sd / cnt, rmse=math.sqrt(sd2 / cnt),
                psnr=float("inf") if sd2 == 0 else 10.0 * math.log10(255.0 * 255.0 * cnt / sd2), p90=p90)


def photo_summary(stats, hist) -> dict:
    """stats int64 [Q][2][3] and hist int64 [Q][2][256] of a Photo run -> dict(views=[dict(own=, cross=) per view], own=, cross=
    pooled over the views), each dict(count, mae = sum d / count, rmse, psnr = 10 log10(255^2 count / sum d^2) or inf at 0, p90:
    the smallest d with 10 cum(d) >= 9 count); None where count is 0.  Plain Python arithmetic on the integers."""
    stats = np.asarray(stats, np.int64).reshape(-1, 2, 3)
    hist = np.asarray(hist, np.int64).reshape(-1, 2, 256)
    assert len(stats) == len(hist)
    views = [dict(own=_photo_measures(stats[q, 0], hist[q, 0]), cross=_photo_measures(stats[q, 1], hist[q, 1])) for q in range(len(stats))]
    pooled = {}
    for o, name in enumerate(("own", "cross")):
        st = [sum(int(stats[q, o, j]) for q in range(len(stats))) for j in range(3)]
        hs = [sum(int(hist[q, o, d]) for q in range(len(hist))) for d in range(256)]
        pooled[name] = _photo_measures(st, hs)
    return dict(views=views, **pooled)


ALIGN_ITERS_CAP = 64  # SFMX_ALIGN_ITERS_CAP
ALIGN_CONVERGED, ALIGN_MAX_ITERS, ALIGN_TOO_FEW, ALIGN_DEGENERATE = range(4)
ALIGN_STATUS = ("CONVERGED", "MAX_ITERS", "TOO_FEW", "DEGENERATE")


class AlignParams(ctypes.Structure):
    _fields_ = [("max_iters", c_int), ("stride", c_int), ("disp_min", c_double), ("min_weight", c_int), ("min_pixels", c_int),
                ("damping", c_double), ("eps_rot", c_double), ("eps_trans", c_double)]


class AlignResult(ctypes.Structure):
    _fields_ = [("view", FusionView), ("status", c_int), ("iterations", c_int), ("n", c_int32 * ALIGN_ITERS_CAP),
                ("e", c_double * ALIGN_ITERS_CAP), ("rot", c_double * ALIGN_ITERS_CAP), ("trans", c_double * ALIGN_ITERS_CAP)]

    def asdict(self) -> dict:
        """dict(view=dict(R_rw, c_left, f, cx, cy, B, w, h), status, iterations, trace=[(n, e, |omega|, |v|), ...])"""
        v = self.view
        k = int(self.iterations)
        return dict(view=dict(R_rw=np.array(v.R_rw[:]).reshape(3, 3), c_left=np.array(v.c_left[:]), f=v.f, cx=v.cx, cy=v.cy, B=v.B,
                              w=int(v.w), h=int(v.h)),
                    status=int(self.status), iterations=k,
                    trace=[(int(self.n[i]), float(self.e[i]), float(self.rot[i]), float(self.trans[i])) for i in range(k)])


ALIGN_DEFAULTS = dict(max_iters=10, stride=1, disp_min=1.0, min_weight=0, min_pixels=64, damping=0.0, eps_rot=1e-6, eps_trans=1e-4)


def align_params(**kw) -> AlignParams:
    unknown = set(kw) - set(ALIGN_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown align parameters {sorted(unknown)}")
    d = {**ALIGN_DEFAULTS, **kw}
    return AlignParams(int(d["max_iters"]), int(d["stride"]), float(d["disp_min"]), int(d["min_weight"]), int(d["min_pixels"]),
                       float(d["damping"]), float(d["eps_rot"]), float(d["eps_trans"]))


def align_default_params() -> dict:
    """sfmx_align_default_params as a dict (needs no device)"""
    p = AlignParams()
    load_library().sfmx_align_default_params(byref(p))
    return {k: getattr(p, k) for k, _ in AlignParams._fields_}


def align_check_params(**kw) -> bool:
    """True if the sfmx_align entries would accept the parameters; needs no device"""
    return load_library().sfmx_align_check_params(byref(align_params(**kw))) == SFMX_OK


PALIGN_ITERS_CAP = 64  # SFMX_PALIGN_ITERS_CAP
PALIGN_MARGIN_CAP = 64  # SFMX_PALIGN_MARGIN_CAP
PALIGN_STATUS = ("CONVERGED", "MAX_ITERS", "TOO_FEW", "DEGENERATE")


class PAlignParams(ctypes.Structure):
    _fields_ = [("z_min", c_double), ("pivot", c_double * 3), ("max_iters", c_int), ("stride", c_int), ("margin", c_int),
                ("min_pixels", c_int), ("r_max", c_double), ("damping", c_double), ("eps_rot", c_double), ("eps_trans", c_double)]


class PAlignResult(ctypes.Structure):
    _fields_ = AlignResult._fields_

    asdict = AlignResult.asdict


# z_min and pivot have no default (a depth and a point in the mesh's units)
PALIGN_DEFAULTS = dict(max_iters=10, stride=1, margin=4, min_pixels=64, r_max=255.0, damping=0.0, eps_rot=5e-5, eps_trans=1e-6)


def palign_params(z_min=0.0, pivot=(0.0, 0.0, 0.0), **kw) -> PAlignParams:
    unknown = set(kw) - set(PALIGN_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown palign parameters {sorted(unknown)}")
    d = {**PALIGN_DEFAULTS, **kw}
    p = PAlignParams()
    p.z_min = float(z_min)
    p.pivot[:] = [float(v) for v in np.asarray(pivot, np.float64).reshape(3)]
    for k in ("max_iters", "stride", "margin", "min_pixels"):
        setattr(p, k, int(d[k]))
    for k in ("r_max", "damping", "eps_rot", "eps_trans"):
        setattr(p, k, float(d[k]))
    return p


def palign_default_params() -> dict:
    """sfmx_palign_default_params as a dict (needs no device); z_min and pivot come back as zeros: they have no default"""
    p = PAlignParams()
    load_library().sfmx_palign_default_params(byref(p))
    return {k: (tuple(p.pivot) if k == "pivot" else getattr(p, k)) for k, _ in PAlignParams._fields_}


def palign_check_params(z_min=0.0, pivot=(0.0, 0.0, 0.0), **kw) -> bool:
    """True if the sfmx_palign entries would accept the parameters; needs no device"""
    return load_library().sfmx_palign_check_params(byref(palign_params(z_min, pivot, **kw))) == SFMX_OK


REGISTER_ITERS_CAP = 64  # SFMX_REGISTER_ITERS_CAP
REGISTER_TERMS = 37      # SFMX_REGISTER_TERMS
REGISTER_STATUS = ("CONVERGED", "MAX_ITERS", "TOO_FEW", "DEGENERATE")


class RegisterParams(ctypes.Structure):
    _fields_ = [("d_max", c_double), ("cell", c_double), ("max_iters", c_int), ("stride", c_int), ("min_points", c_int),
                ("with_scale", c_int), ("damping", c_double), ("eps_rot", c_double), ("eps_scale", c_double), ("eps_trans", c_double)]


class RegisterTransform(ctypes.Structure):
    _fields_ = [("s", c_double), ("R", c_double * 9), ("t", c_double * 3)]

    def asdict(self) -> dict:
        return dict(s=float(self.s), R=np.array(self.R[:]).reshape(3, 3), t=np.array(self.t[:]))


class RegisterResult(ctypes.Structure):
    _fields_ = [("T", RegisterTransform), ("status", c_int), ("iterations", c_int), ("n", c_int32 * REGISTER_ITERS_CAP),
                ("e", c_double * REGISTER_ITERS_CAP), ("c", c_double * REGISTER_ITERS_CAP), ("rot", c_double * REGISTER_ITERS_CAP),
                ("trans", c_double * REGISTER_ITERS_CAP), ("sigma", c_double * REGISTER_ITERS_CAP)]

    def asdict(self) -> dict:
        """dict(T=dict(s, R, t), status, iterations, trace=[(n_used, e, c, |omega|, |v|, sigma), ...])"""
        k = int(self.iterations)
        return dict(T=self.T.asdict(), status=int(self.status), iterations=k,
                    trace=[(int(self.n[i]), float(self.e[i]), float(self.c[i]), float(self.rot[i]), float(self.trans[i]),
                            float(self.sigma[i])) for i in range(k)])


# d_max has no default (a length in the caller's units)
REGISTER_DEFAULTS = dict(cell=0.0, max_iters=20, stride=1, min_points=16, with_scale=1, damping=0.0, eps_rot=1e-4, eps_scale=1e-4,
                         eps_trans=1e-3)


def register_params(d_max, **kw) -> RegisterParams:
    unknown = set(kw) - set(REGISTER_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown register parameters {sorted(unknown)}")
    d = {**REGISTER_DEFAULTS, **kw}
    return RegisterParams(float(d_max), float(d["cell"]), int(d["max_iters"]), int(d["stride"]), int(d["min_points"]),
                          int(bool(d["with_scale"])), float(d["damping"]), float(d["eps_rot"]), float(d["eps_scale"]), float(d["eps_trans"]))


def register_default_params() -> dict:
    """sfmx_register_default_params as a dict (needs no device)"""
    p = RegisterParams()
    load_library().sfmx_register_default_params(byref(p))
    return {k: getattr(p, k) for k, _ in RegisterParams._fields_}


def register_check_params(d_max, **kw) -> bool:
    """True if the sfmx_register entries would accept the parameters; needs no device"""
    return load_library().sfmx_register_check_params(byref(register_params(d_max, **kw))) == SFMX_OK


def register_transform(T=None) -> RegisterTransform:
    """T: None (the identity), or dict(s, R [3][3], t [3])"""
    if T is None:
        T = dict(s=1.0, R=np.eye(3), t=np.zeros(3))
    unknown = set(T) - {"s", "R", "t"}
    if unknown or set(T) != {"s", "R", "t"}:
        raise TypeError("a transform is dict(s=, R=, t=)")
    R, t = _f64(T["R"]).reshape(9), _f64(T["t"]).reshape(3)
    return RegisterTransform(float(T["s"]), (c_double * 9)(*R), (c_double * 3)(*t))


def stereo_check_params(w: int, h: int, **kw) -> bool:
    """True if sfmx_stereo_create would accept (w, h, params); needs no device"""
    return load_library().sfmx_stereo_check_params(c_int(w), c_int(h), byref(stereo_params(**kw))) == SFMX_OK


_lib = None


def load_library() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SfmxError(SFMX_ERR_NO_DEVICE, f"{LIB_PATH} not built: run __graft_entry__.build() (hipcc, gfx950)")
        # PyTorch-ROCm ships its own libamdhip64.so.7; load it first so that torch (device memory,
        # torch.distributed) and libsfmx share ONE HIP runtime in this process.
        if "torch" not in __import__("sys").modules and not os.environ.get("SFMX_NO_TORCH_PRELOAD"):
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.sfmx_last_error.restype = c_char_p
        _lib.sfmx_last_kernel_us.restype = c_double
        _lib.sfmx_stream.restype = c_void_p
        _lib.sfmx_kernel_profile_name.restype = c_char_p
        _lib.sfmx_debug_klt_slow_steps.restype = c_uint64
        _lib.sfmx_stereo_last_us.restype = c_double
        _lib.sfmx_fusion_last_us.restype = c_double
        _lib.sfmx_fusion_normals_us.restype = c_double
        _lib.sfmx_shade_last_us.restype = c_double
        _lib.sfmx_consist_last_us.restype = c_double
        _lib.sfmx_clean_last_us.restype = c_double
        _lib.sfmx_sdist_last_us.restype = c_double
        _lib.sfmx_raycast_last_us.restype = c_double
        _lib.sfmx_raycast_last_samples.restype = c_uint64
        _lib.sfmx_align_last_us.restype = c_double
        _lib.sfmx_register_last_us.restype = c_double
        _lib.sfmx_register_last_query_us.restype = c_double
        _lib.sfmx_simplify_last_us.restype = c_double
        _lib.sfmx_smooth_last_us.restype = c_double
        _lib.sfmx_fill_last_us.restype = c_double
        _lib.sfmx_raster_last_us.restype = c_double
        _lib.sfmx_visib_last_us.restype = c_double
        _lib.sfmx_texture_last_us.restype = c_double
        _lib.sfmx_texture_last_bake_us.restype = c_double
        _lib.sfmx_level_last_us.restype = c_double
        _lib.sfmx_level_last_sweeps_us.restype = c_double
        _lib.sfmx_level_last_bake_us.restype = c_double
        _lib.sfmx_photo_last_us.restype = c_double
        _lib.sfmx_photo_last_resolve_us.restype = c_double
        _lib.sfmx_palign_last_us.restype = c_double
        _lib.sfmx_palign_last_zbuffer_us.restype = c_double
        _lib.sfmx_palign_last_system_us.restype = c_double
        _lib.sfmx_carve_last_us.restype = c_double
        _lib.sfmx_carve_last_edt_us.restype = c_double
    return _lib


def _p(a, t):
    return a.ctypes.data_as(POINTER(t))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Pyramid:
    def __init__(self, ctx: "Context", w: int, h: int, levels: int):
        self.ctx, self.w, self.h, self.levels = ctx, w, h, levels
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_pyramid_create(ctx.h_, c_int(w), c_int(h), c_int(levels), byref(self.h_)))

    def upload(self, img: np.ndarray):
        img = np.ascontiguousarray(img, np.uint8)
        assert img.shape == (self.h, self.w)
        self.ctx._chk(self.ctx.lib.sfmx_pyramid_upload(self.ctx.h_, self.h_, _p(img, c_uint8)))
        return self

    def set_device(self, dev_ptr: int):
        self.ctx._chk(self.ctx.lib.sfmx_pyramid_set_device(self.ctx.h_, self.h_, c_void_p(dev_ptr)))
        return self

    def level(self, l: int) -> np.ndarray:
        w, h = c_int(), c_int()
        self.ctx._chk(self.ctx.lib.sfmx_pyramid_level_size(self.h_, c_int(l), byref(w), byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        self.ctx._chk(self.ctx.lib.sfmx_pyramid_download_level(self.ctx.h_, self.h_, c_int(l), _p(out, c_uint8)))
        return out

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_pyramid_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Fusion:
    """sfmx_fusion: a TSDF volume of dims = (nx, ny, nz) grid points at origin + (i, j, k) * voxel, plus its pending views."""

    def __init__(self, ctx: "Context", origin, voxel, dims, **params):
        self.ctx = ctx
        self.params = fusion_params(origin, voxel, dims, **params)
        self.dims = tuple(int(v) for v in dims)
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_fusion_create(ctx.h_, byref(self.params), byref(self.h_)))

    def add_view(self, cam: dict, disp16, shape=None):
        """disp16: int16 [h][w] numpy array, or an int (device pointer) with shape=(h, w)"""
        if isinstance(disp16, int):
            h, w = shape
            ptr, on_dev = c_void_p(disp16), 1
        else:
            disp16 = np.ascontiguousarray(disp16, np.int16)
            h, w = disp16.shape
            ptr, on_dev = disp16.ctypes.data_as(c_void_p), 0
        v = fusion_view(cam, w, h)
        self.ctx._chk(self.ctx.lib.sfmx_fusion_add_view(self.ctx.h_, self.h_, byref(v), ptr, c_int(on_dev)))

    def add_stereo_view(self, cam: dict, st: Stereo):
        """the last disparity map st computed, copied on the device"""
        v = fusion_view(cam, st.w, st.h)
        self.ctx._chk(self.ctx.lib.sfmx_fusion_add_stereo_view(self.ctx.h_, self.h_, byref(v), st.h_))

    def add_consist_view(self, cs: "Consist", i: int):
        """view i of cs with its filtered map (the last cs.filter()), copied on the device"""
        self.ctx._chk(self.ctx.lib.sfmx_fusion_add_consist_view(self.ctx.h_, self.h_, cs.h_, c_int(i)))

    def integrate(self):
        self.ctx._chk(self.ctx.lib.sfmx_fusion_integrate(self.ctx.h_, self.h_))

    def reset(self):
        self.ctx._chk(self.ctx.lib.sfmx_fusion_reset(self.ctx.h_, self.h_))

    def read(self):
        """(sum float64, count int32), both [nz][ny][nx]; integrates the pending views first"""
        nx, ny, nz = self.dims
        s, c = np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_fusion_read(self.ctx.h_, self.h_, _p(s, c_double), _p(c, c_int32)))
        return s, c

    def counts(self):
        """(n_verts, n_faces) of the surface, without the arrays"""
        nv, nf = c_int(0), c_int(0)
        self.ctx._chk(self.ctx.lib.sfmx_fusion_extract(self.ctx.h_, self.h_, None, c_int(0), None, c_int(0), byref(nv), byref(nf)))
        return nv.value, nf.value

    def extract_into(self, verts_cap: int, faces_cap: int):
        """the raw call with caller-chosen caps: (status, verts, faces, n_verts, n_faces); arrays sized by the caps"""
        verts, faces = np.zeros((max(verts_cap, 1), 3)), np.zeros((max(faces_cap, 1), 3), np.int32)
        nv, nf = c_int(0), c_int(0)
        rc = self.ctx.lib.sfmx_fusion_extract(self.ctx.h_, self.h_, _p(verts, c_double), c_int(verts_cap), _p(faces, c_int32),
                                              c_int(faces_cap), byref(nv), byref(nf))
        return rc, verts, faces, nv.value, nf.value

    def extract(self):
        """(verts float64 [n][3], faces int32 [m][3]); integrates the pending views first"""
        nv, nf = self.counts()
        rc, verts, faces, nv, nf = self.extract_into(nv, nf)
        self.ctx._chk(rc)
        return verts[:nv].copy(), faces[:nf].copy()

    def extract_normals(self):
        """extract() plus normals float64 [n][3]; the vertices and normals stay on the device for Shade.shade_fusion"""
        nv, nf = self.counts()
        verts, faces, normals = np.zeros((max(nv, 1), 3)), np.zeros((max(nf, 1), 3), np.int32), np.zeros((max(nv, 1), 3))
        n1, n2 = c_int(0), c_int(0)
        self.ctx._chk(self.ctx.lib.sfmx_fusion_extract_normals(self.ctx.h_, self.h_, _p(verts, c_double), c_int(nv), _p(faces, c_int32),
                                                               c_int(nf), _p(normals, c_double), byref(n1), byref(n2)))
        return verts[:n1.value].copy(), faces[:n2.value].copy(), normals[:n1.value].copy()

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_fusion_last_us(self.h_))

    def normals_us(self) -> float:
        return float(self.ctx.lib.sfmx_fusion_normals_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_fusion_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Shade:
    """sfmx_shade: retained views (camera, disp16 map, left rectified image) on the device, and vertex shading from them."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_shade_create(ctx.h_, byref(self.h_)))

    def add_view(self, cam: dict, disp16, image, shape=None):
        """disp16 int16 [h][w] and image u8 [h][w]: numpy arrays, or ints (device pointers) with shape=(h, w)"""
        if isinstance(disp16, int) != isinstance(image, int):
            raise TypeError("disp16 and image: both host arrays or both device pointers")
        if isinstance(disp16, int):
            h, w = shape
            pd, pi, on_dev = c_void_p(disp16), c_void_p(image), 1
        else:
            disp16 = np.ascontiguousarray(disp16, np.int16)
            image = np.ascontiguousarray(image, np.uint8)
            h, w = disp16.shape
            assert image.shape == (h, w)
            pd, pi, on_dev = disp16.ctypes.data_as(c_void_p), image.ctypes.data_as(c_void_p), 0
        v = fusion_view(cam, w, h)
        self.ctx._chk(self.ctx.lib.sfmx_shade_add_view(self.ctx.h_, self.h_, byref(v), pd, pi, c_int(on_dev)))

    def add_stereo_view(self, cam: dict, st: "Stereo"):
        """the last disparity map and left rectified image st computed, copied on the device"""
        v = fusion_view(cam, st.w, st.h)
        self.ctx._chk(self.ctx.lib.sfmx_shade_add_stereo_view(self.ctx.h_, self.h_, byref(v), st.h_))

    def view_count(self) -> int:
        return int(self.ctx.lib.sfmx_shade_view_count(self.h_))

    def reset(self):
        self.ctx._chk(self.ctx.lib.sfmx_shade_reset(self.ctx.h_, self.h_))

    def shade(self, verts, normals, depth_tol, n=None, **params):
        """(grey u8 [n], views int32 [n]).  verts / normals: float64 [n][3] arrays (normals may be None with cull=0), or ints
        (device pointers) with n given."""
        p = shade_params(depth_tol, **params)
        on_dev = isinstance(verts, int)
        if on_dev:
            pv, pn = c_void_p(verts), (c_void_p(normals) if normals is not None else None)
        else:
            verts = _f64(verts).reshape(-1, 3)
            n = len(verts)
            normals = None if normals is None else _f64(normals).reshape(-1, 3)
            assert normals is None or len(normals) == n
            pv, pn = verts.ctypes.data_as(c_void_p), (normals.ctypes.data_as(c_void_p) if normals is not None else None)
        grey, views = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_shade_vertices(self.ctx.h_, self.h_, pv, pn, c_int(n), c_int(1 if on_dev else 0), byref(p),
                                                       _p(grey, c_uint8), _p(views, c_int32)))
        return grey[:n].copy(), views[:n].copy()

    def shade_fusion(self, fu: Fusion, n: int, depth_tol, **params):
        """the n vertices fu.extract_normals() left on the device: (grey u8 [n], views int32 [n])"""
        p = shade_params(depth_tol, **params)
        grey, views = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_shade_fusion(self.ctx.h_, self.h_, fu.h_, byref(p), _p(grey, c_uint8), _p(views, c_int32)))
        return grey[:n].copy(), views[:n].copy()

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_shade_last_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_shade_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Carve:
    """sfmx_carve: retained views (camera, signed squared distance map of the silhouette) on the device, their visual hull on a
    volume, and carving a Fusion with it."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.shapes = []
        self.dims = None
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_carve_create(ctx.h_, byref(self.h_)))

    def add_view(self, cam: dict, image, shape=None, threshold=1, cap=16):
        """image: u8 [h][w] numpy array (a picture or a mask), or an int (device pointer) with shape=(h, w); cam needs no B"""
        if isinstance(image, int):
            h, w = shape
            ptr, on_dev = c_void_p(image), 1
        else:
            image = np.ascontiguousarray(image, np.uint8)
            h, w = image.shape
            ptr, on_dev = image.ctypes.data_as(c_void_p), 0
        v = fusion_view({**cam, "B": cam.get("B", 0.0)}, w, h)
        self.ctx._chk(self.ctx.lib.sfmx_carve_add_view(self.ctx.h_, self.h_, byref(v), ptr, c_int(on_dev), c_int(int(threshold)),
                                                       c_int(int(cap))))
        self.shapes.append((int(h), int(w)))

    def add_stereo_view(self, cam: dict, st: "Stereo", threshold=1, cap=16):
        """the left rectified image st computed last, from where it lies on the device"""
        v = fusion_view({**cam, "B": cam.get("B", 0.0)}, st.w, st.h)
        self.ctx._chk(self.ctx.lib.sfmx_carve_add_stereo_view(self.ctx.h_, self.h_, byref(v), st.h_, c_int(int(threshold)), c_int(int(cap))))
        self.shapes.append((int(st.h), int(st.w)))

    def view_count(self) -> int:
        return int(self.ctx.lib.sfmx_carve_view_count(self.h_))

    def inside_pixels(self) -> list:
        """per view, the pixels of the inside class"""
        n = self.view_count()
        out = np.zeros(max(n, 1), np.int32)
        if self.ctx.lib.sfmx_carve_inside_pixels(self.h_, _p(out, c_int32)) != SFMX_OK:
            raise SfmxError(SFMX_ERR_INVALID, "sfmx_carve_inside_pixels")
        return [int(v) for v in out[:n]]

    def reset(self):
        self.ctx._chk(self.ctx.lib.sfmx_carve_reset(self.ctx.h_, self.h_))
        self.shapes = []
        self.dims = None

    def read_view(self, i: int) -> np.ndarray:
        """sd2 int16 [h][w] of view i"""
        h, w = self.shapes[i] if 0 <= i < len(self.shapes) else (1, 1)
        sd2 = np.zeros((h, w), np.int16)
        self.ctx._chk(self.ctx.lib.sfmx_carve_read_view(self.ctx.h_, self.h_, c_int(i), sd2.ctypes.data_as(c_void_p)))
        return sd2

    def set_batch(self, k: int):
        """views per launch of the hull kernel (0 = automatic); changes the speed only"""
        if self.ctx.lib.sfmx_carve_set_batch(self.h_, c_int(int(k))) != SFMX_OK:
            raise SfmxError(SFMX_ERR_INVALID, "carve batch outside 0 .. 4096")

    def run(self, origin, voxel, dims, **params):
        """the hull of every view on the volume; params: CARVE_DEFAULTS keys"""
        p = carve_params(**params)
        vol = CarveVolume()
        vol.origin[:] = [float(v) for v in origin]
        vol.voxel = float(voxel)
        vol.nx, vol.ny, vol.nz = (int(v) for v in dims)
        self.dims = None
        self.ctx._chk(self.ctx.lib.sfmx_carve_run(self.ctx.h_, self.h_, byref(vol), byref(p)))
        self.dims = (vol.nx, vol.ny, vol.nz)

    def read(self):
        """(hull float64, views int32), both [nz][ny][nx], of the last run"""
        nx, ny, nz = self.dims if self.dims else (1, 1, 1)
        hull, views = np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_carve_read(self.ctx.h_, self.h_, _p(hull, c_double), _p(views, c_int32)))
        return hull, views

    def apply(self, fu: "Fusion", **params) -> dict:
        """carve fu's volume with the last run; params: CARVE_DEFAULTS keys (margin and mode are read).  dict of CARVE_COUNTS"""
        p = carve_params(**params)
        counts = np.zeros(3, np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_carve_apply(self.ctx.h_, self.h_, fu.h_, byref(p), _p(counts, c_int32)))
        return dict(zip(CARVE_COUNTS, (int(c) for c in counts)))

    def count(self, **params) -> dict:
        """dict of CARVE_COUNTS of the last run from the hull alone (margin is read; changed is 0): apply()'s first two counters"""
        p = carve_params(**params)
        counts = np.zeros(3, np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_carve_count(self.ctx.h_, self.h_, byref(p), _p(counts, c_int32)))
        return dict(zip(CARVE_COUNTS, (int(c) for c in counts)))

    def store(self, fu: "Fusion"):
        """write the last run into fu: the extraction and every stage behind it then work on the hull"""
        self.ctx._chk(self.ctx.lib.sfmx_carve_store(self.ctx.h_, self.h_, fu.h_))

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_carve_last_us(self.h_))

    def last_edt_us(self) -> float:
        return float(self.ctx.lib.sfmx_carve_last_edt_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_carve_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Consist:
    """sfmx_consist: retained views (camera, disp16 map) on the device, and their multi-view consistency filter."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.shapes = []
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_consist_create(ctx.h_, byref(self.h_)))

    def add_view(self, cam: dict, disp16, shape=None):
        """disp16: int16 [h][w] numpy array, or an int (device pointer) with shape=(h, w)"""
        if isinstance(disp16, int):
            h, w = shape
            ptr, on_dev = c_void_p(disp16), 1
        else:
            disp16 = np.ascontiguousarray(disp16, np.int16)
            h, w = disp16.shape
            ptr, on_dev = disp16.ctypes.data_as(c_void_p), 0
        v = fusion_view(cam, w, h)
        self.ctx._chk(self.ctx.lib.sfmx_consist_add_view(self.ctx.h_, self.h_, byref(v), ptr, c_int(on_dev)))
        self.shapes.append((int(h), int(w)))

    def add_stereo_view(self, cam: dict, st: "Stereo"):
        """the last disparity map st computed, copied on the device"""
        v = fusion_view(cam, st.w, st.h)
        self.ctx._chk(self.ctx.lib.sfmx_consist_add_stereo_view(self.ctx.h_, self.h_, byref(v), st.h_))
        self.shapes.append((int(st.h), int(st.w)))

    def view_count(self) -> int:
        return int(self.ctx.lib.sfmx_consist_view_count(self.h_))

    def reset(self):
        self.ctx._chk(self.ctx.lib.sfmx_consist_reset(self.ctx.h_, self.h_))
        self.shapes = []

    def filter(self, **params):
        """every view against every other, one launch; params: CONSIST_DEFAULTS keys"""
        p = consist_params(**params)
        self.ctx._chk(self.ctx.lib.sfmx_consist_filter(self.ctx.h_, self.h_, byref(p)))

    def read(self, i: int):
        """(disp16 int16 [h][w], support u8 [h][w]) of view i after the last filter()"""
        h, w = self.shapes[i] if 0 <= i < len(self.shapes) else (1, 1)
        d16, sup = np.zeros((h, w), np.int16), np.zeros((h, w), np.uint8)
        self.ctx._chk(self.ctx.lib.sfmx_consist_read(self.ctx.h_, self.h_, c_int(i), d16.ctypes.data_as(c_void_p), _p(sup, c_uint8)))
        return d16, sup

    def counts(self):
        """(valid int32 [n], kept int32 [n]) per view of the last filter()"""
        n = self.view_count()
        valid, kept = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_consist_counts(self.ctx.h_, self.h_, _p(valid, c_int32), _p(kept, c_int32)))
        return valid[:n].copy(), kept[:n].copy()

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_consist_last_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_consist_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Clean:
    """sfmx_clean: small connected components of a triangle mesh removed on the device; the work buffers are kept between calls."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_clean_create(ctx.h_, byref(self.h_)))

    @staticmethod
    def _counts(out):
        return dict(n_verts=out[0].value, n_faces=out[1].value, components=out[2].value, largest=out[3].value)

    def run(self, verts, faces, normals=None, n=None, m=None, **params):
        """verts / normals float64 [n][3] and faces int32 [m][3]: numpy arrays, or ints (device pointers) with n and m given;
        normals may be None.  params: CLEAN_DEFAULTS keys.  Returns dict(n_verts, n_faces, components, largest)."""
        p = clean_params(**params)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int) or (normals is not None and on_dev != isinstance(normals, int)):
            raise TypeError("verts, normals and faces: all host arrays or all device pointers")
        if on_dev:
            pv, pf, pn = c_void_p(verts), c_void_p(faces), (c_void_p(normals) if normals is not None else None)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            normals = None if normals is None else _f64(normals).reshape(-1, 3)
            assert normals is None or len(normals) == n
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
            pn = normals.ctypes.data_as(c_void_p) if normals is not None else None
        out = [c_int(0) for _ in range(4)]
        self.ctx._chk(self.ctx.lib.sfmx_clean_run(self.ctx.h_, self.h_, pv, pn, c_int(n), pf, c_int(m), c_int(1 if on_dev else 0),
                                                  byref(p), *[byref(o) for o in out]))
        return self._counts(out)

    def fusion(self, fu: "Fusion", **params):
        """the surface fu.extract() / fu.extract_normals() left on the device; returns run()'s dict"""
        p = clean_params(**params)
        out = [c_int(0) for _ in range(4)]
        self.ctx._chk(self.ctx.lib.sfmx_clean_fusion(self.ctx.h_, self.h_, fu.h_, byref(p), *[byref(o) for o in out]))
        return self._counts(out)

    def sizes(self):
        """(n, m, n', m') of the last successful run: input and cleaned vertices and faces; raises before one"""
        s = [c_int(0) for _ in range(4)]
        rc = self.ctx.lib.sfmx_clean_sizes(self.h_, *[byref(x) for x in s])
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_clean_sizes: no successful run")
        return tuple(x.value for x in s)

    def read(self, normals: bool = False):
        """the last run: dict(verts f64 [n'][3], faces i32 [m'][3], vert_src i32 [n'], face_src i32 [m'], label i32 [n],
        comp_faces i32 [n]), plus normals f64 [n'][3] when asked for (the run must have had them).  The arrays are sized by what
        the library says it will copy."""
        n, _, nv, nf = self.sizes()
        verts, nrm, faces = np.zeros((max(nv, 1), 3)), np.zeros((max(nv, 1), 3)), np.zeros((max(nf, 1), 3), np.int32)
        vsrc, fsrc = np.zeros(max(nv, 1), np.int32), np.zeros(max(nf, 1), np.int32)
        lab, vcf = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_clean_read(self.ctx.h_, self.h_, _p(verts, c_double), _p(nrm, c_double) if normals else None,
                                                   _p(faces, c_int32), _p(vsrc, c_int32), _p(fsrc, c_int32), _p(lab, c_int32),
                                                   _p(vcf, c_int32)))
        out = dict(verts=verts[:nv].copy(), faces=faces[:nf].copy(), vert_src=vsrc[:nv].copy(), face_src=fsrc[:nf].copy(),
                   label=lab[:n].copy(), comp_faces=vcf[:n].copy())
        if normals:
            out["normals"] = nrm[:nv].copy()
        return out

    def device_surface(self):
        """(n', device pointer of the cleaned vertices, of the cleaned normals or None); n' = -1 before a successful run"""
        v, nr = c_void_p(), c_void_p()
        n = int(self.ctx.lib.sfmx_clean_device_surface(self.h_, byref(v), byref(nr)))
        return n, v.value, nr.value

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_clean_last_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_clean_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Simplify:
    """sfmx_simplify: exact vertex clustering of a triangle mesh on a uniform grid; the work buffers are kept
    between calls."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_simplify_create(ctx.h_, byref(self.h_)))

    def run(self, verts, faces, normals=None, n=None, m=None, cell=0.0, **params):
        """verts / normals float64 [n][3] and faces int32 [m][3]: numpy arrays, or ints (device pointers) with n and m given;
        normals may be None.  cell is required; params: SIMPLIFY_DEFAULTS keys.  Returns counts()."""
        p = simplify_params(cell, **params)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int) or (normals is not None and on_dev != isinstance(normals, int)):
            raise TypeError("verts, normals and faces: all host arrays or all device pointers")
        if on_dev:
            pv, pf, pn = c_void_p(verts), c_void_p(faces), (c_void_p(normals) if normals is not None else None)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            normals = None if normals is None else _f64(normals).reshape(-1, 3)
            assert normals is None or len(normals) == n
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
            pn = normals.ctypes.data_as(c_void_p) if normals is not None else None
        self.ctx._chk(self.ctx.lib.sfmx_simplify_run(self.ctx.h_, self.h_, pv, pn, c_int(n), pf, c_int(m), c_int(1 if on_dev else 0),
                                                     byref(p), None, None))
        return self.counts()

    def fusion(self, fu: "Fusion", cell=0.0, **params):
        """the surface fu.extract() / fu.extract_normals() left on the device; returns counts()"""
        p = simplify_params(cell, **params)
        self.ctx._chk(self.ctx.lib.sfmx_simplify_fusion(self.ctx.h_, self.h_, fu.h_, byref(p), None, None))
        return self.counts()

    def clean(self, cl: "Clean", cell=0.0, **params):
        """the cleaned surface of cl's last run, on the device; returns counts()"""
        p = simplify_params(cell, **params)
        self.ctx._chk(self.ctx.lib.sfmx_simplify_clean(self.ctx.h_, self.h_, cl.h_, byref(p), None, None))
        return self.counts()

    def sizes(self):
        """(n, m, n', m') of the last successful run: input and output vertices and faces; raises before one"""
        s = [c_int(0) for _ in range(4)]
        rc = self.ctx.lib.sfmx_simplify_sizes(self.h_, *[byref(x) for x in s])
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_simplify_sizes: no successful run")
        return tuple(x.value for x in s)

    def counts(self) -> dict:
        """dict(clusters, degenerate, duplicates, n_verts, n_faces) of the last successful run; raises before one"""
        s = [c_int(0) for _ in range(5)]
        rc = self.ctx.lib.sfmx_simplify_counts(self.h_, *[byref(x) for x in s])
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_simplify_counts: no successful run")
        return dict(zip(("clusters", "degenerate", "duplicates", "n_verts", "n_faces"), (x.value for x in s)))

    def read(self, normals: bool = False):
        """the last run: dict(verts f64 [n'][3], faces i32 [m'][3], vert_dst i32 [n], face_src i32 [m'], members i32 [n']), plus
        normals f64 [n'][3] when asked for (the run must have had them).  The arrays are sized by what the library says it will
        copy."""
        n, _, nv, nf = self.sizes()
        verts, nrm, faces = np.zeros((max(nv, 1), 3)), np.zeros((max(nv, 1), 3)), np.zeros((max(nf, 1), 3), np.int32)
        vdst, fsrc, mem = np.zeros(max(n, 1), np.int32), np.zeros(max(nf, 1), np.int32), np.zeros(max(nv, 1), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_simplify_read(self.ctx.h_, self.h_, _p(verts, c_double), _p(nrm, c_double) if normals else None,
                                                      _p(faces, c_int32), _p(vdst, c_int32), _p(fsrc, c_int32), _p(mem, c_int32)))
        out = dict(verts=verts[:nv].copy(), faces=faces[:nf].copy(), vert_dst=vdst[:n].copy(), face_src=fsrc[:nf].copy(),
                   members=mem[:nv].copy())
        if normals:
            out["normals"] = nrm[:nv].copy()
        return out

    def device_surface(self):
        """(n', device pointer of the output vertices, of the output normals or None); n' = -1 before a successful run"""
        v, nr = c_void_p(), c_void_p()
        n = int(self.ctx.lib.sfmx_simplify_device_surface(self.h_, byref(v), byref(nr)))
        return n, v.value, nr.value

    def device_mesh(self):
        """(n', device pointer of the output vertices, of the output faces, m'); n' = -1 before a successful run"""
        v, f, m = c_void_p(), c_void_p(), c_int(0)
        n = int(self.ctx.lib.sfmx_simplify_device_mesh(self.h_, byref(v), byref(f), byref(m)))
        return n, v.value, f.value, int(m.value)

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_simplify_last_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_simplify_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Smooth:
    """sfmx_smooth: exact Taubin lambda|mu smoothing of a triangle mesh; the work buffers are kept between calls."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_smooth_create(ctx.h_, byref(self.h_)))

    def run(self, verts, faces, n=None, m=None, unit=0.0, **params):
        """verts float64 [n][3] and faces int32 [m][3]: numpy arrays, or ints (device pointers) with n and m given.  unit is
        required; params: SMOOTH_DEFAULTS keys.  Returns counts()."""
        p = smooth_params(unit, **params)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int):
            raise TypeError("verts and faces: both host arrays or both device pointers")
        if on_dev:
            pv, pf = c_void_p(verts), c_void_p(faces)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
        self.ctx._chk(self.ctx.lib.sfmx_smooth_run(self.ctx.h_, self.h_, pv, c_int(n), pf, c_int(m), c_int(1 if on_dev else 0), byref(p)))
        return self.counts()

    def fusion(self, fu: "Fusion", unit=0.0, **params):
        """the surface fu.extract() / fu.extract_normals() left on the device; returns counts()"""
        p = smooth_params(unit, **params)
        self.ctx._chk(self.ctx.lib.sfmx_smooth_fusion(self.ctx.h_, self.h_, fu.h_, byref(p)))
        return self.counts()

    def clean(self, cl: "Clean", unit=0.0, **params):
        """the cleaned surface of cl's last run, on the device; returns counts()"""
        p = smooth_params(unit, **params)
        self.ctx._chk(self.ctx.lib.sfmx_smooth_clean(self.ctx.h_, self.h_, cl.h_, byref(p)))
        return self.counts()

    def sizes(self):
        """(n, m) of the last successful run; raises before one"""
        s = [c_int(0) for _ in range(2)]
        rc = self.ctx.lib.sfmx_smooth_sizes(self.h_, *[byref(x) for x in s])
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_smooth_sizes: no successful run")
        return tuple(x.value for x in s)

    def counts(self) -> dict:
        """dict(edges, boundary_edges, irregular_edges, pinned, isolated) of the last successful run; raises before one"""
        s = [c_int(0) for _ in range(5)]
        rc = self.ctx.lib.sfmx_smooth_counts(self.h_, *[byref(x) for x in s])
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_smooth_counts: no successful run")
        return dict(zip(SMOOTH_COUNTS, (x.value for x in s)))

    def read(self):
        """the last run: dict(verts f64 [n][3], flags u8 [n]: bit 0 pinned, bit 1 isolated), sized by what the library says it
        will copy"""
        n, _ = self.sizes()
        verts, flags = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), np.uint8)
        self.ctx._chk(self.ctx.lib.sfmx_smooth_read(self.ctx.h_, self.h_, _p(verts, c_double), _p(flags, ctypes.c_uint8)))
        return dict(verts=verts[:n].copy(), flags=flags[:n].copy())

    def device_mesh(self):
        """(n, device pointer of the smoothed vertices, of the input's faces, m); n = -1 before a successful run"""
        v, f, m = c_void_p(), c_void_p(), c_int(0)
        n = int(self.ctx.lib.sfmx_smooth_device_mesh(self.h_, byref(v), byref(f), byref(m)))
        return n, v.value, f.value, int(m.value)

    def device_surface(self):
        """(n, device pointer of the smoothed vertices, of the source's normals or None); n = -1 before a successful run"""
        v, nr = c_void_p(), c_void_p()
        n = int(self.ctx.lib.sfmx_smooth_device_surface(self.h_, byref(v), byref(nr)))
        return n, v.value, nr.value

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_smooth_last_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_smooth_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass



class Fill:
    """sfmx_fill: exact filling of a triangle mesh's small holes by centroid fans; the work buffers are kept between
    calls."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_fill_create(ctx.h_, byref(self.h_)))

    def run(self, verts, faces, normals=None, n=None, m=None, unit=0.0, **params):
        """verts / normals float64 [n][3] and faces int32 [m][3]: numpy arrays, or ints (device pointers, not this object's own
        result) with n and m given; normals may be None.  unit is required; params: FILL_DEFAULTS keys.  Returns counts()."""
        p = fill_params(unit, **params)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int) or (normals is not None and on_dev != isinstance(normals, int)):
            raise TypeError("verts, normals and faces: all host arrays or all device pointers")
        if on_dev:
            pv, pf, pn = c_void_p(verts), c_void_p(faces), (c_void_p(normals) if normals is not None else None)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            normals = None if normals is None else _f64(normals).reshape(-1, 3)
            assert normals is None or len(normals) == n
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
            pn = normals.ctypes.data_as(c_void_p) if normals is not None else None
        self.ctx._chk(self.ctx.lib.sfmx_fill_run(self.ctx.h_, self.h_, pv, pn, c_int(n), pf, c_int(m), c_int(1 if on_dev else 0), byref(p)))
        return self.counts()

    def fusion(self, fu: "Fusion", unit=0.0, **params):
        """the surface fu.extract() / fu.extract_normals() left on the device; returns counts()"""
        p = fill_params(unit, **params)
        self.ctx._chk(self.ctx.lib.sfmx_fill_fusion(self.ctx.h_, self.h_, fu.h_, byref(p)))
        return self.counts()

    def clean(self, cl: "Clean", unit=0.0, **params):
        """the cleaned surface of cl's last run, on the device; returns counts()"""
        p = fill_params(unit, **params)
        self.ctx._chk(self.ctx.lib.sfmx_fill_clean(self.ctx.h_, self.h_, cl.h_, byref(p)))
        return self.counts()

    def sizes(self):
        """(n, m, n + K, m + F) of the last successful run; raises before one"""
        s = [c_int(0) for _ in range(4)]
        rc = self.ctx.lib.sfmx_fill_sizes(self.h_, *[byref(x) for x in s])
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_fill_sizes: no successful run")
        return tuple(x.value for x in s)

    def counts(self) -> dict:
        """dict of FILL_COUNTS of the last successful run; raises before one"""
        s = [c_int(0) for _ in range(8)]
        rc = self.ctx.lib.sfmx_fill_counts(self.h_, *[byref(x) for x in s])
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_fill_counts: no successful run")
        return dict(zip(FILL_COUNTS, (x.value for x in s)))

    def read(self, normals: bool = False):
        """the last run: dict(verts f64 [n + K][3], faces i32 [m + F][3]), plus normals f64 [n + K][3] when asked for (the run
        must have had them), sized by what the library says it will copy"""
        _, _, nv, nf = self.sizes()
        verts, nrm, faces = np.zeros((max(nv, 1), 3)), np.zeros((max(nv, 1), 3)), np.zeros((max(nf, 1), 3), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_fill_read(self.ctx.h_, self.h_, _p(verts, c_double), _p(nrm, c_double) if normals else None,
                                                  _p(faces, c_int32)))
        out = dict(verts=verts[:nv].copy(), faces=faces[:nf].copy())
        if normals:
            out["normals"] = nrm[:nv].copy()
        return out

    def device_mesh(self):
        """(n + K, device pointer of the filled vertices, of the filled faces, m + F); n + K = -1 before a successful run"""
        v, f, nv, m = c_void_p(), c_void_p(), c_int(0), c_int(0)
        n = int(self.ctx.lib.sfmx_fill_device_mesh(self.h_, byref(v), byref(f), byref(nv), byref(m)))
        return n, v.value, f.value, int(m.value)

    def device_surface(self):
        """(n + K, device pointer of the filled vertices, of their normals or None); n + K = -1 before a successful run"""
        v, nr = c_void_p(), c_void_p()
        n = int(self.ctx.lib.sfmx_fill_device_surface(self.h_, byref(v), byref(nr)))
        return n, v.value, nr.value

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_fill_last_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_fill_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

class Sdist:
    """sfmx_sdist: squared distance from points to the nearest point of a target triangle mesh.  One target
    serves many query sets; the target's grid and the work buffers are kept between calls."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_sdist_create(ctx.h_, byref(self.h_)))

    def set_target(self, verts, faces, d_max, cell=0.0, nv=None, m=None):
        """verts float64 [nv][3] and faces int32 [m][3]: numpy arrays, or ints (device pointers) with nv and m given"""
        p = sdist_params(d_max, cell)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int):
            raise TypeError("verts and faces: both host arrays or both device pointers")
        if on_dev:
            pv, pf = c_void_p(verts), c_void_p(faces)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            nv, m = len(verts), len(faces)
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
        self.ctx._chk(self.ctx.lib.sfmx_sdist_set_target(self.ctx.h_, self.h_, pv, c_int(nv), pf, c_int(m), c_int(1 if on_dev else 0),
                                                         byref(p)))

    def set_target_fusion(self, fu: "Fusion", d_max, cell=0.0):
        """the surface fu.extract() / fu.extract_normals() left on the device"""
        p = sdist_params(d_max, cell)
        self.ctx._chk(self.ctx.lib.sfmx_sdist_set_target_fusion(self.ctx.h_, self.h_, fu.h_, byref(p)))

    def set_target_clean(self, cl: "Clean", d_max, cell=0.0):
        """the cleaned surface of cl's last run, on the device"""
        p = sdist_params(d_max, cell)
        self.ctx._chk(self.ctx.lib.sfmx_sdist_set_target_clean(self.ctx.h_, self.h_, cl.h_, byref(p)))

    def query(self, points, n=None):
        """points float64 [n][3]: a numpy array, or an int (device pointer) with n given.  Returns (d2 f64 [n], face i32 [n]):
        the squared distance clipped at d_max^2 and the nearest face (-1 where clipped)."""
        on_dev = isinstance(points, int)
        if on_dev:
            pp = c_void_p(points)
        else:
            points = _f64(points).reshape(-1, 3)
            n = len(points)
            pp = points.ctypes.data_as(c_void_p)
        d2, face = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_sdist_query(self.ctx.h_, self.h_, pp, c_int(n), c_int(1 if on_dev else 0), _p(d2, c_double),
                                                    _p(face, c_int32)))
        return d2[:n].copy(), face[:n].copy()

    def _query_surface(self, fn, obj, cap):
        """the library says how many vertices the device surface has; a surface larger than cap is refused, not written"""
        d2, face, n = np.zeros(max(cap, 1)), np.zeros(max(cap, 1), np.int32), c_int(0)
        self.ctx._chk(fn(self.ctx.h_, self.h_, obj.h_, c_int(cap), _p(d2, c_double), _p(face, c_int32), byref(n)))
        return d2[:n.value].copy(), face[:n.value].copy()

    def query_fusion(self, fu: "Fusion", n=None):
        """the vertices fu.extract() / fu.extract_normals() left on the device as queries; n (optional): the count the caller
        expects, at most that many are accepted (default: fu.counts())"""
        return self._query_surface(self.ctx.lib.sfmx_sdist_query_fusion, fu, fu.counts()[0] if n is None else int(n))

    def query_clean(self, cl: "Clean"):
        """the cleaned vertices of cl's last run, on the device, as queries"""
        return self._query_surface(self.ctx.lib.sfmx_sdist_query_clean, cl, cl.sizes()[2])

    def stats(self) -> dict:
        """dict(dims (cells per axis), cells, entries (triangle-cell pairs), cell (the size used), tests (point-triangle pairs
        the last query visited), kernel_us (the query kernel alone inside the last query, when timing is on), chunk (triangles
        staged through LDS at a time)); raises without a target"""
        dims, ent, cell, tests, kus = (c_int * 3)(), c_int(0), c_double(0.0), c_uint64(0), c_double(0.0)
        rc = self.ctx.lib.sfmx_sdist_stats(self.h_, dims, byref(ent), byref(cell), byref(tests), byref(kus))
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_sdist_stats: no target")
        d = tuple(int(v) for v in dims)
        return dict(dims=d, cells=d[0] * d[1] * d[2], entries=int(ent.value), cell=float(cell.value), tests=int(tests.value),
                    kernel_us=float(kus.value), chunk=SDIST_CHUNK)

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_sdist_last_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_sdist_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Raycast:
    """sfmx_raycast: depth, point, normal and head-light shade per pixel of a pinhole camera, ray cast from a TSDF volume
    (DESIGN.md 18).  The device outputs grow on demand and are kept between renders."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.shape = None  # (h, w) of the last render
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_raycast_create(ctx.h_, byref(self.h_)))

    def render(self, vol, cam: dict, z_min, z_max, step=0.0, min_weight=0, background=0, w=None, h=None, read=True):
        """vol: a Fusion (its pending views are integrated first), or (sum, count, origin, voxel) with sum float64 / count int32
        [nz][ny][nx] numpy arrays, or ints (device pointers) followed by dims: (sum, count, origin, voxel, (nx, ny, nz)).
        cam: dict(R_rw, c_left, f, cx, cy, w, h) (B is not used; w= / h= override the dict's image size).  Returns dict(depth f64 [h][w], normals / points
        f64 [h][w][3], shaded u8 [h][w], hits), or None with read=False (the result stays on the device for read() / shade())."""
        self.shape = None
        p = raycast_params(z_min, z_max, step, min_weight, background)
        w, h = int(cam["w"] if w is None else w), int(cam["h"] if h is None else h)
        v = fusion_view({**cam, "B": cam.get("B", 0.0)}, w, h)
        if isinstance(vol, Fusion):
            self.ctx._chk(self.ctx.lib.sfmx_raycast_render(self.ctx.h_, self.h_, vol.h_, byref(v), byref(p)))
        else:
            sum_, count, origin, voxel = vol[:4]
            on_dev = isinstance(sum_, int)
            if on_dev != isinstance(count, int):
                raise TypeError("sum and count: both host arrays or both device pointers")
            if on_dev:
                dims = vol[4]
                ps, pc = c_void_p(sum_), c_void_p(count)
            else:
                sum_ = _f64(sum_)
                count = np.ascontiguousarray(count, np.int32)
                assert sum_.ndim == 3 and count.shape == sum_.shape
                dims = sum_.shape[::-1]
                ps, pc = sum_.ctypes.data_as(c_void_p), count.ctypes.data_as(c_void_p)
            fp = fusion_params(origin, voxel, dims)
            self.ctx._chk(self.ctx.lib.sfmx_raycast_render_arrays(self.ctx.h_, self.h_, byref(fp), ps, pc, c_int(1 if on_dev else 0),
                                                                  byref(v), byref(p)))
        self.shape = (int(h), int(w))
        return self.read() if read else None

    def read(self) -> dict:
        """the last render: dict(depth, normals, points, shaded, hits)"""
        h, w = self.shape or (1, 1)
        depth, normals, points = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
        shaded, hits = np.zeros((h, w), np.uint8), c_int32(0)
        self.ctx._chk(self.ctx.lib.sfmx_raycast_read(self.ctx.h_, self.h_, _p(depth, c_double), _p(normals, c_double), _p(points, c_double),
                                                     _p(shaded, c_uint8), byref(hits)))
        return dict(depth=depth, normals=normals, points=points, shaded=shaded, hits=int(hits.value))

    def device_surface(self):
        """(n = w * h, device pointer of the points, of the normals) of the last render; raises before one"""
        pts, nrm, n = c_void_p(), c_void_p(), c_int(0)
        rc = self.ctx.lib.sfmx_raycast_device_surface(self.h_, byref(pts), byref(nrm), byref(n))
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_raycast_device_surface: no render")
        return n.value, pts.value, nrm.value

    def shade(self, sh: "Shade", depth_tol, **params):
        """a novel-view grey image of the last render from sh's retained views: (grey u8 [h][w], views int32 [h][w]); pixels
        without a hit get the render's background and 0 views.  params: SHADE_DEFAULTS keys."""
        p = shade_params(depth_tol, **params)
        h, w = self.shape or (1, 1)
        grey, views = np.zeros((h, w), np.uint8), np.zeros((h, w), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_raycast_shade(self.ctx.h_, self.h_, sh.h_, byref(p), _p(grey, c_uint8), _p(views, c_int32)))
        return grey, views

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_raycast_last_us(self.h_))

    def last_samples(self) -> int:
        """samples the last render evaluated (inside the grid, up to each ray's hit)"""
        return int(self.ctx.lib.sfmx_raycast_last_samples(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_raycast_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Raster:
    """sfmx_raster: the visible face, depth, point, normal, head-light shade and interpolated grey per pixel of a pinhole camera,
    from an exact z-buffer over a triangle mesh.  The device buffers grow on demand and are kept between runs."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.shape = None  # (h, w) of the last render
        self.has_grey = False
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_raster_create(ctx.h_, byref(self.h_)))

    def render(self, verts, faces, cam: dict, z_min, normals=None, grey=None, n=None, m=None, w=None, h=None, read=True, **params):
        """verts float64 [n][3], faces int32 [m][3], normals float64 [n][3] or None, grey uint8 [n] or None: numpy arrays, or ints
        (device pointers, read in place) with n= and m= given.  cam: dict(R_rw, c_left, f, cx, cy, w, h) (B is not used; w= / h=
        override the dict's image size).  params: RASTER_DEFAULTS keys.  Returns read()'s dict, or None with read=False."""
        p = raster_params(z_min, **params)
        w, h = int(cam["w"] if w is None else w), int(cam["h"] if h is None else h)
        v = fusion_view({**cam, "B": cam.get("B", 0.0)}, w, h)
        on_dev = isinstance(verts, int)
        if on_dev:
            if not isinstance(faces, int) or any(a is not None and not isinstance(a, int) for a in (normals, grey)):
                raise TypeError("verts, faces, normals and grey: all host arrays or all device pointers")
            pv, pf = c_void_p(verts), c_void_p(faces)
            pn, pg = c_void_p(normals), c_void_p(grey)
            n, m = int(n), int(m)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
            pn = pg = None
            if normals is not None:
                normals = _f64(normals).reshape(-1, 3)
                assert len(normals) == n
                pn = normals.ctypes.data_as(c_void_p)
            if grey is not None:
                grey = np.ascontiguousarray(grey, np.uint8).reshape(-1)
                assert len(grey) == n
                pg = grey.ctypes.data_as(c_void_p)
        self.shape = None  # only now: a call refused above, in Python, leaves the library's result and its shape alone
        self.ctx._chk(self.ctx.lib.sfmx_raster_run(self.ctx.h_, self.h_, pv, pn, pg, c_int(n), pf, c_int(m), c_int(1 if on_dev else 0),
                                                   byref(v), byref(p)))
        self.shape, self.has_grey = (h, w), grey is not None
        return self.read() if read else None

    def read(self) -> dict:
        """the last render: dict(depth f64 [h][w], face int32 [h][w], points / normals f64 [h][w][3], shaded u8 [h][w], grey u8
        [h][w] when the run had grey, the RASTER_COUNTS and fragments)"""
        if self.shape is None:  # no render: the library says so, and copies nothing
            self.ctx._chk(self.ctx.lib.sfmx_raster_read(self.ctx.h_, self.h_, None, None, None, None, None, None))
            raise SfmxError(SFMX_ERR_INVALID, "sfmx_raster_read: no render made through this object")
        h, w = self.shape
        depth, face = np.zeros((h, w)), np.zeros((h, w), np.int32)
        points, normals = np.zeros((h, w, 3)), np.zeros((h, w, 3))
        shaded = np.zeros((h, w), np.uint8)
        grey = np.zeros((h, w), np.uint8) if self.has_grey else None
        self.ctx._chk(self.ctx.lib.sfmx_raster_read(self.ctx.h_, self.h_, _p(depth, c_double), _p(face, c_int32), _p(points, c_double),
                                                    _p(normals, c_double), _p(shaded, c_uint8), _p(grey, c_uint8) if self.has_grey else None))
        out = dict(depth=depth, face=face, points=points, normals=normals, shaded=shaded, **self.counts())
        if self.has_grey:
            out["grey"] = grey
        return out

    def counts(self) -> dict:
        """the RASTER_COUNTS and fragments of the last render; raises before one"""
        c, fr = (c_int32 * 8)(), c_uint64(0)
        rc = self.ctx.lib.sfmx_raster_counts(self.h_, c, byref(fr))
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_raster_counts: no render")
        return dict(zip(RASTER_COUNTS, (int(x) for x in c)), fragments=int(fr.value))

    def device_surface(self):
        """(n = w * h, device pointer of the points, of the normals) of the last render; raises before one"""
        pts, nrm, n = c_void_p(), c_void_p(), c_int(0)
        rc = self.ctx.lib.sfmx_raster_device_surface(self.h_, byref(pts), byref(nrm), byref(n))
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_raster_device_surface: no render")
        return n.value, pts.value, nrm.value

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_raster_last_us(self.h_))

    def last_big_faces(self) -> int:
        """faces of the last render that went to the tiled path"""
        return int(self.ctx.lib.sfmx_raster_last_big_faces(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_raster_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Visib:
    """sfmx_visib: which faces and vertices of a mesh a list of cameras really sees, from the exact z-buffer of every camera
    (DESIGN.md 24): per-face and per-vertex view counts, the mesh without the faces too few cameras see from the front, and a
    grey value per vertex from the cameras that see it.  The views, their images and the work buffers are kept between runs."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_visib_create(ctx.h_, byref(self.h_)))
        self.images = 0  # views added with an image
        self.has_normals = self.has_grey = False  # of the last successful run

    def reset(self):
        self.ctx._chk(self.ctx.lib.sfmx_visib_reset(self.ctx.h_, self.h_))
        self.images = 0

    def add_view(self, cam: dict, image=None, w=None, h=None):
        """cam: dict(R_rw, c_left, f, cx, cy, w, h) (B is not used; w= / h= override the dict's image size).  image: uint8 [h][w]
        numpy array, an int (device pointer), or None."""
        w, h = int(cam["w"] if w is None else w), int(cam["h"] if h is None else h)
        v = fusion_view({**cam, "B": cam.get("B", 0.0)}, w, h)
        on_dev = isinstance(image, int)
        if image is None:
            pi = None
        elif on_dev:
            pi = c_void_p(image)
        else:
            image = np.ascontiguousarray(image, np.uint8)
            assert image.shape == (h, w), (image.shape, h, w)
            pi = image.ctypes.data_as(c_void_p)
        self.ctx._chk(self.ctx.lib.sfmx_visib_add_view(self.ctx.h_, self.h_, byref(v), pi, c_int(1 if on_dev else 0)))
        self.images += image is not None

    def view_count(self) -> int:
        return int(self.ctx.lib.sfmx_visib_view_count(self.h_))

    def set_batch(self, k: int):
        """k >= 1 forces k views per batch, 0 restores the automatic size; the result does not depend on it"""
        rc = self.ctx.lib.sfmx_visib_set_batch(self.h_, c_int(int(k)))
        if rc != SFMX_OK:
            raise SfmxError(rc, f"sfmx_visib_set_batch: {k} is not in 0 .. {VISIB_MAX_BATCH}")

    def run(self, verts, faces, z_min=0.0, depth_tol=-1.0, normals=None, n=None, m=None, read=True, **params):
        """verts / normals float64 [n][3] and faces int32 [m][3]: numpy arrays, or ints (device pointers, not this object's own
        result) with n and m given; normals may be None.  z_min and depth_tol are required; params: VISIB_DEFAULTS keys.  Returns
        read()'s dict, or counts() with read=False."""
        p = visib_params(z_min, depth_tol, **params)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int) or (normals is not None and on_dev != isinstance(normals, int)):
            raise TypeError("verts, normals and faces: all host arrays or all device pointers")
        if on_dev:
            pv, pf, pn = c_void_p(verts), c_void_p(faces), (c_void_p(normals) if normals is not None else None)
            n, m = int(n), int(m)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            normals = None if normals is None else _f64(normals).reshape(-1, 3)
            assert normals is None or len(normals) == n
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
            pn = normals.ctypes.data_as(c_void_p) if normals is not None else None
        self.ctx._chk(self.ctx.lib.sfmx_visib_run(self.ctx.h_, self.h_, pv, pn, c_int(n), pf, c_int(m), c_int(1 if on_dev else 0), byref(p)))
        self.has_normals, self.has_grey = normals is not None, self.images > 0
        return self.read() if read else self.counts()

    def sizes(self):
        """(n, m, n', m') of the last successful run; raises before one"""
        s = [c_int(0) for _ in range(4)]
        rc = self.ctx.lib.sfmx_visib_sizes(self.h_, *[byref(x) for x in s])
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_visib_sizes: no successful run")
        return tuple(x.value for x in s)

    def counts(self) -> dict:
        """dict of VISIB_COUNTS of the last successful run; raises before one"""
        c, pr = (c_int32 * 5)(), (c_uint64 * 3)()
        rc = self.ctx.lib.sfmx_visib_counts(self.h_, c, pr)
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_visib_counts: no successful run")
        return dict(zip(VISIB_COUNTS, [int(x) for x in c] + [int(x) for x in pr]))

    def read(self, normals=None, grey=None) -> dict:
        """the last run: dict(verts f64 [n'][3], faces i32 [m'][3], vert_src i32 [n'], face_src i32 [m'], face_views /
        face_back_views i32 [m], vert_views i32 [n], the VISIB_COUNTS), plus normals f64 [n'][3] and grey u8 [n] / grey_views i32
        [n].  normals / grey: True asks for them (the library refuses what the run did not have), None takes what there is."""
        n, m, nv, nf = self.sizes()
        lib = self.ctx.lib
        normals = self.has_normals if normals is None else normals
        grey = self.has_grey if grey is None else grey
        z = lambda k, *s, t=np.float64: np.zeros((max(k, 1),) + s, t)
        verts, nrm, faces = z(nv, 3), z(nv, 3), z(nf, 3, t=np.int32)
        vsrc, fsrc = z(nv, t=np.int32), z(nf, t=np.int32)
        fviews, fback, vviews = z(m, t=np.int32), z(m, t=np.int32), z(n, t=np.int32)
        g, gv = z(n, t=np.uint8), z(n, t=np.int32)
        self.ctx._chk(lib.sfmx_visib_read(self.ctx.h_, self.h_, _p(verts, c_double), _p(nrm, c_double) if normals else None,
                                          _p(faces, c_int32), _p(vsrc, c_int32), _p(fsrc, c_int32), _p(fviews, c_int32), _p(fback, c_int32),
                                          _p(vviews, c_int32), _p(g, c_uint8) if grey else None, _p(gv, c_int32) if grey else None))
        out = dict(verts=verts[:nv].copy(), faces=faces[:nf].copy(), vert_src=vsrc[:nv].copy(), face_src=fsrc[:nf].copy(),
                   face_views=fviews[:m].copy(), face_back_views=fback[:m].copy(), vert_views=vviews[:n].copy(), **self.counts())
        if normals:
            out["normals"] = nrm[:nv].copy()
        if grey:
            out["grey"], out["grey_views"] = g[:n].copy(), gv[:n].copy()
        return out

    def device_mesh(self):
        """(n', device pointer of the kept vertices, of the kept faces, m'); n' = -1 before a successful run"""
        v, f, nv, m = c_void_p(), c_void_p(), c_int(0), c_int(0)
        n = int(self.ctx.lib.sfmx_visib_device_mesh(self.h_, byref(v), byref(f), byref(nv), byref(m)))
        return n, v.value, f.value, int(m.value)

    def device_surface(self):
        """(n', device pointer of the kept vertices, of their normals or None); n' = -1 before a successful run"""
        v, nr = c_void_p(), c_void_p()
        n = int(self.ctx.lib.sfmx_visib_device_surface(self.h_, byref(v), byref(nr)))
        return n, v.value, nr.value

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_visib_last_us(self.h_))

    def last_batch(self) -> int:
        """the largest number of views the last run put into one batch"""
        return int(self.ctx.lib.sfmx_visib_last_batch(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_visib_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Texture:
    """sfmx_texture: a texture atlas for a mesh from the cameras that see it: per face the view that sees it from
    the front with the largest image area, two faces to a cell of (patch + 1) x patch texels, every texel sampled bilinearly
    from that view's image.  The views, their images and the work buffers are kept between runs."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_texture_create(ctx.h_, byref(self.h_)))
        self.shapes = []  # (h, w) of every view

    def reset(self):
        self.ctx._chk(self.ctx.lib.sfmx_texture_reset(self.ctx.h_, self.h_))
        self.shapes = []

    def add_view(self, cam: dict, image=None, w=None, h=None):
        """cam: dict(R_rw, c_left, f, cx, cy, w, h) (B is not used; w= / h= override the dict's image size).  image: uint8 [h][w]
        numpy array or an int (device pointer); None is accepted here and refused by run()."""
        w, h = int(cam["w"] if w is None else w), int(cam["h"] if h is None else h)
        v = fusion_view({**cam, "B": cam.get("B", 0.0)}, w, h)
        on_dev = isinstance(image, int)
        if image is None:
            pi = None
        elif on_dev:
            pi = c_void_p(image)
        else:
            image = np.ascontiguousarray(image, np.uint8)
            assert image.shape == (h, w), (image.shape, h, w)
            pi = image.ctypes.data_as(c_void_p)
        self.ctx._chk(self.ctx.lib.sfmx_texture_add_view(self.ctx.h_, self.h_, byref(v), pi, c_int(1 if on_dev else 0)))
        self.shapes.append((h, w))

    def add_stereo_view(self, cam: dict, stereo: "Stereo"):
        """the view with the left rectified image of stereo's last disparity call, from where it lies on the device"""
        v = fusion_view({**cam, "B": cam.get("B", 0.0)}, stereo.w, stereo.h)
        self.ctx._chk(self.ctx.lib.sfmx_texture_add_stereo_view(self.ctx.h_, self.h_, byref(v), stereo.h_))
        self.shapes.append((int(stereo.h), int(stereo.w)))

    def view_count(self) -> int:
        return int(self.ctx.lib.sfmx_texture_view_count(self.h_))

    def set_batch(self, k: int):
        """k >= 1 forces k views per batch, 0 restores the automatic size; the result does not depend on it"""
        rc = self.ctx.lib.sfmx_texture_set_batch(self.h_, c_int(int(k)))
        if rc != SFMX_OK:
            raise SfmxError(rc, f"sfmx_texture_set_batch: {k} is not in 0 .. {VISIB_MAX_BATCH}")

    def run(self, verts, faces, z_min=0.0, depth_tol=-1.0, n=None, m=None, read=True, **params):
        """verts float64 [n][3] and faces int32 [m][3]: numpy arrays, or ints (device pointers) with n and m given.  z_min and
        depth_tol are required; params: TEXTURE_DEFAULTS keys.  Returns read()'s dict, or counts() with read=False."""
        p = texture_params(z_min, depth_tol, **params)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int):
            raise TypeError("verts and faces: both host arrays or both device pointers")
        if on_dev:
            pv, pf = c_void_p(verts), c_void_p(faces)
            n, m = int(n), int(m)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
        self.ctx._chk(self.ctx.lib.sfmx_texture_run(self.ctx.h_, self.h_, pv, c_int(n), pf, c_int(m), c_int(1 if on_dev else 0), byref(p)))
        return self.read() if read else self.counts()

    def sizes(self):
        """(n, m, V, W, H) of the last successful run; raises before one"""
        s = [c_int(0) for _ in range(5)]
        rc = self.ctx.lib.sfmx_texture_sizes(self.h_, *[byref(x) for x in s])
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_texture_sizes: no successful run")
        return tuple(x.value for x in s)

    def counts(self) -> dict:
        """dict of TEXTURE_COUNTS of the last successful run; raises before one"""
        c = (c_int32 * 6)()
        rc = self.ctx.lib.sfmx_texture_counts(self.h_, c)
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_texture_counts: no successful run")
        return dict(zip(TEXTURE_COUNTS, [int(x) for x in c]))

    def read(self) -> dict:
        """the last run: dict(atlas u8 [H][W], face_view i32 [m], face_area i64 [m], uv_half i32 [m][3][2], uv f64 [m][3][2],
        view_faces i32 [V], the TEXTURE_COUNTS)"""
        n, m, V, W, H = self.sizes()
        atlas = np.zeros(max(W * H, 1), np.uint8)
        fview, farea = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int64)
        uvh, vfaces = np.zeros((max(m, 1), 3, 2), np.int32), np.zeros(max(V, 1), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_texture_read(self.ctx.h_, self.h_, _p(atlas, c_uint8), _p(fview, c_int32),
                                                     farea.ctypes.data_as(c_void_p), _p(uvh, c_int32), _p(vfaces, c_int32)))
        return dict(atlas=atlas[:W * H].reshape(H, W).copy(), face_view=fview[:m].copy(), face_area=farea[:m].copy(), uv_half=uvh[:m].copy(),
                    uv=texture_uv(uvh[:m], W, H), view_faces=vfaces[:V].copy(), **self.counts())

    def device_atlas(self):
        """(W H, device pointer of the atlas, W, H); W H = -1 before a successful run"""
        a, W, H = c_void_p(), c_int(0), c_int(0)
        k = int(self.ctx.lib.sfmx_texture_device_atlas(self.h_, byref(a), byref(W), byref(H)))
        return k, a.value, int(W.value), int(H.value)

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_texture_last_us(self.h_))

    def last_bake_us(self) -> float:
        return float(self.ctx.lib.sfmx_texture_last_bake_us(self.h_))

    def last_batch(self) -> int:
        """the largest number of views the last run put into one batch"""
        return int(self.ctx.lib.sfmx_texture_last_batch(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_texture_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Level:
    """sfmx_level: the seams of a texture atlas levelled: one offset per (vertex, view), pinned to the mean of the
    views' samples on the seams and relaxed by Jacobi sweeps elsewhere, added to every texel of the texture object's atlas before
    its rounding.  The work buffers are kept between runs."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        self.n_ = self.m_ = 0
        ctx._chk(ctx.lib.sfmx_level_create(ctx.h_, byref(self.h_)))

    def run(self, tx: "Texture", verts, faces, n=None, m=None, read=True, **params):
        """tx: the Texture whose last run was on this mesh.  verts float64 [n][3] and faces int32 [m][3]: numpy arrays, or ints
        (device pointers) with n and m given.  params: LEVEL_DEFAULTS keys.  Returns read()'s dict, or counts() with read=False."""
        p = level_params(**params)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int):
            raise TypeError("verts and faces: both host arrays or both device pointers")
        if on_dev:
            pv, pf = c_void_p(verts), c_void_p(faces)
            n, m = int(n), int(m)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
        self.ctx._chk(self.ctx.lib.sfmx_level_run(self.ctx.h_, self.h_, tx.h_, pv, c_int(n), pf, c_int(m), c_int(1 if on_dev else 0), byref(p)))
        self.n_, self.m_ = n, m
        return self.read() if read else self.counts()

    def counts(self) -> dict:
        """dict of LEVEL_COUNTS of the last successful run; raises before one"""
        c = (c_int32 * 6)()
        rc = self.ctx.lib.sfmx_level_counts(self.h_, c)
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_level_counts: no successful run")
        return dict(zip(LEVEL_COUNTS, [int(x) for x in c]))

    def read(self) -> dict:
        """the last run: dict(atlas u8 [H][W], corner_adj i32 [m][3], corner_sample i32 [m][3], vertex_views i32 [n], the
        LEVEL_COUNTS)"""
        k, _, W, H = self.device_atlas()
        if k < 0:
            raise SfmxError(SFMX_ERR_INVALID, "sfmx_level_read: no successful run")
        n, m = self.n_, self.m_
        atlas = np.zeros(max(W * H, 1), np.uint8)
        cadj, csamp = np.zeros((max(m, 1), 3), np.int32), np.zeros((max(m, 1), 3), np.int32)
        vviews = np.zeros(max(n, 1), np.int32)
        self.ctx._chk(self.ctx.lib.sfmx_level_read(self.ctx.h_, self.h_, _p(atlas, c_uint8), _p(cadj, c_int32), _p(csamp, c_int32),
                                                   _p(vviews, c_int32)))
        return dict(atlas=atlas[:W * H].reshape(H, W).copy(), corner_adj=cadj[:m].copy(), corner_sample=csamp[:m].copy(),
                    vertex_views=vviews[:n].copy(), **self.counts())

    def device_atlas(self):
        """(W H, device pointer of the levelled atlas, W, H); W H = -1 before a successful run"""
        a, W, H = c_void_p(), c_int(0), c_int(0)
        k = int(self.ctx.lib.sfmx_level_device_atlas(self.h_, byref(a), byref(W), byref(H)))
        return k, a.value, int(W.value), int(H.value)

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_level_last_us(self.h_))

    def last_sweeps_us(self) -> float:
        return float(self.ctx.lib.sfmx_level_last_sweeps_us(self.h_))

    def last_bake_us(self) -> float:
        return float(self.ctx.lib.sfmx_level_last_bake_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_level_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Photo:
    """sfmx_photo: the textured mesh rendered back into cameras and compared with their pictures: per pixel the
    rendered grey, its class (PHOTO_CLASSES) and the visible face; per view the class counts and, for the pixels textured from
    this view (own) and from another (cross), the count, the sums of |d| and d^2 and the histogram of |d|.  The views, their
    images and the work buffers are kept between runs."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_photo_create(ctx.h_, byref(self.h_)))
        self.shapes = []  # (h, w) of every view

    def reset(self):
        self.ctx._chk(self.ctx.lib.sfmx_photo_reset(self.ctx.h_, self.h_))
        self.shapes = []

    def add_view(self, cam: dict, image=None, tex_view=-1, w=None, h=None):
        """cam: dict(R_rw, c_left, f, cx, cy, w, h) (B is not used; w= / h= override the dict's image size).  image: uint8 [h][w]
        numpy array, an int (device pointer), or None.  tex_view: this camera's index in the texture object's list, or -1."""
        w, h = int(cam["w"] if w is None else w), int(cam["h"] if h is None else h)
        v = fusion_view({**cam, "B": cam.get("B", 0.0)}, w, h)
        on_dev = isinstance(image, int)
        if image is None:
            pi = None
        elif on_dev:
            pi = c_void_p(image)
        else:
            image = np.ascontiguousarray(image, np.uint8)
            assert image.shape == (h, w), (image.shape, h, w)
            pi = image.ctypes.data_as(c_void_p)
        self.ctx._chk(self.ctx.lib.sfmx_photo_add_view(self.ctx.h_, self.h_, byref(v), pi, c_int(1 if on_dev else 0), c_int(int(tex_view))))
        self.shapes.append((h, w))

    def add_texture_views(self, tx: "Texture"):
        """appends all of tx's views with their images, device to device, view k with tex_view = k"""
        assert len(tx.shapes) == tx.view_count(), (len(tx.shapes), tx.view_count())
        self.ctx._chk(self.ctx.lib.sfmx_photo_add_texture_views(self.ctx.h_, self.h_, tx.h_))
        self.shapes += tx.shapes

    def view_count(self) -> int:
        return int(self.ctx.lib.sfmx_photo_view_count(self.h_))

    def set_batch(self, k: int):
        """k >= 1 forces k views per batch, 0 restores the automatic size; the result does not depend on it"""
        rc = self.ctx.lib.sfmx_photo_set_batch(self.h_, c_int(int(k)))
        if rc != SFMX_OK:
            raise SfmxError(rc, f"sfmx_photo_set_batch: {k} is not in 0 .. {VISIB_MAX_BATCH}")

    def run(self, tx: "Texture", verts, faces, z_min=0.0, lv: "Level" = None, n=None, m=None, read=True, **params):
        """tx: the Texture whose last run was on this mesh; lv: a Level whose last run was on tx, or None.  verts float64 [n][3]
        and faces int32 [m][3]: numpy arrays, or ints (device pointers) with n and m given.  z_min is required; params:
        PHOTO_DEFAULTS keys.  Returns read()'s dict, or sizes() with read=False."""
        p = photo_params(z_min, **params)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int):
            raise TypeError("verts and faces: both host arrays or both device pointers")
        if on_dev:
            pv, pf = c_void_p(verts), c_void_p(faces)
            n, m = int(n), int(m)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
        self.ctx._chk(self.ctx.lib.sfmx_photo_run(self.ctx.h_, self.h_, tx.h_, lv.h_ if lv is not None else None, pv, c_int(n), pf, c_int(m),
                                                  c_int(1 if on_dev else 0), byref(p)))
        return self.read() if read else self.sizes()

    def sizes(self):
        """(Q, the sum of w h) of the last successful run; raises before one"""
        q, px = c_int(0), c_int(0)
        rc = self.ctx.lib.sfmx_photo_sizes(self.h_, byref(q), byref(px))
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_photo_sizes: no successful run")
        return q.value, px.value

    def read(self) -> dict:
        """the last run: dict(rendered u8 / cls u8 / face i32 [sum w h], classes i64 [Q][5], stats i64 [Q][2][3], hist i64
        [Q][2][256], offsets i64 [Q + 1]: view q's pixels are [offsets[q], offsets[q + 1]))"""
        Q, px = self.sizes()
        rendered, cls, face = np.zeros(max(px, 1), np.uint8), np.zeros(max(px, 1), np.uint8), np.zeros(max(px, 1), np.int32)
        classes, stats, hist = np.zeros((max(Q, 1), 5), np.int64), np.zeros((max(Q, 1), 2, 3), np.int64), np.zeros((max(Q, 1), 2, 256), np.int64)
        self.ctx._chk(self.ctx.lib.sfmx_photo_read(self.ctx.h_, self.h_, _p(rendered, c_uint8), _p(cls, c_uint8), _p(face, c_int32),
                                                   classes.ctypes.data_as(c_void_p), stats.ctypes.data_as(c_void_p),
                                                   hist.ctypes.data_as(c_void_p)))
        off = np.zeros(Q + 1, np.int64)
        if len(self.shapes) == Q:
            off[1:] = np.cumsum([a * b for a, b in self.shapes], dtype=np.int64)
            assert int(off[-1]) == px, (int(off[-1]), px)
        return dict(rendered=rendered[:px].copy(), cls=cls[:px].copy(), face=face[:px].copy(), classes=classes[:Q].copy(),
                    stats=stats[:Q].copy(), hist=hist[:Q].copy(), offsets=off)

    def view_image(self, res: dict, q: int, key="rendered"):
        """[h][w] of view q out of read()'s dict"""
        h, w = self.shapes[q]
        return res[key][int(res["offsets"][q]):int(res["offsets"][q + 1])].reshape(h, w)

    def device_rendered(self):
        """(the sum of w h, device pointer of the rendered pixels); -1 before a successful run"""
        a = c_void_p()
        k = int(self.ctx.lib.sfmx_photo_device_rendered(self.h_, byref(a)))
        return k, a.value

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_photo_last_us(self.h_))

    def last_resolve_us(self) -> float:
        return float(self.ctx.lib.sfmx_photo_last_resolve_us(self.h_))

    def last_batch(self) -> int:
        """the largest number of views the last run put into one batch"""
        return int(self.ctx.lib.sfmx_photo_last_batch(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_photo_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Align:
    """sfmx_align: registration of a view to a TSDF volume by direct Gauss-Newton alignment.  The device work
    buffers grow on demand and are kept between calls."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_align_create(ctx.h_, byref(self.h_)))

    def _volume(self, vol):
        """(fusion handle or None, the arguments of the _arrays entries, what must stay alive)"""
        if isinstance(vol, Fusion):
            return vol.h_, None, None
        sum_, count, origin, voxel = vol[:4]
        on_dev = isinstance(sum_, int)
        if on_dev != isinstance(count, int):
            raise TypeError("sum and count: both host arrays or both device pointers")
        if on_dev:
            dims = vol[4]
            ps, pc = c_void_p(sum_), c_void_p(count)
        else:
            sum_ = _f64(sum_)
            count = np.ascontiguousarray(count, np.int32)
            assert sum_.ndim == 3 and count.shape == sum_.shape
            dims = sum_.shape[::-1]
            ps, pc = sum_.ctypes.data_as(c_void_p), count.ctypes.data_as(c_void_p)
        fp = fusion_params(origin, voxel, dims)
        return None, (byref(fp), ps, pc, c_int(1 if on_dev else 0)), (fp, sum_, count)

    @staticmethod
    def _map(cam, disp16, shape):
        if isinstance(disp16, int):
            h, w = shape
            return fusion_view(cam, w, h), c_void_p(disp16), 1, None
        disp16 = np.ascontiguousarray(disp16, np.int16)
        h, w = disp16.shape
        return fusion_view(cam, w, h), disp16.ctypes.data_as(c_void_p), 0, disp16

    def system(self, vol, cam: dict, disp16, shape=None, **params):
        """one evaluation at cam's pose, no step: (sums f64 [28] = A row by row upper, b, e; n).  vol: a Fusion (its pending
        views are integrated first), or (sum, count, origin, voxel) host arrays, or ints (device pointers) followed by dims.
        cam: dict(R_rw, c_left, f, cx, cy, B); disp16: int16 [h][w] array, or an int (device pointer) with shape=(h, w).
        params: ALIGN_DEFAULTS keys."""
        p = align_params(**params)
        fu, arr, keep = self._volume(vol)
        v, pd, on_dev, keep2 = self._map(cam, disp16, shape)
        sums, n = np.zeros(28), c_int32(0)
        if fu is not None:
            self.ctx._chk(self.ctx.lib.sfmx_align_system(self.ctx.h_, self.h_, fu, byref(v), pd, c_int(on_dev), byref(p), _p(sums, c_double),
                                                         byref(n)))
        else:
            self.ctx._chk(self.ctx.lib.sfmx_align_system_arrays(self.ctx.h_, self.h_, *arr, byref(v), pd, c_int(on_dev), byref(p),
                                                                _p(sums, c_double), byref(n)))
        return sums, int(n.value)

    def view(self, vol, cam: dict, disp16, shape=None, **params) -> dict:
        """the Gauss-Newton loop from cam's pose: AlignResult.asdict().  disp16 may also be a Stereo: its last map is read in
        place on the device (vol must then be a Fusion)."""
        p = align_params(**params)
        fu, arr, keep = self._volume(vol)
        out = AlignResult()
        if isinstance(disp16, Stereo):
            if fu is None:
                raise TypeError("a Stereo map needs a Fusion volume")
            v = fusion_view(cam, disp16.w, disp16.h)
            self.ctx._chk(self.ctx.lib.sfmx_align_stereo_view(self.ctx.h_, self.h_, fu, byref(v), disp16.h_, byref(p), byref(out)))
            return out.asdict()
        v, pd, on_dev, keep2 = self._map(cam, disp16, shape)
        if fu is not None:
            self.ctx._chk(self.ctx.lib.sfmx_align_view(self.ctx.h_, self.h_, fu, byref(v), pd, c_int(on_dev), byref(p), byref(out)))
        else:
            self.ctx._chk(self.ctx.lib.sfmx_align_view_arrays(self.ctx.h_, self.h_, *arr, byref(v), pd, c_int(on_dev), byref(p), byref(out)))
        return out.asdict()

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_align_last_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_align_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PAlign:
    """sfmx_palign: registration of a camera to the textured mesh by direct photometric Gauss-Newton alignment.
    The model (a Texture's last run, optionally a Level's atlas, and the mesh) and one picture are set once and serve many
    calls; the work buffers grow on demand and are kept."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_palign_create(ctx.h_, byref(self.h_)))
        self.shape = None  # (h, w) of the picture
        self._keep = None  # the Texture and Level the model refers to

    def set_model(self, tx: "Texture", verts, faces, lv: "Level" = None, n=None, m=None):
        """tx: the Texture whose last run was on this mesh; lv: a Level whose last run was on tx, or None.  verts float64 [n][3]
        and faces int32 [m][3]: numpy arrays, or ints (device pointers) with n and m given; they are copied.  tx may also be a
        texture result on the host, dict(face_view, uv_half, atlas) (lv then a level result dict(atlas) or None; host mesh)."""
        if isinstance(tx, dict):
            if isinstance(verts, int) or isinstance(faces, int):
                raise TypeError("a texture result on the host goes with a host mesh")
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            fv = np.ascontiguousarray(tx["face_view"], np.int32).reshape(-1)
            uvh = np.ascontiguousarray(tx["uv_half"], np.int32).reshape(-1, 3, 2)
            atlas = np.ascontiguousarray((lv if lv is not None else tx)["atlas"], np.uint8)
            if len(fv) != len(faces) or len(uvh) != len(faces) or atlas.ndim != 2:
                raise SfmxError(SFMX_ERR_INVALID, "sfmx_palign: face_view and uv_half are per face, the atlas u8 [H][W]")
            self.ctx._chk(self.ctx.lib.sfmx_palign_set_model_arrays(self.ctx.h_, self.h_, _p(fv, c_int32), _p(uvh, c_int32), _p(atlas, c_uint8),
                                                                    c_int(atlas.shape[1]), c_int(atlas.shape[0]),
                                                                    verts.ctypes.data_as(c_void_p), c_int(len(verts)),
                                                                    faces.ctypes.data_as(c_void_p), c_int(len(faces))))
            self._keep = None
            return
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int):
            raise TypeError("verts and faces: both host arrays or both device pointers")
        if on_dev:
            pv, pf = c_void_p(verts), c_void_p(faces)
            n, m = int(n), int(m)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            n, m = len(verts), len(faces)
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
        self.ctx._chk(self.ctx.lib.sfmx_palign_set_model(self.ctx.h_, self.h_, tx.h_, lv.h_ if lv is not None else None, pv, c_int(n), pf,
                                                         c_int(m), c_int(1 if on_dev else 0)))
        self._keep = (tx, lv)

    def set_image(self, image, shape=None):
        """image: uint8 [h][w] numpy array, or an int (device pointer) with shape=(h, w); it is copied"""
        if isinstance(image, int):
            h, w = (int(v) for v in shape)
            pi, on_dev = c_void_p(image), 1
        else:
            image = np.ascontiguousarray(image, np.uint8)
            if image.ndim != 2:
                raise TypeError("the picture is uint8 [h][w]")
            h, w = image.shape
            pi, on_dev = image.ctypes.data_as(c_void_p), 0
        self.ctx._chk(self.ctx.lib.sfmx_palign_set_image(self.ctx.h_, self.h_, pi, c_int(w), c_int(h), c_int(on_dev)))
        self.shape = (h, w)

    def _view(self, cam: dict):
        if self.shape is None:
            raise SfmxError(SFMX_ERR_INVALID, "sfmx_palign: set_image first")
        h, w = self.shape  # a camera that states another size is refused by the library
        return fusion_view({**cam, "B": cam.get("B", 0.0)}, cam.get("w", w), cam.get("h", h))

    def system(self, cam: dict, z_min=0.0, pivot=(0.0, 0.0, 0.0), **params):
        """one evaluation at cam's pose, no step: (sums f64 [28] = A row by row upper, b, e; n).  cam: dict(R_rw, c_left, f, cx,
        cy[, w, h]); z_min and pivot are required; params: PALIGN_DEFAULTS keys."""
        p = palign_params(z_min, pivot, **params)
        v = self._view(cam)
        sums, n = np.zeros(28), c_int32(0)
        self.ctx._chk(self.ctx.lib.sfmx_palign_system(self.ctx.h_, self.h_, byref(v), byref(p), _p(sums, c_double), byref(n)))
        return sums, int(n.value)

    def view(self, cam: dict, z_min=0.0, pivot=(0.0, 0.0, 0.0), **params) -> dict:
        """the Gauss-Newton loop from cam's pose: dict(view, status, iterations, trace=[(n, e, |omega|, |v|), ...])"""
        p = palign_params(z_min, pivot, **params)
        v = self._view(cam)
        out = PAlignResult()
        self.ctx._chk(self.ctx.lib.sfmx_palign_view(self.ctx.h_, self.h_, byref(v), byref(p), byref(out)))
        return out.asdict()

    def sizes(self):
        """(nsy, nsx) of the last evaluation; raises before one"""
        nsx, nsy = c_int(0), c_int(0)
        rc = self.ctx.lib.sfmx_palign_sizes(self.h_, byref(nsx), byref(nsy))
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_palign_sizes: no evaluation")
        return nsy.value, nsx.value

    def read(self):
        """(state u8 [nsy][nsx]: 0 not a candidate, 1 trimmed by r_max, 2 used; r f64 [nsy][nsx]) of the last evaluation"""
        nsy, nsx = self.sizes()
        state, r = np.zeros((nsy, nsx), np.uint8), np.zeros((nsy, nsx))
        self.ctx._chk(self.ctx.lib.sfmx_palign_read(self.ctx.h_, self.h_, _p(state, c_uint8), _p(r, c_double)))
        return state, r

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_palign_last_us(self.h_))

    def last_zbuffer_us(self) -> float:
        return float(self.ctx.lib.sfmx_palign_last_zbuffer_us(self.h_))

    def last_system_us(self) -> float:
        """k_pa_system and the tree's levels alone; last_us - last_zbuffer_us - this is the mask and its erosion"""
        return float(self.ctx.lib.sfmx_palign_last_system_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_palign_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Register:
    """sfmx_register: Sim(3) point-to-plane registration of source points to a target mesh.  One target serves
    many sources; the target's grid and the work buffers are kept between calls."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h_ = c_void_p()
        self.d_max = None
        self.cell = 0.0
        ctx._chk(ctx.lib.sfmx_register_create(ctx.h_, byref(self.h_)))

    def set_target(self, verts, faces, d_max, cell=0.0, nv=None, m=None):
        """verts float64 [nv][3] and faces int32 [m][3]: numpy arrays, or ints (device pointers) with nv and m given; d_max is
        the trimming distance of every later call"""
        p = register_params(d_max, cell=cell)
        on_dev = isinstance(verts, int)
        if on_dev != isinstance(faces, int):
            raise TypeError("verts and faces: both host arrays or both device pointers")
        if on_dev:
            pv, pf = c_void_p(verts), c_void_p(faces)
        else:
            verts = _f64(verts).reshape(-1, 3)
            faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
            nv, m = len(verts), len(faces)
            pv, pf = verts.ctypes.data_as(c_void_p), faces.ctypes.data_as(c_void_p)
        self.d_max = None
        self.ctx._chk(self.ctx.lib.sfmx_register_set_target(self.ctx.h_, self.h_, pv, c_int(nv), pf, c_int(m), c_int(1 if on_dev else 0),
                                                            byref(p)))
        self.d_max, self.cell = float(d_max), float(cell)

    def _params(self, params) -> RegisterParams:
        if "d_max" in params or "cell" in params:
            raise TypeError("d_max and cell belong to set_target")
        # without a target the library refuses the call; any valid d_max lets it get that far
        return register_params(1.0 if self.d_max is None else self.d_max, cell=self.cell, **params)

    @staticmethod
    def _points(points, n):
        if isinstance(points, int):
            return c_void_p(points), int(n), 1, None
        points = _f64(points).reshape(-1, 3)
        return points.ctypes.data_as(c_void_p), len(points), 0, points

    def pivot(self) -> np.ndarray:
        p = np.zeros(3)
        rc = self.ctx.lib.sfmx_register_pivot(self.h_, _p(p, c_double))
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_register_pivot: no target")
        return p

    def system(self, points, T=None, n=None, **params):
        """one evaluation at T (None: the identity), no step: (sums f64 [37] = A row by row upper, b, e, c; n_used).  points:
        float64 [n][3], or an int (device pointer) with n given.  params: REGISTER_DEFAULTS keys but cell."""
        p = self._params(params)
        pp, n, on_dev, keep = self._points(points, n)
        t = register_transform(T)
        sums, nu = np.zeros(REGISTER_TERMS), c_int32(0)
        self.ctx._chk(self.ctx.lib.sfmx_register_system(self.ctx.h_, self.h_, pp, c_int(n), c_int(on_dev), byref(t), byref(p),
                                                        _p(sums, c_double), byref(nu)))
        return sums, int(nu.value)

    def run(self, points, init=None, n=None, **params) -> dict:
        """the Gauss-Newton loop from init (None: the identity): RegisterResult.asdict()"""
        p = self._params(params)
        pp, n, on_dev, keep = self._points(points, n)
        t = register_transform(init) if init is not None else None
        out = RegisterResult()
        self.ctx._chk(self.ctx.lib.sfmx_register_run(self.ctx.h_, self.h_, pp, c_int(n), c_int(on_dev), byref(t) if t is not None else None,
                                                     byref(p), byref(out)))
        return out.asdict()

    def apply(self, T, points, n=None) -> np.ndarray:
        """float64 [n][3]: every point moved by T"""
        pp, n, on_dev, keep = self._points(points, n)
        t = register_transform(T)
        out = np.zeros((max(n, 1), 3))
        self.ctx._chk(self.ctx.lib.sfmx_register_apply(self.ctx.h_, self.h_, byref(t), pp, c_int(n), c_int(on_dev), _p(out, c_double)))
        return out[:n].copy()

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_register_last_us(self.h_))

    def last_query_us(self) -> float:
        return float(self.ctx.lib.sfmx_register_last_query_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_register_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stereo:
    """Device buffers of sfmx_stereo for one (w, h, params); disparity() runs rectify -> census -> SGM -> select -> speckle."""

    def __init__(self, ctx: "Context", w: int, h: int, **params):
        self.ctx, self.w, self.h = ctx, w, h
        self.params = stereo_params(**params)
        self.D = self.params.num_disparities
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_stereo_create(ctx.h_, c_int(w), c_int(h), byref(self.params), byref(self.h_)))

    def rectify(self, img_l, img_r, H_l, H_r):
        """the rectification alone (no disparity): both rectified images stay on the device for the add_stereo_view entries that
        take the left one.  img_l / img_r as disparity() takes them."""
        on_dev = isinstance(img_l, int)
        if on_dev != isinstance(img_r, int):
            raise TypeError("img_l and img_r: both host arrays or both device pointers")
        if on_dev:
            pl, pr = c_void_p(img_l), c_void_p(img_r)
        else:
            img_l = np.ascontiguousarray(img_l, np.uint8)
            img_r = np.ascontiguousarray(img_r, np.uint8)
            assert img_l.shape == (self.h, self.w) and img_r.shape == (self.h, self.w)
            pl, pr = _p(img_l, c_uint8), _p(img_r, c_uint8)
        Hl, Hr = _f64(H_l).reshape(9), _f64(H_r).reshape(9)
        self.ctx._chk(self.ctx.lib.sfmx_stereo_rectify(self.ctx.h_, self.h_, pl, pr, c_int(1 if on_dev else 0), _p(Hl, c_double),
                                                       _p(Hr, c_double)))

    def disparity(self, img_l, img_r, H_l, H_r, want_rect: bool = False, want_sum: bool = False):
        """img_l / img_r: u8 [h][w] numpy arrays, or ints (device pointers of u8 [h][w] in HBM).
        Returns disp16 int16 [h][w] (-16 invalid), or dict(disp16, rect, S) when want_rect / want_sum."""
        on_dev = isinstance(img_l, int)
        if on_dev != isinstance(img_r, int):
            raise TypeError("img_l and img_r: both host arrays or both device pointers")
        if on_dev:
            pl, pr = c_void_p(img_l), c_void_p(img_r)
        else:
            img_l = np.ascontiguousarray(img_l, np.uint8)
            img_r = np.ascontiguousarray(img_r, np.uint8)
            assert img_l.shape == (self.h, self.w) and img_r.shape == (self.h, self.w)
            pl, pr = _p(img_l, c_uint8), _p(img_r, c_uint8)
        Hl, Hr = _f64(H_l).reshape(9), _f64(H_r).reshape(9)
        d16 = np.zeros((self.h, self.w), np.int16)
        rect = np.zeros((2, self.h, self.w), np.uint8) if want_rect else None
        S = np.zeros((self.h, self.w, self.D), np.uint16) if want_sum else None
        self.ctx._chk(self.ctx.lib.sfmx_stereo_disparity(self.ctx.h_, self.h_, pl, pr, c_int(1 if on_dev else 0), _p(Hl, c_double),
                                                         _p(Hr, c_double), d16.ctypes.data_as(c_void_p),
                                                         rect.ctypes.data_as(c_void_p) if want_rect else None,
                                                         S.ctypes.data_as(c_void_p) if want_sum else None))
        if want_rect or want_sum:
            return dict(disp16=d16, rect=rect, S=S)
        return d16

    def last_us(self) -> float:
        return float(self.ctx.lib.sfmx_stereo_last_us(self.h_))

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_stereo_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BaProblem:
    def __init__(self, ctx: "Context", W: int, X, obs_ptr, obs_li, obs_uv):
        self.ctx, self.W = ctx, W
        X = _f64(X)
        obs_ptr = np.ascontiguousarray(obs_ptr, np.int32)
        obs_li = np.ascontiguousarray(obs_li, np.int32)
        obs_uv = _f64(obs_uv)
        self.P = X.shape[0]
        self.h_ = c_void_p()
        ctx._chk(ctx.lib.sfmx_ba_create(ctx.h_, c_int(W), c_int(self.P), _p(X, c_double), _p(obs_ptr, c_int32),
                                        _p(obs_li, c_int32), _p(obs_uv, c_double), byref(self.h_)))

    def reset(self, W: int, X, obs_ptr, obs_li, obs_uv):
        """re-target this object at another window (sfmx_ba_reset): the device buffers are kept and only grow"""
        X = _f64(X)
        obs_ptr = np.ascontiguousarray(obs_ptr, np.int32)
        obs_li = np.ascontiguousarray(obs_li, np.int32)
        obs_uv = _f64(obs_uv)
        self.ctx._chk(self.ctx.lib.sfmx_ba_reset(self.ctx.h_, self.h_, c_int(W), c_int(X.shape[0]), _p(X, c_double), _p(obs_ptr, c_int32),
                                                 _p(obs_li, c_int32), _p(obs_uv, c_double)))
        self.W, self.P = W, X.shape[0]

    def build(self, poses_wc, fx, fy, cx, cy, huber, lam, damp=True):
        D = 6 * self.W
        poses = _f64(poses_wc)
        S = np.zeros((D, D))
        b = np.zeros(D)
        self.ctx._chk(self.ctx.lib.sfmx_ba_build(self.ctx.h_, self.h_, _p(poses, c_double), c_double(fx), c_double(fy),
                                                 c_double(cx), c_double(cy), c_double(huber), c_double(lam),
                                                 c_int(1 if damp else 0), _p(S, c_double), _p(b, c_double)))
        return S, b

    def step(self, poses_wc, fx, fy, cx, cy, huber, lam):
        """returns (status, dx): status SFMX_OK or SFMX_ERR_SINGULAR"""
        poses = _f64(poses_wc)
        dx = np.zeros(6 * self.W)
        rc = self.ctx.lib.sfmx_ba_step(self.ctx.h_, self.h_, _p(poses, c_double), c_double(fx), c_double(fy), c_double(cx),
                                       c_double(cy), c_double(huber), c_double(lam), _p(dx, c_double))
        if rc not in (SFMX_OK, SFMX_ERR_SINGULAR):
            self.ctx._chk(rc)
        return rc, dx

    def begin(self, iters, fx, fy, cx, cy, huber, lam):
        """bracket of a job of `iters` step() calls (resident kernel for window-sized problems)"""
        self.ctx._chk(self.ctx.lib.sfmx_ba_begin(self.ctx.h_, self.h_, c_int(iters), c_double(fx), c_double(fy), c_double(cx), c_double(cy),
                                                 c_double(huber), c_double(lam)))

    def end(self):
        self.ctx._chk(self.ctx.lib.sfmx_ba_end(self.ctx.h_, self.h_))

    def step_sharded(self, comm, poses_wc, fx, fy, cx, cy, huber, lam):
        """point-sharded iteration: partial build, RCCL all-reduce of S|b in HBM, damping + gauge, solve (comm None = 1 rank)"""
        poses = _f64(poses_wc)
        dx = np.zeros(6 * self.W)
        rc = self.ctx.lib.sfmx_ba_step_sharded(self.ctx.h_, comm.h_ if comm is not None else None, self.h_, _p(poses, c_double), c_double(fx),
                                               c_double(fy), c_double(cx), c_double(cy), c_double(huber), c_double(lam), _p(dx, c_double))
        if rc not in (SFMX_OK, SFMX_ERR_SINGULAR):
            self.ctx._chk(rc)
        return rc, dx

    def step_sharded_elements(self, comm, poses_wc, fx, fy, cx, cy, huber, lam):
        """element-sharded iteration (this problem holds the WHOLE window): bit-identical to step() at any world size"""
        poses = _f64(poses_wc)
        dx = np.zeros(6 * self.W)
        rc = self.ctx.lib.sfmx_ba_step_sharded_elements(self.ctx.h_, comm.h_ if comm is not None else None, self.h_, _p(poses, c_double),
                                                        c_double(fx), c_double(fy), c_double(cx), c_double(cy), c_double(huber), c_double(lam),
                                                        _p(dx, c_double))
        if rc not in (SFMX_OK, SFMX_ERR_SINGULAR):
            self.ctx._chk(rc)
        return rc, dx

    def build_partial(self, poses_wc, fx, fy, cx, cy, huber):
        """device pointers (S, b) of this shard's raw sums — for RCCL all-reduce by the caller"""
        poses = _f64(poses_wc)
        S, b = c_void_p(), c_void_p()
        self.ctx._chk(self.ctx.lib.sfmx_ba_build_partial(self.ctx.h_, self.h_, _p(poses, c_double), c_double(fx), c_double(fy),
                                                         c_double(cx), c_double(cy), c_double(huber), byref(S), byref(b)))
        return S.value, b.value

    def close(self):
        if self.h_:
            self.ctx.lib.sfmx_ba_destroy(self.ctx.h_, self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """rank 0: the 128-byte RCCL unique id the other ranks need for Comm(...)"""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    rc = load_library().sfmx_comm_get_unique_id(buf)
    if rc != SFMX_OK:
        raise SfmxError(rc, "sfmx_comm_get_unique_id (is librccl loadable?)")
    return buf.raw


class Comm:
    """One RCCL communicator (one per host thread / lane that issues collectives)."""

    def __init__(self, device: int, unique_id: bytes | None, rank: int, world: int):
        self.lib = load_library()
        self.h_ = c_void_p()
        rc = self.lib.sfmx_comm_create(c_int(device), unique_id, c_int(rank), c_int(world), byref(self.h_))
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_comm_create")
        self.rank, self.world = rank, world

    def close(self):
        if self.h_:
            self.lib.sfmx_comm_destroy(self.h_)
            self.h_ = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_range(n: int, rank: int, world: int):
    lo, hi = c_int(), c_int()
    load_library().sfmx_shard_range(c_int(n), c_int(rank), c_int(world), byref(lo), byref(hi))
    return lo.value, hi.value


class Context:
    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.h_ = c_void_p()
        rc = self.lib.sfmx_ctx_create(c_int(device), byref(self.h_))
        if rc != SFMX_OK:
            raise SfmxError(rc, "sfmx_ctx_create failed: no usable MI355X (gfx950) device — there is no CPU fallback")

    def _chk(self, rc: int):
        if rc != SFMX_OK:
            raise SfmxError(rc, (self.lib.sfmx_last_error(self.h_) or b"").decode())

    def close(self):
        if self.h_:
            self.lib.sfmx_ctx_destroy(self.h_)
            self.h_ = c_void_p()

    def set_timing(self, on: bool):
        self._chk(self.lib.sfmx_set_timing(self.h_, c_int(1 if on else 0)))

    def last_kernel_us(self) -> float:
        return float(self.lib.sfmx_last_kernel_us(self.h_))

    def kernel_profile(self, reset: bool = False) -> dict:
        """{kernel name: (gpu_us, launches)} accumulated on this context since timing was enabled"""
        us = (c_double * 32)()
        calls = (c_uint64 * 32)()
        n = self.lib.sfmx_kernel_profile(self.h_, c_int(1 if reset else 0), c_int(32), us, calls)
        return {self.lib.sfmx_kernel_profile_name(c_int(i)).decode(): (float(us[i]), int(calls[i])) for i in range(n)}

    def sync(self):
        self._chk(self.lib.sfmx_sync(self.h_))

    def pyramid(self, img: np.ndarray, levels: int) -> Pyramid:
        h, w = img.shape
        return Pyramid(self, w, h, levels).upload(img)

    def shi_score(self, pyr: Pyramid):
        score = np.zeros((pyr.h, pyr.w))
        mx = c_double()
        self._chk(self.lib.sfmx_shi_tomasi_score(self.h_, pyr.h_, _p(score, c_double), byref(mx)))
        return score, mx.value

    def shi_candidates(self, pyr: Pyramid, quality: float, cap: int | None = None):
        cap = cap or pyr.w * pyr.h
        xy = np.zeros(cap, np.uint32)
        sc = np.zeros(cap)
        n = c_int()
        mx = c_double()
        self._chk(self.lib.sfmx_shi_tomasi_candidates(self.h_, pyr.h_, c_double(quality), c_int(cap), _p(xy, c_uint32),
                                                      _p(sc, c_double), byref(n), byref(mx)))
        m = min(n.value, cap)
        return (xy[:m] & 0xFFFF).astype(np.int32), (xy[:m] >> 16).astype(np.int32), sc[:m].copy(), n.value, mx.value

    def shi_candidates_pruned(self, pyr: Pyramid, quality: float, min_dist: int, cap: int | None = None):
        cap = cap or pyr.w * pyr.h
        xy = np.zeros(cap, np.uint32)
        sc = np.zeros(cap)
        n, ntot = c_int(), c_int()
        mx = c_double()
        full = np.zeros(cap, np.int32)
        self._chk(self.lib.sfmx_shi_tomasi_candidates_pruned(self.h_, pyr.h_, c_double(quality), c_int(min_dist), c_int(cap),
                                                             _p(xy, c_uint32), _p(sc, c_double), _p(full, c_int32), byref(n),
                                                             byref(ntot), byref(mx)))
        m = min(n.value, cap)
        return ((xy[:m] & 0x7FFF).astype(np.int32), ((xy[:m] >> 16) & 0x7FFF).astype(np.int32), (xy[:m] >> 31).astype(bool),
                sc[:m].copy(), n.value, ntot.value)

    def klt_track(self, pa: Pyramid, pb: Pyramid, xy, levels=3, radius=5, iters=10, fb=1.0, want_back=True):
        """want_back=False passes xy_back = NULL (the backward pass still runs: keep needs it); back is then None"""
        xy = _f64(xy).reshape(-1, 2)
        n = xy.shape[0]
        fwd = np.zeros((n, 2))
        back = np.zeros((n, 2)) if want_back else None
        keep = np.zeros(n, np.uint8)
        steps = c_uint64()
        cfg = KltCfg(levels, radius, iters, fb)
        self._chk(self.lib.sfmx_klt_track(self.h_, pa.h_, pb.h_, _p(xy, c_double), c_int(n), byref(cfg), _p(fwd, c_double),
                                          _p(back, c_double) if want_back else None, _p(keep, c_uint8), byref(steps)))
        return fwd, back, keep, steps.value

    def klt_slow_steps(self) -> int:
        return int(self.lib.sfmx_debug_klt_slow_steps(self.h_))

    def ransac_score(self, xi, xj, idx8, thr, want_E=False):
        xi, xj = _f64(xi), _f64(xj)
        idx8 = np.ascontiguousarray(idx8, np.int32)
        H = idx8.shape[0]
        counts = np.zeros(H, np.int32)
        bi, bc = c_int32(), c_int32()
        E = np.zeros((H, 3, 3)) if want_E else None
        self._chk(self.lib.sfmx_ransac_score(self.h_, _p(xi, c_double), _p(xj, c_double), c_int(xi.shape[0]), _p(idx8, c_int32),
                                             c_int(H), c_double(thr), _p(counts, c_int32), byref(bi), byref(bc),
                                             _p(E, c_double) if want_E else None))
        return counts, bi.value, bc.value, E

    def ransac_score_ex(self, xi, xj, idx8, thr):
        """dict(counts, lo, hi, flags, cond, best_iter, best_count, E): certified per-hypothesis inlier counts"""
        xi, xj = _f64(xi), _f64(xj)
        idx8 = np.ascontiguousarray(idx8, np.int32)
        H = idx8.shape[0]
        counts, lo, hi = np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros(H, np.int32)
        flags = np.zeros(H, np.uint8)
        cond = np.zeros(H)
        E = np.zeros((H, 3, 3))
        bi, bc = c_int32(), c_int32()
        self._chk(self.lib.sfmx_ransac_score_ex(self.h_, _p(xi, c_double), _p(xj, c_double), c_int(xi.shape[0]), _p(idx8, c_int32),
                                                c_int(H), c_double(thr), _p(counts, c_int32), _p(lo, c_int32), _p(hi, c_int32),
                                                _p(flags, c_uint8), _p(cond, c_double), byref(bi), byref(bc), _p(E, c_double)))
        return dict(counts=counts, lo=lo, hi=hi, flags=flags, cond=cond, best_iter=bi.value, best_count=bc.value, E=E)

    def sampson_mask(self, xi, xj, E, thr):
        xi, xj, E = _f64(xi), _f64(xj), _f64(E)
        n = xi.shape[0]
        mask = np.zeros(n, np.uint8)
        cnt = c_int32()
        self._chk(self.lib.sfmx_sampson_mask(self.h_, _p(xi, c_double), _p(xj, c_double), c_int(n), _p(E, c_double), c_double(thr),
                                             _p(mask, c_uint8), byref(cnt)))
        return mask, cnt.value

    def ba_problem(self, W, X, obs_ptr, obs_li, obs_uv) -> BaProblem:
        return BaProblem(self, W, X, obs_ptr, obs_li, obs_uv)

    def solve_dense(self, A, b):
        A, b = _f64(A), _f64(b)
        n = b.shape[0]
        x = np.zeros(n)
        rc = self.lib.sfmx_solve_dense(self.h_, _p(A, c_double), _p(b, c_double), c_int(n), _p(x, c_double))
        if rc not in (SFMX_OK, SFMX_ERR_SINGULAR):
            self._chk(rc)
        return rc, x

    def posegraph_solve(self, n, entries_ij, entries_v, g3):
        """structured pose-graph solve (tolerance mode): lower-triangle entries of L, g [n][3] -> (status, x [n][3])"""
        ij = np.ascontiguousarray(entries_ij, np.int32).reshape(-1, 2)
        v = _f64(entries_v)
        g = _f64(g3).reshape(n, 3)
        x = np.zeros((n, 3))
        rc = self.lib.sfmx_posegraph_solve(self.h_, c_int(n), _p(ij, c_int32), _p(v, c_double), c_int(len(v)), _p(g, c_double), _p(x, c_double))
        if rc not in (SFMX_OK, SFMX_ERR_SINGULAR):
            self._chk(rc)
        return rc, x

    def fusion(self, origin, voxel, dims, **params) -> "Fusion":
        return Fusion(self, origin, voxel, dims, **params)

    def shade(self) -> "Shade":
        return Shade(self)

    def consist(self) -> "Consist":
        return Consist(self)

    def carve(self) -> "Carve":
        return Carve(self)

    def clean(self) -> "Clean":
        return Clean(self)

    def simplify(self) -> "Simplify":
        return Simplify(self)

    def smooth(self) -> "Smooth":
        return Smooth(self)

    def fill(self) -> "Fill":
        return Fill(self)

    def sdist(self) -> "Sdist":
        return Sdist(self)

    def raycast(self) -> "Raycast":
        return Raycast(self)

    def align(self) -> "Align":
        return Align(self)

    def register(self) -> "Register":
        return Register(self)

    def raster(self) -> "Raster":
        return Raster(self)

    def visib(self) -> "Visib":
        return Visib(self)

    def texture(self) -> "Texture":
        return Texture(self)

    def level(self) -> "Level":
        return Level(self)

    def photo(self) -> "Photo":
        return Photo(self)

    def palign(self) -> "PAlign":
        return PAlign(self)

    def stereo(self, w: int, h: int, **params) -> Stereo:
        return Stereo(self, w, h, **params)

    def stereo_disparity(self, img_l, img_r, H_l, H_r, want_rect: bool = False, want_sum: bool = False, **params):
        """the device stereo stage alone on one pair (buffers created and released around the call); see Stereo.disparity"""
        h, w = np.shape(img_l) if not isinstance(img_l, int) else params.pop("shape")
        st = Stereo(self, w, h, **params)
        try:
            return st.disparity(img_l, img_r, H_l, H_r, want_rect, want_sum)
        finally:
            st.close()

    def debug_hypot(self, x, y):
        x, y = _f64(x), _f64(y)
        out = np.zeros_like(x)
        self._chk(self.lib.sfmx_debug_hypot(self.h_, _p(x, c_double), _p(y, c_double), c_int(x.size), _p(out, c_double)))
        return out

    def debug_divsqrt(self, x, y):
        x, y = _f64(x), _f64(y)
        d, s = np.zeros_like(x), np.zeros_like(x)
        self._chk(self.lib.sfmx_debug_divsqrt(self.h_, _p(x, c_double), _p(y, c_double), c_int(x.size), _p(d, c_double),
                                              _p(s, c_double)))
        return d, s

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
