// shade.hip — vertex intensity of a surface from the views that see it.
//
// A sfmx_shade keeps, for every view added, the rectified left camera, its disparity map (int16) and its left rectified image
// (u8) on the device.  Shading projects every vertex into every view with the integration's own expressions (fusion.hip,
// DESIGN.md 13), keeps the views whose depth at that pixel agrees with the vertex's, and averages their pixels in integers.
//
// Exactness: IEEE double in one fixed expression order up to the depth test (built with -ffp-contract=off), int32 after it, so
// the result does not depend on the launch shape.  tests/appearance_ref.py restates it in NumPy; the tests compare bytes.
//
// Kernel layout:
//   k_sh_shade   one thread per vertex, blocks of 256; acc / cnt stay in registers across ALL views (one launch, no view
//                limit, no atomics).  The camera of view n is read from a device array with a wave-uniform index, i.e. through
//                the scalar cache.  Vertices come in ascending 7 L + slot, so the 64 vertices of a wave are neighbours on the
//                surface and their pixels lie on one short image segment per view.
#include <cmath>

#include "sfmx_internal.h"

namespace {

struct ShView {
  double R[9], c[3], f, cx, cy, fB;
  long long off;  // first pixel of the view in the disparity slab and in the image slab
  int w, h;
};

__global__ __launch_bounds__(256) void k_sh_shade(const double* __restrict__ verts, const double* __restrict__ normals, int n,
                                                  const ShView* __restrict__ views, int nv, const int16_t* __restrict__ disp,
                                                  const uint8_t* __restrict__ img, double depth_tol, double disp_min, int cull, int fill,
                                                  uint8_t* __restrict__ grey, int* __restrict__ seen) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double X0 = verts[3 * (size_t)i], X1 = verts[3 * (size_t)i + 1], X2 = verts[3 * (size_t)i + 2];
  double n0 = 0.0, n1 = 0.0, n2 = 0.0;
  if (cull) {
    n0 = normals[3 * (size_t)i];
    n1 = normals[3 * (size_t)i + 1];
    n2 = normals[3 * (size_t)i + 2];
  }
  int acc = 0, cnt = 0;
  for (int k = 0; k < nv; k++) {
    const ShView& V = views[k];
    const double p0 = X0 - V.c[0], p1 = X1 - V.c[1], p2 = X2 - V.c[2];
    const double q2 = (V.R[6] * p0 + V.R[7] * p1) + V.R[8] * p2;
    if (!(q2 > 0.0)) continue;
    if (cull && !(((n0 * p0 + n1 * p1) + n2 * p2) < 0.0)) continue;
    const double q0 = (V.R[0] * p0 + V.R[1] * p1) + V.R[2] * p2;
    const double q1 = (V.R[3] * p0 + V.R[4] * p1) + V.R[5] * p2;
    const double u = (V.f * q0) / q2 + V.cx;
    const double v = (V.f * q1) / q2 + V.cy;
    const double x = floor(u + 0.5), y = floor(v + 0.5);
    if (!(x >= 0.0 && x < (double)V.w && y >= 0.0 && y < (double)V.h)) continue;
    const long long px = V.off + (long long)(int)y * V.w + (int)x;
    const int d = disp[px];
    const double dd = (double)d / 16.0;
    if (d == -16 || !(dd >= disp_min)) continue;
    const double Z = V.fB / dd;
    if (!(fabs(Z - q2) <= depth_tol)) continue;
    acc += (int)img[px];
    cnt += 1;
  }
  grey[i] = (uint8_t)(cnt ? (2 * acc + cnt) / (2 * cnt) : fill);
  seen[i] = cnt;
}

}  // namespace

struct sfmx_shade {
  std::vector<ShView> views;
  long long used = 0;  // pixels held in each slab
  DevBuf disp, img;    // int16 / u8 of every view, back to back (view k at views[k].off in both)
  DevBuf d_views;
  bool views_dirty = true;
  DevBuf in_v, in_n, out_g, out_c;  // staging of sfmx_shade_vertices and the results
  hipEvent_t ev[2] = {};
  double last_us = 0.0;
};

namespace {

bool sh_view_ok(const sfmx_fusion_view* v) {
  if (!v || v->w <= 0 || v->h <= 0 || v->w > 4096 || (long long)v->w * v->h >= (1ll << 30)) return false;
  for (double x : v->R_rw)
    if (!std::isfinite(x)) return false;
  for (double x : v->c_left)
    if (!std::isfinite(x)) return false;
  return std::isfinite(v->f) && std::isfinite(v->cx) && std::isfinite(v->cy) && std::isfinite(v->B);
}

// room for `bytes` in a slab that already holds `used` bytes: a grown slab gets the old contents (DevBuf parks the old block, so
// it is still there to copy from)
int sh_grow(sfmx_ctx* ctx, DevBuf& b, size_t used, size_t bytes) {
  if (bytes <= b.cap) return SFMX_OK;
  const void* old = b.p;
  SFMX_HIP(ctx, b.ensure(bytes + bytes / 2));
  if (old && used) SFMX_HIP(ctx, hipMemcpyAsync(b.p, old, used, hipMemcpyDeviceToDevice, ctx->stream));
  return SFMX_OK;
}

int sh_add(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion_view* v, const int16_t* disp16, const uint8_t* image, hipMemcpyKind kind) {
  const long long px = (long long)v->w * v->h;
  SFMX_REQUIRE(ctx, sh->used + px < (1ll << 40));
  int rc = sh_grow(ctx, sh->disp, (size_t)sh->used * 2, (size_t)(sh->used + px) * 2);
  if (rc == SFMX_OK) rc = sh_grow(ctx, sh->img, (size_t)sh->used, (size_t)(sh->used + px));
  if (rc != SFMX_OK) return rc;
  SFMX_HIP(ctx, hipMemcpyAsync(sh->disp.as<int16_t>() + sh->used, disp16, (size_t)px * 2, kind, ctx->stream));
  SFMX_HIP(ctx, hipMemcpyAsync(sh->img.as<uint8_t>() + sh->used, image, (size_t)px, kind, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may reuse its buffers (a stereo object its maps)
  ShView sv{};
  std::memcpy(sv.R, v->R_rw, sizeof sv.R);
  std::memcpy(sv.c, v->c_left, sizeof sv.c);
  sv.f = v->f;
  sv.cx = v->cx;
  sv.cy = v->cy;
  sv.fB = v->f * v->B;
  sv.off = sh->used;
  sv.w = v->w;
  sv.h = v->h;
  sh->views.push_back(sv);
  sh->used += px;
  sh->views_dirty = true;
  return SFMX_OK;
}

// shade n vertices that are on the device; results to the host
int sh_run(sfmx_ctx* ctx, sfmx_shade* sh, const double* d_verts, const double* d_normals, int n, const sfmx_shade_params* p,
           uint8_t* grey_out, int32_t* views_out) {
  sh->last_us = 0.0;
  if (n == 0) return SFMX_OK;
  hipStream_t s = ctx->stream;
  const int nv = (int)sh->views.size();
  if (sh->views_dirty && nv > 0) {
    SFMX_HIP(ctx, hipStreamSynchronize(s));  // an earlier launch may still read the array
    SFMX_HIP(ctx, sh->d_views.ensure(sizeof(ShView) * (size_t)nv));
    SFMX_HIP(ctx, hipMemcpyAsync(sh->d_views.p, sh->views.data(), sizeof(ShView) * (size_t)nv, hipMemcpyHostToDevice, s));
    SFMX_HIP(ctx, hipStreamSynchronize(s));
    sh->views_dirty = false;
  }
  SFMX_HIP(ctx, sh->out_g.ensure((size_t)n));
  SFMX_HIP(ctx, sh->out_c.ensure((size_t)n * 4));
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(sh->ev[0], s));
  k_sh_shade<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_verts, d_normals, n, sh->d_views.as<ShView>(), nv, sh->disp.as<int16_t>(),
                                                          sh->img.as<uint8_t>(), p->depth_tol, p->disp_min, p->cull, p->fill,
                                                          sh->out_g.as<uint8_t>(), sh->out_c.as<int>());
  SFMX_HIP(ctx, hipGetLastError());
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(sh->ev[1], s));
  if (grey_out) SFMX_HIP(ctx, hipMemcpyAsync(grey_out, sh->out_g.p, (size_t)n, hipMemcpyDeviceToHost, s));
  if (views_out) SFMX_HIP(ctx, hipMemcpyAsync(views_out, sh->out_c.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  if (ctx->timing) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, sh->ev[0], sh->ev[1]) == hipSuccess) sh->last_us = (double)ms * 1000.0;
  }
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_shade_default_params(sfmx_shade_params* p) {
  if (!p) return;
  *p = sfmx_shade_params{};
  p->depth_tol = 0.0;
  p->disp_min = 1.0;
  p->cull = 1;
  p->fill = 0;
}

int sfmx_shade_check_params(const sfmx_shade_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!(p->depth_tol > 0.0) || std::isnan(p->disp_min)) return SFMX_ERR_INVALID;
  if ((p->cull != 0 && p->cull != 1) || p->fill < 0 || p->fill > 255) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_shade_create(sfmx_ctx* ctx, sfmx_shade** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* sh = new sfmx_shade;
  hipError_t e = hipEventCreate(&sh->ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&sh->ev[1]);
  if (e != hipSuccess) {
    sfmx_shade_destroy(ctx, sh);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_shade_create", e);
  }
  *out = sh;
  return SFMX_OK;
}

void sfmx_shade_destroy(sfmx_ctx* ctx, sfmx_shade* sh) {
  if (!sh) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* b : {&sh->disp, &sh->img, &sh->d_views, &sh->in_v, &sh->in_n, &sh->out_g, &sh->out_c}) b->release();
  for (hipEvent_t ev : sh->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete sh;
}

int sfmx_shade_reset(sfmx_ctx* ctx, sfmx_shade* sh) {
  SFMX_REQUIRE(ctx, ctx && sh);
  sh->views.clear();
  sh->used = 0;
  sh->views_dirty = true;
  sh->last_us = 0.0;
  return SFMX_OK;
}

int sfmx_shade_add_view(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion_view* view, const int16_t* disp16, const uint8_t* image,
                        int on_device) {
  SFMX_REQUIRE(ctx, ctx && sh && disp16 && image && sh_view_ok(view));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sh_add(ctx, sh, view, disp16, image, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
}

int sfmx_shade_add_stereo_view(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion_view* view, const sfmx_stereo* st) {
  SFMX_REQUIRE(ctx, ctx && sh && st && sh_view_ok(view));
  int w = 0, h = 0, wi = 0, hi = 0;
  const int16_t* d16 = sfmx_stereo_device_disp16(st, &w, &h);
  const uint8_t* im = sfmx_stereo_device_rect_left(st, &wi, &hi);
  SFMX_REQUIRE(ctx, view->w == w && view->h == h && wi == w && hi == h);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sh_add(ctx, sh, view, d16, im, hipMemcpyDeviceToDevice);
}

int sfmx_shade_view_count(const sfmx_shade* sh) { return sh ? (int)sh->views.size() : 0; }

int sfmx_shade_vertices(sfmx_ctx* ctx, sfmx_shade* sh, const double* verts, const double* normals, int n, int on_device,
                        const sfmx_shade_params* p, uint8_t* grey_out, int32_t* views_out) {
  SFMX_REQUIRE(ctx, ctx && sh && n >= 0 && sfmx_shade_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, n == 0 || (verts && (normals || !p->cull)));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0 || on_device) return sh_run(ctx, sh, verts, normals, n, p, grey_out, views_out);
  const size_t bytes = (size_t)n * 24;
  SFMX_HIP(ctx, sh->in_v.ensure(bytes));
  SFMX_HIP(ctx, hipMemcpyAsync(sh->in_v.p, verts, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (normals) {
    SFMX_HIP(ctx, sh->in_n.ensure(bytes));
    SFMX_HIP(ctx, hipMemcpyAsync(sh->in_n.p, normals, bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  return sh_run(ctx, sh, sh->in_v.as<double>(), normals ? sh->in_n.as<double>() : nullptr, n, p, grey_out, views_out);
}

int sfmx_shade_fusion(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion* fu, const sfmx_shade_params* p, uint8_t* grey_out,
                      int32_t* views_out) {
  SFMX_REQUIRE(ctx, ctx && sh && fu && sfmx_shade_check_params(p) == SFMX_OK);
  const double *v = nullptr, *nr = nullptr;
  const int n = sfmx_fusion_device_surface(fu, &v, &nr);
  SFMX_REQUIRE(ctx, n >= 0);  // no sfmx_fusion_extract_normals result on the device
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sh_run(ctx, sh, v, nr, n, p, grey_out, views_out);
}

double sfmx_shade_last_us(const sfmx_shade* sh) { return sh ? sh->last_us : 0.0; }

}  // extern "C"
