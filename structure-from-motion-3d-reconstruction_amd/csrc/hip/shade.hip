// shade.hip — vertex intensity of a surface from the views that see it.
//
// A sfmx_shade keeps, for every view added, the rectified left camera, its disparity map (int16) and its left rectified image
// (u8) on the device.  Shading projects every vertex into every view with the integration's own expressions (sfmx_view.h,
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
#include "sfmx_view.h"

namespace {

__global__ __launch_bounds__(256) void k_sh_shade(const double* __restrict__ verts, const double* __restrict__ normals, int n,
                                                  const DevView* __restrict__ views, int nv, const int16_t* __restrict__ disp,
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
    const DevView& V = views[k];  // its off holds for the disparity slab and for the image slab
    double p0, p1, p2, x, y;
    const double q2 = dv_depth(V, X0, X1, X2, p0, p1, p2);
    if (!(q2 > 0.0)) continue;
    if (cull && !(((n0 * p0 + n1 * p1) + n2 * p2) < 0.0)) continue;
    if (!dv_pixel(V, p0, p1, p2, q2, x, y)) continue;
    const long long px = dv_index(V, x, y);
    const int d = disp[px];
    if (!dv_disp_ok(d, disp_min)) continue;
    const double Z = dv_disp_depth(V, d);
    if (!(fabs(Z - q2) <= depth_tol)) continue;
    acc += (int)img[px];
    cnt += 1;
  }
  grey[i] = (uint8_t)(cnt ? (2 * acc + cnt) / (2 * cnt) : fill);
  seen[i] = cnt;
}

}  // namespace

struct sfmx_shade {
  std::vector<DevView> views;
  long long used = 0;  // pixels held in each slab
  DevBuf disp, img;    // int16 / u8 of every view, back to back (view k at views[k].off in both)
  DevBuf d_views;
  bool views_dirty = true;
  DevBuf in_v, in_n, out_g, out_c;  // staging of sfmx_shade_vertices and the results
  StageTimer t;
};

namespace {

int sh_add(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion_view* v, const int16_t* disp16, const uint8_t* image, hipMemcpyKind kind) {
  const long long px = (long long)v->w * v->h;
  SFMX_REQUIRE(ctx, sh->used + px < (1ll << 40));
  SFMX_HIP(ctx, sfmx_grow_keep(sh->disp, (size_t)sh->used * 2, (size_t)(sh->used + px) * 2, ctx->stream));
  SFMX_HIP(ctx, sfmx_grow_keep(sh->img, (size_t)sh->used, (size_t)(sh->used + px), ctx->stream));
  SFMX_HIP(ctx, hipMemcpyAsync(sh->disp.as<int16_t>() + sh->used, disp16, (size_t)px * 2, kind, ctx->stream));
  SFMX_HIP(ctx, hipMemcpyAsync(sh->img.as<uint8_t>() + sh->used, image, (size_t)px, kind, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may reuse its buffers (a stereo object its maps)
  sh->views.push_back(sfmx_dev_view(v, sh->used));
  sh->used += px;
  sh->views_dirty = true;
  return SFMX_OK;
}

// shade n vertices that are on the device; results to the host
int sh_run(sfmx_ctx* ctx, sfmx_shade* sh, const double* d_verts, const double* d_normals, int n, const sfmx_shade_params* p,
           uint8_t* grey_out, int32_t* views_out) {
  sh->t.us = 0.0;
  if (n == 0) return SFMX_OK;
  hipStream_t s = ctx->stream;
  const int nv = (int)sh->views.size();
  if (sh->views_dirty && nv > 0) {
    SFMX_HIP(ctx, hipStreamSynchronize(s));  // an earlier launch may still read the array
    SFMX_HIP(ctx, sh->d_views.ensure(sizeof(DevView) * (size_t)nv));
    SFMX_HIP(ctx, hipMemcpyAsync(sh->d_views.p, sh->views.data(), sizeof(DevView) * (size_t)nv, hipMemcpyHostToDevice, s));
    SFMX_HIP(ctx, hipStreamSynchronize(s));
    sh->views_dirty = false;
  }
  SFMX_HIP(ctx, sh->out_g.ensure((size_t)n));
  SFMX_HIP(ctx, sh->out_c.ensure((size_t)n * 4));
  SFMX_HIP(ctx, sh->t.begin(ctx));
  k_sh_shade<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_verts, d_normals, n, sh->d_views.as<DevView>(), nv, sh->disp.as<int16_t>(),
                                                          sh->img.as<uint8_t>(), p->depth_tol, p->disp_min, p->cull, p->fill,
                                                          sh->out_g.as<uint8_t>(), sh->out_c.as<int>());
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, sh->t.end(ctx));
  if (grey_out) SFMX_HIP(ctx, hipMemcpyAsync(grey_out, sh->out_g.p, (size_t)n, hipMemcpyDeviceToHost, s));
  if (views_out) SFMX_HIP(ctx, hipMemcpyAsync(views_out, sh->out_c.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  sh->t.collect(ctx);
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
  const hipError_t e = sh->t.create();
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
  sh->t.destroy();
  delete sh;
}

int sfmx_shade_reset(sfmx_ctx* ctx, sfmx_shade* sh) {
  SFMX_REQUIRE(ctx, ctx && sh);
  sh->views.clear();
  sh->used = 0;
  sh->views_dirty = true;
  sh->t.us = 0.0;
  return SFMX_OK;
}

int sfmx_shade_add_view(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion_view* view, const int16_t* disp16, const uint8_t* image,
                        int on_device) {
  SFMX_REQUIRE(ctx, ctx && sh && disp16 && image && sfmx_view_ok(view));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sh_add(ctx, sh, view, disp16, image, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
}

int sfmx_shade_add_stereo_view(sfmx_ctx* ctx, sfmx_shade* sh, const sfmx_fusion_view* view, const sfmx_stereo* st) {
  SFMX_REQUIRE(ctx, ctx && sh && st && sfmx_view_ok(view));
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

double sfmx_shade_last_us(const sfmx_shade* sh) { return sh ? sh->t.us : 0.0; }

}  // extern "C"
