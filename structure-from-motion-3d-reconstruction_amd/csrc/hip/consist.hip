// consist.hip — multi-view consistency filtering of disparity maps before fusion.
//
// A sfmx_consist keeps, for every view added, the rectified left camera and its disparity map (int16) on the device.  The
// filter lifts every valid pixel of every view to its 3-D point, projects it into every OTHER view with the integration's own
// expressions (sfmx_view.h), and counts the views whose depth at that pixel agrees and whose own 3-D point
// projects back onto the pixel.  A pixel with fewer than min_support such views becomes -16 in a second slab; the inputs are
// never written, so the result does not depend on the schedule.
//
// Exactness: IEEE double in one fixed expression order up to each comparison (built with -ffp-contract=off), an integer count
// after it, so no launch shape can change a byte.  tests/consist_ref.py restates it in NumPy; the tests compare bytes.
//
// Kernel layout:
//   k_cs_filter  one thread per reference pixel, blocks of 64 (x) x 4 (y): a wave is 64 consecutive pixels of one row, so its
//                projections into another view lie on one short image curve.  Every reference view goes in ONE launch: a
//                block finds its view in a table of first blocks (a search on blockIdx, so the index is wave-uniform and both
//                cameras arrive through the scalar cache).  The 3-D point and the support stay in registers across all the
//                other views; a wave without a valid pixel leaves before the loop; the per-view counters take one ballot,
//                one popcount and one atomicAdd per wave.  No LDS, no inter-workgroup waiting, no scratch.
#include <cmath>

#include "sfmx_internal.h"
#include "sfmx_view.h"

namespace {

struct CsView : DevView {  // off: first pixel of the view in the three slabs
  int first;  // the view's first block in the launch
  int bx;     // blocks per tile row: ceil(w / 64)
};

__global__ __launch_bounds__(256) void k_cs_filter(const CsView* __restrict__ views, int nv, const int16_t* __restrict__ disp,
                                                   int16_t* __restrict__ out, uint8_t* __restrict__ sup, int* __restrict__ counts,
                                                   double rel_tol, double reproj2, double disp_min, int min_support) {
  // the last view whose first block is not after this one
  const int b = (int)blockIdx.x;
  int lo = 0, hi = nv - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (views[mid].first <= b) lo = mid;
    else hi = mid - 1;
  }
  const int i = __builtin_amdgcn_readfirstlane(lo);
  const CsView& V = views[i];
  const int lb = b - V.first;
  const int x = (lb % V.bx) * 64 + (int)threadIdx.x, y = (lb / V.bx) * 4 + (int)threadIdx.y;
  const bool in = x < V.w && y < V.h;
  const long long px = V.off + (long long)y * V.w + x;
  const int d = in ? (int)disp[px] : -16;
  const bool valid = dv_disp_ok(d, disp_min);  // never a pixel outside the image: its d is the invalid mark
  const unsigned long long vmask = __ballot(valid);
  if (vmask == 0ull) {  // the whole wave (one row of 64 pixels)
    if (in) {
      out[px] = -16;
      sup[px] = 0;
    }
    return;
  }
  int support = 0;
  if (valid) {
    const double xd = (double)x, yd = (double)y;
    double X0, X1, X2;
    dv_lift(V, xd, yd, dv_disp_depth(V, d), X0, X1, X2);
    for (int j = 0; j < nv; j++) {
      if (j == i) continue;
      const DevView& W = views[j];
      double p0, p1, p2, xr, yr;
      const double q2 = dv_depth(W, X0, X1, X2, p0, p1, p2);
      if (!(q2 > 0.0)) continue;
      if (!dv_pixel(W, p0, p1, p2, q2, xr, yr)) continue;
      const int d2 = disp[dv_index(W, xr, yr)];
      if (!dv_disp_ok(d2, disp_min)) continue;
      const double Z2 = dv_disp_depth(W, d2);
      if (!(fabs(Z2 - q2) <= rel_tol * q2)) continue;
      // the other view's own point, and where this view sees it
      double Y0, Y1, Y2, s0, s1, s2, ub, vb;
      dv_lift(W, xr, yr, Z2, Y0, Y1, Y2);
      const double t2 = dv_depth(V, Y0, Y1, Y2, s0, s1, s2);
      if (!(t2 > 0.0)) continue;
      dv_project(V, s0, s1, s2, t2, ub, vb);
      const double e0 = ub - xd, e1 = vb - yd;
      if (!((e0 * e0 + e1 * e1) <= reproj2)) continue;
      support += 1;
    }
  }
  const bool kept = valid && support >= min_support;
  if (in) {
    out[px] = (int16_t)(kept ? d : -16);
    sup[px] = (uint8_t)(support < 255 ? support : 255);
  }
  const unsigned long long kmask = __ballot(kept);
  if (threadIdx.x == 0) {
    atomicAdd(&counts[i], __popcll(vmask));
    if (kmask) atomicAdd(&counts[nv + i], __popcll(kmask));
  }
}

}  // namespace

struct sfmx_consist {
  std::vector<CsView> views;
  std::vector<sfmx_fusion_view> src;  // the views as they were added (sfmx_fusion_add_consist_view hands them on unchanged)
  long long used = 0;                 // pixels held in each slab
  DevBuf disp;                        // int16 of every view, back to back (view k at views[k].off)
  DevBuf out, sup;                    // the last filter: int16 / u8, same layout
  DevBuf d_views, d_counts;
  std::vector<int32_t> counts;        // valid [n], kept [n] of the last filter
  bool filtered = false;
  StageTimer t;
};

namespace {

int cs_add(sfmx_ctx* ctx, sfmx_consist* cs, const sfmx_fusion_view* v, const int16_t* disp16, hipMemcpyKind kind) {
  const long long px = (long long)v->w * v->h;
  SFMX_REQUIRE(ctx, cs->used + px < (1ll << 40));
  SFMX_HIP(ctx, sfmx_grow_keep(cs->disp, (size_t)cs->used * 2, (size_t)(cs->used + px) * 2, ctx->stream));
  SFMX_HIP(ctx, hipMemcpyAsync(cs->disp.as<int16_t>() + cs->used, disp16, (size_t)px * 2, kind, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may reuse its buffer (a stereo object its map)
  cs->views.push_back(CsView{sfmx_dev_view(v, cs->used), 0, (v->w + 63) / 64});
  cs->src.push_back(*v);
  cs->used += px;
  cs->filtered = false;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_consist_default_params(sfmx_consist_params* p) {
  if (!p) return;
  *p = sfmx_consist_params{};
  p->rel_tol = 0.01;
  p->reproj_px = 1.0;
  p->disp_min = 1.0;
  p->min_support = 2;
}

int sfmx_consist_check_params(const sfmx_consist_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!(p->rel_tol > 0.0) || !std::isfinite(p->rel_tol)) return SFMX_ERR_INVALID;
  if (!(p->reproj_px >= 0.0) || !std::isfinite(p->reproj_px)) return SFMX_ERR_INVALID;
  if (std::isnan(p->disp_min) || p->min_support < 0) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_consist_create(sfmx_ctx* ctx, sfmx_consist** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* cs = new sfmx_consist;
  const hipError_t e = cs->t.create();
  if (e != hipSuccess) {
    sfmx_consist_destroy(ctx, cs);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_consist_create", e);
  }
  *out = cs;
  return SFMX_OK;
}

void sfmx_consist_destroy(sfmx_ctx* ctx, sfmx_consist* cs) {
  if (!cs) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* b : {&cs->disp, &cs->out, &cs->sup, &cs->d_views, &cs->d_counts}) b->release();
  cs->t.destroy();
  delete cs;
}

int sfmx_consist_reset(sfmx_ctx* ctx, sfmx_consist* cs) {
  SFMX_REQUIRE(ctx, ctx && cs);
  cs->views.clear();
  cs->src.clear();
  cs->counts.clear();
  cs->used = 0;
  cs->filtered = false;
  cs->t.us = 0.0;
  return SFMX_OK;
}

int sfmx_consist_add_view(sfmx_ctx* ctx, sfmx_consist* cs, const sfmx_fusion_view* view, const int16_t* disp16, int on_device) {
  SFMX_REQUIRE(ctx, ctx && cs && disp16 && sfmx_view_ok(view));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return cs_add(ctx, cs, view, disp16, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
}

int sfmx_consist_add_stereo_view(sfmx_ctx* ctx, sfmx_consist* cs, const sfmx_fusion_view* view, const sfmx_stereo* st) {
  SFMX_REQUIRE(ctx, ctx && cs && st && sfmx_view_ok(view));
  int w = 0, h = 0;
  const int16_t* d16 = sfmx_stereo_device_disp16(st, &w, &h);
  SFMX_REQUIRE(ctx, view->w == w && view->h == h);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return cs_add(ctx, cs, view, d16, hipMemcpyDeviceToDevice);
}

int sfmx_consist_view_count(const sfmx_consist* cs) { return cs ? (int)cs->views.size() : 0; }

int sfmx_consist_filter(sfmx_ctx* ctx, sfmx_consist* cs, const sfmx_consist_params* p) {
  SFMX_REQUIRE(ctx, ctx && cs && sfmx_consist_check_params(p) == SFMX_OK);
  cs->t.us = 0.0;
  cs->filtered = false;
  const int nv = (int)cs->views.size();
  cs->counts.assign(2 * (size_t)nv, 0);
  if (nv == 0) {
    cs->filtered = true;
    return SFMX_OK;
  }
  long long blocks = 0;
  for (CsView& v : cs->views) {
    SFMX_REQUIRE(ctx, blocks < (1ll << 31));  // first fits an int
    v.first = (int)blocks;
    blocks += (long long)v.bx * ((v.h + 3) / 4);
  }
  SFMX_REQUIRE(ctx, blocks < (1ll << 31));  // one launch, one grid dimension
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  SFMX_HIP(ctx, hipStreamSynchronize(s));  // an earlier launch may still read the view array
  SFMX_HIP(ctx, cs->d_views.ensure(sizeof(CsView) * (size_t)nv));
  SFMX_HIP(ctx, cs->d_counts.ensure(2 * (size_t)nv * 4));
  SFMX_HIP(ctx, cs->out.ensure((size_t)cs->used * 2));
  SFMX_HIP(ctx, cs->sup.ensure((size_t)cs->used));
  SFMX_HIP(ctx, hipMemcpyAsync(cs->d_views.p, cs->views.data(), sizeof(CsView) * (size_t)nv, hipMemcpyHostToDevice, s));
  SFMX_HIP(ctx, hipMemsetAsync(cs->d_counts.p, 0, 2 * (size_t)nv * 4, s));
  SFMX_HIP(ctx, cs->t.begin(ctx));
  k_cs_filter<<<(unsigned)blocks, dim3(64, 4), 0, s>>>(cs->d_views.as<CsView>(), nv, cs->disp.as<int16_t>(), cs->out.as<int16_t>(),
                                                        cs->sup.as<uint8_t>(), cs->d_counts.as<int>(), p->rel_tol,
                                                        p->reproj_px * p->reproj_px, p->disp_min, p->min_support);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, cs->t.end(ctx));
  SFMX_HIP(ctx, hipMemcpyAsync(cs->counts.data(), cs->d_counts.p, 2 * (size_t)nv * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  cs->t.collect(ctx);
  cs->filtered = true;
  return SFMX_OK;
}

int sfmx_consist_read(sfmx_ctx* ctx, sfmx_consist* cs, int i, int16_t* disp16_out, uint8_t* support_out) {
  SFMX_REQUIRE(ctx, ctx && cs && cs->filtered && i >= 0 && i < (int)cs->views.size());
  const DevView& v = cs->views[(size_t)i];
  const size_t px = (size_t)v.w * v.h;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (disp16_out) SFMX_HIP(ctx, hipMemcpyAsync(disp16_out, cs->out.as<int16_t>() + v.off, px * 2, hipMemcpyDeviceToHost, ctx->stream));
  if (support_out) SFMX_HIP(ctx, hipMemcpyAsync(support_out, cs->sup.as<uint8_t>() + v.off, px, hipMemcpyDeviceToHost, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SFMX_OK;
}

int sfmx_consist_counts(sfmx_ctx* ctx, sfmx_consist* cs, int32_t* valid_out, int32_t* kept_out) {
  SFMX_REQUIRE(ctx, ctx && cs && cs->filtered);
  const size_t n = cs->views.size();
  if (valid_out && n) std::memcpy(valid_out, cs->counts.data(), n * 4);
  if (kept_out && n) std::memcpy(kept_out, cs->counts.data() + n, n * 4);
  return SFMX_OK;
}

double sfmx_consist_last_us(const sfmx_consist* cs) { return cs ? cs->t.us : 0.0; }

}  // extern "C"

bool sfmx_consist_device_view(const sfmx_consist* cs, int i, sfmx_fusion_view* view, const int16_t** filtered) {
  if (!cs || !cs->filtered || i < 0 || i >= (int)cs->views.size()) return false;
  *view = cs->src[(size_t)i];
  *filtered = cs->out.as<int16_t>() + cs->views[(size_t)i].off;
  return true;
}
