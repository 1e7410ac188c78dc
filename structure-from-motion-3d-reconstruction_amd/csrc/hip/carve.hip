// carve.hip — shape from silhouette: the exact visual hull of a set of views on the fusion grid, and carving a fusion volume
// with it.
//
// A sfmx_carve keeps, for every view added, the rectified left camera and the signed squared distance map of its silhouette
// (int16, the exact Euclidean distance transform truncated at cap, negative inside) on the device; the picture itself is not
// kept.  sfmx_carve_run projects every grid point into every view with the integration's own expressions (sfmx_view.h,
// DESIGN.md 13), turns the map's entry into a signed distance in units of the truncation and keeps the largest over the views:
// a point that some camera sees outside its silhouette is outside the hull.  sfmx_carve_store writes the hull into a fusion
// object, sfmx_carve_apply carves the object's volume with it.
//
// Exactness: the distance maps are integers (a minimum over integer candidates: no schedule can change it); the hull is IEEE
// double in one fixed expression order per view (built with -ffp-contract=off), the square roots come from a table the host
// fills, and the views are combined by max, which is associative and commutative on these values (never NaN), so neither the
// batching nor the order of the views changes a byte.  tests/carve_ref.py restates it in NumPy; the tests compare bytes.
//
// Kernel layout:
//   k_cv_cols    one thread per pixel, blocks of 64 (x) x 4 (y): thresholds the picture and scans the pixel's column outwards,
//                up to cap rows either way, for the nearest pixel of the other class.  One byte per pixel: the class in bit 7,
//                the vertical distance (1 .. cap, 127 = none in the window) below it.  It also counts the inside pixels (one
//                ballot and one integer atomicAdd per wave).
//   k_cv_rows    one block per CV_TILE pixels of one row: the segment's bytes and a halo of cap on either side go to LDS
//                (0xFE = outside the image: neither class), each thread walks outwards from its pixel, dx = 0, 1, 2, ..., and
//                stops as soon as dx * dx cannot beat the best dx * dx + g * g it holds.  Writes -D2 / +D2 as int16.
//   k_cv_hull    one thread per grid point in k_fu_integrate's 64 x 4 tiling; the sqrt table sits in LDS ((cap^2 + 1) doubles,
//                33 KB at cap 64); H and n stay in registers across the batch's views, read and written once per launch.
//   k_cv_store / k_cv_apply / k_cv_count   one thread per grid point; apply's three counters (count's two, from the hull alone)
//                are summed per block, one integer atomicAdd per counter and block.
// No kernel waits on another workgroup, none uses float atomics or scratch.
#include <cmath>

#include "sfmx_internal.h"
#include "sfmx_tsdf.h"
#include "sfmx_view.h"

namespace {

constexpr int CV_TILE = 256;         // pixels of a row per block of k_cv_rows
constexpr int CV_CAP_MAX = 64;       // so that cap^2 fits an int16 and a column distance 7 bits
constexpr int CV_NONE = 127;         // no pixel of the other class within cap rows
constexpr int CV_OFF_IMAGE = 0xFE;   // a halo byte outside the image: neither class
constexpr int CV_AUTO_BATCH = 64;

struct CvView : DevView {  // off: first element of the view's map in the sd2 slab
  double ft;               // f * trunc of the run
};

__global__ __launch_bounds__(256) void k_cv_cols(const uint8_t* __restrict__ img, int w, int h, int threshold, int cap,
                                                 uint8_t* __restrict__ col, int* __restrict__ inside, int bx) {
  // one grid dimension (a picture may be 2^30 / w rows tall: more blocks than the second dimension holds)
  const int x = ((int)blockIdx.x % bx) * 64 + (int)threadIdx.x, y = ((int)blockIdx.x / bx) * 4 + (int)threadIdx.y;
  const bool in = x < w && y < h;
  const size_t p = in ? (size_t)y * w + x : 0;
  const bool m = in && img[p] >= threshold;
  const unsigned long long mm = __ballot(m);  // a wave is one row of 64 pixels: one integer atomicAdd for it
  if (threadIdx.x == 0 && mm) atomicAdd(inside, __popcll(mm));
  if (!in) return;
  int g = CV_NONE;
  for (int d = 1; d <= cap; d++) {
    const bool up = y - d >= 0 && (img[p - (size_t)d * w] >= threshold) != m;
    const bool dn = y + d < h && (img[p + (size_t)d * w] >= threshold) != m;
    if (up || dn) {
      g = d;
      break;
    }
  }
  col[p] = (uint8_t)((m ? 0x80 : 0) | g);
}

__global__ __launch_bounds__(CV_TILE) void k_cv_rows(const uint8_t* __restrict__ col, int w, int cap, int tiles,
                                                     int16_t* __restrict__ sd2) {
  __shared__ uint8_t seg[CV_TILE + 2 * CV_CAP_MAX];
  const int y = (int)blockIdx.x / tiles, x0 = ((int)blockIdx.x % tiles) * CV_TILE;
  const uint8_t* row = col + (size_t)y * w;
  for (int q = (int)threadIdx.x; q < CV_TILE + 2 * cap; q += CV_TILE) {
    const int xs = x0 - cap + q;
    seg[q] = xs >= 0 && xs < w ? row[xs] : (uint8_t)CV_OFF_IMAGE;
  }
  __syncthreads();
  const int x = x0 + (int)threadIdx.x;
  if (x >= w) return;
  const int c = (int)threadIdx.x + cap;
  const int own = seg[c], m = own >> 7, g0 = own & 127;
  int best = cap * cap;
  if (g0 != CV_NONE && g0 * g0 < best) best = g0 * g0;
  for (int dx = 1; dx <= cap; dx++) {
    const int dx2 = dx * dx;
    if (dx2 >= best) break;
#pragma unroll
    for (int side = 0; side < 2; side++) {
      const int b = seg[side ? c + dx : c - dx];
      if (b == CV_OFF_IMAGE) continue;
      int cand;
      if ((b >> 7) != m) cand = dx2;
      else {
        const int g = b & 127;
        if (g == CV_NONE) continue;
        cand = dx2 + g * g;
      }
      if (cand < best) best = cand;
    }
  }
  sd2[(size_t)y * w + x] = (int16_t)(m ? -best : best);
}

__global__ __launch_bounds__(256) void k_cv_hull(double* __restrict__ hull, int* __restrict__ nviews, FuGrid g,
                                                 const CvView* __restrict__ views, int nv, const int16_t* __restrict__ sd2,
                                                 const double* __restrict__ tab, int cap2, int first, int bx, int by) {
  extern __shared__ double tab_s[];
  for (int q = (int)threadIdx.y * 64 + (int)threadIdx.x; q <= cap2; q += 256) tab_s[q] = tab[q];
  __syncthreads();
  int b = blockIdx.x;
  const int bi = b % bx;
  b /= bx;
  const int bj = b % by, k = b / by;
  const int i = bi * 64 + (int)threadIdx.x, j = bj * 4 + (int)threadIdx.y;
  if (i >= g.nx || j >= g.ny) return;
  const size_t L = (size_t)i + (size_t)g.nx * ((size_t)j + (size_t)g.ny * k);
  const double X0 = g.ox + (double)i * g.vs, X1 = g.oy + (double)j * g.vs, X2 = g.oz + (double)k * g.vs;
  double H = first ? -1.0 : hull[L];
  int n = first ? 0 : nviews[L];
  for (int v = 0; v < nv; v++) {
    const CvView& V = views[v];
    double p0, p1, p2, x, y;
    const double q2 = dv_depth(V, X0, X1, X2, p0, p1, p2);
    if (!(q2 > 0.0)) continue;
    if (!dv_pixel(V, p0, p1, p2, q2, x, y)) continue;
    const int kk = sd2[dv_index(V, x, y)];
    const double d = kk < 0 ? -tab_s[-kk] : tab_s[kk];
    double t = (d * q2) / V.ft;
    t = t >= 1.0 ? 1.0 : (t <= -1.0 ? -1.0 : t);
    if (t > H) H = t;
    n += 1;
  }
  hull[L] = H;
  nviews[L] = n;
}

__global__ __launch_bounds__(256) void k_cv_store(const double* __restrict__ hull, const int* __restrict__ nviews, int n, int min_views,
                                                  int W, double* __restrict__ sum, int* __restrict__ cnt) {
  const int L = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (L >= n) return;
  const bool defined = nviews[L] >= min_views;
  cnt[L] = defined ? W : 0;
  sum[L] = defined ? hull[L] * (double)W : 0.0;
}

// counters: defined, outside, changed
__global__ __launch_bounds__(256) void k_cv_apply(const double* __restrict__ hull, const int* __restrict__ nviews, int n, int min_views,
                                                  int W, int minw, double margin, int clear, double* __restrict__ sum,
                                                  int* __restrict__ cnt, int* __restrict__ counters) {
  const int L = (int)blockIdx.x * 256 + (int)threadIdx.x;
  int c[3] = {0, 0, 0};
  if (L < n && nviews[L] >= min_views) {
    c[0] = 1;
    const double h = hull[L];
    if (h > margin) {
      c[1] = 1;
      const double hm = h - margin;
      const int c0 = cnt[L];
      const double s0 = sum[L];
      int c1 = c0;
      double s1 = s0;
      if (clear) {
        c1 = 0;
        s1 = 0.0;
      } else {
        const bool def = c0 >= minw;
        const double s = def ? s0 / (double)c0 : 0.0;
        const double v = def ? (s > hm ? s : hm) : hm;
        if (!def || hm > s) {
          c1 = W;
          s1 = v * (double)W;
        }
      }
      if (c1 != c0 || __double_as_longlong(s1) != __double_as_longlong(s0)) {
        c[2] = 1;
        cnt[L] = c1;
        sum[L] = s1;
      }
    }
  }
  const int tot = sfmx_block_sums<int, 3>(c);
  if (threadIdx.x < 3 && tot) atomicAdd(&counters[threadIdx.x], tot);
}

// defined, outside: what k_cv_apply would count, from the hull alone
__global__ __launch_bounds__(256) void k_cv_count(const double* __restrict__ hull, const int* __restrict__ nviews, int n, int min_views,
                                                  double margin, int* __restrict__ counters) {
  const int L = (int)blockIdx.x * 256 + (int)threadIdx.x;
  int c[2] = {0, 0};
  if (L < n && nviews[L] >= min_views) {
    c[0] = 1;
    c[1] = hull[L] > margin ? 1 : 0;
  }
  const int tot = sfmx_block_sums<int, 2>(c);
  if (threadIdx.x < 2 && tot) atomicAdd(&counters[threadIdx.x], tot);
}

bool cv_volume_ok(const sfmx_carve_volume* v) {
  if (!v) return false;
  for (double x : v->origin)
    if (!std::isfinite(x)) return false;
  if (!(v->voxel > 0.0) || !std::isfinite(v->voxel)) return false;
  if (v->nx < 2 || v->ny < 2 || v->nz < 2) return false;
  return (long long)v->nx * v->ny * v->nz <= (1ll << 27);  // DESIGN.md 13's limit
}

}  // namespace

struct sfmx_carve {
  std::vector<CvView> views;
  std::vector<int> caps;  // the cap each view's map was built with
  std::vector<int32_t> inside;  // the pixels of each view's inside class
  long long used = 0;     // elements held in the sd2 slab
  DevBuf sd2;             // int16 maps of every view, back to back (view k at views[k].off)
  DevBuf img, col;        // one view's picture (host feed) and its column pass
  DevBuf d_views, tab, hull, nviews, d_counters;
  int tab_cap = 0;        // the cap the table on the device was filled for (0: none)
  int batch = 0;          // views per launch of k_cv_hull (0: automatic)
  // the last successful run
  bool done = false;
  sfmx_carve_volume vol{};
  int n = 0, min_views = 0;
  StageTimer t, te;
};

extern "C" {

void sfmx_carve_default_params(sfmx_carve_params* p) {
  if (!p) return;
  *p = sfmx_carve_params{};
  p->cap = 16;
  p->min_views = 1;
  p->margin = 0.5;
  p->mode = SFMX_CARVE_INTERSECT;
  p->trunc = 0.0;
}

int sfmx_carve_check_params(const sfmx_carve_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (p->cap < 1 || p->cap > CV_CAP_MAX || p->min_views < 1) return SFMX_ERR_INVALID;
  if (!std::isfinite(p->margin) || !(p->margin >= 0.0) || !(p->margin < 1.0)) return SFMX_ERR_INVALID;
  if (p->mode != SFMX_CARVE_INTERSECT && p->mode != SFMX_CARVE_CLEAR) return SFMX_ERR_INVALID;
  if (!std::isfinite(p->trunc) || !(p->trunc >= 0.0)) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_carve_create(sfmx_ctx* ctx, sfmx_carve** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* cv = new sfmx_carve;
  hipError_t e = cv->t.create();
  if (e == hipSuccess) e = cv->te.create();
  if (e != hipSuccess) {
    sfmx_carve_destroy(ctx, cv);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_carve_create", e);
  }
  *out = cv;
  return SFMX_OK;
}

void sfmx_carve_destroy(sfmx_ctx* ctx, sfmx_carve* cv) {
  if (!cv) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* b : {&cv->sd2, &cv->img, &cv->col, &cv->d_views, &cv->tab, &cv->hull, &cv->nviews, &cv->d_counters}) b->release();
  cv->t.destroy();
  cv->te.destroy();
  delete cv;
}

int sfmx_carve_reset(sfmx_ctx* ctx, sfmx_carve* cv) {
  SFMX_REQUIRE(ctx, ctx && cv);
  cv->views.clear();
  cv->caps.clear();
  cv->inside.clear();
  cv->used = 0;
  cv->done = false;
  cv->t.us = cv->te.us = 0.0;
  return SFMX_OK;
}

int sfmx_carve_add_view(sfmx_ctx* ctx, sfmx_carve* cv, const sfmx_fusion_view* view, const uint8_t* image, int on_device, int threshold,
                        int cap) {
  SFMX_REQUIRE(ctx, ctx && cv && image && sfmx_view_ok(view) && view->f > 0.0);
  SFMX_REQUIRE(ctx, threshold >= 1 && threshold <= 255 && cap >= 1 && cap <= CV_CAP_MAX);
  const int w = view->w, h = view->h;
  const long long px = (long long)w * h;
  SFMX_REQUIRE(ctx, cv->used + px < (1ll << 40));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  cv->te.us = 0.0;
  const uint8_t* src = image;
  if (!on_device) {
    SFMX_HIP(ctx, cv->img.ensure((size_t)px));
    SFMX_HIP(ctx, hipMemcpyAsync(cv->img.p, image, (size_t)px, hipMemcpyHostToDevice, s));
    src = cv->img.as<uint8_t>();
  }
  SFMX_HIP(ctx, cv->col.ensure((size_t)px));
  SFMX_HIP(ctx, cv->d_counters.ensure(4 * 4));
  int* d_inside = cv->d_counters.as<int>() + 3;
  SFMX_HIP(ctx, hipMemsetAsync(d_inside, 0, 4, s));
  SFMX_HIP(ctx, sfmx_grow_keep(cv->sd2, (size_t)cv->used * 2, (size_t)(cv->used + px) * 2, s));
  const int tiles = (w + CV_TILE - 1) / CV_TILE;
  SFMX_HIP(ctx, cv->te.begin(ctx));
  const int cbx = (w + 63) / 64;  // cbx * ceil(h / 4) < 2^30 / 64 + h + cbx: far below 2^31
  k_cv_cols<<<(unsigned)((long long)cbx * ((h + 3) / 4)), dim3(64, 4), 0, s>>>(src, w, h, threshold, cap, cv->col.as<uint8_t>(), d_inside, cbx);
  k_cv_rows<<<(unsigned)((long long)tiles * h), CV_TILE, 0, s>>>(cv->col.as<uint8_t>(), w, cap, tiles, cv->sd2.as<int16_t>() + cv->used);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, cv->te.end(ctx));
  int32_t inside = 0;
  SFMX_HIP(ctx, hipMemcpyAsync(&inside, d_inside, 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));  // the caller may reuse its picture, the next view the staging
  cv->te.collect(ctx);
  CvView v{};
  static_cast<DevView&>(v) = sfmx_dev_view(view, cv->used);
  cv->views.push_back(v);
  cv->caps.push_back(cap);
  cv->inside.push_back(inside);
  cv->used += px;
  cv->done = false;
  return SFMX_OK;
}

int sfmx_carve_add_stereo_view(sfmx_ctx* ctx, sfmx_carve* cv, const sfmx_fusion_view* view, const sfmx_stereo* st, int threshold, int cap) {
  SFMX_REQUIRE(ctx, ctx && cv && st && view);
  int w = 0, h = 0;
  const uint8_t* im = sfmx_stereo_device_rect_left(st, &w, &h);
  SFMX_REQUIRE(ctx, im && view->w == w && view->h == h);
  return sfmx_carve_add_view(ctx, cv, view, im, 1, threshold, cap);
}

int sfmx_carve_inside_pixels(const sfmx_carve* cv, int32_t* out) {
  if (!cv || !out) return SFMX_ERR_INVALID;
  if (!cv->inside.empty()) std::memcpy(out, cv->inside.data(), cv->inside.size() * 4);
  return SFMX_OK;
}

int sfmx_carve_view_count(const sfmx_carve* cv) { return cv ? (int)cv->views.size() : 0; }

int sfmx_carve_read_view(sfmx_ctx* ctx, sfmx_carve* cv, int i, int16_t* sd2_out) {
  SFMX_REQUIRE(ctx, ctx && cv && sd2_out && i >= 0 && i < (int)cv->views.size());
  const DevView& v = cv->views[(size_t)i];
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  SFMX_HIP(ctx, hipMemcpyAsync(sd2_out, cv->sd2.as<int16_t>() + v.off, (size_t)v.w * v.h * 2, hipMemcpyDeviceToHost, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SFMX_OK;
}

int sfmx_carve_set_batch(sfmx_carve* cv, int k) {
  if (!cv || k < 0 || k > 4096) return SFMX_ERR_INVALID;
  cv->batch = k;
  return SFMX_OK;
}

int sfmx_carve_run(sfmx_ctx* ctx, sfmx_carve* cv, const sfmx_carve_volume* vol, const sfmx_carve_params* p) {
  SFMX_REQUIRE(ctx, ctx && cv);
  cv->done = false;
  cv->t.us = 0.0;
  SFMX_REQUIRE(ctx, sfmx_carve_check_params(p) == SFMX_OK && cv_volume_ok(vol) && !cv->views.empty());
  for (int c : cv->caps) SFMX_REQUIRE(ctx, c == p->cap);
  const int nv = (int)cv->views.size();
  const int n = vol->nx * vol->ny * vol->nz;
  const int cap2 = p->cap * p->cap;
  const double trunc = p->trunc == 0.0 ? 4.0 * vol->voxel : p->trunc;
  for (CvView& v : cv->views) v.ft = v.f * trunc;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  SFMX_HIP(ctx, hipStreamSynchronize(s));  // an earlier launch may still read the view array or the table
  SFMX_HIP(ctx, cv->d_views.ensure(sizeof(CvView) * (size_t)nv));
  SFMX_HIP(ctx, cv->hull.ensure((size_t)n * 8));
  SFMX_HIP(ctx, cv->nviews.ensure((size_t)n * 4));
  SFMX_HIP(ctx, hipMemcpyAsync(cv->d_views.p, cv->views.data(), sizeof(CvView) * (size_t)nv, hipMemcpyHostToDevice, s));
  if (cv->tab_cap != p->cap) {
    std::vector<double> tab((size_t)cap2 + 1);
    for (int k = 0; k <= cap2; k++) tab[(size_t)k] = std::sqrt((double)k) - 0.5;
    cv->tab_cap = 0;
    SFMX_HIP(ctx, cv->tab.ensure(tab.size() * 8));
    SFMX_HIP(ctx, hipMemcpyAsync(cv->tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    SFMX_HIP(ctx, hipStreamSynchronize(s));  // tab leaves scope
    cv->tab_cap = p->cap;
  }
  const FuGrid g{vol->origin[0], vol->origin[1], vol->origin[2], vol->voxel, vol->nx, vol->ny, vol->nz, 1};
  const int bx = (g.nx + 63) / 64, by = (g.ny + 3) / 4;
  const int batch = cv->batch > 0 ? cv->batch : CV_AUTO_BATCH;
  SFMX_HIP(ctx, cv->t.begin(ctx));
  for (int v0 = 0; v0 < nv; v0 += batch) {
    const int k = nv - v0 < batch ? nv - v0 : batch;
    k_cv_hull<<<(unsigned)((long long)bx * by * g.nz), dim3(64, 4), (size_t)(cap2 + 1) * 8, s>>>(
        cv->hull.as<double>(), cv->nviews.as<int>(), g, cv->d_views.as<CvView>() + v0, k, cv->sd2.as<int16_t>(), cv->tab.as<double>(),
        cap2, v0 == 0 ? 1 : 0, bx, by);
  }
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, cv->t.end(ctx));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  cv->t.collect(ctx);
  cv->vol = *vol;
  cv->n = n;
  cv->min_views = p->min_views;
  cv->done = true;
  return SFMX_OK;
}

int sfmx_carve_read(sfmx_ctx* ctx, sfmx_carve* cv, double* hull, int32_t* views) {
  SFMX_REQUIRE(ctx, ctx && cv && cv->done);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (hull) SFMX_HIP(ctx, hipMemcpyAsync(hull, cv->hull.p, (size_t)cv->n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (views) SFMX_HIP(ctx, hipMemcpyAsync(views, cv->nviews.p, (size_t)cv->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SFMX_OK;
}

}  // extern "C"

namespace {

// the fusion object's arrays for writing, if its grid is the last run's
int cv_target(sfmx_ctx* ctx, sfmx_carve* cv, sfmx_fusion* fu, double** sum, int32_t** cnt, sfmx_fusion_params* fp) {
  SFMX_REQUIRE(ctx, ctx && cv && fu && cv->done);
  // the grid first, from the parameters alone: a refused call leaves fu as it was (pending views, cached surface)
  int rc = sfmx_fusion_mutable_volume(ctx, fu, nullptr, nullptr, fp);
  if (rc != SFMX_OK) return rc;
  const sfmx_carve_volume& v = cv->vol;
  SFMX_REQUIRE(ctx, fp->origin[0] == v.origin[0] && fp->origin[1] == v.origin[1] && fp->origin[2] == v.origin[2] &&
                        fp->voxel == v.voxel && fp->nx == v.nx && fp->ny == v.ny && fp->nz == v.nz);
  return sfmx_fusion_mutable_volume(ctx, fu, sum, cnt, fp);
}

}  // namespace

extern "C" {

int sfmx_carve_store(sfmx_ctx* ctx, sfmx_carve* cv, sfmx_fusion* fu) {
  double* sum = nullptr;
  int32_t* cnt = nullptr;
  sfmx_fusion_params fp{};
  const int rc = cv_target(ctx, cv, fu, &sum, &cnt, &fp);
  if (rc != SFMX_OK) return rc;
  cv->t.us = 0.0;
  hipStream_t s = ctx->stream;
  const int W = fp.min_weight > 1 ? fp.min_weight : 1;
  SFMX_HIP(ctx, cv->t.begin(ctx));
  k_cv_store<<<(unsigned)((cv->n + 255) / 256), 256, 0, s>>>(cv->hull.as<double>(), cv->nviews.as<int>(), cv->n, cv->min_views, W, sum, cnt);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, cv->t.end(ctx));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  cv->t.collect(ctx);
  return SFMX_OK;
}

int sfmx_carve_apply(sfmx_ctx* ctx, sfmx_carve* cv, sfmx_fusion* fu, const sfmx_carve_params* p, int32_t* counts) {
  SFMX_REQUIRE(ctx, ctx && cv && sfmx_carve_check_params(p) == SFMX_OK);
  double* sum = nullptr;
  int32_t* cnt = nullptr;
  sfmx_fusion_params fp{};
  const int rc = cv_target(ctx, cv, fu, &sum, &cnt, &fp);
  if (rc != SFMX_OK) return rc;
  cv->t.us = 0.0;
  hipStream_t s = ctx->stream;
  const int W = fp.min_weight > 1 ? fp.min_weight : 1;
  SFMX_HIP(ctx, cv->d_counters.ensure(4 * 4));
  SFMX_HIP(ctx, hipMemsetAsync(cv->d_counters.p, 0, 3 * 4, s));
  SFMX_HIP(ctx, cv->t.begin(ctx));
  k_cv_apply<<<(unsigned)((cv->n + 255) / 256), 256, 0, s>>>(cv->hull.as<double>(), cv->nviews.as<int>(), cv->n, cv->min_views, W,
                                                             fp.min_weight, p->margin, p->mode == SFMX_CARVE_CLEAR ? 1 : 0, sum, cnt,
                                                             cv->d_counters.as<int>());
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, cv->t.end(ctx));
  int32_t c[3] = {0, 0, 0};
  SFMX_HIP(ctx, hipMemcpyAsync(c, cv->d_counters.p, sizeof c, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  cv->t.collect(ctx);
  if (counts) std::memcpy(counts, c, sizeof c);
  return SFMX_OK;
}

int sfmx_carve_count(sfmx_ctx* ctx, sfmx_carve* cv, const sfmx_carve_params* p, int32_t* counts) {
  SFMX_REQUIRE(ctx, ctx && cv && counts && sfmx_carve_check_params(p) == SFMX_OK && cv->done);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  SFMX_HIP(ctx, cv->d_counters.ensure(4 * 4));
  SFMX_HIP(ctx, hipMemsetAsync(cv->d_counters.p, 0, 3 * 4, s));
  k_cv_count<<<(unsigned)((cv->n + 255) / 256), 256, 0, s>>>(cv->hull.as<double>(), cv->nviews.as<int>(), cv->n, cv->min_views, p->margin,
                                                             cv->d_counters.as<int>());
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, hipMemcpyAsync(counts, cv->d_counters.p, 3 * 4, hipMemcpyDeviceToHost, s));  // the third stays 0: nothing changes
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

double sfmx_carve_last_us(const sfmx_carve* cv) { return cv ? cv->t.us : 0.0; }
double sfmx_carve_last_edt_us(const sfmx_carve* cv) { return cv ? cv->te.us : 0.0; }

}  // extern "C"

int sfmx_carve_device_volume(const sfmx_carve* cv, const double** hull, const int32_t** views, sfmx_carve_volume* vol, int* min_views) {
  if (!cv || !cv->done) return -1;
  *hull = cv->hull.as<double>();
  *views = cv->nviews.as<int32_t>();
  *vol = cv->vol;
  *min_views = cv->min_views;
  return cv->n;
}
