// palign.hip — register a camera to the textured mesh: direct photometric alignment.  The textured (optionally
// seam-levelled) mesh is rendered at the current pose, every pixel well inside the textured silhouette compares the atlas value
// it sees with the picture, and sum r^2 is minimised over the six pose parameters by Gauss-Newton.  A sample is a pixel centre
// of the current view, so the picture is read at integer positions only: no interpolation of the picture and no warp.
//
// Exactness: the key image is the renderer's (sfmx_raster_dev.h: the same kernels), g is sfmx_photo's expression before its
// rounding, the row of a sample is IEEE double in the definition's order (built with -ffp-contract=off), the 28 sums are taken
// in the view alignment's fixed tree (sfmx_tree.h) and solved and applied by its host code (sfmx_pose_step.h).  Sums, n and
// every iterate equal tests/palign_ref.py bit for bit.
//
// Kernel layout (blocks of 256, the context's stream, no inter-workgroup hand-off, no float atomics):
//   k_pa_check      once per set_model, one thread per face: the range check of its indices
// Per evaluation:
//   k_rs_project / k_rs_faces / k_rs_big <true>   the key image of the one view (RsViewSet::zbuffer, a batch of one)
//   k_pa_mask       one thread per pixel: ok = a winner that is front-facing and textured, one byte
//   k_pa_erode<0>   rows: a byte is 1 iff the 2 margin + 1 bytes around it in its row are (outside the image: 0)
//   k_pa_erode<1>   columns of that: the candidates.  Two passes over bytes, exact, instead of (2 margin + 1)^2 keys per sample
//   k_pa_system     one thread per sample in k_al_system's tiling; J and r stay in registers, each of the 28 products is
//                   reduced as soon as it is formed (al_wave_sum), 28 x 4 doubles of LDS, one integer atomicAdd per wave for n;
//                   it also stores the sample's state and r for sfmx_palign_read
//   k_al_tree<28>   the levels of the tree
// One host synchronisation per evaluation (the 28 sums and n).
#include <cmath>
#include <vector>

#include "sfmx_internal.h"
#include "sfmx_pose_step.h"
#include "sfmx_raster_dev.h"
#include "sfmx_texture_dev.h"
#include "sfmx_tree.h"
#include "sfmx_view.h"

namespace {

constexpr int PA_TERMS = 28;

struct PaArgs {
  const unsigned long long* keys;
  const int* faces;
  const RsVert* pv;
  RsCam cam;
  const int* fview;
  const int* uvh;
  const uint8_t* atlas;
  int W, H;
  const uint8_t* img;
  const uint8_t* cand;
  double p[3], r_max;
  int stride, nsx, nsy;
};

__global__ __launch_bounds__(256) void k_pa_check(const int* __restrict__ faces, int m, int n, int* flag) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int a, b, c;
  if (!mesh_face(faces, f, n, a, b, c)) atomicOr(flag, 1);  // the call fails; nothing is read through the index
}

__global__ __launch_bounds__(256) void k_pa_mask(const unsigned long long* __restrict__ keys, const int* __restrict__ faces,
                                                 const RsVert* __restrict__ pv, const int* __restrict__ fview, int npx,
                                                 uint8_t* __restrict__ ok) {
  const int px = blockIdx.x * 256 + threadIdx.x;  // npx <= 2^24
  if (px >= npx) return;
  const unsigned long long key = keys[px];
  bool good = false;
  if (key != ~0ull) {
    const int f = (int)(unsigned)(key & 0xffffffffull);
    const RsVert P[3] = {pv[faces[3 * (size_t)f]], pv[faces[3 * (size_t)f + 1]], pv[faces[3 * (size_t)f + 2]]};  // checked by k_rs_faces
    good = rs_area(P) < 0 && fview[f] >= 0;
  }
  ok[px] = good ? 1 : 0;
}

// COLS = 0: out[y][x] = and of in[y][x - margin .. x + margin]; COLS = 1: of in[y - margin .. y + margin][x]; outside: 0
template <int COLS>
__global__ __launch_bounds__(256) void k_pa_erode(const uint8_t* __restrict__ in, int w, int h, int margin, uint8_t* __restrict__ out) {
  const int px = blockIdx.x * 256 + threadIdx.x;
  if (px >= w * h) return;
  const int y = px / w, x = px - y * w;
  const int at = COLS ? y : x, top = COLS ? h : w;
  bool all = at - margin >= 0 && at + margin < top;
  if (all) {
    const size_t step = COLS ? (size_t)w : 1;
    const uint8_t* q = in + (size_t)px - (size_t)margin * step;
    for (int k = 0; k <= 2 * margin; k++) all &= q[(size_t)k * step] != 0;
  }
  out[px] = all ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_pa_system(PaArgs a, double* __restrict__ partial, int* __restrict__ used,
                                                   uint8_t* __restrict__ state, double* __restrict__ res) {
  __shared__ double part[PA_TERMS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int si = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int sj = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool in_grid = si < a.nsx && sj < a.nsy;  // then stride si < w and stride sj < h
  const int w = a.cam.w;
  const int x = in_grid ? si * a.stride : 0, y = in_grid ? sj * a.stride : 0;
  const size_t px = (size_t)y * w + x;

  double J[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r = 0.0;
  bool ok = false;
  int st = 0;
  if (in_grid && a.cand[px]) {  // the pixel and its 8 neighbours are inside the image and have textured front-facing winners
    const int f = (int)(unsigned)(a.keys[px] & 0xffffffffull);
    const RsVert P[3] = {a.pv[a.faces[3 * (size_t)f]], a.pv[a.faces[3 * (size_t)f + 1]], a.pv[a.faces[3 * (size_t)f + 2]]};
    RsFace F;
    rs_setup(P, F);
    const long long e0 = rs_edge(F, 0, x, y), e1 = rs_edge(F, 1, x, y), e2 = rs_edge(F, 2, x, y);
    const double s = rs_s(e0, e1, e2, P);
    const double t0 = (double)e0 * P[0].r, t1 = (double)e1 * P[1].r, t2 = (double)e2 * P[2].r;
    const int* hc = a.uvh + 6 * (size_t)f;
    const double hx = ((t0 * (double)hc[0] + t1 * (double)hc[2]) + t2 * (double)hc[4]) / s;
    const double hy = ((t0 * (double)hc[1] + t1 * (double)hc[3]) + t2 * (double)hc[5]) / s;
    const double ax = hx * 0.5 - 0.5, ay = hy * 0.5 - 0.5;
    const double acx = fmin(fmax(ax, 0.0), (double)(a.W - 1)), acy = fmin(fmax(ay, 0.0), (double)(a.H - 1));
    const double x0 = floor(acx), y0 = floor(acy);
    const double fx = acx - x0, fy = acy - y0;
    const int xi0 = (int)x0, xi1 = min(xi0 + 1, a.W - 1);
    const int yi0 = (int)y0, yi1 = min(yi0 + 1, a.H - 1);
    const uint8_t* A0 = a.atlas + (size_t)yi0 * a.W;
    const uint8_t* A1 = a.atlas + (size_t)yi1 * a.W;
    const double top = (1.0 - fx) * (double)A0[xi0] + fx * (double)A0[xi1];
    const double bot = (1.0 - fx) * (double)A1[xi0] + fx * (double)A1[xi1];
    const double g = (1.0 - fy) * top + fy * bot;
    const double z = (double)F.absA / s;
    const uint8_t* I = a.img + px;
    r = (double)I[0] - g;
    ok = fabs(r) <= a.r_max;  // false for a NaN
    st = ok ? 2 : 1;
    if (ok) {
      const double Gx = 0.5 * ((double)I[1] - (double)I[-1]);
      const double Gy = 0.5 * ((double)I[w] - (double)I[-w]);
      const double dx = ((double)x - a.cam.cx) / a.cam.f, dy = ((double)y - a.cam.cy) / a.cam.f;
      const double q0 = dx * z, q1 = dy * z, q2 = z, iz = 1.0 / z;
      const double a0 = (Gx * a.cam.f) * iz, a1 = (Gy * a.cam.f) * iz, a2 = -((a0 * dx) + (a1 * dy));
      const double* R = a.cam.R;
      double gw[3], Q[3];
#pragma unroll
      for (int b = 0; b < 3; b++) {
        gw[b] = (a0 * R[b] + a1 * R[3 + b]) + a2 * R[6 + b];
        Q[b] = (a.cam.c[b] + ((R[b] * q0 + R[3 + b] * q1) + R[6 + b] * q2)) - a.p[b];
      }
      J[0] = Q[2] * gw[1] - Q[1] * gw[2];
      J[1] = Q[0] * gw[2] - Q[2] * gw[0];
      J[2] = Q[1] * gw[0] - Q[0] * gw[1];
      J[3] = -gw[0];
      J[4] = -gw[1];
      J[5] = -gw[2];
    }
  }
  if (in_grid) {
    const size_t o = (size_t)sj * a.nsx + si;
    state[o] = (uint8_t)st;
    res[o] = st ? r : 0.0;
  }

  int term = 0;
#pragma unroll
  for (int m = 0; m < 6; m++) {
#pragma unroll
    for (int n = m; n < 6; n++) {
      const double v = al_wave_sum(ok ? J[m] * J[n] : 0.0);
      if (lane == 0) part[term][wave] = v;
      term++;
    }
  }
#pragma unroll
  for (int m = 0; m < 6; m++) {
    const double v = al_wave_sum(ok ? J[m] * r : 0.0);
    if (lane == 0) part[term][wave] = v;
    term++;
  }
  {
    const double v = al_wave_sum(ok ? r * r : 0.0);
    if (lane == 0) part[term][wave] = v;
  }
  const unsigned long long ub = __ballot(ok);
  if (lane == 0 && ub) atomicAdd(used, __popcll(ub));
  __syncthreads();
  if (threadIdx.x < PA_TERMS) {
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partial[blk * PA_TERMS + threadIdx.x] = al_cross(part[threadIdx.x]);
  }
}

}  // namespace

struct sfmx_palign {
  RsViewSet vs;                    // the one current camera and its z-buffer (no image: the picture is kept here)
  const sfmx_texture* tx = nullptr;
  const sfmx_level* lv = nullptr;
  DevBuf verts, faces, img;        // the model's mesh and the picture, copied
  DevBuf own_fview, own_uvh, own_atlas;  // set_model_arrays: the texture result, copied (then tx is null)
  int own_W = 0, own_H = 0;
  DevBuf flag;                     // k_pa_check's word
  DevBuf mask[2];                  // ok, rows eroded; then the candidates in mask[0]
  DevBuf part[2], used;            // block partials, ping-pong over the tree's levels; int32 n
  DevBuf state, res;               // per sample of the last evaluation
  bool have_model = false, have_image = false, have_eval = false;
  int n = 0, m = 0, w = 0, h = 0, nsx = 0, nsy = 0;
  StageTimer t, tz, ts;  // an evaluation; its z-buffer; k_pa_system and the tree.  us: summed over the evaluations of the last call
};

namespace {

bool pa_view_finite(const sfmx_fusion_view* v) {
  for (double x : v->R_rw)
    if (!std::isfinite(x)) return false;
  for (double x : v->c_left)
    if (!std::isfinite(x)) return false;
  return true;
}

// the texture result an evaluation reads: the texture (and level) object's, or the object's own copy
struct PaTex {
  const int *fview, *uvh;
  const uint8_t* atlas;
  int W, H;
};

// what system and view check before any launch
int pa_ready(sfmx_ctx* ctx, sfmx_palign* pa, const sfmx_fusion_view* view, const sfmx_palign_params* p, PaTex* t) {
  SFMX_REQUIRE(ctx, pa->have_model && pa->have_image && "set_model and set_image first");
  SFMX_REQUIRE(ctx, sfmx_palign_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, rs_view_ok(view) && sfmx_view_ok(view));
  SFMX_REQUIRE(ctx, view->w == pa->w && view->h == pa->h && "the view has the picture's size");
  const sfmx_texture* tx = pa->tx;
  if (!tx) {
    *t = PaTex{pa->own_fview.as<int>(), pa->own_uvh.as<int>(), pa->own_atlas.as<uint8_t>(), pa->own_W, pa->own_H};
    return SFMX_OK;
  }
  SFMX_REQUIRE(ctx, tx->done && tx->n == pa->n && tx->m == pa->m && "the texture object still holds the model's run");
  *t = PaTex{tx->fview.as<int>(), tx->uvh.as<int>(), tx->atlas.as<uint8_t>(), tx->lay.W, tx->lay.H};
  if (pa->lv) {
    int W = 0, H = 0;
    SFMX_REQUIRE(ctx, sfmx_level_device_atlas(pa->lv, &t->atlas, &W, &H) >= 0 && "the level object needs a successful run");
    SFMX_REQUIRE(ctx, W == tx->lay.W && H == tx->lay.H && "the level object's atlas has the texture object's size");
  }
  return SFMX_OK;
}

// one evaluation at `v`: sums[28] and n
int pa_eval(sfmx_ctx* ctx, sfmx_palign* pa, const PaTex& tex, const sfmx_fusion_view* v, const sfmx_palign_params* p, double* sums,
            int32_t* n) {
  hipStream_t s = ctx->stream;
  RsViewSet& vs = pa->vs;
  pa->have_eval = false;
  const int w = pa->w, h = pa->h, npx = w * h;  // w h <= 2^24
  vs.views.assign(1, *v);
  vs.img_off.assign(1, -1);
  if (const int rc = vs.prepare(ctx, pa->n, pa->m)) return rc;
  const RsBatch& b = vs.batches[0];
  const int nsx = (int)(((long long)w + p->stride - 1) / p->stride), nsy = (int)(((long long)h + p->stride - 1) / p->stride);
  const int nbx = (nsx + 15) / 16, nby = (nsy + 15) / 16;
  int rows = nbx * nby;  // w <= 4096 and w h <= 2^24: below 2^17
  const size_t ns = (size_t)nsx * nsy;
  SFMX_HIP(ctx, pa->mask[0].ensure((size_t)npx));
  SFMX_HIP(ctx, pa->mask[1].ensure((size_t)npx));
  SFMX_HIP(ctx, pa->part[0].ensure((size_t)rows * PA_TERMS * 8));
  SFMX_HIP(ctx, pa->part[1].ensure((size_t)((rows + 255) / 256) * PA_TERMS * 8));
  SFMX_HIP(ctx, pa->used.ensure(4));
  SFMX_HIP(ctx, pa->state.ensure(ns));
  SFMX_HIP(ctx, pa->res.ensure(ns * 8));

  SFMX_HIP(ctx, pa->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(pa->used.p, 0, 4, s));
  SFMX_HIP(ctx, pa->tz.begin(ctx));
  if (pa->n > 0 && pa->m > 0) {
    SFMX_HIP(ctx, vs.zbuffer(b, pa->verts.as<double>(), pa->n, pa->faces.as<int32_t>(), pa->m, p->z_min, s));
  } else {  // nothing to draw
    SFMX_HIP(ctx, hipMemsetAsync(vs.keys.p, 0xFF, b.px * 8, s));
  }
  SFMX_HIP(ctx, pa->tz.end(ctx));
  const unsigned pb = (unsigned)((npx + 255) / 256);
  uint8_t *m0 = pa->mask[0].as<uint8_t>(), *m1 = pa->mask[1].as<uint8_t>();
  k_pa_mask<<<pb, 256, 0, s>>>(vs.keys.as<unsigned long long>(), pa->faces.as<int>(), vs.pv.as<RsVert>(), tex.fview, npx, m0);
  k_pa_erode<0><<<pb, 256, 0, s>>>(m0, w, h, p->margin, m1);
  k_pa_erode<1><<<pb, 256, 0, s>>>(m1, w, h, p->margin, m0);
  PaArgs a{};
  a.keys = vs.keys.as<unsigned long long>();
  a.faces = pa->faces.as<int>();
  a.pv = vs.pv.as<RsVert>();
  a.cam = rs_cam(v);
  a.fview = tex.fview;
  a.uvh = tex.uvh;
  a.atlas = tex.atlas;
  a.W = tex.W;
  a.H = tex.H;
  a.img = pa->img.as<uint8_t>();
  a.cand = m0;
  for (int k = 0; k < 3; k++) a.p[k] = p->pivot[k];
  a.r_max = p->r_max;
  a.stride = p->stride;
  a.nsx = nsx;
  a.nsy = nsy;
  SFMX_HIP(ctx, pa->ts.begin(ctx));
  k_pa_system<<<dim3((unsigned)nbx, (unsigned)nby), 256, 0, s>>>(a, pa->part[0].as<double>(), pa->used.as<int>(), pa->state.as<uint8_t>(),
                                                                 pa->res.as<double>());
  SFMX_HIP(ctx, hipGetLastError());
  int cur = 0;
  while (rows > 1) {
    const int groups = (rows + 255) / 256;
    k_al_tree<PA_TERMS><<<(unsigned)groups, 256, 0, s>>>(pa->part[cur].as<double>(), rows, pa->part[cur ^ 1].as<double>());
    SFMX_HIP(ctx, hipGetLastError());
    rows = groups;
    cur ^= 1;
  }
  SFMX_HIP(ctx, pa->ts.end(ctx));
  SFMX_HIP(ctx, pa->t.end(ctx));
  SFMX_HIP(ctx, hipMemcpyAsync(sums, pa->part[cur].p, PA_TERMS * 8, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipMemcpyAsync(n, pa->used.p, 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  for (StageTimer* st : {&pa->t, &pa->tz, &pa->ts}) {
    const double before = st->us;
    st->us = 0.0;
    st->collect(ctx);
    st->us += before;
  }
  pa->nsx = nsx;
  pa->nsy = nsy;
  pa->have_eval = true;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_palign_default_params(sfmx_palign_params* p) {
  if (!p) return;
  *p = sfmx_palign_params{};
  p->max_iters = 10;
  p->stride = 1;
  p->margin = 4;
  p->min_pixels = 64;
  p->r_max = 255.0;
  p->damping = 0.0;
  p->eps_rot = 5e-5;
  p->eps_trans = 1e-6;
}

int sfmx_palign_check_params(const sfmx_palign_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!(p->z_min > 0.0) || !std::isfinite(p->z_min)) return SFMX_ERR_INVALID;
  for (double x : p->pivot)
    if (!std::isfinite(x)) return SFMX_ERR_INVALID;
  if (p->max_iters < 1 || p->max_iters > SFMX_PALIGN_ITERS_CAP || p->stride < 1 || p->min_pixels < 1) return SFMX_ERR_INVALID;
  if (p->margin < 1 || p->margin > SFMX_PALIGN_MARGIN_CAP) return SFMX_ERR_INVALID;
  if (!(p->r_max >= 0.0) || !std::isfinite(p->r_max)) return SFMX_ERR_INVALID;
  if (!(p->damping >= 0.0) || !std::isfinite(p->damping)) return SFMX_ERR_INVALID;
  if (!(p->eps_rot >= 0.0) || !std::isfinite(p->eps_rot) || !(p->eps_trans >= 0.0) || !std::isfinite(p->eps_trans)) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_palign_create(sfmx_ctx* ctx, sfmx_palign** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* pa = new sfmx_palign;
  hipError_t e = pa->t.create();
  if (e == hipSuccess) e = pa->tz.create();
  if (e == hipSuccess) e = pa->ts.create();
  if (e != hipSuccess) {
    sfmx_palign_destroy(ctx, pa);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_palign_create", e);
  }
  *out = pa;
  return SFMX_OK;
}

void sfmx_palign_destroy(sfmx_ctx* ctx, sfmx_palign* pa) {
  if (!pa) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  pa->vs.release();
  for (DevBuf* b : {&pa->verts, &pa->faces, &pa->img, &pa->flag, &pa->mask[0], &pa->mask[1], &pa->part[0], &pa->part[1], &pa->used, &pa->state,
                    &pa->res, &pa->own_fview, &pa->own_uvh, &pa->own_atlas})
    b->release();
  pa->t.destroy();
  pa->tz.destroy();
  pa->ts.destroy();
  delete pa;
}

}  // extern "C"

namespace {

// the mesh part of both set_model entries: the range check, then the copies.  tx / lv, or the host arrays of a texture result
int pa_set_model(sfmx_ctx* ctx, sfmx_palign* pa, const sfmx_texture* tx, const sfmx_level* lv, const int32_t* face_view, const int32_t* uv_half,
                 const uint8_t* atlas, int W, int H, const double* verts, int n, const int32_t* faces, int m, int on_device) {
  SFMX_REQUIRE(ctx, (verts || n == 0) && (faces || m == 0));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  SFMX_HIP(ctx, pa->flag.ensure(4));
  SFMX_HIP(ctx, hipMemsetAsync(pa->flag.p, 0, 4, s));
  // the range check runs on the caller's faces (a device copy of host ones lands in a scratch slab first), so that a refused
  // mesh leaves the model set before untouched
  const int32_t* df = faces;
  if (m > 0 && !on_device) {
    SFMX_HIP(ctx, pa->mask[1].ensure((size_t)m * 12));
    SFMX_HIP(ctx, hipMemcpyAsync(pa->mask[1].p, faces, (size_t)m * 12, hipMemcpyHostToDevice, s));
    df = pa->mask[1].as<int32_t>();
  }
  if (m > 0) k_pa_check<<<(unsigned)(((size_t)m + 255) / 256), 256, 0, s>>>(df, m, n, pa->flag.as<int>());
  SFMX_HIP(ctx, hipGetLastError());
  int flag = 0;
  SFMX_HIP(ctx, hipMemcpyAsync(&flag, pa->flag.p, 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  SFMX_REQUIRE(ctx, flag == 0 && "a face index outside [0, n)");
  pa->have_model = false;  // a HIP failure from here on leaves no model
  pa->have_eval = false;
  SFMX_HIP(ctx, pa->verts.ensure((size_t)n * 24));
  SFMX_HIP(ctx, pa->faces.ensure((size_t)m * 12));
  if (n > 0) SFMX_HIP(ctx, hipMemcpyAsync(pa->verts.p, verts, (size_t)n * 24, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  if (m > 0) SFMX_HIP(ctx, hipMemcpyAsync(pa->faces.p, df, (size_t)m * 12, hipMemcpyDeviceToDevice, s));
  if (!tx) {
    const size_t px = (size_t)W * H;
    SFMX_HIP(ctx, pa->own_fview.ensure((size_t)m * 4));
    SFMX_HIP(ctx, pa->own_uvh.ensure((size_t)m * 24));
    SFMX_HIP(ctx, pa->own_atlas.ensure(px));
    if (m > 0) SFMX_HIP(ctx, hipMemcpyAsync(pa->own_fview.p, face_view, (size_t)m * 4, hipMemcpyHostToDevice, s));
    if (m > 0) SFMX_HIP(ctx, hipMemcpyAsync(pa->own_uvh.p, uv_half, (size_t)m * 24, hipMemcpyHostToDevice, s));
    if (px > 0) SFMX_HIP(ctx, hipMemcpyAsync(pa->own_atlas.p, atlas, px, hipMemcpyHostToDevice, s));
    pa->own_W = W;
    pa->own_H = H;
  }
  SFMX_HIP(ctx, hipStreamSynchronize(s));  // the caller may reuse its arrays
  pa->tx = tx;
  pa->lv = lv;
  pa->n = n;
  pa->m = m;
  pa->have_model = true;
  return SFMX_OK;
}

}  // namespace

extern "C" {

int sfmx_palign_set_model(sfmx_ctx* ctx, sfmx_palign* pa, const sfmx_texture* tx, const sfmx_level* lv, const double* verts, int n,
                          const int32_t* faces, int m, int on_device) {
  SFMX_REQUIRE(ctx, ctx && pa);
  SFMX_REQUIRE(ctx, tx && tx->done && "the texture object needs a successful run");
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && n == tx->n && m == tx->m && "the mesh of the texture object's last run");
  if (lv) {
    const uint8_t* atlas = nullptr;
    int W = 0, H = 0;
    SFMX_REQUIRE(ctx, sfmx_level_device_atlas(lv, &atlas, &W, &H) >= 0 && "the level object needs a successful run");
    SFMX_REQUIRE(ctx, W == tx->lay.W && H == tx->lay.H && "the level object's atlas has the texture object's size");
  }
  return pa_set_model(ctx, pa, tx, lv, nullptr, nullptr, nullptr, 0, 0, verts, n, faces, m, on_device);
}

int sfmx_palign_set_model_arrays(sfmx_ctx* ctx, sfmx_palign* pa, const int32_t* face_view, const int32_t* uv_half, const uint8_t* atlas, int W,
                                 int H, const double* verts, int n, const int32_t* faces, int m) {
  SFMX_REQUIRE(ctx, ctx && pa);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && W >= 0 && H >= 0 && (long long)W * H < (1ll << 31));
  SFMX_REQUIRE(ctx, (m == 0 || (face_view && uv_half)) && (atlas || (long long)W * H == 0));
  for (int f = 0; f < m; f++) SFMX_REQUIRE(ctx, (face_view[f] < 0 || (W >= 1 && H >= 1)) && "a textured face needs an atlas");
  return pa_set_model(ctx, pa, nullptr, nullptr, face_view, uv_half, atlas, W, H, verts, n, faces, m, 0);
}

int sfmx_palign_set_image(sfmx_ctx* ctx, sfmx_palign* pa, const uint8_t* image, int w, int h, int on_device) {
  SFMX_REQUIRE(ctx, ctx && pa && image);
  SFMX_REQUIRE(ctx, w >= 1 && h >= 1 && w <= 4096 && (long long)w * h <= (long long)SFMX_RASTER_MAX_PIXELS);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  pa->have_image = false;  // a HIP failure from here on leaves no picture
  pa->have_eval = false;
  const size_t px = (size_t)w * h;
  SFMX_HIP(ctx, pa->img.ensure(px));
  SFMX_HIP(ctx, hipMemcpyAsync(pa->img.p, image, px, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may reuse its buffer
  pa->w = w;
  pa->h = h;
  pa->have_image = true;
  return SFMX_OK;
}

int sfmx_palign_system(sfmx_ctx* ctx, sfmx_palign* pa, const sfmx_fusion_view* view, const sfmx_palign_params* p, double* sums, int32_t* n) {
  SFMX_REQUIRE(ctx, ctx && pa && sums && n);
  pa->have_eval = false;  // every failure from here on leaves no result behind
  pa->t.us = 0.0;
  pa->tz.us = 0.0;
  pa->ts.us = 0.0;
  PaTex tex{};
  if (const int rc = pa_ready(ctx, pa, view, p, &tex)) return rc;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return pa_eval(ctx, pa, tex, view, p, sums, n);
}

int sfmx_palign_view(sfmx_ctx* ctx, sfmx_palign* pa, const sfmx_fusion_view* view, const sfmx_palign_params* p, sfmx_palign_result* out) {
  SFMX_REQUIRE(ctx, ctx && pa && out);
  pa->have_eval = false;  // every failure from here on leaves no result behind
  pa->t.us = 0.0;
  pa->tz.us = 0.0;
  pa->ts.us = 0.0;
  PaTex tex{};
  if (const int rc = pa_ready(ctx, pa, view, p, &tex)) return rc;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  sfmx_palign_result res{};
  res.view = *view;
  res.status = SFMX_PALIGN_MAX_ITERS;
  sfmx_fusion_view cur = *view, good = *view;
  for (int it = 0; it < p->max_iters; it++) {
    double sums[PA_TERMS];
    int32_t n = 0;
    const int st = pa_eval(ctx, pa, tex, &cur, p, sums, &n);
    if (st != SFMX_OK) return st;
    res.iterations = it + 1;
    res.n[it] = n;
    res.e[it] = sums[27];
    double delta[6];
    if (n < p->min_pixels) {
      res.status = SFMX_PALIGN_TOO_FEW;
      cur = good;
      break;
    }
    sfmx_fusion_view next = cur;
    bool ok = al_solve(sums, p->damping, delta);
    if (ok) {
      al_update(&next, p->pivot, delta);
      ok = pa_view_finite(&next);  // an update that overflowed is no step
    }
    if (!ok) {
      res.status = SFMX_PALIGN_DEGENERATE;
      cur = good;
      break;
    }
    good = cur;
    cur = next;
    const double rot = al_norm3(delta), tr = al_norm3(delta + 3);
    res.rot[it] = rot;
    res.trans[it] = tr;
    if (rot <= p->eps_rot && tr <= p->eps_trans) {
      res.status = SFMX_PALIGN_CONVERGED;
      break;
    }
  }
  res.view = cur;
  *out = res;
  return SFMX_OK;
}

int sfmx_palign_read(sfmx_ctx* ctx, sfmx_palign* pa, uint8_t* state, double* r) {
  SFMX_REQUIRE(ctx, ctx && pa && pa->have_model && pa->have_image && pa->have_eval);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ns = (size_t)pa->nsx * pa->nsy;
  if (state) SFMX_HIP(ctx, hipMemcpyAsync(state, pa->state.p, ns, hipMemcpyDeviceToHost, ctx->stream));
  if (r) SFMX_HIP(ctx, hipMemcpyAsync(r, pa->res.p, ns * 8, hipMemcpyDeviceToHost, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SFMX_OK;
}

int sfmx_palign_sizes(const sfmx_palign* pa, int* nsx, int* nsy) {
  const bool have = pa && pa->have_model && pa->have_image && pa->have_eval;
  if (nsx) *nsx = have ? pa->nsx : 0;
  if (nsy) *nsy = have ? pa->nsy : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

double sfmx_palign_last_us(const sfmx_palign* pa) { return pa ? pa->t.us : 0.0; }

double sfmx_palign_last_zbuffer_us(const sfmx_palign* pa) { return pa ? pa->tz.us : 0.0; }

double sfmx_palign_last_system_us(const sfmx_palign* pa) { return pa ? pa->ts.us : 0.0; }

}  // extern "C"
