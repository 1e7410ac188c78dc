// align.hip — register a view to the fused volume: direct TSDF pose alignment.  Every valid pixel of the view's
// disparity map is lifted with the current pose, the signed distance s and its gradient are read there by trilinear
// interpolation, and sum s^2 is minimised over the six pose parameters by Gauss-Newton (Bylow et al., RSS 2013).  No ray cast,
// no correspondence search, no normal map of the new frame.
//
// Exactness: IEEE double in the definition's expression order (built with -ffp-contract=off); the 28 sums are taken in one
// fixed tree, so they equal tests/align_ref.py bit for bit, and so do the host's 6 x 6 Cholesky solve and the rational
// (Cayley) pose update (sfmx_pose_step.h, shared with palign.hip), whose only library function is sqrt.
//
// Kernel layout:
//   k_al_system   one thread per sample (pixel (stride i, stride j)); a wave is an 8 x 8 tile of samples and a block of 256 a
//                 16 x 16 one, as in k_rc_render.  The camera, the grid and the parameters are kernel arguments.  The 8 counts
//                 are read before the 8 sums.  Each of the 28 products is reduced as soon as it is formed, so a thread holds
//                 the 7 values (J, s) and one running term.  TREE INDEX of a thread: t = 4 lane + wave.  The halving tree over
//                 t (offsets 128 .. 4) is then __shfl_xor over the lane (offsets 32 .. 1), and its last two levels (offsets 2
//                 and 1) combine the four waves through 28 x 4 doubles of LDS: (p0 + p2) + (p1 + p3).
//   k_al_tree     the same tree over 256 rows of block partials per workgroup (row r of the group at tree index r, padded with
//                 +0.0), launched once per level until one row is left.  No floating-point atomics; no workgroup waits on
//                 another inside a launch.  n is an integer sum, one atomicAdd per wave.  The tree's device functions and
//                 k_al_tree live in sfmx_tree.h, which register.hip shares.
#include <cmath>

#include "sfmx_internal.h"
#include "sfmx_pose_step.h"
#include "sfmx_tree.h"
#include "sfmx_tsdf.h"
#include "sfmx_view.h"

namespace {

constexpr int AL_TERMS = 28;

struct AlParams {
  double disp_min;
  double p[3];  // the pivot: the box centre
  int stride;
};

__global__ __launch_bounds__(256) void k_al_system(const double* __restrict__ sum, const int* __restrict__ cnt, FuGrid g, DevView V,
                                                   AlParams P, const int16_t* __restrict__ disp, double* __restrict__ partial,
                                                   int* __restrict__ used) {
  __shared__ double part[AL_TERMS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int si = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int sj = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const long long xl = (long long)si * P.stride, yl = (long long)sj * P.stride;
  const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
  const double o[3] = {g.ox, g.oy, g.oz};
  const double top[3] = {(double)(g.nx - 1), (double)(g.ny - 1), (double)(g.nz - 1)};
  const double inv = 1.0 / g.vs;

  double J[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, s = 0.0;
  bool ok = xl < (long long)V.w && yl < (long long)V.h;
  if (ok) {
    const int d = disp[(size_t)yl * (size_t)V.w + (size_t)xl];
    ok = dv_disp_ok(d, P.disp_min);
    if (ok) {
      const double Z = dv_disp_depth(V, d);
      double X[3], gp[3];
      dv_lift(V, (double)xl, (double)yl, Z, X[0], X[1], X[2]);
#pragma unroll
      for (int a = 0; a < 3; a++) {
        gp[a] = (X[a] - o[a]) * inv;
        ok &= 0.0 <= gp[a] && gp[a] < top[a];  // false for NaN
      }
      if (ok) {
        const int i = (int)floor(gp[0]), j = (int)floor(gp[1]), k = (int)floor(gp[2]);
        const size_t L = (size_t)i + sy * (size_t)j + sz * (size_t)k;
        int c[8];
#pragma unroll
        for (int b = 0; b < 8; b++) c[b] = cnt[L + (b & 1) + ((b >> 1) & 1) * sy + ((b >> 2) & 1) * sz];
#pragma unroll
        for (int b = 0; b < 8; b++) ok &= c[b] >= g.minw;
        if (ok) {
          double sv[8];
#pragma unroll
          for (int b = 0; b < 8; b++) sv[b] = sum[L + (b & 1) + ((b >> 1) & 1) * sy + ((b >> 2) & 1) * sz] / (double)c[b];
          const double fx = gp[0] - (double)i, fy = gp[1] - (double)j, fz = gp[2] - (double)k;
          const double sq = fu_trilerp(sv, fx, fy, fz);
          ok = fabs(sq) < 1.0;
          if (ok) {
            double G[3];
            fu_grad_trilerp(sum, cnt, g, i, j, k, L, fx, fy, fz, G);
            const double gw0 = G[0] * inv, gw1 = G[1] * inv, gw2 = G[2] * inv;
            const double q0 = X[0] - P.p[0], q1 = X[1] - P.p[1], q2 = X[2] - P.p[2];
            J[0] = q1 * gw2 - q2 * gw1;
            J[1] = q2 * gw0 - q0 * gw2;
            J[2] = q0 * gw1 - q1 * gw0;
            J[3] = gw0;
            J[4] = gw1;
            J[5] = gw2;
            s = sq;
          }
        }
      }
    }
  }
  if (!ok) {  // an unused sample contributes +0.0 to every term
#pragma unroll
    for (int m = 0; m < 6; m++) J[m] = 0.0;
    s = 0.0;
  }

  int term = 0;
#pragma unroll
  for (int m = 0; m < 6; m++) {
#pragma unroll
    for (int n = m; n < 6; n++) {
      const double r = al_wave_sum(ok ? J[m] * J[n] : 0.0);
      if (lane == 0) part[term][wave] = r;
      term++;
    }
  }
#pragma unroll
  for (int m = 0; m < 6; m++) {
    const double r = al_wave_sum(ok ? J[m] * s : 0.0);
    if (lane == 0) part[term][wave] = r;
    term++;
  }
  {
    const double r = al_wave_sum(ok ? s * s : 0.0);
    if (lane == 0) part[term][wave] = r;
  }
  const unsigned long long ub = __ballot(ok);
  if (lane == 0 && ub) atomicAdd(used, __popcll(ub));
  __syncthreads();
  if (threadIdx.x < AL_TERMS) {
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partial[blk * AL_TERMS + threadIdx.x] = al_cross(part[threadIdx.x]);
  }
}

}  // namespace

struct sfmx_align {
  DevBuf map;             // a host disparity map, copied
  DevBuf part[2];         // block partials, ping-pong over the tree's levels
  DevBuf used;            // int32 n
  DevBuf in_sum, in_cnt;  // the _arrays entries' copy of host volumes
  StageTimer t;           // t.us: device time of the evaluations of the last call
};

namespace {

// where a call's volume and map come from, resolved to device pointers
struct AlInput {
  sfmx_fusion_params vol;
  const double* sum;
  const int32_t* cnt;
  const int16_t* disp;
};

// one evaluation at `v`: sums[28] and n
int al_eval(sfmx_ctx* ctx, sfmx_align* al, const AlInput& in, const sfmx_fusion_view* v, const sfmx_align_params* p, double* sums, int32_t* n) {
  const sfmx_fusion_params& vol = in.vol;
  const FuGrid g{vol.origin[0], vol.origin[1], vol.origin[2], vol.voxel, vol.nx, vol.ny, vol.nz, p->min_weight == 0 ? vol.min_weight : p->min_weight};
  const DevView V = sfmx_dev_view(v, 0);
  AlParams P{};
  P.disp_min = p->disp_min;
  P.stride = p->stride;
  const int dims[3] = {vol.nx, vol.ny, vol.nz};
  for (int a = 0; a < 3; a++) P.p[a] = vol.origin[a] + 0.5 * ((double)(dims[a] - 1) * vol.voxel);
  const int nsx = (int)(((long long)v->w + p->stride - 1) / p->stride), nsy = (int)(((long long)v->h + p->stride - 1) / p->stride);
  const int nbx = (nsx + 15) / 16, nby = (nsy + 15) / 16;
  int rows = nbx * nby;  // w <= 4096 and w h < 2^30: below 2^22
  hipStream_t s = ctx->stream;
  SFMX_HIP(ctx, al->part[0].ensure((size_t)rows * AL_TERMS * 8));
  SFMX_HIP(ctx, al->part[1].ensure((size_t)((rows + 255) / 256) * AL_TERMS * 8));
  SFMX_HIP(ctx, al->used.ensure(4));
  SFMX_HIP(ctx, hipMemsetAsync(al->used.p, 0, 4, s));
  SFMX_HIP(ctx, al->t.begin(ctx));
  k_al_system<<<dim3((unsigned)nbx, (unsigned)nby), 256, 0, s>>>(in.sum, in.cnt, g, V, P, in.disp, al->part[0].as<double>(), al->used.as<int>());
  SFMX_HIP(ctx, hipGetLastError());
  int cur = 0;
  while (rows > 1) {
    const int groups = (rows + 255) / 256;
    k_al_tree<AL_TERMS><<<(unsigned)groups, 256, 0, s>>>(al->part[cur].as<double>(), rows, al->part[cur ^ 1].as<double>());
    SFMX_HIP(ctx, hipGetLastError());
    rows = groups;
    cur ^= 1;
  }
  SFMX_HIP(ctx, al->t.end(ctx));
  SFMX_HIP(ctx, hipMemcpyAsync(sums, al->part[cur].p, AL_TERMS * 8, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipMemcpyAsync(n, al->used.p, 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  const double before = al->t.us;
  al->t.us = 0.0;
  al->t.collect(ctx);
  al->t.us += before;
  return SFMX_OK;
}

int al_loop(sfmx_ctx* ctx, sfmx_align* al, const AlInput& in, const sfmx_fusion_view* view, const sfmx_align_params* p, sfmx_align_result* out) {
  *out = sfmx_align_result{};
  out->view = *view;
  out->status = SFMX_ALIGN_MAX_ITERS;
  const int dims[3] = {in.vol.nx, in.vol.ny, in.vol.nz};
  double piv[3];
  for (int a = 0; a < 3; a++) piv[a] = in.vol.origin[a] + 0.5 * ((double)(dims[a] - 1) * in.vol.voxel);
  sfmx_fusion_view cur = *view, good = *view;
  for (int it = 0; it < p->max_iters; it++) {
    double sums[AL_TERMS];
    int32_t n = 0;
    const int st = al_eval(ctx, al, in, &cur, p, sums, &n);
    if (st != SFMX_OK) return st;
    out->iterations = it + 1;
    out->n[it] = n;
    out->e[it] = sums[27];
    double delta[6];
    if (n < p->min_pixels) {
      out->status = SFMX_ALIGN_TOO_FEW;
      cur = good;
      break;
    }
    if (!al_solve(sums, p->damping, delta)) {
      out->status = SFMX_ALIGN_DEGENERATE;
      cur = good;
      break;
    }
    good = cur;
    al_update(&cur, piv, delta);
    const double rot = al_norm3(delta), tr = al_norm3(delta + 3);
    out->rot[it] = rot;
    out->trans[it] = tr;
    if (rot <= p->eps_rot && tr <= p->eps_trans * in.vol.voxel) {
      out->status = SFMX_ALIGN_CONVERGED;
      break;
    }
  }
  out->view = cur;
  return SFMX_OK;
}

// the volume of a fusion object, its pending views integrated first
int al_from_fusion(sfmx_ctx* ctx, sfmx_fusion* fu, AlInput* in) {
  const int st = sfmx_fusion_integrate(ctx, fu);
  if (st != SFMX_OK) return st;
  SFMX_REQUIRE(ctx, sfmx_fusion_device_volume(fu, &in->sum, &in->cnt, &in->vol) > 0);
  return SFMX_OK;
}

int al_from_arrays(sfmx_ctx* ctx, sfmx_align* al, const sfmx_fusion_params* vol, const double* sum, const int32_t* count, int on_device,
                   AlInput* in) {
  in->vol = *vol;
  if (!on_device) {
    const size_t n = (size_t)vol->nx * vol->ny * vol->nz;
    SFMX_HIP(ctx, al->in_sum.ensure(n * 8));
    SFMX_HIP(ctx, al->in_cnt.ensure(n * 4));
    SFMX_HIP(ctx, hipMemcpyAsync(al->in_sum.p, sum, n * 8, hipMemcpyHostToDevice, ctx->stream));
    SFMX_HIP(ctx, hipMemcpyAsync(al->in_cnt.p, count, n * 4, hipMemcpyHostToDevice, ctx->stream));
    sum = al->in_sum.as<double>();
    count = al->in_cnt.as<int32_t>();
  }
  in->sum = sum;
  in->cnt = count;
  return SFMX_OK;
}

int al_map(sfmx_ctx* ctx, sfmx_align* al, const sfmx_fusion_view* v, const int16_t* disp16, int on_device, AlInput* in) {
  if (!on_device) {
    const size_t bytes = (size_t)v->w * v->h * 2;
    SFMX_HIP(ctx, al->map.ensure(bytes));
    SFMX_HIP(ctx, hipMemcpyAsync(al->map.p, disp16, bytes, hipMemcpyHostToDevice, ctx->stream));
    disp16 = al->map.as<int16_t>();
  }
  in->disp = disp16;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_align_default_params(sfmx_align_params* p) {
  if (!p) return;
  *p = sfmx_align_params{};
  p->max_iters = 10;
  p->stride = 1;
  p->disp_min = 1.0;
  p->min_weight = 0;
  p->min_pixels = 64;
  p->damping = 0.0;
  p->eps_rot = 1e-6;
  p->eps_trans = 1e-4;
}

int sfmx_align_check_params(const sfmx_align_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (p->max_iters < 1 || p->max_iters > SFMX_ALIGN_ITERS_CAP || p->stride < 1 || p->min_weight < 0 || p->min_pixels < 1) return SFMX_ERR_INVALID;
  if (!std::isfinite(p->disp_min)) return SFMX_ERR_INVALID;
  if (!(p->damping >= 0.0) || !std::isfinite(p->damping)) return SFMX_ERR_INVALID;
  if (!(p->eps_rot >= 0.0) || !std::isfinite(p->eps_rot) || !(p->eps_trans >= 0.0) || !std::isfinite(p->eps_trans)) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_align_create(sfmx_ctx* ctx, sfmx_align** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* al = new sfmx_align;
  const hipError_t e = al->t.create();
  if (e != hipSuccess) {
    sfmx_align_destroy(ctx, al);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_align_create", e);
  }
  *out = al;
  return SFMX_OK;
}

void sfmx_align_destroy(sfmx_ctx* ctx, sfmx_align* al) {
  if (!al) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* b : {&al->map, &al->part[0], &al->part[1], &al->used, &al->in_sum, &al->in_cnt}) b->release();
  al->t.destroy();
  delete al;
}

int sfmx_align_system(sfmx_ctx* ctx, sfmx_align* al, sfmx_fusion* fu, const sfmx_fusion_view* view, const int16_t* disp16, int on_device,
                      const sfmx_align_params* p, double* sums, int32_t* n) {
  SFMX_REQUIRE(ctx, ctx && al && fu && disp16 && sums && n);
  al->t.us = 0.0;
  SFMX_REQUIRE(ctx, sfmx_view_ok(view) && sfmx_align_check_params(p) == SFMX_OK);
  AlInput in{};
  int st = al_from_fusion(ctx, fu, &in);
  if (st != SFMX_OK) return st;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  st = al_map(ctx, al, view, disp16, on_device, &in);
  if (st != SFMX_OK) return st;
  return al_eval(ctx, al, in, view, p, sums, n);
}

int sfmx_align_system_arrays(sfmx_ctx* ctx, sfmx_align* al, const sfmx_fusion_params* vol, const double* sum, const int32_t* count,
                             int volume_on_device, const sfmx_fusion_view* view, const int16_t* disp16, int on_device,
                             const sfmx_align_params* p, double* sums, int32_t* n) {
  SFMX_REQUIRE(ctx, ctx && al && disp16 && sums && n);
  al->t.us = 0.0;
  SFMX_REQUIRE(ctx, sum && count && sfmx_fusion_check_params(vol) == SFMX_OK);
  SFMX_REQUIRE(ctx, sfmx_view_ok(view) && sfmx_align_check_params(p) == SFMX_OK);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  AlInput in{};
  int st = al_from_arrays(ctx, al, vol, sum, count, volume_on_device, &in);
  if (st == SFMX_OK) st = al_map(ctx, al, view, disp16, on_device, &in);
  if (st != SFMX_OK) return st;
  return al_eval(ctx, al, in, view, p, sums, n);  // synchronises: the caller may reuse its arrays
}

int sfmx_align_view(sfmx_ctx* ctx, sfmx_align* al, sfmx_fusion* fu, const sfmx_fusion_view* view, const int16_t* disp16, int on_device,
                    const sfmx_align_params* p, sfmx_align_result* out) {
  SFMX_REQUIRE(ctx, ctx && al && fu && disp16 && out);
  al->t.us = 0.0;
  SFMX_REQUIRE(ctx, sfmx_view_ok(view) && sfmx_align_check_params(p) == SFMX_OK);
  AlInput in{};
  int st = al_from_fusion(ctx, fu, &in);
  if (st != SFMX_OK) return st;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  st = al_map(ctx, al, view, disp16, on_device, &in);
  if (st != SFMX_OK) return st;
  return al_loop(ctx, al, in, view, p, out);
}

int sfmx_align_view_arrays(sfmx_ctx* ctx, sfmx_align* al, const sfmx_fusion_params* vol, const double* sum, const int32_t* count,
                           int volume_on_device, const sfmx_fusion_view* view, const int16_t* disp16, int on_device,
                           const sfmx_align_params* p, sfmx_align_result* out) {
  SFMX_REQUIRE(ctx, ctx && al && disp16 && out);
  al->t.us = 0.0;
  SFMX_REQUIRE(ctx, sum && count && sfmx_fusion_check_params(vol) == SFMX_OK);
  SFMX_REQUIRE(ctx, sfmx_view_ok(view) && sfmx_align_check_params(p) == SFMX_OK);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  AlInput in{};
  int st = al_from_arrays(ctx, al, vol, sum, count, volume_on_device, &in);
  if (st == SFMX_OK) st = al_map(ctx, al, view, disp16, on_device, &in);
  if (st != SFMX_OK) return st;
  return al_loop(ctx, al, in, view, p, out);
}

int sfmx_align_stereo_view(sfmx_ctx* ctx, sfmx_align* al, sfmx_fusion* fu, const sfmx_fusion_view* view, const sfmx_stereo* st,
                           const sfmx_align_params* p, sfmx_align_result* out) {
  SFMX_REQUIRE(ctx, ctx && al && fu && st && out);
  al->t.us = 0.0;
  SFMX_REQUIRE(ctx, sfmx_view_ok(view) && sfmx_align_check_params(p) == SFMX_OK);
  int w = 0, h = 0;
  const int16_t* d16 = sfmx_stereo_device_disp16(st, &w, &h);
  SFMX_REQUIRE(ctx, d16 && view->w == w && view->h == h);
  AlInput in{};
  const int rc = al_from_fusion(ctx, fu, &in);
  if (rc != SFMX_OK) return rc;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  in.disp = d16;
  return al_loop(ctx, al, in, view, p, out);
}

double sfmx_align_last_us(const sfmx_align* al) { return al ? al->t.us : 0.0; }

}  // extern "C"
