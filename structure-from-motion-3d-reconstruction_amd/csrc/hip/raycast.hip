// raycast.hip — the fused volume seen from any pinhole camera: depth, point, normal and a head-light shade per pixel, taken
// straight from sum / count by marching each pixel's ray.
//
// Exactness: IEEE double in the definition's expression order (built with -ffp-contract=off), one sample lattice
// z_k = z_min + k step that never moves.  The only samples a ray skips are ones outside the grid, which have no value by
// definition: per axis the grid coordinate of sample k is a monotone function of k in floating point (every operation in it
// rounds monotonically), so the samples inside the grid are one run [k0, k1).  The run is estimated from the ray-box
// intersection and then VERIFIED with the definition's own expressions (rc_before / rc_after), so the estimate's rounding
// cannot cost a sample.  tests/raycast_ref.py restates the definition in NumPy over every k; the tests compare bits.
//
// Kernel layout:
//   k_rc_render   one thread per pixel; a wave is an 8 x 8 pixel tile and a block of 256 a 16 x 16 one, so the rays of a wave
//                 walk through neighbouring cells.  The camera and the grid are kernel arguments (scalar loads).  The loop keeps
//                 the previous sample's value and the 8 corner values of the current cell in registers: with the default step a
//                 cell holds about two samples, and the 8 divisions and 16 loads happen once per cell.  Counts are read first
//                 and the sums only when all 8 are defined.  Hit lanes go on to the normal (the gradient at the 8 corners of
//                 the hit point's cell) and the shade in the same launch.  hits and the sample counter are integer sums, one
//                 atomicAdd per wave each.  No LDS, no inter-workgroup hand-off.
#include <cmath>

#include "sfmx_internal.h"
#include "sfmx_tsdf.h"

namespace {

struct RcCam {
  double R[9], c[3], f, cx, cy;
  int w, h;
};

struct RcMarch {
  double z_min, step;
  int K;
  int background;
};

// grid coordinate of sample k on one axis: the definition's expression
__device__ __forceinline__ double rc_coord(double c, double dw, double o, double inv, double z) { return ((c + z * dw) - o) * inv; }

__device__ __forceinline__ double rc_z(const RcMarch& m, int k) { return m.z_min + (double)k * m.step; }

// sample k lies before (after) the run of samples inside the grid: on some axis its coordinate has not yet reached (has left)
// the grid in the direction the ray moves.  By monotonicity this then holds for every smaller (larger) k as well.
__device__ __forceinline__ bool rc_before(const double* c, const double* dw, const double* o, double inv, const double* top, double z) {
  bool r = false;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double g = rc_coord(c[a], dw[a], o[a], inv, z);
    r |= (dw[a] > 0.0 && g < 0.0) || (dw[a] < 0.0 && g >= top[a]);
  }
  return r;
}
__device__ __forceinline__ bool rc_after(const double* c, const double* dw, const double* o, double inv, const double* top, double z) {
  bool r = false;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double g = rc_coord(c[a], dw[a], o[a], inv, z);
    r |= (dw[a] > 0.0 && g >= top[a]) || (dw[a] < 0.0 && g < 0.0);
  }
  return r;
}

__global__ __launch_bounds__(256) void k_rc_render(const double* __restrict__ sum, const int* __restrict__ cnt, FuGrid g, RcCam cam, RcMarch m,
                                                   double* __restrict__ depth, double* __restrict__ points, double* __restrict__ normals,
                                                   uint8_t* __restrict__ shaded, int* __restrict__ hits, unsigned long long* __restrict__ samples) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool live = x < cam.w && y < cam.h;
  const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
  const double o[3] = {g.ox, g.oy, g.oz};
  const double top[3] = {(double)(g.nx - 1), (double)(g.ny - 1), (double)(g.nz - 1)};
  const double inv = 1.0 / g.vs;
  const double dc0 = ((double)x - cam.cx) / cam.f, dc1 = ((double)y - cam.cy) / cam.f;
  double dw[3];
#pragma unroll
  for (int a = 0; a < 3; a++) dw[a] = (cam.R[a] * dc0 + cam.R[3 + a] * dc1) + cam.R[6 + a] * 1.0;

  // ---- the run of samples inside the grid: estimate, then verify --------------------------------------------------------
  int k0 = 0, k1 = live ? m.K : 0;
  if (live) {
    double zlo = -INFINITY, zhi = INFINITY;
    bool never = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (dw[a] == 0.0) {
        const double g0 = rc_coord(cam.c[a], dw[a], o[a], inv, m.z_min);  // the same for every k
        never |= !(0.0 <= g0 && g0 < top[a]);
      } else {
        const double za = (o[a] - cam.c[a]) / dw[a], zb = ((o[a] + top[a] * g.vs) - cam.c[a]) / dw[a];
        zlo = fmax(zlo, fmin(za, zb));
        zhi = fmin(zhi, fmax(za, zb));
      }
    }
    if (never) {
      k1 = 0;
    } else {
      const double e0 = floor((zlo - m.z_min) / m.step) - 1.0, e1 = ceil((zhi - m.z_min) / m.step) + 2.0;
      // a non-finite estimate (no bounded axis, overflow) keeps the whole range; the comparisons are false for NaN
      if (e0 > 0.0) k0 = e0 < (double)m.K ? (int)e0 : m.K;
      if (e1 < (double)m.K) k1 = e1 > 0.0 ? (int)e1 : 0;
      if (k1 < k0) k1 = k0;
      while (k0 > 0 && !rc_before(cam.c, dw, o, inv, top, rc_z(m, k0 - 1))) k0--;
      while (k1 < m.K && !rc_after(cam.c, dw, o, inv, top, rc_z(m, k1))) k1++;
    }
  }

  // ---- the march ---------------------------------------------------------------------------------------------------------
  double s[8] = {};
  int ci = -1, cj = -1, ck = -1;
  bool cell_ok = false;
  double prev = 0.0, cur = 0.0;
  bool prev_ok = false, hit = false;
  int kh = 0, evaluated = 0;
  for (int k = k0; k < k1; k++) {
    const double z = rc_z(m, k);
    const double g0 = rc_coord(cam.c[0], dw[0], o[0], inv, z), g1 = rc_coord(cam.c[1], dw[1], o[1], inv, z),
                 g2 = rc_coord(cam.c[2], dw[2], o[2], inv, z);
    bool ok = 0.0 <= g0 && g0 < top[0] && 0.0 <= g1 && g1 < top[1] && 0.0 <= g2 && g2 < top[2];
    if (ok) {
      evaluated++;
      const int i = (int)floor(g0), j = (int)floor(g1), kk = (int)floor(g2);
      if (i != ci || j != cj || kk != ck) {
        ci = i;
        cj = j;
        ck = kk;
        const size_t L = (size_t)i + sy * (size_t)j + sz * (size_t)kk;
        int c[8];
#pragma unroll
        for (int b = 0; b < 8; b++) c[b] = cnt[L + (b & 1) + ((b >> 1) & 1) * sy + ((b >> 2) & 1) * sz];
        cell_ok = true;
#pragma unroll
        for (int b = 0; b < 8; b++) cell_ok &= c[b] >= g.minw;
        if (cell_ok) {
#pragma unroll
          for (int b = 0; b < 8; b++) s[b] = sum[L + (b & 1) + ((b >> 1) & 1) * sy + ((b >> 2) & 1) * sz] / (double)c[b];
        }
      }
      ok = cell_ok;
      if (ok) {
        const double fx = g0 - (double)i, fy = g1 - (double)j, fz = g2 - (double)kk;
        cur = fu_trilerp(s, fx, fy, fz);
        if (prev_ok && prev > 0.0 && cur <= 0.0) {
          hit = true;
          kh = k;
          break;
        }
      }
    }
    prev_ok = ok;
    prev = cur;
  }

  // ---- hit point, normal, shade ---------------------------------------------------------------------------------------------
  double d = 0.0, P[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
  int grey = m.background;
  if (hit) {
    const double zp = rc_z(m, kh - 1), z = rc_z(m, kh);
    const double t = prev / (prev - cur);
    d = zp + t * (z - zp);
    double gp[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      P[a] = cam.c[a] + d * dw[a];
      gp[a] = (P[a] - o[a]) * inv;
      ok &= 0.0 <= gp[a] && gp[a] < top[a];
    }
    double N[3] = {0.0, 0.0, 0.0};
    if (ok) {
      const int i = (int)floor(gp[0]), j = (int)floor(gp[1]), kk = (int)floor(gp[2]);
      const size_t L = (size_t)i + sy * (size_t)j + sz * (size_t)kk;
#pragma unroll
      for (int b = 0; b < 8; b++) ok &= cnt[L + (b & 1) + ((b >> 1) & 1) * sy + ((b >> 2) & 1) * sz] >= g.minw;
      if (ok) {
        const double fx = gp[0] - (double)i, fy = gp[1] - (double)j, fz = gp[2] - (double)kk;
        fu_grad_trilerp(sum, cnt, g, i, j, kk, L, fx, fy, fz, N);
      }
    }
    const double len = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
    const bool nz = len > 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) n[a] = nz ? N[a] / len : 0.0;
    const double Ld = sqrt((dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2]);
    const double lam = -(((n[0] * dw[0] + n[1] * dw[1]) + n[2] * dw[2]) / Ld);
    grey = lam > 0.0 ? (int)fmin(255.0, floor(lam * 255.0 + 0.5)) : 0;
  }
  if (live) {
    const size_t px = (size_t)y * cam.w + x;
    depth[px] = d;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      points[3 * px + a] = P[a];
      normals[3 * px + a] = n[a];
    }
    shaded[px] = (uint8_t)grey;
  }
  // integer sums over the wave, then one atomic each (order-free)
  const unsigned long long hb = __ballot(hit);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) evaluated += __shfl_xor(evaluated, off, 64);
  if (lane == 0) {
    if (hb) atomicAdd(hits, __popcll(hb));
    if (evaluated) atomicAdd(samples, (unsigned long long)evaluated);
  }
}

}  // namespace

struct sfmx_raycast {
  DevBuf depth, normals, points, shaded, counters;  // counters: u64 samples, then int32 hits
  DevBuf in_sum, in_cnt;                            // sfmx_raycast_render_arrays' copy of host arrays
  int w = 0, h = 0;                                 // size of the last render; 0 before one
  int hits = 0;
  unsigned long long samples = 0;
  int background = 0;
  StageTimer t;
};

namespace {

bool rc_view_ok(const sfmx_fusion_view* v) {
  if (!v || v->w < 1 || v->h < 1 || v->w > 4096 || (long long)v->w * v->h > (long long)SFMX_RAYCAST_MAX_PIXELS) return false;
  for (double x : v->R_rw)
    if (!std::isfinite(x)) return false;
  for (double x : v->c_left)
    if (!std::isfinite(x)) return false;
  return std::isfinite(v->f) && v->f > 0.0 && std::isfinite(v->cx) && std::isfinite(v->cy);
}

// K for a resolved step, or 0 when it is over the limit
int rc_samples(const sfmx_raycast_params* p, double step) {
  const double q = std::floor((p->z_max - p->z_min) / step);
  return q < (double)SFMX_RAYCAST_MAX_SAMPLES ? (int)q + 1 : 0;
}

int rc_render(sfmx_ctx* ctx, sfmx_raycast* rc, const sfmx_fusion_params* vol, const double* d_sum, const int32_t* d_cnt,
              const sfmx_fusion_view* v, const sfmx_raycast_params* p) {
  rc->w = rc->h = 0;  // a failed render leaves no result
  rc->t.us = 0.0;
  const double step = p->step == 0.0 ? vol->voxel / 2.0 : p->step;
  SFMX_REQUIRE(ctx, step > 0.0);
  const int K = rc_samples(p, step);
  SFMX_REQUIRE(ctx, K >= 1);
  const FuGrid g{vol->origin[0], vol->origin[1], vol->origin[2], vol->voxel, vol->nx, vol->ny, vol->nz,
                 p->min_weight == 0 ? vol->min_weight : p->min_weight};
  RcCam cam{};
  std::memcpy(cam.R, v->R_rw, sizeof cam.R);
  std::memcpy(cam.c, v->c_left, sizeof cam.c);
  cam.f = v->f;
  cam.cx = v->cx;
  cam.cy = v->cy;
  cam.w = v->w;
  cam.h = v->h;
  const RcMarch m{p->z_min, step, K, (int)p->background};
  const size_t n = (size_t)v->w * v->h;
  hipStream_t s = ctx->stream;
  SFMX_HIP(ctx, rc->depth.ensure(n * 8));
  SFMX_HIP(ctx, rc->normals.ensure(n * 24));
  SFMX_HIP(ctx, rc->points.ensure(n * 24));
  SFMX_HIP(ctx, rc->shaded.ensure(n));
  SFMX_HIP(ctx, rc->counters.ensure(16));
  SFMX_HIP(ctx, hipMemsetAsync(rc->counters.p, 0, 16, s));
  unsigned long long* d_samples = rc->counters.as<unsigned long long>();
  int* d_hits = reinterpret_cast<int*>(d_samples + 1);
  SFMX_HIP(ctx, rc->t.begin(ctx));
  k_rc_render<<<dim3((unsigned)((v->w + 15) / 16), (unsigned)((v->h + 15) / 16)), 256, 0, s>>>(
      d_sum, d_cnt, g, cam, m, rc->depth.as<double>(), rc->points.as<double>(), rc->normals.as<double>(), rc->shaded.as<uint8_t>(), d_hits,
      d_samples);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, rc->t.end(ctx));
  unsigned long long back[2] = {0, 0};
  SFMX_HIP(ctx, hipMemcpyAsync(back, rc->counters.p, 16, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  rc->samples = back[0];
  std::memcpy(&rc->hits, &back[1], sizeof rc->hits);
  rc->background = (int)p->background;
  rc->w = v->w;
  rc->h = v->h;
  rc->t.collect(ctx);
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_raycast_default_params(sfmx_raycast_params* p) {
  if (!p) return;
  *p = sfmx_raycast_params{};
}

int sfmx_raycast_check_params(const sfmx_raycast_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!(p->z_min > 0.0) || !std::isfinite(p->z_min) || !(p->z_max > p->z_min) || !std::isfinite(p->z_max)) return SFMX_ERR_INVALID;
  if (!(p->step >= 0.0) || !std::isfinite(p->step) || p->min_weight < 0) return SFMX_ERR_INVALID;
  if (p->step > 0.0 && rc_samples(p, p->step) < 1) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_raycast_create(sfmx_ctx* ctx, sfmx_raycast** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* rc = new sfmx_raycast;
  const hipError_t e = rc->t.create();
  if (e != hipSuccess) {
    sfmx_raycast_destroy(ctx, rc);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_raycast_create", e);
  }
  *out = rc;
  return SFMX_OK;
}

void sfmx_raycast_destroy(sfmx_ctx* ctx, sfmx_raycast* rc) {
  if (!rc) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* b : {&rc->depth, &rc->normals, &rc->points, &rc->shaded, &rc->counters, &rc->in_sum, &rc->in_cnt}) b->release();
  rc->t.destroy();
  delete rc;
}

int sfmx_raycast_render(sfmx_ctx* ctx, sfmx_raycast* rc, sfmx_fusion* fu, const sfmx_fusion_view* view, const sfmx_raycast_params* p) {
  SFMX_REQUIRE(ctx, ctx && rc && fu);
  rc->w = rc->h = 0;
  SFMX_REQUIRE(ctx, rc_view_ok(view) && sfmx_raycast_check_params(p) == SFMX_OK);
  const int st = sfmx_fusion_integrate(ctx, fu);
  if (st != SFMX_OK) return st;
  const double* sum = nullptr;
  const int32_t* cnt = nullptr;
  sfmx_fusion_params vol{};
  SFMX_REQUIRE(ctx, sfmx_fusion_device_volume(fu, &sum, &cnt, &vol) > 0);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return rc_render(ctx, rc, &vol, sum, cnt, view, p);
}

int sfmx_raycast_render_arrays(sfmx_ctx* ctx, sfmx_raycast* rc, const sfmx_fusion_params* vol, const double* sum, const int32_t* count,
                               int on_device, const sfmx_fusion_view* view, const sfmx_raycast_params* p) {
  SFMX_REQUIRE(ctx, ctx && rc);
  rc->w = rc->h = 0;
  SFMX_REQUIRE(ctx, sum && count && sfmx_fusion_check_params(vol) == SFMX_OK);
  SFMX_REQUIRE(ctx, rc_view_ok(view) && sfmx_raycast_check_params(p) == SFMX_OK);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (!on_device) {
    const size_t n = (size_t)vol->nx * vol->ny * vol->nz;
    SFMX_HIP(ctx, rc->in_sum.ensure(n * 8));
    SFMX_HIP(ctx, rc->in_cnt.ensure(n * 4));
    SFMX_HIP(ctx, hipMemcpyAsync(rc->in_sum.p, sum, n * 8, hipMemcpyHostToDevice, ctx->stream));
    SFMX_HIP(ctx, hipMemcpyAsync(rc->in_cnt.p, count, n * 4, hipMemcpyHostToDevice, ctx->stream));
    sum = rc->in_sum.as<double>();
    count = rc->in_cnt.as<int32_t>();
  }
  return rc_render(ctx, rc, vol, sum, count, view, p);  // synchronises: the caller may reuse its arrays
}

int sfmx_raycast_read(sfmx_ctx* ctx, sfmx_raycast* rc, double* depth, double* normals, double* points, uint8_t* shaded, int32_t* hits) {
  SFMX_REQUIRE(ctx, ctx && rc && rc->w > 0);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)rc->w * rc->h;
  hipStream_t s = ctx->stream;
  if (depth) SFMX_HIP(ctx, hipMemcpyAsync(depth, rc->depth.p, n * 8, hipMemcpyDeviceToHost, s));
  if (normals) SFMX_HIP(ctx, hipMemcpyAsync(normals, rc->normals.p, n * 24, hipMemcpyDeviceToHost, s));
  if (points) SFMX_HIP(ctx, hipMemcpyAsync(points, rc->points.p, n * 24, hipMemcpyDeviceToHost, s));
  if (shaded) SFMX_HIP(ctx, hipMemcpyAsync(shaded, rc->shaded.p, n, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  if (hits) *hits = rc->hits;
  return SFMX_OK;
}

int sfmx_raycast_device_surface(const sfmx_raycast* rc, const double** points, const double** normals, int* n) {
  const bool have = rc && rc->w > 0;
  if (points) *points = have ? rc->points.as<double>() : nullptr;
  if (normals) *normals = have ? rc->normals.as<double>() : nullptr;
  if (n) *n = have ? rc->w * rc->h : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_raycast_shade(sfmx_ctx* ctx, sfmx_raycast* rc, sfmx_shade* sh, const sfmx_shade_params* p, uint8_t* grey_out,
                       int32_t* views_out) {
  SFMX_REQUIRE(ctx, ctx && rc && sh && rc->w > 0);
  const int n = rc->w * rc->h;
  int st = sfmx_shade_vertices(ctx, sh, rc->points.as<double>(), rc->normals.as<double>(), n, 1, p, grey_out, views_out);
  if (st != SFMX_OK || (!grey_out && !views_out)) return st;
  // a hit has depth >= z_min > 0, a pixel without one exactly 0
  std::vector<double> depth((size_t)n);
  SFMX_HIP(ctx, hipMemcpyAsync(depth.data(), rc->depth.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < n; i++)
    if (depth[(size_t)i] == 0.0) {
      if (grey_out) grey_out[i] = (uint8_t)rc->background;
      if (views_out) views_out[i] = 0;
    }
  return SFMX_OK;
}

double sfmx_raycast_last_us(const sfmx_raycast* rc) { return rc ? rc->t.us : 0.0; }

uint64_t sfmx_raycast_last_samples(const sfmx_raycast* rc) { return rc && rc->w > 0 ? rc->samples : 0; }

}  // extern "C"
