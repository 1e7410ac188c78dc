// register.hip — register a surface to a reference mesh: Sim(3) point-to-plane Gauss-Newton.  Every sampled
// source point is moved by the current transform, the sdist stage (unchanged) names its nearest face, and the
// squared distance to that face's plane, sum (h h) / nn, is minimised over rotation, translation and scale (Chen-Medioni).
//
// Exactness: IEEE double in the definition's expression order (built with -ffp-contract=off); the correspondences are sdist's
// (d2, face), the 37 sums are taken in DESIGN.md 19's fixed tree, and the host's Cholesky solve and rational (Cayley) update use
// sqrt as their only library function.  So sums, n_used, the pivot and every iterate equal tests/register_ref.py bit for bit.
//
// Kernel layout, blocks of 256 on the context's stream:
//   k_rg_bbox     per target face: its nine coordinates as order-preserving integer keys, wave-reduced, then atomicMin /
//                 atomicMax (integers: any order gives the same bits).  Run once per set_target, after sdist has checked the faces.
//   k_rg_apply    one thread per sample k (point stride k): y = s (R x) + t into the buffer sdist's device-pointer query reads; a
//                 non-finite source coordinate sets a flag (atomicOr)
//   k_rg_system   one thread per sample: reads y and the query's (d2, face) where sdist left them, and the target copy sdist
//                 holds.  J[7], h, w and d2 stay in registers; each of the 37 products is reduced as soon as it is formed
//                 (al_wave_sum), the four waves meet through 37 x 4 doubles of LDS.  Sample k sits in block k / 256 at lane k % 64
//                 of wave (k % 256) / 64, tree index 4 lane + wave.  n_used is an integer sum, one atomicAdd per wave.
//   k_al_tree<37> the tree's further levels (sfmx_tree.h), one launch per level until one row is left
// No floating-point atomics; no kernel waits on another workgroup.
#include <cmath>

#include "sfmx_internal.h"
#include "sfmx_sdist_math.h"
#include "sfmx_tree.h"

namespace {

constexpr int RG_TERMS = SFMX_REGISTER_TERMS;

struct RgT {  // a transform as a kernel argument
  double s, R[9], t[3];
};

// x -> an integer whose unsigned order is the order of the finite doubles (-0.0 below +0.0)
__host__ __device__ inline unsigned long long rg_key(double x) {
  unsigned long long b;
  memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
inline double rg_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  double x;
  memcpy(&x, &b, 8);
  return x;
}

__device__ __forceinline__ bool rg_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }  // false for NaN

// keys[0..2] = min, keys[3..5] = max over the corners of every face; the indices were checked by sdist's set_target
__global__ __launch_bounds__(256) void k_rg_bbox(const double* __restrict__ V, const int* __restrict__ F, int m,
                                                 unsigned long long* __restrict__ keys) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
  if (f < m) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const size_t i = (size_t)F[3 * (size_t)f + j];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const unsigned long long key = rg_key(V[3 * i + k]);
        mn[k] = key < mn[k] ? key : mn[k];
        mx[k] = key > mx[k] ? key : mx[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long y = __shfl_xor(mn[k], o, 64), z = __shfl_xor(mx[k], o, 64);
      mn[k] = y < mn[k] ? y : mn[k];
      mx[k] = z > mx[k] ? z : mx[k];
    }
  if ((threadIdx.x & 63) == 0 && mn[0] <= mx[0]) {  // a wave with at least one face
#pragma unroll
    for (int k = 0; k < 3; k++) {
      atomicMin(&keys[k], mn[k]);
      atomicMax(&keys[3 + k], mx[k]);
    }
  }
}

// sample k is point stride k; y [ns][3]
__global__ __launch_bounds__(256) void k_rg_apply(const double* __restrict__ X, int stride, int ns, RgT T, double* __restrict__ Y,
                                                  int* __restrict__ flag) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= ns) return;
  const size_t i = (size_t)k * (size_t)stride;
  const double x0 = X[3 * i], x1 = X[3 * i + 1], x2 = X[3 * i + 2];
  if (!(rg_finite(x0) && rg_finite(x1) && rg_finite(x2))) atomicOr(flag, 1);
#pragma unroll
  for (int a = 0; a < 3; a++) Y[3 * (size_t)k + a] = T.s * ((T.R[3 * a] * x0 + T.R[3 * a + 1] * x1) + T.R[3 * a + 2] * x2) + T.t[a];
}

__global__ __launch_bounds__(256) void k_rg_system(const double* __restrict__ Y, const double* __restrict__ d2q, const int* __restrict__ face,
                                                   const double* __restrict__ V, const int* __restrict__ F, int ns, double p0, double p1,
                                                   double p2, double* __restrict__ partial, int* __restrict__ used) {
  __shared__ double part[RG_TERMS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  double J[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, h = 0.0, w = 0.0, c = 0.0;
  bool ok = k < (long long)ns;
  if (ok) {
    const int f = face[k];
    ok = f >= 0;
    if (ok) {
      const size_t i0 = (size_t)F[3 * (size_t)f], i1 = (size_t)F[3 * (size_t)f + 1], i2 = (size_t)F[3 * (size_t)f + 2];
      const double a0 = V[3 * i0], a1 = V[3 * i0 + 1], a2 = V[3 * i0 + 2];
      const double u0 = V[3 * i1] - a0, u1 = V[3 * i1 + 1] - a1, u2 = V[3 * i1 + 2] - a2;  // b - a
      const double v0 = V[3 * i2] - a0, v1 = V[3 * i2 + 1] - a1, v2 = V[3 * i2 + 2] - a2;  // c - a
      const double n0 = u1 * v2 - u2 * v1, n1 = u2 * v0 - u0 * v2, n2 = u0 * v1 - u1 * v0;
      const double nn = sfmx::sd_dot(n0, n1, n2, n0, n1, n2);
      ok = nn > 0.0;
      if (ok) {
        const double y0 = Y[3 * (size_t)k], y1 = Y[3 * (size_t)k + 1], y2 = Y[3 * (size_t)k + 2];
        h = sfmx::sd_dot(y0 - a0, y1 - a1, y2 - a2, n0, n1, n2);
        const double q0 = y0 - p0, q1 = y1 - p1, q2 = y2 - p2;
        w = 1.0 / nn;
        J[0] = q1 * n2 - q2 * n1;
        J[1] = q2 * n0 - q0 * n2;
        J[2] = q0 * n1 - q1 * n0;
        J[3] = n0;
        J[4] = n1;
        J[5] = n2;
        J[6] = sfmx::sd_dot(q0, q1, q2, n0, n1, n2);
        c = d2q[k];
      }
    }
  }

  int term = 0;
#pragma unroll
  for (int m = 0; m < 7; m++) {
#pragma unroll
    for (int n = m; n < 7; n++) {
      const double r = al_wave_sum(ok ? (J[m] * J[n]) * w : 0.0);
      if (lane == 0) part[term][wave] = r;
      term++;
    }
  }
#pragma unroll
  for (int m = 0; m < 7; m++) {
    const double r = al_wave_sum(ok ? (J[m] * h) * w : 0.0);
    if (lane == 0) part[term][wave] = r;
    term++;
  }
  {
    const double r = al_wave_sum(ok ? (h * h) * w : 0.0);
    if (lane == 0) part[term][wave] = r;
    term++;
  }
  {
    const double r = al_wave_sum(ok ? c : 0.0);
    if (lane == 0) part[term][wave] = r;
  }
  const unsigned long long ub = __ballot(ok);
  if (lane == 0 && ub) atomicAdd(used, __popcll(ub));
  __syncthreads();
  if (threadIdx.x < RG_TERMS) partial[(size_t)blockIdx.x * RG_TERMS + threadIdx.x] = al_cross(part[threadIdx.x]);
}

}  // namespace

struct sfmx_register {
  sfmx_sdist* sd = nullptr;  // the target, its grid and the query's buffers
  DevBuf src;                // a host source, copied
  DevBuf y;                  // the transformed samples
  DevBuf part[2];            // block partials, ping-pong over the tree's levels
  DevBuf words;              // 6 x u64 box keys, then int32 n_used and int32 flag
  bool ready = false;
  int m = 0;
  double d_max = 0.0, cell = 0.0;
  double pivot[3] = {};
  StageTimer ta, ts;         // k_rg_apply; k_rg_system and the tree
  double us = 0.0, query_us = 0.0;
};

namespace {

bool rg_transform_ok(const sfmx_register_transform* T) {
  if (!std::isfinite(T->s) || !(T->s > 0.0)) return false;
  for (double v : T->R)
    if (!std::isfinite(v)) return false;
  for (double v : T->t)
    if (!std::isfinite(v)) return false;
  return true;
}

sfmx_register_transform rg_identity() {
  sfmx_register_transform T{};
  T.s = 1.0;
  T.R[0] = T.R[4] = T.R[8] = 1.0;
  return T;
}

RgT rg_arg(const sfmx_register_transform& T) {
  RgT a;
  a.s = T.s;
  for (int i = 0; i < 9; i++) a.R[i] = T.R[i];
  for (int i = 0; i < 3; i++) a.t[i] = T.t[i];
  return a;
}

int* rg_used(sfmx_register* rg) { return reinterpret_cast<int*>(rg->words.as<unsigned long long>() + 6); }

// the source on the device
int rg_source(sfmx_ctx* ctx, sfmx_register* rg, const double* points, int n, int on_device, const double** dev) {
  *dev = points;
  if (on_device || n == 0) return SFMX_OK;
  SFMX_HIP(ctx, rg->src.ensure((size_t)n * 24));
  SFMX_HIP(ctx, hipMemcpyAsync(rg->src.p, points, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
  *dev = rg->src.as<double>();
  return SFMX_OK;
}

// one evaluation at T: sums[37] and n_used; X is a device pointer
int rg_eval(sfmx_ctx* ctx, sfmx_register* rg, const double* X, int n, const sfmx_register_transform& T, const sfmx_register_params* p,
            double* sums, int32_t* n_used) {
  for (int t = 0; t < RG_TERMS; t++) sums[t] = 0.0;
  *n_used = 0;
  const int ns = (int)(((long long)n + p->stride - 1) / p->stride);
  if (ns == 0) return SFMX_OK;
  hipStream_t s = ctx->stream;
  int rows = (ns + 255) / 256;
  SFMX_HIP(ctx, rg->y.ensure((size_t)ns * 24));
  SFMX_HIP(ctx, rg->part[0].ensure((size_t)rows * RG_TERMS * 8));
  SFMX_HIP(ctx, rg->part[1].ensure((size_t)((rows + 255) / 256) * RG_TERMS * 8));
  int* used = rg_used(rg);
  int flag = 0;
  SFMX_HIP(ctx, hipMemsetAsync(used, 0, 8, s));  // n_used and the flag
  SFMX_HIP(ctx, rg->ta.begin(ctx));
  k_rg_apply<<<(unsigned)rows, 256, 0, s>>>(X, p->stride, ns, rg_arg(T), rg->y.as<double>(), used + 1);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, rg->ta.end(ctx));
  SFMX_HIP(ctx, hipMemcpyAsync(&flag, used + 1, 4, hipMemcpyDeviceToHost, s));
  const int rc = sfmx_sdist_query(ctx, rg->sd, rg->y.as<double>(), ns, 1, nullptr, nullptr);  // synchronises
  const hipError_t se = hipStreamSynchronize(s);  // a query refused before its own synchronise leaves the flag's copy pending
  if (rc == SFMX_ERR_HIP) return rc;
  SFMX_HIP(ctx, se);
  SFMX_REQUIRE(ctx, flag == 0);  // a non-finite source coordinate
  if (rc != SFMX_OK) return rc;  // a transformed point that is not finite
  rg->query_us += sfmx_sdist_last_us(rg->sd);
  rg->ta.us = 0.0;
  rg->ta.collect(ctx);
  rg->us += rg->ta.us;
  const double *V = nullptr, *d2 = nullptr;
  const int32_t *F = nullptr, *face = nullptr;
  int m = 0;
  SFMX_REQUIRE(ctx, sfmx_sdist_device_state(rg->sd, &V, &F, &m, &d2, &face) >= 0 && d2 && face);
  SFMX_HIP(ctx, rg->ts.begin(ctx));
  k_rg_system<<<(unsigned)rows, 256, 0, s>>>(rg->y.as<double>(), d2, face, V, F, ns, rg->pivot[0], rg->pivot[1], rg->pivot[2],
                                            rg->part[0].as<double>(), used);
  SFMX_HIP(ctx, hipGetLastError());
  int cur = 0;
  while (rows > 1) {
    const int groups = (rows + 255) / 256;
    k_al_tree<RG_TERMS><<<(unsigned)groups, 256, 0, s>>>(rg->part[cur].as<double>(), rows, rg->part[cur ^ 1].as<double>());
    SFMX_HIP(ctx, hipGetLastError());
    rows = groups;
    cur ^= 1;
  }
  SFMX_HIP(ctx, rg->ts.end(ctx));
  SFMX_HIP(ctx, hipMemcpyAsync(sums, rg->part[cur].p, RG_TERMS * 8, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipMemcpyAsync(n_used, used, 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  rg->ts.us = 0.0;
  rg->ts.collect(ctx);
  rg->us += rg->ts.us;
  return SFMX_OK;
}

// (A + damping I) delta = -b by Cholesky at dimension dim (7, or 6: rows and columns 0 .. 5), one written order; false when a
// pivot is <= 0 or not finite.  delta[6] = 0 at dimension 6.
bool rg_solve(const double* sums, double damping, int dim, double* delta) {
  double M[7][7], L[7][7] = {};
  int t = 0;
  for (int m = 0; m < 7; m++)
    for (int n = m; n < 7; n++) M[m][n] = M[n][m] = sums[t++];
  for (int m = 0; m < dim; m++) M[m][m] = M[m][m] + damping;
  const double* b = sums + 28;
  for (int j = 0; j < dim; j++) {
    double d = M[j][j];
    for (int k = 0; k < j; k++) d = d - L[j][k] * L[j][k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < dim; i++) {
      double v = M[i][j];
      for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  double y[7];
  for (int i = 0; i < dim; i++) {
    double v = -b[i];
    for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  delta[6] = 0.0;
  for (int i = dim - 1; i >= 0; i--) {
    double v = y[i];
    for (int k = i + 1; k < dim; k++) v = v - L[k][i] * delta[k];
    delta[i] = v / L[i][i];
  }
  return true;
}

// the step delta = (omega, v, sigma) about the pivot p; g = 1 + sigma
sfmx_register_transform rg_update(const sfmx_register_transform& T, const double* p, const double* delta, double g) {
  const double a0 = 0.5 * delta[0], a1 = 0.5 * delta[1], a2 = 0.5 * delta[2];
  const double k = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2));
  double D[3][3];
  D[0][0] = 1.0 - k * (a1 * a1 + a2 * a2);
  D[0][1] = k * (a0 * a1 - a2);
  D[0][2] = k * (a0 * a2 + a1);
  D[1][0] = k * (a0 * a1 + a2);
  D[1][1] = 1.0 - k * (a0 * a0 + a2 * a2);
  D[1][2] = k * (a1 * a2 - a0);
  D[2][0] = k * (a0 * a2 - a1);
  D[2][1] = k * (a1 * a2 + a0);
  D[2][2] = 1.0 - k * (a0 * a0 + a1 * a1);
  sfmx_register_transform N{};
  N.s = g * T.s;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) N.R[3 * a + b] = (D[a][0] * T.R[b] + D[a][1] * T.R[3 + b]) + D[a][2] * T.R[6 + b];
  const double u0 = T.t[0] - p[0], u1 = T.t[1] - p[1], u2 = T.t[2] - p[2];
  for (int a = 0; a < 3; a++) N.t[a] = (p[a] + g * ((D[a][0] * u0 + D[a][1] * u1) + D[a][2] * u2)) + delta[3 + a];
  return N;
}

// what every entry checks before it touches the device
int rg_check(sfmx_ctx* ctx, const sfmx_register* rg, const double* points, int n, const sfmx_register_params* p) {
  SFMX_REQUIRE(ctx, rg->ready);  // no successful set_target
  SFMX_REQUIRE(ctx, n >= 0 && n < (1 << 30) && (n == 0 || points));
  if (p) {
    SFMX_REQUIRE(ctx, sfmx_register_check_params(p) == SFMX_OK);
    SFMX_REQUIRE(ctx, p->d_max == rg->d_max && p->cell == rg->cell);  // the target was built with these
  }
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_register_default_params(sfmx_register_params* p) {
  if (!p) return;
  *p = sfmx_register_params{};
  p->d_max = 0.0;  // no default: it is a length in the caller's units
  p->cell = 0.0;
  p->max_iters = 20;
  p->stride = 1;
  p->min_points = 16;
  p->damping = 0.0;
  p->with_scale = 1;
  p->eps_rot = 1e-4;
  p->eps_scale = 1e-4;
  p->eps_trans = 1e-3;
}

int sfmx_register_check_params(const sfmx_register_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  sfmx_sdist_params sp;
  sp.d_max = p->d_max;
  sp.cell = p->cell;
  if (sfmx_sdist_check_params(&sp) != SFMX_OK) return SFMX_ERR_INVALID;
  if (p->max_iters < 1 || p->max_iters > SFMX_REGISTER_ITERS_CAP || p->stride < 1 || p->min_points < 7) return SFMX_ERR_INVALID;
  if (!(p->damping >= 0.0) || !std::isfinite(p->damping)) return SFMX_ERR_INVALID;
  if (!(p->eps_rot >= 0.0) || !std::isfinite(p->eps_rot) || !(p->eps_scale >= 0.0) || !std::isfinite(p->eps_scale) ||
      !(p->eps_trans >= 0.0) || !std::isfinite(p->eps_trans))
    return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_register_create(sfmx_ctx* ctx, sfmx_register** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* rg = new sfmx_register;
  int st = sfmx_sdist_create(ctx, &rg->sd);
  if (st == SFMX_OK) {
    hipError_t e = rg->ta.create();
    if (e == hipSuccess) e = rg->ts.create();
    if (e == hipSuccess) e = rg->words.ensure(64);
    if (e != hipSuccess) st = sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_register_create", e);
  }
  if (st != SFMX_OK) {
    sfmx_register_destroy(ctx, rg);
    return st;
  }
  *out = rg;
  return SFMX_OK;
}

void sfmx_register_destroy(sfmx_ctx* ctx, sfmx_register* rg) {
  if (!rg) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  sfmx_sdist_destroy(ctx, rg->sd);
  for (DevBuf* b : {&rg->src, &rg->y, &rg->part[0], &rg->part[1], &rg->words}) b->release();
  rg->ta.destroy();
  rg->ts.destroy();
  delete rg;
}

int sfmx_register_set_target(sfmx_ctx* ctx, sfmx_register* rg, const double* verts, int nv, const int32_t* faces, int m, int on_device,
                             const sfmx_register_params* p) {
  SFMX_REQUIRE(ctx, ctx && rg);
  rg->ready = false;  // every failure from here on leaves no target behind
  rg->us = rg->query_us = 0.0;
  SFMX_REQUIRE(ctx, sfmx_register_check_params(p) == SFMX_OK);
  sfmx_sdist_params sp;
  sp.d_max = p->d_max;
  sp.cell = p->cell;
  const int st = sfmx_sdist_set_target(ctx, rg->sd, verts, nv, faces, m, on_device, &sp);
  if (st != SFMX_OK) return st;
  rg->query_us = sfmx_sdist_last_us(rg->sd);
  rg->pivot[0] = rg->pivot[1] = rg->pivot[2] = 0.0;
  if (m > 0) {
    hipStream_t s = ctx->stream;
    const double* V = nullptr;
    const int32_t* F = nullptr;
    SFMX_REQUIRE(ctx, sfmx_sdist_device_state(rg->sd, &V, &F, nullptr, nullptr, nullptr) >= 0);
    unsigned long long keys[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
    unsigned long long* dk = rg->words.as<unsigned long long>();
    SFMX_HIP(ctx, hipMemcpyAsync(dk, keys, sizeof keys, hipMemcpyHostToDevice, s));
    SFMX_HIP(ctx, rg->ts.begin(ctx));
    k_rg_bbox<<<(unsigned)(((size_t)m + 255) / 256), 256, 0, s>>>(V, F, m, dk);
    SFMX_HIP(ctx, hipGetLastError());
    SFMX_HIP(ctx, rg->ts.end(ctx));
    SFMX_HIP(ctx, hipMemcpyAsync(keys, dk, sizeof keys, hipMemcpyDeviceToHost, s));
    SFMX_HIP(ctx, hipStreamSynchronize(s));
    rg->ts.us = 0.0;
    rg->ts.collect(ctx);
    rg->us = rg->ts.us;
    for (int a = 0; a < 3; a++) rg->pivot[a] = 0.5 * (rg_unkey(keys[a]) + rg_unkey(keys[3 + a]));
  }
  rg->m = m;
  rg->d_max = p->d_max;
  rg->cell = p->cell;
  rg->ready = true;
  return SFMX_OK;
}

int sfmx_register_pivot(const sfmx_register* rg, double* pivot3) {
  if (pivot3) pivot3[0] = pivot3[1] = pivot3[2] = 0.0;
  if (!rg || !rg->ready || !pivot3) return SFMX_ERR_INVALID;
  for (int a = 0; a < 3; a++) pivot3[a] = rg->pivot[a];
  return SFMX_OK;
}

int sfmx_register_system(sfmx_ctx* ctx, sfmx_register* rg, const double* points, int n, int on_device, const sfmx_register_transform* T,
                         const sfmx_register_params* p, double* sums, int32_t* n_used) {
  SFMX_REQUIRE(ctx, ctx && rg && sums && n_used && p);
  rg->us = rg->query_us = 0.0;
  int st = rg_check(ctx, rg, points, n, p);
  if (st != SFMX_OK) return st;
  const sfmx_register_transform cur = T ? *T : rg_identity();
  SFMX_REQUIRE(ctx, rg_transform_ok(&cur));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  const double* X = nullptr;
  st = rg_source(ctx, rg, points, n, on_device, &X);
  if (st != SFMX_OK) return st;
  return rg_eval(ctx, rg, X, n, cur, p, sums, n_used);  // synchronises: the caller may reuse its arrays
}

int sfmx_register_run(sfmx_ctx* ctx, sfmx_register* rg, const double* points, int n, int on_device, const sfmx_register_transform* init,
                      const sfmx_register_params* p, sfmx_register_result* out) {
  SFMX_REQUIRE(ctx, ctx && rg && out && p);
  rg->us = rg->query_us = 0.0;
  int st = rg_check(ctx, rg, points, n, p);
  if (st != SFMX_OK) return st;
  sfmx_register_transform cur = init ? *init : rg_identity();
  SFMX_REQUIRE(ctx, rg_transform_ok(&cur));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  const double* X = nullptr;
  st = rg_source(ctx, rg, points, n, on_device, &X);
  if (st != SFMX_OK) return st;
  sfmx_register_result res{};
  res.status = SFMX_REGISTER_MAX_ITERS;
  sfmx_register_transform good = cur;
  const int dim = p->with_scale ? 7 : 6;
  for (int it = 0; it < p->max_iters; it++) {
    double sums[RG_TERMS];
    int32_t nu = 0;
    st = rg_eval(ctx, rg, X, n, cur, p, sums, &nu);
    if (st != SFMX_OK) return st;
    res.iterations = it + 1;
    res.n[it] = nu;
    res.e[it] = sums[35];
    res.c[it] = sums[36];
    if (nu < p->min_points) {
      res.status = SFMX_REGISTER_TOO_FEW;
      cur = good;
      break;
    }
    double delta[7];
    const bool solved = rg_solve(sums, p->damping, dim, delta);
    const double g = solved ? 1.0 + delta[6] : 0.0;
    sfmx_register_transform next{};
    bool ok = solved && g > 0.0;
    if (ok) {
      next = rg_update(cur, rg->pivot, delta, g);
      ok = rg_transform_ok(&next);  // an update that overflowed, or whose scale underflowed, is no step
    }
    if (!ok) {
      res.status = SFMX_REGISTER_DEGENERATE;
      cur = good;
      break;
    }
    good = cur;
    cur = next;
    const double rot = sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]);
    const double tr = sqrt((delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5]);
    res.rot[it] = rot;
    res.trans[it] = tr;
    res.sigma[it] = delta[6];
    if (rot <= p->eps_rot && fabs(delta[6]) <= p->eps_scale && tr <= p->eps_trans * p->d_max) {
      res.status = SFMX_REGISTER_CONVERGED;
      break;
    }
  }
  res.T = cur;
  *out = res;
  return SFMX_OK;
}

int sfmx_register_apply(sfmx_ctx* ctx, sfmx_register* rg, const sfmx_register_transform* T, const double* points, int n, int on_device,
                        double* out) {
  SFMX_REQUIRE(ctx, ctx && rg && T);
  rg->us = rg->query_us = 0.0;
  int st = rg_check(ctx, rg, points, n, nullptr);
  if (st != SFMX_OK) return st;
  SFMX_REQUIRE(ctx, rg_transform_ok(T) && (n == 0 || out));
  if (n == 0) return SFMX_OK;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  const double* X = nullptr;
  st = rg_source(ctx, rg, points, n, on_device, &X);
  if (st != SFMX_OK) return st;
  hipStream_t s = ctx->stream;
  SFMX_HIP(ctx, rg->y.ensure((size_t)n * 24));
  int* used = rg_used(rg);
  int flag = 0;
  SFMX_HIP(ctx, hipMemsetAsync(used, 0, 8, s));
  SFMX_HIP(ctx, rg->ta.begin(ctx));
  k_rg_apply<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(X, 1, n, rg_arg(*T), rg->y.as<double>(), used + 1);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, rg->ta.end(ctx));
  SFMX_HIP(ctx, hipMemcpyAsync(&flag, used + 1, 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  SFMX_REQUIRE(ctx, flag == 0);  // a non-finite source coordinate
  SFMX_HIP(ctx, hipMemcpyAsync(out, rg->y.p, (size_t)n * 24, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  rg->ta.us = 0.0;
  rg->ta.collect(ctx);
  rg->us = rg->ta.us;
  return SFMX_OK;
}

double sfmx_register_last_us(const sfmx_register* rg) { return rg ? rg->us : 0.0; }
double sfmx_register_last_query_us(const sfmx_register* rg) { return rg ? rg->query_us : 0.0; }

}  // extern "C"
