// stereo.hip — keyframe-pair dense disparity: rectification, census, 4-path SGM, winner selection, speckle filter.
//
// Exactness: the remap is IEEE double in one fixed expression order (built with -ffp-contract=off, as everything here);
// every later stage is integer arithmetic, and the four path sums are integers, so neither the order of the passes nor
// the schedule inside a pass can change S.  tests/stereo_ref.py restates every stage in NumPy; the tests compare bits.
//
// Kernel layout:
//   k_st_rectify   one thread per rectified pixel and view
//   k_st_census    one thread per pixel and view; bit 63 of the code marks an invalid window
//   k_st_path<K>   one wave64 per image line of one path direction; lane l holds disparities l*K .. l*K+K-1 in registers,
//                  d-1 / d+1 across lanes come from one lane shift each, m_q from a wave min; the Hamming cost is formed on
//                  the fly from the two census images (no cost volume).  S is [h][w][D] (D-contiguous), so horizontal and
//                  vertical passes both read and write whole per-pixel rows.  The first pass stores, the other three add.
//   k_st_select<K> one block per image row: per pixel a wave finds the winner (packed (S << 16) | d min), the uniqueness
//                  test (ballot) and the sub-pixel step; the right view's winners come from the same S rows through LDS
//                  atomicMin on the packed key at x - d; then the left-right check.
//   k_st_uf_*      speckle filter: union-find over 4-connected valid pixels (link to the smaller root by CAS), flatten,
//                  component sizes by atomicAdd, invalidate the small ones.  A set partition: any schedule, same output.
#include "sfmx_internal.h"

namespace {

constexpr int kInf = 1 << 20;
constexpr uint64_t kBad = 1ull << 63;

struct H9 { double a[9]; };

struct StereoDims {
  int w, h, D, nbits, p1, p2;
};

__global__ __launch_bounds__(256) void k_st_rectify(const uint8_t* __restrict__ img_l, const uint8_t* __restrict__ img_r, H9 Hl, H9 Hr,
                                                    int w, int h, uint8_t* __restrict__ rect, uint8_t* __restrict__ valid) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, v = blockIdx.z;
  if (x >= w) return;
  const uint8_t* img = v ? img_r : img_l;
  const double* H = v ? Hr.a : Hl.a;
  const double xd = (double)x, yd = (double)y;
  const double den = H[6] * xd + H[7] * yd + H[8];
  const double sx = (H[0] * xd + H[1] * yd + H[2]) / den;
  const double sy = (H[3] * xd + H[4] * yd + H[5]) / den;
  const size_t o = (size_t)v * w * h + (size_t)y * w + x;
  if (!(sx >= 0.0 && sx <= (double)(w - 1) && sy >= 0.0 && sy <= (double)(h - 1))) {
    rect[o] = 0;
    valid[o] = 0;
    return;
  }
  const double fx = floor(sx), fy = floor(sy);
  const int x0 = (int)fx, y0 = (int)fy;
  const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
  const double ax = sx - fx, ay = sy - fy;
  const double i00 = img[(size_t)y0 * w + x0], i01 = img[(size_t)y0 * w + x1];
  const double i10 = img[(size_t)y1 * w + x0], i11 = img[(size_t)y1 * w + x1];
  const double val = (1.0 - ay) * ((1.0 - ax) * i00 + ax * i01) + ay * ((1.0 - ax) * i10 + ax * i11);
  rect[o] = (uint8_t)floor(val + 0.5);
  valid[o] = 1;
}

__global__ __launch_bounds__(256) void k_st_census(const uint8_t* __restrict__ rect, const uint8_t* __restrict__ valid, int w, int h, int r,
                                                   uint64_t* __restrict__ cen) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, v = blockIdx.z;
  if (x >= w) return;
  const size_t plane = (size_t)v * w * h;
  uint64_t code = 0;
  if (x < r || x >= w - r || y < r || y >= h - r) {
    code = kBad;
  } else {
    const uint8_t* I = rect + plane;
    const uint8_t* V = valid + plane;
    const int c = I[(size_t)y * w + x];
    int bit = 0;
    bool bad = false;
    for (int dy = -r; dy <= r; dy++)
      for (int dx = -r; dx <= r; dx++) {
        const size_t o = (size_t)(y + dy) * w + (x + dx);
        bad |= V[o] == 0;
        if (dy == 0 && dx == 0) continue;
        code |= (uint64_t)(I[o] < c) << bit;
        bit++;
      }
    if (bad) code = kBad;
  }
  cen[plane + (size_t)y * w + x] = code;
}

__device__ __forceinline__ int st_cost(uint64_t cl, const uint64_t* __restrict__ crow, int x, int d, int nbits) {
  const int xr = x - d;
  if (xr < 0 || (cl & kBad)) return nbits;
  const uint64_t cr = crow[xr];
  if (cr & kBad) return nbits;
  return __popcll(cl ^ cr);
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// one path direction: dir 0 left->right, 1 right->left, 2 top->bottom, 3 bottom->top; blockIdx.x = line
template <int K>
__global__ __launch_bounds__(64) void k_st_path(const uint64_t* __restrict__ cen_l, const uint64_t* __restrict__ cen_r,
                                                uint16_t* __restrict__ S, StereoDims g, int dir, int accumulate) {
  const int lane = threadIdx.x, line = blockIdx.x;
  const bool horiz = dir < 2;
  const int n = horiz ? g.w : g.h;
  const int D = g.D;
  auto px = [&](int i, int& x, int& y) {
    const int s = (dir & 1) ? n - 1 - i : i;
    x = horiz ? s : line;
    y = horiz ? line : s;
  };
  int c[K], cn[K], Lp[K];
  uint16_t s[K], sn[K];
  auto load = [&](int i, int* cc, uint16_t* ss) {
    int x, y;
    px(i, x, y);
    const uint64_t cl = cen_l[(size_t)y * g.w + x];
    const uint64_t* crow = cen_r + (size_t)y * g.w;
    const size_t base = ((size_t)y * g.w + x) * D;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int d = lane * K + k;
      cc[k] = d < D ? st_cost(cl, crow, x, d, g.nbits) : kInf;
      ss[k] = (accumulate && d < D) ? S[base + d] : (uint16_t)0;
    }
  };
  load(0, c, s);
  int m = kInf;
  for (int i = 0; i < n; i++) {
    if (i + 1 < n) load(i + 1, cn, sn);
    int L[K];
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < K; k++) L[k] = c[k];
    } else {
      int lo = __shfl_up(Lp[K - 1], 1, 64);
      int hi = __shfl_down(Lp[0], 1, 64);
      if (lane == 0) lo = kInf;
      if (lane == 63) hi = kInf;
#pragma unroll
      for (int k = 0; k < K; k++) {
        const int dm = k > 0 ? Lp[k - 1] : lo;
        const int dp = k < K - 1 ? Lp[k + 1] : hi;
        const int best = min(min(Lp[k], min(dm, dp) + g.p1), m + g.p2);
        L[k] = (lane * K + k) < D ? c[k] + best - m : kInf;
      }
    }
    int lm = L[0];
#pragma unroll
    for (int k = 1; k < K; k++) lm = min(lm, L[k]);
    m = wave_min(lm);
    int x, y;
    px(i, x, y);
    const size_t base = ((size_t)y * g.w + x) * D;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int d = lane * K + k;
      if (d < D) S[base + d] = (uint16_t)(s[k] + L[k]);
      Lp[k] = L[k];
      c[k] = cn[k];
      s[k] = sn[k];
    }
  }
}

// winner, uniqueness, sub-pixel, right-view winners (LDS), left-right check; one block (4 waves) per row
template <int K>
__global__ __launch_bounds__(256) void k_st_select(const uint16_t* __restrict__ S, const uint64_t* __restrict__ cen_l, StereoDims g,
                                                   int uniqueness, int lr_max_diff, int16_t* __restrict__ d16_out) {
  extern __shared__ unsigned char st_lds[];
  const int w = g.w, D = g.D, y = blockIdx.x;
  unsigned* rkey = reinterpret_cast<unsigned*>(st_lds);  // [w] packed (S << 16) | d of the right view
  int* dstar = reinterpret_cast<int*>(rkey + w);         // [w] left winner, -1 = invalid
  int* dsub = dstar + w;                                 // [w] 16 * disparity after the sub-pixel step
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int x = threadIdx.x; x < w; x += 256) rkey[x] = 0xFFFFFFFFu;
  __syncthreads();
  for (int x = wave; x < w; x += 4) {
    const size_t base = ((size_t)y * w + x) * D;
    unsigned sv[K];
    unsigned key = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int d = lane * K + k;
      sv[k] = d < D ? (unsigned)S[base + d] : 0xFFFFu;
      if (d < D) {
        const unsigned kk = (sv[k] << 16) | (unsigned)d;
        key = min(key, kk);
        if (x - d >= 0) atomicMin(&rkey[x - d], kk);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o, 64));
    const int ds = (int)(key & 0xFFFFu);
    const int smin = (int)(key >> 16);
    bool reject = false;
    if (uniqueness > 0) {
      bool any = false;
#pragma unroll
      for (int k = 0; k < K; k++) {
        const int d = lane * K + k;
        if (d < D && abs(d - ds) > 1 && (int)sv[k] * (100 - uniqueness) < smin * 100) any = true;
      }
      reject = __any(any);
    }
    if (lane == 0) {
      int v = 16 * ds;
      if (ds > 0 && ds < D - 1) {
        const int sm = S[base + ds - 1], sp = S[base + ds + 1];
        const int den2 = max(sm + sp - 2 * smin, 1);
        v += ((sm - sp) * 16 + den2) / (den2 * 2);
      }
      const bool bad = reject || (cen_l[(size_t)y * w + x] & kBad) != 0;
      dstar[x] = bad ? -1 : ds;
      dsub[x] = v;
    }
  }
  __syncthreads();
  for (int x = threadIdx.x; x < w; x += 256) {
    const int ds = dstar[x];
    bool ok = ds >= 0;
    if (ok && lr_max_diff >= 0 && x - ds >= 0) ok = abs((int)(rkey[x - ds] & 0xFFFFu) - ds) <= lr_max_diff;
    d16_out[(size_t)y * w + x] = ok ? (int16_t)dsub[x] : (int16_t)-16;
  }
}

__device__ __forceinline__ int uf_find(int* lab, int x) {
  int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) {
    x = p;
    p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return x;
}

__device__ __forceinline__ void uf_unite(int* lab, int a, int b) {
  while (true) {
    a = uf_find(lab, a);
    b = uf_find(lab, b);
    if (a == b) return;
    const int lo = min(a, b), hi = max(a, b);
    if (atomicCAS(&lab[hi], hi, lo) == hi) return;  // hi was still a root: linked
  }
}

__global__ __launch_bounds__(256) void k_st_uf_init(const int16_t* __restrict__ d16, int n, int* __restrict__ lab, int* __restrict__ size) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  lab[p] = d16[p] != -16 ? p : -1;
  size[p] = 0;
}

__global__ __launch_bounds__(256) void k_st_uf_merge(const int16_t* __restrict__ d16, int w, int h, int lim, int* lab) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= w * h) return;
  const int a = d16[p];
  if (a == -16) return;
  const int x = p % w, y = p / w;
  if (x + 1 < w) {
    const int b = d16[p + 1];
    if (b != -16 && abs(a - b) <= lim) uf_unite(lab, p, p + 1);
  }
  if (y + 1 < h) {
    const int b = d16[p + w];
    if (b != -16 && abs(a - b) <= lim) uf_unite(lab, p, p + w);
  }
}

__global__ __launch_bounds__(256) void k_st_uf_count(int n, int* lab, int* __restrict__ size) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n || lab[p] < 0) return;
  const int r = uf_find(lab, p);
  atomicAdd(&size[r], 1);
}

__global__ __launch_bounds__(256) void k_st_uf_apply(int n, int* lab, const int* __restrict__ size, int window, int16_t* __restrict__ d16) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n || lab[p] < 0) return;
  if (size[uf_find(lab, p)] < window) d16[p] = -16;
}

}  // namespace

struct sfmx_stereo {
  int w = 0, h = 0, K = 1;
  sfmx_stereo_params p{};
  void* slab = nullptr;
  uint8_t *img = nullptr, *rect = nullptr, *valid = nullptr;
  uint64_t* cen = nullptr;
  uint16_t* S = nullptr;
  int16_t* d16 = nullptr;
  int *lab = nullptr, *size = nullptr;
  bool d16_current = true;  // false after sfmx_stereo_rectify: the map no longer belongs to the rectified images
  StageTimer t;
};

// after a rectification alone there is no map: NULL and a size of 0 x 0, which every _add_stereo_view entry that takes the map
// refuses as a view of another size
const int16_t* sfmx_stereo_device_disp16(const sfmx_stereo* st, int* w, int* h) {
  *w = st->d16_current ? st->w : 0;
  *h = st->d16_current ? st->h : 0;
  return st->d16_current ? st->d16 : nullptr;
}

const uint8_t* sfmx_stereo_device_rect_left(const sfmx_stereo* st, int* w, int* h) {
  *w = st->w;
  *h = st->h;
  return st->rect;  // plane 0 of u8 [2][h][w]
}

extern "C" {

void sfmx_stereo_default_params(sfmx_stereo_params* p) {
  if (p) *p = sfmx_stereo_params{128, 5, 8, 96, 10, 1, 100, 2};
}

int sfmx_stereo_check_params(int w, int h, const sfmx_stereo_params* p) {
  // w <= 4096: k_st_select keeps 12 bytes per column of a row in LDS
  if (!p || w <= 0 || h <= 0 || w > 4096 || (long long)w * h >= (1ll << 30)) return SFMX_ERR_INVALID;
  if (p->num_disparities < 16 || p->num_disparities > 256 || p->num_disparities % 16 != 0) return SFMX_ERR_INVALID;
  if (p->census != 3 && p->census != 5 && p->census != 7) return SFMX_ERR_INVALID;
  if (!(0 < p->p1 && p->p1 < p->p2 && p->p2 <= 2048)) return SFMX_ERR_INVALID;
  if (p->uniqueness < 0 || p->uniqueness > 100 || p->speckle_window < 0 || p->speckle_range < 0) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_stereo_create(sfmx_ctx* ctx, int w, int h, const sfmx_stereo_params* p, sfmx_stereo** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_REQUIRE(ctx, sfmx_stereo_check_params(w, h, p) == SFMX_OK);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* st = new sfmx_stereo;
  st->w = w;
  st->h = h;
  st->p = *p;
  st->K = (p->num_disparities + 63) / 64;
  const size_t n = (size_t)w * h, D = (size_t)p->num_disparities;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_img = 0, o_rect = o_img + up(2 * n), o_valid = o_rect + up(2 * n), o_cen = o_valid + up(2 * n),
               o_S = o_cen + up(2 * n * 8), o_d16 = o_S + up(n * D * 2), o_lab = o_d16 + up(n * 2), o_size = o_lab + up(n * 4),
               total = o_size + up(n * 4);
  hipError_t e = hipMalloc(&st->slab, total);
  if (e == hipSuccess) e = st->t.create();
  if (e != hipSuccess) {
    sfmx_stereo_destroy(ctx, st);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_stereo_create", e);
  }
  auto* b = static_cast<uint8_t*>(st->slab);
  st->img = b + o_img;
  st->rect = b + o_rect;
  st->valid = b + o_valid;
  st->cen = reinterpret_cast<uint64_t*>(b + o_cen);
  st->S = reinterpret_cast<uint16_t*>(b + o_S);
  st->d16 = reinterpret_cast<int16_t*>(b + o_d16);
  st->lab = reinterpret_cast<int*>(b + o_lab);
  st->size = reinterpret_cast<int*>(b + o_size);
  *out = st;
  return SFMX_OK;
}

void sfmx_stereo_destroy(sfmx_ctx* ctx, sfmx_stereo* st) {
  if (!st) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  if (st->slab) (void)hipFree(st->slab);
  st->t.destroy();
  delete st;
}

double sfmx_stereo_last_us(const sfmx_stereo* st) { return st ? st->t.us : 0.0; }

int sfmx_stereo_disparity(sfmx_ctx* ctx, sfmx_stereo* st, const uint8_t* img_l, const uint8_t* img_r, int on_device, const double* H_l,
                          const double* H_r, int16_t* disp16_out, uint8_t* rect_out, uint16_t* sum_out) {
  SFMX_REQUIRE(ctx, ctx && st && img_l && img_r && H_l && H_r && disp16_out);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  st->d16_current = true;
  const int w = st->w, h = st->h, D = st->p.num_disparities;
  const size_t n = (size_t)w * h;
  hipStream_t s = ctx->stream;
  const uint8_t *il = img_l, *ir = img_r;
  if (!on_device) {
    SFMX_HIP(ctx, hipMemcpyAsync(st->img, img_l, n, hipMemcpyHostToDevice, s));
    SFMX_HIP(ctx, hipMemcpyAsync(st->img + n, img_r, n, hipMemcpyHostToDevice, s));
    il = st->img;
    ir = st->img + n;
  }
  H9 hl, hr;
  std::memcpy(hl.a, H_l, sizeof hl.a);
  std::memcpy(hr.a, H_r, sizeof hr.a);
  const StereoDims g{w, h, D, st->p.census * st->p.census - 1, st->p.p1, st->p.p2};
  SFMX_HIP(ctx, st->t.begin(ctx));
  const dim3 pix((unsigned)((w + 255) / 256), (unsigned)h, 2u);
  k_st_rectify<<<pix, 256, 0, s>>>(il, ir, hl, hr, w, h, st->rect, st->valid);
  k_st_census<<<pix, 256, 0, s>>>(st->rect, st->valid, w, h, st->p.census / 2, st->cen);
  const uint64_t *cl = st->cen, *cr = st->cen + n;
  for (int dir = 0; dir < 4; dir++) {
    const unsigned lines = (unsigned)(dir < 2 ? h : w);
    switch (st->K) {
      case 1: k_st_path<1><<<lines, 64, 0, s>>>(cl, cr, st->S, g, dir, dir > 0); break;
      case 2: k_st_path<2><<<lines, 64, 0, s>>>(cl, cr, st->S, g, dir, dir > 0); break;
      case 3: k_st_path<3><<<lines, 64, 0, s>>>(cl, cr, st->S, g, dir, dir > 0); break;
      default: k_st_path<4><<<lines, 64, 0, s>>>(cl, cr, st->S, g, dir, dir > 0); break;
    }
  }
  const size_t lds = (size_t)w * 12;
  switch (st->K) {
    case 1: k_st_select<1><<<h, 256, lds, s>>>(st->S, cl, g, st->p.uniqueness, st->p.lr_max_diff, st->d16); break;
    case 2: k_st_select<2><<<h, 256, lds, s>>>(st->S, cl, g, st->p.uniqueness, st->p.lr_max_diff, st->d16); break;
    case 3: k_st_select<3><<<h, 256, lds, s>>>(st->S, cl, g, st->p.uniqueness, st->p.lr_max_diff, st->d16); break;
    default: k_st_select<4><<<h, 256, lds, s>>>(st->S, cl, g, st->p.uniqueness, st->p.lr_max_diff, st->d16); break;
  }
  if (st->p.speckle_window > 0) {
    const unsigned nb = (unsigned)((n + 255) / 256);
    k_st_uf_init<<<nb, 256, 0, s>>>(st->d16, (int)n, st->lab, st->size);
    k_st_uf_merge<<<nb, 256, 0, s>>>(st->d16, w, h, 16 * st->p.speckle_range, st->lab);
    k_st_uf_count<<<nb, 256, 0, s>>>((int)n, st->lab, st->size);
    k_st_uf_apply<<<nb, 256, 0, s>>>((int)n, st->lab, st->size, st->p.speckle_window, st->d16);
  }
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, st->t.end(ctx));
  SFMX_HIP(ctx, hipMemcpyAsync(disp16_out, st->d16, n * 2, hipMemcpyDeviceToHost, s));
  if (rect_out) SFMX_HIP(ctx, hipMemcpyAsync(rect_out, st->rect, 2 * n, hipMemcpyDeviceToHost, s));
  if (sum_out) SFMX_HIP(ctx, hipMemcpyAsync(sum_out, st->S, n * (size_t)D * 2, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  st->t.us = 0.0;
  st->t.collect(ctx);
  return SFMX_OK;
}

int sfmx_stereo_rectify(sfmx_ctx* ctx, sfmx_stereo* st, const uint8_t* img_l, const uint8_t* img_r, int on_device, const double* H_l,
                        const double* H_r) {
  SFMX_REQUIRE(ctx, ctx && st && img_l && img_r && H_l && H_r);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  st->d16_current = false;
  const int w = st->w, h = st->h;
  const size_t n = (size_t)w * h;
  hipStream_t s = ctx->stream;
  const uint8_t *il = img_l, *ir = img_r;
  if (!on_device) {
    SFMX_HIP(ctx, hipMemcpyAsync(st->img, img_l, n, hipMemcpyHostToDevice, s));
    SFMX_HIP(ctx, hipMemcpyAsync(st->img + n, img_r, n, hipMemcpyHostToDevice, s));
    il = st->img;
    ir = st->img + n;
  }
  H9 hl, hr;
  std::memcpy(hl.a, H_l, sizeof hl.a);
  std::memcpy(hr.a, H_r, sizeof hr.a);
  SFMX_HIP(ctx, st->t.begin(ctx));
  k_st_rectify<<<dim3((unsigned)((w + 255) / 256), (unsigned)h, 2u), 256, 0, s>>>(il, ir, hl, hr, w, h, st->rect, st->valid);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, st->t.end(ctx));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  st->t.us = 0.0;
  st->t.collect(ctx);
  return SFMX_OK;
}

}  // extern "C"
