// sfmx_raster_dev.h - the exact z-buffer as the device kernels build it: the camera, the projected vertex, the
// oriented edge functions of a face, the key of a fragment and its contest, and the three kernels that turn a mesh into a key
// image (project, faces, big).  Shared by raster.hip (one camera per run, with the face counts) and visib.hip (a batch of
// cameras per launch, the view being the grid's second dimension, without the counts), so that both evaluate the same
// expressions in the same order: visibility compares a vertex with the key image the renderer would have made.
//
// BATCH = false is the renderer's form: the camera by value, one set of buffers.  BATCH = true reads view blockIdx.y's camera and
// the place of its key image from slots[] (a wave-uniform index, so through the scalar cache) and finds its projected vertices,
// flags, list of big faces and counters at view * n, view * n, view * m and view * RS_NWORDS.
#pragma once
#include <cmath>

#include "sfmx_internal.h"

namespace {

// k_rs_faces<BATCH, SMALL>: a box of at most SMALL pixel centres is walked by the face's own thread; each user states its own
constexpr int RS_FACE_BLOCKS = 1024;  // blocks of k_rs_faces at most (per view)
constexpr int RS_BIG_BLOCKS = 512;    // blocks of k_rs_big (the renderer's; a batch uses fewer per view)

enum { RS_BEHIND = 0, RS_OUTSIDE, RS_DEGENERATE, RS_BACK, RS_CULLED, RS_DRAWN, RS_BIG, RS_FRAGMENTS, RS_NPART };
// device counters: four uint32 (below), then (the renderer only) the RS_NPART uint64 totals
enum { RS_FLAG = 0, RS_NBIG, RS_HITS, RS_BACKPX, RS_NWORDS };

struct RsCam {
  double R[9], c[3], f, cx, cy;
  int w, h;
};

// one view of a batch: its camera, where its key image lies in the batch's key slab and its image in the object's image slab
// (both in pixels)
struct RsSlot {
  RsCam cam;
  long long key_off, img_off;
};

struct RsVert {
  int U, V;  // image position in 1 / 256 pixel
  double r;  // 1 / depth
};

// the oriented edge functions of one face: e_i(x, y) = dx_i (256 y - Vj_i) - dy_i (256 x - Uj_i), covered iff e_i >= bias_i
struct RsFace {
  long long dx[3], dy[3], absA;
  int Uj[3], Vj[3], bias[3];
  bool back;
};

// what the renderer and the visibility stage accept as a camera (B is not used)
inline bool rs_view_ok(const sfmx_fusion_view* v) {
  if (!v || v->w < 1 || v->h < 1 || v->w > 4096 || (long long)v->w * v->h > (long long)SFMX_RASTER_MAX_PIXELS) return false;
  for (double x : v->R_rw)
    if (!std::isfinite(x)) return false;
  for (double x : v->c_left)
    if (!std::isfinite(x)) return false;
  return std::isfinite(v->f) && v->f > 0.0 && std::isfinite(v->cx) && std::isfinite(v->cy);
}

inline RsCam rs_cam(const sfmx_fusion_view* view) {
  RsCam cam{};
  std::memcpy(cam.R, view->R_rw, sizeof cam.R);
  std::memcpy(cam.c, view->c_left, sizeof cam.c);
  cam.f = view->f;
  cam.cx = view->cx;
  cam.cy = view->cy;
  cam.w = view->w;
  cam.h = view->h;
  return cam;
}

// the integer area of a face from its snapped corners: < 0 front-facing, > 0 back-facing (the image's y points down)
__device__ __forceinline__ long long rs_area(const RsVert* P) {
  return (long long)(P[1].U - P[0].U) * (long long)(P[2].V - P[0].V) - (long long)(P[1].V - P[0].V) * (long long)(P[2].U - P[0].U);
}

// false for a degenerate face (A == 0)
__device__ __forceinline__ bool rs_setup(const RsVert* P, RsFace& F) {
  const long long A = rs_area(P);
  if (A == 0) return false;
  const long long sg = A > 0 ? 1 : -1;
  F.back = A > 0;
  F.absA = A > 0 ? A : -A;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    F.dx[i] = sg * (long long)(P[k].U - P[j].U);
    F.dy[i] = sg * (long long)(P[k].V - P[j].V);
    F.Uj[i] = P[j].U;
    F.Vj[i] = P[j].V;
    F.bias[i] = (F.dy[i] < 0 || (F.dy[i] == 0 && F.dx[i] > 0)) ? 0 : 1;  // the top-left rule: such an edge owns its points
  }
  return true;
}

__device__ __forceinline__ long long rs_edge(const RsFace& F, int i, int x, int y) {
  return F.dx[i] * (256ll * y - F.Vj[i]) - F.dy[i] * (256ll * x - F.Uj[i]);
}

// the pixel centres a face can cover: ceiling and floor of the snapped extremes, clamped to the image (empty when x1 < x0 or
// y1 < y0).  A covered centre has all three e_i >= 0, so it lies in the closed triangle and hence in this box.
__device__ __forceinline__ void rs_box(const RsVert* P, int w, int h, int& x0, int& y0, int& x1, int& y1) {
  const int Ulo = min(P[0].U, min(P[1].U, P[2].U)), Uhi = max(P[0].U, max(P[1].U, P[2].U));
  const int Vlo = min(P[0].V, min(P[1].V, P[2].V)), Vhi = max(P[0].V, max(P[1].V, P[2].V));
  x0 = max((Ulo + 255) >> 8, 0);
  y0 = max((Vlo + 255) >> 8, 0);
  x1 = min(Uhi >> 8, w - 1);
  y1 = min(Vhi >> 8, h - 1);
}

__device__ __forceinline__ double rs_s(long long e0, long long e1, long long e2, const RsVert* P) {
  return ((double)e0 * P[0].r + (double)e1 * P[1].r) + (double)e2 * P[2].r;
}

__device__ __forceinline__ unsigned long long rs_key(double depth, int face) {
  return ((unsigned long long)__float_as_uint((float)depth) << 32) | (unsigned long long)(unsigned)face;
}

__device__ __forceinline__ void rs_contest(unsigned long long* slot, unsigned long long key) {
  if (key < *(volatile unsigned long long*)slot) atomicMin(slot, key);
}

// camera-frame depth q2 of a vertex, with p = X - c (k_rs_project's expressions; the visibility test evaluates them again)
__device__ __forceinline__ double rs_depth(const RsCam& cam, double X0, double X1, double X2, double& p0, double& p1, double& p2) {
  p0 = X0 - cam.c[0];
  p1 = X1 - cam.c[1];
  p2 = X2 - cam.c[2];
  return (cam.R[6] * p0 + cam.R[7] * p1) + cam.R[8] * p2;
}

// the block's sums of v[] into out[0 .. RS_NPART)
__device__ __forceinline__ void rs_block_sums(unsigned long long (&v)[RS_NPART], unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh[4][RS_NPART];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < RS_NPART; k++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < RS_NPART; k++) sh[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < RS_NPART) out[threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

template <bool BATCH>
__global__ __launch_bounds__(256) void k_rs_project(const double* __restrict__ verts, int n, RsCam cam, const RsSlot* __restrict__ slots,
                                                    double z_min, RsVert* __restrict__ pv, uint8_t* __restrict__ fl) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  if (BATCH) {
    cam = slots[blockIdx.y].cam;
    pv += (size_t)blockIdx.y * (size_t)n;
    fl += (size_t)blockIdx.y * (size_t)n;
  }
  double p0, p1, p2;
  const double q2 = rs_depth(cam, verts[3 * (size_t)v], verts[3 * (size_t)v + 1], verts[3 * (size_t)v + 2], p0, p1, p2);
  const double q0 = (cam.R[0] * p0 + cam.R[1] * p1) + cam.R[2] * p2;
  const double q1 = (cam.R[3] * p0 + cam.R[4] * p1) + cam.R[5] * p2;
  const bool near = q2 >= z_min;  // false for a NaN
  RsVert o{0, 0, 0.0};
  bool inband = false;
  if (near) {
    const double u = (cam.f * q0) / q2 + cam.cx, vv = (cam.f * q1) / q2 + cam.cy;
    inband = fabs(u) <= 16384.0 && fabs(vv) <= 16384.0;
    if (inband) {
      o.U = (int)(long long)floor(u * 256.0 + 0.5);
      o.V = (int)(long long)floor(vv * 256.0 + 0.5);
      o.r = 1.0 / q2;
    }
  }
  pv[v] = o;
  fl[v] = (uint8_t)((near ? 1 : 0) | (inband ? 2 : 0));
}

template <bool BATCH, int SMALL>
__global__ __launch_bounds__(256) void k_rs_faces(const int* __restrict__ faces, int m, int n, const RsVert* __restrict__ pv,
                                                  const uint8_t* __restrict__ fl, int w, int h, int cull, unsigned long long* keys,
                                                  int* __restrict__ big, unsigned* counters, unsigned long long* __restrict__ parts,
                                                  const RsSlot* __restrict__ slots) {
  const int lane = threadIdx.x & 63;
  if (BATCH) {
    const RsSlot& S = slots[blockIdx.y];
    w = S.cam.w;
    h = S.cam.h;
    keys += S.key_off;
    pv += (size_t)blockIdx.y * (size_t)n;
    fl += (size_t)blockIdx.y * (size_t)n;
    big += (size_t)blockIdx.y * (size_t)m;
    counters += (size_t)blockIdx.y * RS_NWORDS;
  }
  unsigned long long cnt[RS_NPART] = {};
  for (int base = blockIdx.x * 256; base < m; base += gridDim.x * 256) {  // uniform over the block: the ballot below needs whole waves
    const int f = base + threadIdx.x;
    bool is_big = false;
    if (f < m) {
      const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
      if ((unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n || (unsigned)c >= (unsigned)n) {
        atomicOr(&counters[RS_FLAG], 1u);  // the call fails; nothing is read through the index
      } else {
        const unsigned fa = fl[a], fb = fl[b], fc = fl[c], all = fa & fb & fc;
        if (!(all & 1u)) {
          cnt[RS_BEHIND]++;
        } else if (!(all & 2u)) {
          cnt[RS_OUTSIDE]++;
        } else {
          const RsVert P[3] = {pv[a], pv[b], pv[c]};
          RsFace F;
          if (!rs_setup(P, F)) {
            cnt[RS_DEGENERATE]++;
          } else {
            if (F.back) cnt[RS_BACK]++;
            if ((cull == 1 && F.back) || (cull == 2 && !F.back)) {
              cnt[RS_CULLED]++;
            } else {
              int x0, y0, x1, y1;
              rs_box(P, w, h, x0, y0, x1, y1);
              if (x0 <= x1 && y0 <= y1) {
                if ((long long)(x1 - x0 + 1) * (y1 - y0 + 1) > SMALL) {
                  is_big = true;
                  cnt[RS_BIG]++;
                } else {
                  unsigned frags = 0;
                  long long row[3], step[3];
#pragma unroll
                  for (int i = 0; i < 3; i++) {
                    row[i] = rs_edge(F, i, x0, y0) - F.bias[i];
                    step[i] = -256ll * F.dy[i];
                  }
                  for (int y = y0; y <= y1; y++) {
                    long long e0 = row[0], e1 = row[1], e2 = row[2];
                    for (int x = x0; x <= x1; x++) {
                      if ((e0 | e1 | e2) >= 0) {  // all three e_i - bias_i >= 0
                        const double s = rs_s(e0 + F.bias[0], e1 + F.bias[1], e2 + F.bias[2], P);
                        rs_contest(&keys[(size_t)y * w + x], rs_key((double)F.absA / s, f));
                        frags++;
                      }
                      e0 += step[0];
                      e1 += step[1];
                      e2 += step[2];
                    }
#pragma unroll
                    for (int i = 0; i < 3; i++) row[i] += 256ll * F.dx[i];
                  }
                  cnt[RS_FRAGMENTS] += frags;
                  if (frags) cnt[RS_DRAWN]++;
                }
              }
            }
          }
        }
      }
    }
    const unsigned long long bm = __ballot(is_big);
    if (bm) {
      const int first = __ffsll((long long)bm) - 1;
      unsigned at = 0;
      if (lane == first) at = atomicAdd(&counters[RS_NBIG], (unsigned)__popcll(bm));
      at = __shfl(at, first, 64);
      if (is_big) big[at + __popcll(bm & ((1ull << lane) - 1ull))] = f;
    }
  }
  if (!BATCH) rs_block_sums(cnt, parts + (size_t)blockIdx.x * RS_NPART);
}

template <bool BATCH>
__global__ __launch_bounds__(256) void k_rs_big(const int* __restrict__ faces, int m, int n, const RsVert* __restrict__ pv, int w, int h,
                                                unsigned long long* keys, const int* __restrict__ big,
                                                const unsigned* __restrict__ counters, unsigned long long* __restrict__ parts,
                                                const RsSlot* __restrict__ slots) {
  __shared__ int drawn;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (BATCH) {
    const RsSlot& S = slots[blockIdx.y];
    w = S.cam.w;
    h = S.cam.h;
    keys += S.key_off;
    pv += (size_t)blockIdx.y * (size_t)n;
    big += (size_t)blockIdx.y * (size_t)m;
    counters += (size_t)blockIdx.y * RS_NWORDS;
  }
  const int nbig = (int)counters[RS_NBIG];
  unsigned long long cnt[RS_NPART] = {};
  for (int q = blockIdx.x; q < nbig; q += gridDim.x) {  // uniform over the block
    const int f = big[q];
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];  // checked by k_rs_faces
    const RsVert P[3] = {pv[a], pv[b], pv[c]};
    RsFace F;
    rs_setup(P, F);
    int x0, y0, x1, y1;
    rs_box(P, w, h, x0, y0, x1, y1);
    const int tw = (x1 - x0 + 8) >> 3, th = (y1 - y0 + 8) >> 3;
    if (threadIdx.x == 0) drawn = 0;
    __syncthreads();
    unsigned frags = 0;
    for (int t = wave; t < tw * th; t += 4) {
      const int tx = x0 + (t % tw) * 8, ty = y0 + (t / tw) * 8;
      // largest e_i - bias_i over the tile's 8 x 8 centres: the value at (tx, ty) plus the positive steps
      bool none = false;
      long long e[3];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const long long e00 = rs_edge(F, i, tx, ty) - F.bias[i];
        const long long sx = -256ll * F.dy[i], sy = 256ll * F.dx[i];
        none |= e00 + 7 * (sx > 0 ? sx : 0) + 7 * (sy > 0 ? sy : 0) < 0;
        e[i] = e00 + (lane & 7) * sx + (lane >> 3) * sy;
      }
      if (none) continue;
      const int x = tx + (lane & 7), y = ty + (lane >> 3);
      const bool in = x <= x1 && y <= y1 && (e[0] | e[1] | e[2]) >= 0;
      if (in) {
        const double s = rs_s(e[0] + F.bias[0], e[1] + F.bias[1], e[2] + F.bias[2], P);
        rs_contest(&keys[(size_t)y * w + x], rs_key((double)F.absA / s, f));
      }
      frags += (unsigned)__popcll(__ballot(in));
    }
    if (lane == 0) {
      cnt[RS_FRAGMENTS] += frags;
      if (frags) drawn = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0 && drawn) cnt[RS_DRAWN]++;
  }
  if (!BATCH) rs_block_sums(cnt, parts + (size_t)blockIdx.x * RS_NPART);
}

}  // namespace
