// sfmx_raster_dev.h - the exact z-buffer as the device kernels build it: the camera, the projected vertex, the
// oriented edge functions of a face, the key of a fragment and its contest, and the three kernels that turn a mesh into a key
// image (project, faces, big).  Shared by raster.hip (one camera per run, with the face counts) and, through RsViewSet, by
// visib.hip, texture.hip and level.hip (a batch of cameras per launch, the view being the grid's second dimension, without the
// counts), so that all evaluate the same expressions in the same order: visibility and texturing compare a vertex with the key
// image the renderer would have made, through the one test rs_vertex_sees.
//
// BATCH = false is the renderer's form: the camera by value, one set of buffers.  BATCH = true reads view blockIdx.y's camera and
// the place of its key image from slots[] (a wave-uniform index, so through the scalar cache) and finds its projected vertices,
// flags, list of big faces and counters at view * n, view * n, view * m and view * RS_NWORDS.
//
// RsViewSet is the multi-view z-buffer as one object: the ordered list of cameras with an optional u8 image each, the batches
// of a run and the launch group that builds one batch's key images.
#pragma once
#include <cmath>
#include <vector>

#include "sfmx_internal.h"
#include "sfmx_mesh_dev.h"

namespace {

// k_rs_faces<BATCH, SMALL>: a box of at most SMALL pixel centres is walked by the face's own thread; each user states its own
constexpr int RS_FACE_BLOCKS = 1024;  // blocks of k_rs_faces at most (per view)
constexpr int RS_BIG_BLOCKS = 512;    // blocks of k_rs_big (the renderer's; a batch uses fewer per view)
// a batch of views (RsViewSet); they change the speed only
constexpr size_t RS_BATCH_BUDGET = (size_t)256 << 20;  // bytes a batch's key slab, per-(view, vertex) records and big-face lists may take
constexpr int RS_MAX_BATCH = 64;                       // one bit per view in a vertex's mask
constexpr int RS_BATCH_BIG_BLOCKS = 64;                // blocks of k_rs_big per view
constexpr int RS_BATCH_SMALL = 64;                     // as raster.hip's RS_SMALL: a larger box of pixel centres goes to k_rs_big

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

// What view S of a batch sees of vertex i (X0, X1, X2), whose projection and flags lie at `at` = view * n + i: the vertex is off
// the image (not inband, or its snapped pixel outside), occluded (deeper than the key there by more than depth_tol) or visible;
// then px is its pixel and p = X - c.  One double addition and one comparison against the key.
enum { RS_SEES_OFF = 0, RS_SEES_OCCLUDED, RS_SEES_VISIBLE };
struct RsSight {
  int state;
  long long px;
  double p0, p1, p2;
};
__device__ __forceinline__ RsSight rs_vertex_sees(const RsSlot& S, const RsVert* __restrict__ pv, const uint8_t* __restrict__ fl,
                                                  const unsigned long long* __restrict__ keys, size_t at, double X0, double X1,
                                                  double X2, double depth_tol) {
  RsSight r{RS_SEES_OFF, 0, 0.0, 0.0, 0.0};
  if (!(fl[at] & 2u)) return r;  // not inband
  const RsVert P = pv[at];
  const int x = (P.U + 128) >> 8, y = (P.V + 128) >> 8;
  if (x < 0 || x >= S.cam.w || y < 0 || y >= S.cam.h) return r;
  r.px = (long long)y * S.cam.w + x;
  const unsigned long long key = keys[S.key_off + r.px];
  const double q2 = rs_depth(S.cam, X0, X1, X2, r.p0, r.p1, r.p2);
  bool visible = true;
  if (key != ~0ull) {
    const double D = (double)__uint_as_float((unsigned)(key >> 32));
    visible = q2 <= D + depth_tol;  // false for a NaN
  }
  r.state = visible ? RS_SEES_VISIBLE : RS_SEES_OCCLUDED;
  return r;
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
      int a, b, c;
      if (!mesh_face(faces, f, n, a, b, c)) {
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
  if (!BATCH) {
    const unsigned long long sum = sfmx_block_sums(cnt);
    if (threadIdx.x < RS_NPART) parts[(size_t)blockIdx.x * RS_NPART + threadIdx.x] = sum;
  }
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
  if (!BATCH) {
    const unsigned long long sum = sfmx_block_sums(cnt);
    if (threadIdx.x < RS_NPART) parts[(size_t)blockIdx.x * RS_NPART + threadIdx.x] = sum;
  }
}

// views [first, first + count) of a view set, and the pixels of their key images
struct RsBatch {
  int first, count;
  size_t px;
};

// An ordered list of cameras, each with or without a u8 image in one slab on the device, and the exact z-buffers of a mesh for
// them, a batch at a time.  A batch is sized so that its key images, projected vertices (16 + 1 bytes per view and vertex) and
// lists of big faces stay within RS_BATCH_BUDGET, unless set_batch forces its size.  Which views need an image is the owner's rule.
struct RsViewSet {
  std::vector<sfmx_fusion_view> views;
  std::vector<long long> img_off;  // of a view's image in the image slab, -1 without one
  std::vector<RsSlot> slots;       // of the last prepare, as uploaded
  std::vector<RsBatch> batches;    // of the last plan
  long long img_used = 0;
  int forced_batch = 0, last_batch = 0;
  size_t key_px = 0;  // of the last plan: the most key pixels of a batch
  int widest = 0;     // and the most views
  DevBuf img, d_slots;
  DevBuf keys, pv, fl, big, rcounters;  // one batch's z-buffers

  int reset() {
    views.clear();
    img_off.clear();
    img_used = 0;
    return SFMX_OK;
  }

  int add_view(sfmx_ctx* ctx, const sfmx_fusion_view* view, const uint8_t* image, int on_device) {
    SFMX_REQUIRE(ctx, rs_view_ok(view));
    long long off = -1;
    if (image) {
      SFMX_HIP(ctx, hipSetDevice(ctx->device));
      const long long px = (long long)view->w * view->h;
      SFMX_REQUIRE(ctx, img_used + px < (1ll << 40));
      SFMX_HIP(ctx, sfmx_grow_keep(img, (size_t)img_used, (size_t)(img_used + px), ctx->stream));
      SFMX_HIP(ctx, hipMemcpyAsync(img.as<uint8_t>() + img_used, image, (size_t)px, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                   ctx->stream));
      SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may reuse its buffer
      off = img_used;
      img_used += px;
    }
    views.push_back(*view);
    img_off.push_back(off);
    return SFMX_OK;
  }

  int add_stereo_view(sfmx_ctx* ctx, const sfmx_fusion_view* view, const sfmx_stereo* st) {
    SFMX_REQUIRE(ctx, st && view);
    int w = 0, h = 0;
    const uint8_t* im = sfmx_stereo_device_rect_left(st, &w, &h);
    SFMX_REQUIRE(ctx, im && view->w == w && view->h == h);
    return add_view(ctx, view, im, 1);
  }

  int view_count() const { return (int)views.size(); }

  int set_batch(int k) {
    if (k < 0 || k > RS_MAX_BATCH) return SFMX_ERR_INVALID;
    forced_batch = k;
    return SFMX_OK;
  }

  // the batches for a mesh of n vertices and m faces, with key_px and widest
  void plan(int n, int m) {
    batches.clear();
    const int V = (int)views.size();
    key_px = 0;
    widest = 0;
    int k = 0;
    while (k < V) {
      size_t bytes = 0, px = 0;
      int c = 0;
      while (k + c < V && c < RS_MAX_BATCH) {
        const size_t p = (size_t)views[k + c].w * (size_t)views[k + c].h;
        const size_t one = p * 8 + (size_t)n * 17 + (size_t)m * 4;
        if (forced_batch ? c >= forced_batch : (c > 0 && bytes + one > RS_BATCH_BUDGET)) break;
        bytes += one;
        px += p;
        c++;
      }
      batches.push_back({k, c, px});
      key_px = px > key_px ? px : key_px;
      widest = c > widest ? c : widest;
      k += c;
    }
  }

  // plans, sizes the z-buffer slabs and uploads the slots of all views: a batch's key images lie back to back in the key slab
  int prepare(sfmx_ctx* ctx, int n, int m) {
    plan(n, m);
    const size_t nn = (size_t)n, mm = (size_t)m, V = views.size();
    SFMX_HIP(ctx, keys.ensure(key_px * 8));
    SFMX_HIP(ctx, pv.ensure((size_t)widest * nn * sizeof(RsVert)));
    SFMX_HIP(ctx, fl.ensure((size_t)widest * nn));
    SFMX_HIP(ctx, big.ensure((size_t)widest * mm * 4));
    SFMX_HIP(ctx, rcounters.ensure((size_t)RS_MAX_BATCH * RS_NWORDS * 4));
    slots.resize(V);
    for (const RsBatch& b : batches) {
      long long at = 0;
      for (int k = b.first; k < b.first + b.count; k++) {
        slots[k].cam = rs_cam(&views[k]);
        slots[k].key_off = at;
        slots[k].img_off = img_off[k] >= 0 ? img_off[k] : 0;
        at += (long long)views[k].w * views[k].h;
      }
    }
    if (V > 0) {
      SFMX_HIP(ctx, d_slots.ensure(sizeof(RsSlot) * V));
      SFMX_HIP(ctx, hipMemcpyAsync(d_slots.p, slots.data(), sizeof(RsSlot) * V, hipMemcpyHostToDevice, ctx->stream));
    }
    return SFMX_OK;
  }

  const RsSlot* batch_slots(const RsBatch& b) const { return d_slots.as<RsSlot>() + b.first; }

  // the key images of batch b for the mesh (n > 0): clear, project, and with faces the two face kernels.  A template, so that
  // only the files that build z-buffers instantiate the batch kernels (raster.hip and level.hip include this header too).
  template <int SMALL = RS_BATCH_SMALL> hipError_t zbuffer(const RsBatch& b, const double* verts, int n, const int32_t* faces, int m, double z_min, hipStream_t s) {
    const unsigned nbv = (unsigned)(((size_t)n + 255) / 256);
    const int fb = m > (RS_FACE_BLOCKS - 1) * 256 ? RS_FACE_BLOCKS : (m + 255) / 256;
    const RsSlot* sl = batch_slots(b);
    hipError_t e = hipMemsetAsync(keys.p, 0xFF, b.px * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(rcounters.p, 0, (size_t)b.count * RS_NWORDS * 4, s);
    if (e != hipSuccess) return e;
    k_rs_project<true><<<dim3(nbv, (unsigned)b.count), 256, 0, s>>>(verts, n, RsCam{}, sl, z_min, pv.as<RsVert>(), fl.as<uint8_t>());
    if (m > 0) {
      k_rs_faces<true, SMALL><<<dim3((unsigned)fb, (unsigned)b.count), 256, 0, s>>>(
          faces, m, n, pv.as<RsVert>(), fl.as<uint8_t>(), 0, 0, 0, keys.as<unsigned long long>(), big.as<int>(), rcounters.as<unsigned>(), nullptr, sl);
      k_rs_big<true><<<dim3(RS_BATCH_BIG_BLOCKS, (unsigned)b.count), 256, 0, s>>>(faces, m, n, pv.as<RsVert>(), 0, 0, keys.as<unsigned long long>(),
                                                                                  big.as<int>(), rcounters.as<unsigned>(), nullptr, sl);
    }
    return hipSuccess;
  }

  void release() {
    for (DevBuf* b : {&img, &d_slots, &keys, &pv, &fl, &big, &rcounters}) b->release();
  }
};

}  // namespace
