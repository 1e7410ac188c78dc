// fusion.hip — multi-pair depth fusion: TSDF integration of rectified disparity maps and marching-tetrahedra extraction.
//
// Exactness: integration is IEEE double in one fixed expression order (built with -ffp-contract=off, as everything here),
// views in the order they were added, one running sum per grid point; extraction is integer (classification, scans, ids)
// plus one fixed double expression per vertex, evaluated from the lower endpoint of its edge.  tests/fusion_ref.py restates
// it in NumPy, with a triangle table derived there on its own from the same rule; the tests compare bits.
//
// Kernel layout:
//   k_fu_integrate     one thread per grid point, blocks of 64 (i) x 4 (j): a wave is 64 consecutive points of one row, so
//                      the volume loads are contiguous and its projected pixels lie on one short image segment; sum / count
//                      stay in registers across the pending views (read and written once per launch)
//   k_fu_classify      one thread per cell: triangle count, and the edge slots its triangles use (atomicOr of 7-bit masks on
//                      the edges' lower grid points)
//   k_scan_*           exclusive int32 scans over the triangle counts and the slot popcounts (scan.hip)
//   k_fu_emit_verts    one thread per grid point: its used slots, in slot order
//   k_fu_emit_faces    one thread per cell: its triangles, in (tet, triangle) order
//   k_fu_emit_normals  one thread per grid point, as k_fu_emit_verts: the volume's gradient at both ends of each used edge,
//                      interpolated with the vertex's own t and normalised
#include <cmath>

#include "sfmx_internal.h"
#include "sfmx_tsdf.h"
#include "sfmx_view.h"

namespace {

// ---- the triangle table, generated from the rule at compile time (integer geometry only) -------------------------------
struct FuTable {
  int8_t ntri[6][16];
  uint8_t e[6][16][2][3];  // lower corner * 8 + slot
};

constexpr int fu_slot_of_mask(int m) { return m == 1 ? 0 : m == 2 ? 1 : m == 4 ? 2 : m == 3 ? 3 : m == 5 ? 4 : m == 6 ? 5 : 6; }

constexpr FuTable fu_make_table() {
  FuTable T{};
  // permutations (a, b, c) of the axes in lexicographic order: chain (0, e_a, e_a + e_b, 7)
  const int pa[6] = {0, 0, 1, 1, 2, 2}, pb[6] = {1, 2, 0, 2, 0, 1};
  for (int t = 0; t < 6; t++) {
    const int chain[4] = {0, 1 << pa[t], (1 << pa[t]) | (1 << pb[t]), 7};
    int P[4][3] = {};
    for (int q = 0; q < 4; q++)
      for (int a = 0; a < 3; a++) P[q][a] = (chain[q] >> a) & 1;
    for (int cs = 0; cs < 16; cs++) {
      int ins[4] = {}, outs[4] = {}, ni = 0, no = 0;
      for (int q = 0; q < 4; q++) {
        if ((cs >> q) & 1) ins[ni++] = q;
        else outs[no++] = q;
      }
      T.ntri[t][cs] = 0;
      if (ni == 0 || ni == 4) continue;
      int tri[2][3][2] = {};
      int nt = 0;
      if (ni == 2) {  // quad (a,c) -> (a,d) -> (b,d) -> (b,c), split on (a,c)-(b,d)
        const int a = ins[0], b = ins[1], c = outs[0], d = outs[1];
        const int q0[2][3][2] = {{{a, c}, {a, d}, {b, d}}, {{a, c}, {b, d}, {b, c}}};
        for (int k = 0; k < 2; k++)
          for (int v = 0; v < 3; v++)
            for (int z = 0; z < 2; z++) tri[k][v][z] = q0[k][v][z];
        nt = 2;
      } else {  // the lone corner's three edges, the others in chain order
        const int lone = ni == 1 ? ins[0] : outs[0];
        int v = 0;
        for (int q = 0; q < 4; q++)
          if (q != lone) {
            tri[0][v][0] = lone;
            tri[0][v][1] = q;
            v++;
          }
        nt = 1;
      }
      // orientation: cross(p1 - p0, p2 - p0) . (centroid(out) - centroid(in)) > 0 with the vertices at edge midpoints
      // (coordinates x 2, centroids x |in| |out|: integers)
      int dir[3] = {};
      for (int a = 0; a < 3; a++) {
        int so = 0, si = 0;
        for (int q = 0; q < no; q++) so += P[outs[q]][a];
        for (int q = 0; q < ni; q++) si += P[ins[q]][a];
        dir[a] = so * ni - si * no;
      }
      for (int k = 0; k < nt; k++) {
        int m[3][3] = {};
        for (int v = 0; v < 3; v++)
          for (int a = 0; a < 3; a++) m[v][a] = P[tri[k][v][0]][a] + P[tri[k][v][1]][a];
        const int e1[3] = {m[1][0] - m[0][0], m[1][1] - m[0][1], m[1][2] - m[0][2]};
        const int e2[3] = {m[2][0] - m[0][0], m[2][1] - m[0][1], m[2][2] - m[0][2]};
        const int cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const int s = cr[0] * dir[0] + cr[1] * dir[1] + cr[2] * dir[2];
        int order[3] = {0, 1, 2};
        if (s < 0) {
          order[1] = 2;
          order[2] = 1;
        }
        for (int v = 0; v < 3; v++) {
          const int c0 = chain[tri[k][order[v]][0]], c1 = chain[tri[k][order[v]][1]];
          const int lo = c0 < c1 ? c0 : c1, hi = c0 < c1 ? c1 : c0;
          T.e[t][cs][k][v] = (uint8_t)(lo * 8 + fu_slot_of_mask(hi ^ lo));
        }
      }
      T.ntri[t][cs] = (int8_t)nt;
    }
  }
  return T;
}

__constant__ const FuTable kFuTab = fu_make_table();
// tet t's chain corners 1 and 2 (corners 0 and 3 are always 0 and 7)
__constant__ const int kFuChain1[6] = {1, 1, 2, 2, 4, 4};
__constant__ const int kFuChain2[6] = {3, 5, 3, 6, 5, 6};

__global__ __launch_bounds__(256) void k_fu_integrate(double* __restrict__ sum, int* __restrict__ cnt, FuGrid g,
                                                      const DevView* __restrict__ views, int nv, const int16_t* __restrict__ stack,
                                                      double trunc, double disp_min, int bx, int by) {
  int b = blockIdx.x;
  const int bi = b % bx;
  b /= bx;
  const int bj = b % by, k = b / by;
  const int i = bi * 64 + (int)threadIdx.x, j = bj * 4 + (int)threadIdx.y;
  if (i >= g.nx || j >= g.ny) return;
  const size_t L = (size_t)i + (size_t)g.nx * ((size_t)j + (size_t)g.ny * k);
  const double X0 = g.ox + (double)i * g.vs, X1 = g.oy + (double)j * g.vs, X2 = g.oz + (double)k * g.vs;
  double s = sum[L];
  int c = cnt[L];
  const double ntrunc = -trunc;
  for (int n = 0; n < nv; n++) {
    const DevView& V = views[n];
    double p0, p1, p2, x, y;
    const double q2 = dv_depth(V, X0, X1, X2, p0, p1, p2);
    if (!(q2 > 0.0)) continue;
    if (!dv_pixel(V, p0, p1, p2, q2, x, y)) continue;
    const int d = stack[dv_index(V, x, y)];
    if (!dv_disp_ok(d, disp_min)) continue;
    const double Z = dv_disp_depth(V, d);
    const double sdf = Z - q2;
    if (sdf < ntrunc) continue;
    s += sdf >= trunc ? 1.0 : sdf / trunc;
    c += 1;
  }
  sum[L] = s;
  cnt[L] = c;
}

// inside bits of a cell's 8 corners (bit b = corner b inside), or -1 if the cell is not meshed
__device__ __forceinline__ int fu_cell(const double* __restrict__ sum, const int* __restrict__ cnt, const FuGrid& g, int i, int j, int k,
                                       size_t L) {
  if (i >= g.nx - 1 || j >= g.ny - 1 || k >= g.nz - 1) return -1;
  const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
  int m = 0;
  bool ok = true;
#pragma unroll
  for (int b = 0; b < 8; b++) {
    double s;
    ok &= fu_value(sum, cnt, L + (b & 1) + ((b >> 1) & 1) * sy + ((b >> 2) & 1) * sz, g.minw, s);
    m |= (s < 0.0 ? 1 : 0) << b;
  }
  return ok ? m : -1;
}

__device__ __forceinline__ int fu_case(int m, int t) {
  return (m & 1) | (((m >> kFuChain1[t]) & 1) << 1) | (((m >> kFuChain2[t]) & 1) << 2) | (((m >> 7) & 1) << 3);
}

__device__ __forceinline__ size_t fu_corner_off(int lo, const FuGrid& g) {
  return (size_t)(lo & 1) + (size_t)((lo >> 1) & 1) * g.nx + (size_t)((lo >> 2) & 1) * ((size_t)g.nx * g.ny);
}

__global__ __launch_bounds__(256) void k_fu_classify(const double* __restrict__ sum, const int* __restrict__ cnt, FuGrid g, int n,
                                                     int* __restrict__ tri_cnt, unsigned* vmask) {
  const int L = blockIdx.x * 256 + threadIdx.x;
  if (L >= n) return;
  const int i = L % g.nx, j = (L / g.nx) % g.ny, k = L / (g.nx * g.ny);
  const int m = fu_cell(sum, cnt, g, i, j, k, (size_t)L);
  int nt = 0;
  if (m > 0 && m < 255) {
    uint64_t used = 0;  // bit lo * 8 + slot
    for (int t = 0; t < 6; t++) {
      const int cs = fu_case(m, t);
      const int ntt = kFuTab.ntri[t][cs];
      for (int r = 0; r < ntt; r++)
        for (int v = 0; v < 3; v++) used |= 1ull << kFuTab.e[t][cs][r][v];
      nt += ntt;
    }
#pragma unroll
    for (int lo = 0; lo < 8; lo++) {
      const unsigned bits = (unsigned)(used >> (8 * lo)) & 0x7Fu;
      if (bits) atomicOr(&vmask[(size_t)L + fu_corner_off(lo, g)], bits);
    }
  }
  tri_cnt[L] = nt;
}

__global__ __launch_bounds__(256) void k_fu_emit_verts(const double* __restrict__ sum, const int* __restrict__ cnt, FuGrid g, int n,
                                                       const unsigned* __restrict__ vmask, const int* __restrict__ voff,
                                                       double* __restrict__ verts) {
  const int L = blockIdx.x * 256 + threadIdx.x;
  if (L >= n) return;
  const unsigned mask = vmask[L];
  if (!mask) return;
  const int i = L % g.nx, j = (L / g.nx) % g.ny, k = L / (g.nx * g.ny);
  double sg;
  (void)fu_value(sum, cnt, (size_t)L, g.minw, sg);
  const double Xg0 = g.ox + (double)i * g.vs, Xg1 = g.oy + (double)j * g.vs, Xg2 = g.oz + (double)k * g.vs;
  constexpr int D[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
  size_t o = (size_t)voff[L];
#pragma unroll
  for (int sl = 0; sl < 7; sl++) {
    if (!((mask >> sl) & 1u)) continue;
    const int di = D[sl][0], dj = D[sl][1], dk = D[sl][2];
    double sq;
    (void)fu_value(sum, cnt, (size_t)L + di + (size_t)dj * g.nx + (size_t)dk * ((size_t)g.nx * g.ny), g.minw, sq);
    const double t = sg / (sg - sq);
    const double Xq0 = g.ox + (double)(i + di) * g.vs, Xq1 = g.oy + (double)(j + dj) * g.vs, Xq2 = g.oz + (double)(k + dk) * g.vs;
    verts[3 * o + 0] = Xg0 + t * (Xq0 - Xg0);
    verts[3 * o + 1] = Xg1 + t * (Xq1 - Xg1);
    verts[3 * o + 2] = Xg2 + t * (Xq2 - Xg2);
    o++;
  }
}

// ---- vertex normals: the gradient of s ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fu_emit_normals(const double* __restrict__ sum, const int* __restrict__ cnt, FuGrid g, int n,
                                                         const unsigned* __restrict__ vmask, const int* __restrict__ voff,
                                                         double* __restrict__ normals) {
  const int L = blockIdx.x * 256 + threadIdx.x;
  if (L >= n) return;
  const unsigned mask = vmask[L];
  if (!mask) return;
  const int i = L % g.nx, j = (L / g.nx) % g.ny, k = L / (g.nx * g.ny);
  double sg;
  (void)fu_value(sum, cnt, (size_t)L, g.minw, sg);
  double Gg0, Gg1, Gg2;
  fu_grad(sum, cnt, g, i, j, k, (size_t)L, sg, Gg0, Gg1, Gg2);
  constexpr int D[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
  size_t o = (size_t)voff[L];
#pragma unroll
  for (int sl = 0; sl < 7; sl++) {
    if (!((mask >> sl) & 1u)) continue;
    const int di = D[sl][0], dj = D[sl][1], dk = D[sl][2];
    const size_t Lq = (size_t)L + di + (size_t)dj * g.nx + (size_t)dk * ((size_t)g.nx * g.ny);
    double sq;
    (void)fu_value(sum, cnt, Lq, g.minw, sq);
    const double t = sg / (sg - sq);
    double Gq0, Gq1, Gq2;
    fu_grad(sum, cnt, g, i + di, j + dj, k + dk, Lq, sq, Gq0, Gq1, Gq2);
    const double N0 = Gg0 + t * (Gq0 - Gg0), N1 = Gg1 + t * (Gq1 - Gg1), N2 = Gg2 + t * (Gq2 - Gg2);
    const double len = sqrt((N0 * N0 + N1 * N1) + N2 * N2);
    const bool ok = len > 0.0;
    normals[3 * o + 0] = ok ? N0 / len : 0.0;
    normals[3 * o + 1] = ok ? N1 / len : 0.0;
    normals[3 * o + 2] = ok ? N2 / len : 0.0;
    o++;
  }
}

__global__ __launch_bounds__(256) void k_fu_emit_faces(const double* __restrict__ sum, const int* __restrict__ cnt, FuGrid g, int n,
                                                       const int* __restrict__ tri_cnt, const int* __restrict__ foff,
                                                       const unsigned* __restrict__ vmask, const int* __restrict__ voff,
                                                       int* __restrict__ faces) {
  const int L = blockIdx.x * 256 + threadIdx.x;
  if (L >= n || tri_cnt[L] == 0) return;
  const int i = L % g.nx, j = (L / g.nx) % g.ny, k = L / (g.nx * g.ny);
  const int m = fu_cell(sum, cnt, g, i, j, k, (size_t)L);
  size_t o = (size_t)foff[L];
  for (int t = 0; t < 6; t++) {
    const int cs = fu_case(m, t);
    const int ntt = kFuTab.ntri[t][cs];
    for (int r = 0; r < ntt; r++) {
      for (int v = 0; v < 3; v++) {
        const int e = kFuTab.e[t][cs][r][v];
        const size_t Lg = (size_t)L + fu_corner_off(e >> 3, g);
        const unsigned below = vmask[Lg] & ((1u << (e & 7)) - 1u);
        faces[3 * o + v] = voff[Lg] + __popc(below);
      }
      o++;
    }
  }
}

}  // namespace

struct sfmx_fusion {
  sfmx_fusion_params p{};
  double trunc = 0.0;
  int n = 0;  // grid points
  double* sum = nullptr;
  int* cnt = nullptr;
  DevView* d_views = nullptr;
  std::vector<DevView> pending;
  DevBuf stack;            // int16 disparity maps of the pending views
  long long stack_used = 0;
  // extraction: triangle counts, face offsets, slot masks, vertex offsets (int32 [n] each), scan partials, totals
  DevBuf ex, out_v, out_f;
  // the last sfmx_fusion_extract_normals: normals next to out_v, and how many vertices of both are current (-1: none)
  DevBuf out_n;
  int resident = -1;
  // vertices / faces of out_v / out_f that are the volume's current surface (-1: none), whichever extraction wrote them
  int cur_v = -1, cur_f = -1;
  hipEvent_t ev[6] = {};
  double last_us = 0.0, normals_us = 0.0;
};

namespace {

FuGrid fu_grid(const sfmx_fusion* fu) {
  return FuGrid{fu->p.origin[0], fu->p.origin[1], fu->p.origin[2], fu->p.voxel, fu->p.nx, fu->p.ny, fu->p.nz, fu->p.min_weight};
}

int fu_timed(sfmx_ctx* ctx, sfmx_fusion* fu, int e0, int e1) {
  if (!ctx->timing) return SFMX_OK;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, fu->ev[e0], fu->ev[e1]) == hipSuccess) fu->last_us += (double)ms * 1000.0;
  return SFMX_OK;
}

// room for one more view of w x h: integrates the pending views when the stack is full (count or bytes)
int fu_make_room(sfmx_ctx* ctx, sfmx_fusion* fu, int w, int h) {
  const long long need = (long long)w * h;
  if ((int)fu->pending.size() >= fu->p.max_views || (fu->stack_used + need) * 2 > (long long)fu->stack.cap) {
    if (!fu->pending.empty()) {
      const int rc = sfmx_fusion_integrate(ctx, fu);
      if (rc != SFMX_OK) return rc;
    }
    // the stack is empty now; size it for max_views maps of this size at once
    SFMX_HIP(ctx, fu->stack.ensure((size_t)need * 2 * (size_t)fu->p.max_views));
  }
  return SFMX_OK;
}

int fu_queue(sfmx_ctx* ctx, sfmx_fusion* fu, const sfmx_fusion_view* v, const int16_t* src, hipMemcpyKind kind) {
  int rc = fu_make_room(ctx, fu, v->w, v->h);
  if (rc != SFMX_OK) return rc;
  const size_t bytes = (size_t)v->w * v->h * 2;
  SFMX_HIP(ctx, hipMemcpyAsync(fu->stack.as<int16_t>() + fu->stack_used, src, bytes, kind, ctx->stream));
  if (kind == hipMemcpyHostToDevice) SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may reuse its buffer
  fu->pending.push_back(sfmx_dev_view(v, fu->stack_used));
  fu->stack_used += (long long)v->w * v->h;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_fusion_default_params(sfmx_fusion_params* p) {
  if (!p) return;
  *p = sfmx_fusion_params{};
  p->trunc = 0.0;
  p->disp_min = 1.0;
  p->min_weight = 1;
  p->max_views = 64;
}

int sfmx_fusion_check_params(const sfmx_fusion_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  for (double x : p->origin)
    if (!std::isfinite(x)) return SFMX_ERR_INVALID;
  if (!(p->voxel > 0.0) || !std::isfinite(p->voxel)) return SFMX_ERR_INVALID;
  if (p->nx < 2 || p->ny < 2 || p->nz < 2) return SFMX_ERR_INVALID;
  // slot ids 7 L + slot and face counts (<= 12 per cell) stay below 2^31
  if ((long long)p->nx * p->ny * p->nz > (1ll << 27)) return SFMX_ERR_INVALID;
  if (!(p->trunc >= 0.0) || !std::isfinite(p->trunc) || std::isnan(p->disp_min)) return SFMX_ERR_INVALID;
  if (p->min_weight < 1 || p->max_views < 1 || p->max_views > 4096) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_fusion_create(sfmx_ctx* ctx, const sfmx_fusion_params* p, sfmx_fusion** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_REQUIRE(ctx, sfmx_fusion_check_params(p) == SFMX_OK);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* fu = new sfmx_fusion;
  fu->p = *p;
  fu->trunc = p->trunc == 0.0 ? 4.0 * p->voxel : p->trunc;
  fu->n = p->nx * p->ny * p->nz;
  const size_t n = (size_t)fu->n;
  hipError_t e = hipMalloc(&fu->sum, n * 8);
  if (e == hipSuccess) e = hipMalloc(&fu->cnt, n * 4);
  if (e == hipSuccess) e = hipMalloc(&fu->d_views, sizeof(DevView) * (size_t)p->max_views);
  for (int q = 0; q < 6 && e == hipSuccess; q++) e = hipEventCreate(&fu->ev[q]);
  if (e == hipSuccess) e = hipMemsetAsync(fu->sum, 0, n * 8, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(fu->cnt, 0, n * 4, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    sfmx_fusion_destroy(ctx, fu);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_fusion_create", e);
  }
  fu->pending.reserve((size_t)p->max_views);
  *out = fu;
  return SFMX_OK;
}

void sfmx_fusion_destroy(sfmx_ctx* ctx, sfmx_fusion* fu) {
  if (!fu) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  if (fu->sum) (void)hipFree(fu->sum);
  if (fu->cnt) (void)hipFree(fu->cnt);
  if (fu->d_views) (void)hipFree(fu->d_views);
  fu->stack.release();
  fu->ex.release();
  fu->out_v.release();
  fu->out_f.release();
  fu->out_n.release();
  for (hipEvent_t ev : fu->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete fu;
}

double sfmx_fusion_last_us(const sfmx_fusion* fu) { return fu ? fu->last_us : 0.0; }

int sfmx_fusion_reset(sfmx_ctx* ctx, sfmx_fusion* fu) {
  SFMX_REQUIRE(ctx, ctx && fu);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  SFMX_HIP(ctx, hipMemsetAsync(fu->sum, 0, (size_t)fu->n * 8, ctx->stream));
  SFMX_HIP(ctx, hipMemsetAsync(fu->cnt, 0, (size_t)fu->n * 4, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  fu->pending.clear();
  fu->stack_used = 0;
  fu->last_us = 0.0;
  fu->normals_us = 0.0;
  fu->resident = -1;
  fu->cur_v = fu->cur_f = -1;
  return SFMX_OK;
}

int sfmx_fusion_add_view(sfmx_ctx* ctx, sfmx_fusion* fu, const sfmx_fusion_view* view, const int16_t* disp16, int on_device) {
  SFMX_REQUIRE(ctx, ctx && fu && disp16 && sfmx_view_ok(view));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return fu_queue(ctx, fu, view, disp16, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
}

int sfmx_fusion_add_stereo_view(sfmx_ctx* ctx, sfmx_fusion* fu, const sfmx_fusion_view* view, const sfmx_stereo* st) {
  SFMX_REQUIRE(ctx, ctx && fu && st && sfmx_view_ok(view));
  int w = 0, h = 0;
  const int16_t* d16 = sfmx_stereo_device_disp16(st, &w, &h);
  SFMX_REQUIRE(ctx, view->w == w && view->h == h);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return fu_queue(ctx, fu, view, d16, hipMemcpyDeviceToDevice);
}

int sfmx_fusion_add_consist_view(sfmx_ctx* ctx, sfmx_fusion* fu, const sfmx_consist* cs, int i) {
  SFMX_REQUIRE(ctx, ctx && fu && cs);
  sfmx_fusion_view v{};
  const int16_t* d16 = nullptr;
  SFMX_REQUIRE(ctx, sfmx_consist_device_view(cs, i, &v, &d16));  // no current filter result, or i out of range
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return fu_queue(ctx, fu, &v, d16, hipMemcpyDeviceToDevice);
}

int sfmx_fusion_integrate(sfmx_ctx* ctx, sfmx_fusion* fu) {
  SFMX_REQUIRE(ctx, ctx && fu);
  fu->last_us = 0.0;
  if (fu->pending.empty()) return SFMX_OK;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int nv = (int)fu->pending.size();
  fu->resident = -1;  // the volume changes: the surface kept on the device is no longer its surface
  fu->cur_v = fu->cur_f = -1;
  SFMX_HIP(ctx, hipMemcpyAsync(fu->d_views, fu->pending.data(), sizeof(DevView) * (size_t)nv, hipMemcpyHostToDevice, s));
  const FuGrid g = fu_grid(fu);
  const int bx = (g.nx + 63) / 64, by = (g.ny + 3) / 4;
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(fu->ev[0], s));
  k_fu_integrate<<<(unsigned)((long long)bx * by * g.nz), dim3(64, 4), 0, s>>>(fu->sum, fu->cnt, g, fu->d_views, nv,
                                                                                fu->stack.as<int16_t>(), fu->trunc, fu->p.disp_min, bx, by);
  SFMX_HIP(ctx, hipGetLastError());
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(fu->ev[1], s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));  // the host view array and the stack are reused by the next views
  fu->pending.clear();
  fu->stack_used = 0;
  return fu_timed(ctx, fu, 0, 1);
}

int sfmx_fusion_read(sfmx_ctx* ctx, sfmx_fusion* fu, double* sum, int32_t* count) {
  SFMX_REQUIRE(ctx, ctx && fu);
  int rc = sfmx_fusion_integrate(ctx, fu);
  if (rc != SFMX_OK) return rc;
  const size_t n = (size_t)fu->n;
  if (sum) SFMX_HIP(ctx, hipMemcpyAsync(sum, fu->sum, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (count) SFMX_HIP(ctx, hipMemcpyAsync(count, fu->cnt, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SFMX_OK;
}

// sfmx_fusion_extract, and with want_normals sfmx_fusion_extract_normals: the same launches, then the normals
static int fu_extract(sfmx_ctx* ctx, sfmx_fusion* fu, double* verts, int verts_cap, int32_t* faces, int faces_cap, bool want_normals,
               double* normals, int* n_verts, int* n_faces) {
  SFMX_REQUIRE(ctx, ctx && fu && n_verts && n_faces);
  *n_verts = 0;
  *n_faces = 0;
  int rc = sfmx_fusion_integrate(ctx, fu);
  if (rc != SFMX_OK) return rc;
  fu->last_us = 0.0;
  hipStream_t s = ctx->stream;
  const int n = fu->n;
  const size_t aux = sfmx_scan_aux(n);
  SFMX_HIP(ctx, fu->ex.ensure(4 * (size_t)n * 4 + (aux + 2) * 4));
  int* tri = fu->ex.as<int>();
  int* foff = tri + n;
  unsigned* vmask = reinterpret_cast<unsigned*>(foff + n);
  int* voff = reinterpret_cast<int*>(vmask + n);
  int* ax = voff + n;
  int* totals = ax + aux;  // faces, vertices
  const FuGrid g = fu_grid(fu);
  const unsigned nb = (unsigned)((n + 255) / 256);
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(fu->ev[0], s));
  SFMX_HIP(ctx, hipMemsetAsync(vmask, 0, (size_t)n * 4, s));
  k_fu_classify<<<nb, 256, 0, s>>>(fu->sum, fu->cnt, g, n, tri, vmask);
  sfmx_scan(tri, false, n, foff, ax, s);
  sfmx_scan_total(tri, false, foff, n, totals, s);
  sfmx_scan(reinterpret_cast<const int*>(vmask), true, n, voff, ax, s);
  sfmx_scan_total(reinterpret_cast<const int*>(vmask), true, voff, n, totals + 1, s);
  SFMX_HIP(ctx, hipGetLastError());
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(fu->ev[1], s));
  int tot[2] = {0, 0};
  SFMX_HIP(ctx, hipMemcpyAsync(tot, totals, sizeof tot, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  fu_timed(ctx, fu, 0, 1);
  const int nf = tot[0], nvx = tot[1];
  *n_faces = nf;
  *n_verts = nvx;
  if (!verts && !faces && !normals) return SFMX_OK;
  SFMX_REQUIRE(ctx, verts && faces && verts_cap >= nvx && faces_cap >= nf && (!want_normals || normals));
  fu->resident = want_normals ? 0 : -1;  // out_v is rewritten below
  fu->normals_us = 0.0;
  fu->cur_v = fu->cur_f = nf == 0 ? 0 : -1;  // no faces: no edge slot is used either (nvx == 0), an empty surface is current
  if (nf == 0) return SFMX_OK;
  SFMX_HIP(ctx, fu->out_v.ensure((size_t)nvx * 24));
  SFMX_HIP(ctx, fu->out_f.ensure((size_t)nf * 12));
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(fu->ev[2], s));
  k_fu_emit_verts<<<nb, 256, 0, s>>>(fu->sum, fu->cnt, g, n, vmask, voff, fu->out_v.as<double>());
  k_fu_emit_faces<<<nb, 256, 0, s>>>(fu->sum, fu->cnt, g, n, tri, foff, vmask, voff, fu->out_f.as<int>());
  SFMX_HIP(ctx, hipGetLastError());
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(fu->ev[3], s));
  SFMX_HIP(ctx, hipMemcpyAsync(verts, fu->out_v.p, (size_t)nvx * 24, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipMemcpyAsync(faces, fu->out_f.p, (size_t)nf * 12, hipMemcpyDeviceToHost, s));
  if (want_normals) {
    SFMX_HIP(ctx, fu->out_n.ensure((size_t)nvx * 24));
    if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(fu->ev[4], s));
    k_fu_emit_normals<<<nb, 256, 0, s>>>(fu->sum, fu->cnt, g, n, vmask, voff, fu->out_n.as<double>());
    SFMX_HIP(ctx, hipGetLastError());
    if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(fu->ev[5], s));
    SFMX_HIP(ctx, hipMemcpyAsync(normals, fu->out_n.p, (size_t)nvx * 24, hipMemcpyDeviceToHost, s));
  }
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  fu->cur_v = nvx;
  fu->cur_f = nf;
  if (want_normals) {
    fu->resident = nvx;
    float ms = 0.f;
    if (ctx->timing && hipEventElapsedTime(&ms, fu->ev[4], fu->ev[5]) == hipSuccess) fu->normals_us = (double)ms * 1000.0;
    fu->last_us += fu->normals_us;
  }
  return fu_timed(ctx, fu, 2, 3);
}

int sfmx_fusion_extract(sfmx_ctx* ctx, sfmx_fusion* fu, double* verts, int verts_cap, int32_t* faces, int faces_cap, int* n_verts,
                        int* n_faces) {
  return fu_extract(ctx, fu, verts, verts_cap, faces, faces_cap, false, nullptr, n_verts, n_faces);
}

int sfmx_fusion_extract_normals(sfmx_ctx* ctx, sfmx_fusion* fu, double* verts, int verts_cap, int32_t* faces, int faces_cap,
                                double* normals, int* n_verts, int* n_faces) {
  return fu_extract(ctx, fu, verts, verts_cap, faces, faces_cap, true, normals, n_verts, n_faces);
}

double sfmx_fusion_normals_us(const sfmx_fusion* fu) { return fu ? fu->normals_us : 0.0; }

}  // extern "C"

int sfmx_fusion_device_surface(const sfmx_fusion* fu, const double** verts, const double** normals) {
  *verts = fu->out_v.as<double>();
  *normals = fu->out_n.as<double>();
  return fu->resident;
}

int sfmx_fusion_device_mesh(const sfmx_fusion* fu, const double** verts, const double** normals, const int32_t** faces, int* n_faces) {
  *verts = fu->out_v.as<double>();
  *normals = fu->resident >= 0 && fu->resident == fu->cur_v ? fu->out_n.as<double>() : nullptr;
  *faces = fu->out_f.as<int32_t>();
  *n_faces = fu->cur_f;
  return fu->cur_v;
}

int sfmx_fusion_device_volume(const sfmx_fusion* fu, const double** sum, const int32_t** count, sfmx_fusion_params* p) {
  if (!fu->pending.empty()) return -1;
  *sum = fu->sum;
  *count = fu->cnt;
  *p = fu->p;
  return fu->n;
}

int sfmx_fusion_mutable_volume(sfmx_ctx* ctx, sfmx_fusion* fu, double** sum, int32_t** count, sfmx_fusion_params* p) {
  SFMX_REQUIRE(ctx, ctx && fu && p);
  *p = fu->p;
  if (!sum || !count) return SFMX_OK;  // the parameters alone: the object is not touched
  const int rc = sfmx_fusion_integrate(ctx, fu);
  if (rc != SFMX_OK) return rc;
  fu->resident = -1;  // the caller changes the volume: the surface kept on the device is no longer its surface
  fu->cur_v = fu->cur_f = -1;
  *sum = fu->sum;
  *count = fu->cnt;
  return SFMX_OK;
}
