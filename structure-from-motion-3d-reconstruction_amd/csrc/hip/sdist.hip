// sdist.hip — distance from many points to the nearest point of a triangle mesh, on the device.
//
// Exactness: each point-triangle distance is one fixed sequence of double operations (sfmx_sdist_math.h), a triangle counts for
// a point when the point lies in the triangle's grown box (three exact comparisons per axis), and the result is the minimum
// with the smallest face index among equals.  None of this depends on the order the candidates are visited in, and the grid
// only ever drops triangles whose grown box does not hold the point (see sd_cidx), so any cell size and any schedule give the
// bytes of the brute-force NumPy restatement in tests/sdist_ref.py.
//
// Kernel layout, blocks of 256 unless noted, all on the context's stream:
//   k_sd_bbox       per face: indices outside [0, nv) or a non-finite coordinate set the flag (atomicOr) and the face is
//                   skipped; otherwise its corners go into the mesh's bounding box (wave-reduced, then atomicMin / atomicMax on
//                   order-preserving integer keys)
//   k_sd_total      per face: the number of cells its grown box overlaps, summed in 64 bits (the entry count, known before
//                   anything is written, decides whether the cell size fits)
//   k_sd_count      per face: atomicAdd(1) into each of those cells; blockIdx.y strides over a face's cells, so that a face
//                   across the whole grid is not one thread's loop (the host sizes gridDim.y by the largest face)
//   k_scan_*        exclusive int32 scan, one launch per level (scan.hip: no hand-off between workgroups inside a launch)
//   k_sd_fill       per face: its index into each cell's list, at offset + (atomicSub on the cell's count) - 1; the order inside
//                   a list is arbitrary, the tie rule makes the result independent of it
//   k_sd_qcell      per query: a non-finite coordinate sets the flag; a query outside the grid gets (dm2, -1) at once; the others
//                   their cell and an atomicAdd(1) into it
//   k_sd_items      per cell: ceil(queries / 64) work items
//   k_sd_qfill      per query: its index into its cell's run of the sorted list
//   k_sd_query      one wave per work item (64 queries of one cell at most; the cell is found by a search over the cells' item
//                   offsets): the cell's triangles are staged through LDS in
//                   chunks of SFMX_SDIST_CHUNK (corners and grown box, 15 doubles and the index each), every lane keeps
//                   (best d2, best face) of its query in registers
// No kernel waits on another workgroup or spins on a memory word.  A face that failed k_sd_bbox's check stops the call before
// any other kernel runs, so nothing is ever read through a bad index.
#include <algorithm>
#include <cmath>
#include <limits>

#include "sfmx_internal.h"
#include "sfmx_sdist_math.h"

namespace {

constexpr int SD_CHUNK = SFMX_SDIST_CHUNK;
constexpr int SD_MAX_CELLS = 1 << 24;
constexpr unsigned long long SD_MAX_ENTRIES = 1ull << 30;

// counters (unsigned long long each)
enum { SD_FLAG = 0, SD_MIN0, SD_MIN1, SD_MIN2, SD_MAX0, SD_MAX1, SD_MAX2, SD_TOTAL, SD_LARGEST, SD_TESTS, SD_COUNTERS };

struct SdGrid {
  double lo[3];  // the mesh's bounding box minus grow
  double cell;
  double grow;   // d_max plus the safety margin
  int n[3];
};

// x -> an integer whose unsigned order is the order of the finite doubles
__host__ __device__ inline unsigned long long sd_key(double x) {
  unsigned long long b;
  memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
inline double sd_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  double x;
  memcpy(&x, &b, 8);
  return x;
}

// The one cell-index function, for triangle boxes and for queries alike: every step (rounded subtraction, rounded division by
// a positive number, floor, clamp) is non-decreasing in x, so lo' <= x <= hi' implies sd_cidx(lo') <= sd_cidx(x) <= sd_cidx(hi').
// A triangle is entered into the cells sd_cidx(box lo) .. sd_cidx(box hi) of each axis and counts for a query only if the query
// lies inside that same box: its cell is then one of those.  x is finite.
__device__ __forceinline__ int sd_cidx(double x, double lo, double cell, int n) {
  double q = floor((x - lo) / cell);
  q = q < 0.0 ? 0.0 : q;
  const double top = (double)(n - 1);
  q = q > top ? top : q;
  return (int)q;
}

__device__ __forceinline__ bool sd_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }  // false for NaN

// the grown box of a triangle; min / max by comparison, then one subtraction / addition each
__device__ __forceinline__ void sd_box(const double* a, const double* b, const double* c, double grow, double* lo, double* hi) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double mn = a[k] < b[k] ? a[k] : b[k];
    mn = c[k] < mn ? c[k] : mn;
    double mx = a[k] > b[k] ? a[k] : b[k];
    mx = c[k] > mx ? c[k] : mx;
    lo[k] = mn - grow;
    hi[k] = mx + grow;
  }
}

__device__ __forceinline__ void sd_corners(const double* __restrict__ V, const int* __restrict__ F, int f, double* a, double* b, double* c) {
  const size_t i0 = (size_t)F[3 * (size_t)f], i1 = (size_t)F[3 * (size_t)f + 1], i2 = (size_t)F[3 * (size_t)f + 2];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    a[k] = V[3 * i0 + k];
    b[k] = V[3 * i1 + k];
    c[k] = V[3 * i2 + k];
  }
}

// cell ranges of face f
__device__ __forceinline__ void sd_range(const double* __restrict__ V, const int* __restrict__ F, int f, const SdGrid& g, int* c0, int* c1) {
  double a[3], b[3], c[3], lo[3], hi[3];
  sd_corners(V, F, f, a, b, c);
  sd_box(a, b, c, g.grow, lo, hi);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c0[k] = sd_cidx(lo[k], g.lo[k], g.cell, g.n[k]);
    c1[k] = sd_cidx(hi[k], g.lo[k], g.cell, g.n[k]);
  }
}

// the j-th cell of a face's range (x fastest); the range has at most 2^24 cells
__device__ __forceinline__ int sd_cell(const SdGrid& g, const int* c0, int wx, int wy, int j) {
  const int x = c0[0] + j % wx, y = c0[1] + (j / wx) % wy, z = c0[2] + j / (wx * wy);
  return (z * g.n[1] + y) * g.n[0] + x;
}

__global__ __launch_bounds__(256) void k_sd_bbox(const double* __restrict__ V, int nv, const int* __restrict__ F, int m,
                                                 unsigned long long* __restrict__ counters) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  const double inf = std::numeric_limits<double>::infinity();
  double mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
  bool bad = false;
  if (f < m) {
    const int i0 = F[3 * (size_t)f], i1 = F[3 * (size_t)f + 1], i2 = F[3 * (size_t)f + 2];
    bad = !((unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv);
    if (!bad) {
      const int idx[3] = {i0, i1, i2};
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const double x = V[3 * (size_t)idx[j] + k];
          if (!sd_finite(x)) bad = true;
          mn[k] = x < mn[k] ? x : mn[k];
          mx[k] = x > mx[k] ? x : mx[k];
        }
    }
  }
  if (__ballot(bad)) {  // the call fails: the box is not used
    if (bad) atomicOr(&counters[SD_FLAG], 1ull);
    return;
  }
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double y = __shfl_xor(mn[k], o, 64), z = __shfl_xor(mx[k], o, 64);
      mn[k] = y < mn[k] ? y : mn[k];
      mx[k] = z > mx[k] ? z : mx[k];
    }
  if ((threadIdx.x & 63) == 0 && mn[0] <= mx[0]) {  // a wave with at least one face
#pragma unroll
    for (int k = 0; k < 3; k++) {
      atomicMin(&counters[SD_MIN0 + k], sd_key(mn[k]));
      atomicMax(&counters[SD_MAX0 + k], sd_key(mx[k]));
    }
  }
}

__global__ __launch_bounds__(256) void k_sd_total(const double* __restrict__ V, const int* __restrict__ F, int m, SdGrid g,
                                                  unsigned long long* __restrict__ counters) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  unsigned long long t = 0;
  if (f < m) {
    int c0[3], c1[3];
    sd_range(V, F, f, g, c0, c1);
    t = (unsigned long long)(c1[0] - c0[0] + 1) * (unsigned long long)(c1[1] - c0[1] + 1) * (unsigned long long)(c1[2] - c0[2] + 1);
  }
  unsigned long long big = t;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    t += __shfl_xor(t, o, 64);  // < 2^30 faces x 2^24 cells: no overflow
    const unsigned long long y = __shfl_xor(big, o, 64);
    big = y > big ? y : big;
  }
  if ((threadIdx.x & 63) == 0 && t) {
    atomicAdd(&counters[SD_TOTAL], t);
    atomicMax(&counters[SD_LARGEST], big);
  }
}

__global__ __launch_bounds__(256) void k_sd_count(const double* __restrict__ V, const int* __restrict__ F, int m, SdGrid g,
                                                  int* __restrict__ ccnt) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int c0[3], c1[3];
  sd_range(V, F, f, g, c0, c1);
  const int wx = c1[0] - c0[0] + 1, wy = c1[1] - c0[1] + 1, cnt = wx * wy * (c1[2] - c0[2] + 1);
  for (int j = blockIdx.y; j < cnt; j += gridDim.y) atomicAdd(&ccnt[sd_cell(g, c0, wx, wy, j)], 1);
}

// ccnt counts down to zero: each entry of a cell gets one slot of [coff, coff + count)
__global__ __launch_bounds__(256) void k_sd_fill(const double* __restrict__ V, const int* __restrict__ F, int m, SdGrid g,
                                                 int* __restrict__ ccnt, const int* __restrict__ coff, int* __restrict__ ent) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int c0[3], c1[3];
  sd_range(V, F, f, g, c0, c1);
  const int wx = c1[0] - c0[0] + 1, wy = c1[1] - c0[1] + 1, cnt = wx * wy * (c1[2] - c0[2] + 1);
  for (int j = blockIdx.y; j < cnt; j += gridDim.y) {
    const int c = sd_cell(g, c0, wx, wy, j);
    const int slot = atomicSub(&ccnt[c], 1) - 1;
    ent[(size_t)coff[c] + (size_t)slot] = f;
  }
}

__global__ __launch_bounds__(256) void k_sd_qcell(const double* __restrict__ P, int n, SdGrid g, double hi0, double hi1, double hi2,
                                                  int has_grid, double dm2, int* __restrict__ qc, int* __restrict__ qcnt,
                                                  double* __restrict__ d2, int* __restrict__ face, unsigned long long* __restrict__ counters) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = P[3 * (size_t)i], y = P[3 * (size_t)i + 1], z = P[3 * (size_t)i + 2];
  if (!(sd_finite(x) && sd_finite(y) && sd_finite(z))) {
    atomicOr(&counters[SD_FLAG], 1ull);
    qc[i] = -1;
    return;
  }
  // outside the grid no triangle's grown box holds the point
  if (!has_grid || x < g.lo[0] || y < g.lo[1] || z < g.lo[2] || x > hi0 || y > hi1 || z > hi2) {
    qc[i] = -1;
    d2[i] = dm2;
    face[i] = -1;
    return;
  }
  const int c = (sd_cidx(z, g.lo[2], g.cell, g.n[2]) * g.n[1] + sd_cidx(y, g.lo[1], g.cell, g.n[1])) * g.n[0] + sd_cidx(x, g.lo[0], g.cell, g.n[0]);
  qc[i] = c;
  atomicAdd(&qcnt[c], 1);
}

__global__ __launch_bounds__(256) void k_sd_items(const int* __restrict__ qcnt, int ncells, int* __restrict__ icnt) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < ncells) icnt[c] = (qcnt[c] + 63) >> 6;
}

__global__ __launch_bounds__(256) void k_sd_qfill(const int* __restrict__ qc, int n, int* __restrict__ qcnt, const int* __restrict__ qoff,
                                                  int* __restrict__ qidx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = qc[i];
  if (c < 0) return;
  const int slot = atomicSub(&qcnt[c], 1) - 1;
  qidx[(size_t)qoff[c] + (size_t)slot] = i;
}

// One wave per work item; its cell is the last c with ioff[c] <= item (a search on wave-uniform values: ioff does not decrease,
// cells without queries repeat their neighbour's offset, and ioff[ncells] = the number of items > item).  LDS: 15 x 64 doubles and 64 ints, 7 936 bytes; every lane reads the same triangle at the same
// time (a broadcast), the staging lane writes one triangle (consecutive addresses across lanes).
__global__ __launch_bounds__(64) void k_sd_query(const double* __restrict__ P, const double* __restrict__ V, const int* __restrict__ F,
                                                 const int* __restrict__ ioff, int ncells,
                                                 const int* __restrict__ qoff, const int* __restrict__ qidx,
                                                 const int* __restrict__ coff, const int* __restrict__ ent, double grow, double dm2,
                                                 double* __restrict__ d2, int* __restrict__ face,
                                                 unsigned long long* __restrict__ counters) {
  __shared__ double tri[15][SD_CHUNK];  // a, b, c, box lo, box hi
  __shared__ int trif[SD_CHUNK];
  const int lane = threadIdx.x;
  const int item = (int)blockIdx.x;
  int c = 0, above = ncells;  // ioff[c] <= item < ioff[above]
  while (above - c > 1) {
    const int mid = c + ((above - c) >> 1);
    if (ioff[mid] <= item) c = mid;
    else above = mid;
  }
  const int q0 = qoff[c] + 64 * (item - ioff[c]);
  const int nq = min(64, qoff[c + 1] - q0);
  const int e0 = coff[c], ne = coff[c + 1] - e0;
  const bool has = lane < nq;
  const int qi = has ? qidx[q0 + lane] : 0;
  double p[3] = {0.0, 0.0, 0.0};
  if (has) {
    p[0] = P[3 * (size_t)qi];
    p[1] = P[3 * (size_t)qi + 1];
    p[2] = P[3 * (size_t)qi + 2];
  }
  double best = std::numeric_limits<double>::infinity();
  int bestf = 0x7fffffff;
  for (int base = 0; base < ne; base += SD_CHUNK) {
    const int cnt = min(SD_CHUNK, ne - base);
    if (lane < cnt) {
      const int f = ent[(size_t)e0 + base + lane];
      double a[3], b[3], cc[3], lo[3], hi[3];
      sd_corners(V, F, f, a, b, cc);
      sd_box(a, b, cc, grow, lo, hi);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        tri[k][lane] = a[k];
        tri[3 + k][lane] = b[k];
        tri[6 + k][lane] = cc[k];
        tri[9 + k][lane] = lo[k];
        tri[12 + k][lane] = hi[k];
      }
      trif[lane] = f;
    }
    __syncthreads();
    if (has) {
      for (int t = 0; t < cnt; t++) {
        if (p[0] < tri[9][t] || p[1] < tri[10][t] || p[2] < tri[11][t] || p[0] > tri[12][t] || p[1] > tri[13][t] || p[2] > tri[14][t])
          continue;
        const double a[3] = {tri[0][t], tri[1][t], tri[2][t]};
        const double b[3] = {tri[3][t], tri[4][t], tri[5][t]};
        const double cc[3] = {tri[6][t], tri[7][t], tri[8][t]};
        const double d = sfmx::sd_tri(p, a, b, cc);
        const int f = trif[t];
        if (d < best || (d == best && f < bestf)) {
          best = d;
          bestf = f;
        }
      }
    }
    __syncthreads();
  }
  if (has) {
    const bool hit = best < dm2;
    d2[qi] = hit ? best : dm2;
    face[qi] = hit ? bestf : -1;
  }
  if (lane == 0) atomicAdd(&counters[SD_TESTS], (unsigned long long)nq * (unsigned long long)ne);
}

}  // namespace

struct sfmx_sdist {
  DevBuf tv, tf;          // the target, always a copy of the caller's arrays
  DevBuf cells;           // per cell (+1): ccnt, coff
  DevBuf ent;             // the cells' face lists
  DevBuf qcells;          // per cell (+1): qcnt, qoff, icnt, ioff
  DevBuf qwork;           // per query: qc, qidx
  DevBuf aux;             // the scans' partials
  DevBuf counters;
  DevBuf in_p;            // host queries, staged
  DevBuf out_d2, out_f;
  bool ready = false;
  int nv = 0, m = 0;
  bool has_grid = false;  // false: a target without faces
  SdGrid g{};
  double hi[3] = {};
  double d_max = 0.0, dm2 = 0.0;
  int ncells = 0;
  unsigned long long entries = 0, tests = 0;
  hipEvent_t ev[3] = {};  // first launch, last launch, and in a query the launch of k_sd_query
  double last_us = 0.0, kernel_us = 0.0;
};

namespace {

void sd_time(sfmx_ctx* ctx, sfmx_sdist* sd) {  // after the stream has been synchronised
  float ms = 0.f;
  if (ctx->timing && hipEventElapsedTime(&ms, sd->ev[0], sd->ev[1]) == hipSuccess) sd->last_us = (double)ms * 1000.0;
}

// the number of cells along an axis for the extent hi - lo, or 0 when it does not fit
int sd_axis_cells(double lo, double hi, double cell) {
  const double q = std::floor((hi - lo) / cell);
  if (!(q >= 0.0) || q >= (double)SD_MAX_CELLS) return 0;
  return (int)q + 1;
}

bool sd_dims(const double* lo, const double* hi, double cell, int* n) {
  unsigned long long cells = 1;
  for (int k = 0; k < 3; k++) {
    n[k] = sd_axis_cells(lo[k], hi[k], cell);
    if (n[k] == 0) return false;
    cells *= (unsigned long long)n[k];
    if (cells > (unsigned long long)SD_MAX_CELLS) return false;
  }
  return true;
}

// verts / faces are device pointers (the caller's, or the staged copies in sd->tv / sd->tf)
int sd_set_target(sfmx_ctx* ctx, sfmx_sdist* sd, const double* verts, int nv, const int32_t* faces, int m, const sfmx_sdist_params* p) {
  hipStream_t s = ctx->stream;
  sd->ready = false;
  sd->last_us = 0.0;
  const size_t vb = (size_t)nv * 24, fb = (size_t)m * 12;
  SFMX_HIP(ctx, sd->tv.ensure(vb));
  SFMX_HIP(ctx, sd->tf.ensure(fb));
  SFMX_HIP(ctx, sd->counters.ensure(SD_COUNTERS * 8));
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(sd->ev[0], s));
  if (nv > 0 && verts != sd->tv.p) SFMX_HIP(ctx, hipMemcpyAsync(sd->tv.p, verts, vb, hipMemcpyDeviceToDevice, s));
  if (m > 0 && faces != sd->tf.p) SFMX_HIP(ctx, hipMemcpyAsync(sd->tf.p, faces, fb, hipMemcpyDeviceToDevice, s));
  const double* V = sd->tv.as<double>();
  const int* F = sd->tf.as<int>();
  unsigned long long* counters = sd->counters.as<unsigned long long>();
  unsigned long long c[SD_COUNTERS] = {};
  for (int k = 0; k < 3; k++) c[SD_MIN0 + k] = ~0ull;
  SFMX_HIP(ctx, hipMemcpyAsync(counters, c, sizeof c, hipMemcpyHostToDevice, s));
  const unsigned nbf = (unsigned)(((size_t)m + 255) / 256);
  sd->d_max = p->d_max;
  sd->dm2 = p->d_max * p->d_max;
  sd->nv = nv;
  sd->m = m;
  sd->has_grid = false;
  sd->ncells = 0;
  sd->entries = 0;
  sd->tests = 0;
  sd->g = SdGrid{};
  if (m == 0) {  // every query gets (dm2, -1)
    SFMX_HIP(ctx, hipStreamSynchronize(s));
    sd->ready = true;
    return SFMX_OK;
  }
  k_sd_bbox<<<nbf, 256, 0, s>>>(V, nv, F, m, counters);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, hipMemcpyAsync(c, counters, sizeof c, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  SFMX_REQUIRE(ctx, c[SD_FLAG] == 0);  // a face index outside [0, nv), or a non-finite coordinate in a used vertex
  SdGrid g{};
  g.grow = p->d_max * 1.0009765625;  // d_max (1 + 2^-10)
  double amax = 0.0;
  for (int k = 0; k < 3; k++) {
    const double mn = sd_unkey(c[SD_MIN0 + k]), mx = sd_unkey(c[SD_MAX0 + k]);
    amax = std::fmax(amax, std::fmax(std::fabs(mn), std::fabs(mx)));
    g.lo[k] = mn - g.grow;
    sd->hi[k] = mx + g.grow;
  }
  // beyond this the rounding of `corner - grow` could eat the margin
  SFMX_REQUIRE(ctx, amax <= 1099511627776.0 * p->d_max);
  double cell = p->cell > 0.0 ? p->cell : 2.0 * p->d_max;
  while (true) {
    bool fits = sd_dims(g.lo, sd->hi, cell, g.n);
    if (fits) {
      g.cell = cell;
      SFMX_HIP(ctx, hipMemsetAsync(counters + SD_TOTAL, 0, 16, s));  // and SD_LARGEST
      k_sd_total<<<nbf, 256, 0, s>>>(V, F, m, g, counters);
      SFMX_HIP(ctx, hipGetLastError());
      SFMX_HIP(ctx, hipMemcpyAsync(&c[SD_TOTAL], counters + SD_TOTAL, 16, hipMemcpyDeviceToHost, s));
      SFMX_HIP(ctx, hipStreamSynchronize(s));
      fits = c[SD_TOTAL] <= SD_MAX_ENTRIES;
    }
    if (fits) break;
    SFMX_REQUIRE(ctx, p->cell == 0.0);  // an explicit cell size that does not fit
    cell *= 2.0;
    SFMX_REQUIRE(ctx, std::isfinite(cell));
  }
  const int ncells = g.n[0] * g.n[1] * g.n[2];
  const size_t nc1 = (size_t)ncells + 1;
  SFMX_HIP(ctx, sd->cells.ensure(2 * nc1 * 4));
  SFMX_HIP(ctx, sd->ent.ensure((size_t)c[SD_TOTAL] * 4));
  SFMX_HIP(ctx, sd->aux.ensure(sfmx_scan_aux((int)nc1) * 4));
  int* ccnt = sd->cells.as<int>();
  int* coff = ccnt + nc1;
  SFMX_HIP(ctx, hipMemsetAsync(ccnt, 0, nc1 * 4, s));
  // threads per face: 64 cells each for the largest face, but no more than 2^24 threads in all
  const unsigned long long want = (c[SD_LARGEST] + 63) / 64, room = (1ull << 24) / (unsigned long long)m;
  const unsigned slices = (unsigned)std::max(1ull, std::min(std::min(want, room), 65535ull));
  k_sd_count<<<dim3(nbf, slices), 256, 0, s>>>(V, F, m, g, ccnt);
  sfmx_scan(ccnt, false, (int)nc1, coff, sd->aux.as<int>(), s);
  k_sd_fill<<<dim3(nbf, slices), 256, 0, s>>>(V, F, m, g, ccnt, coff, sd->ent.as<int>());
  SFMX_HIP(ctx, hipGetLastError());
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(sd->ev[1], s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  sd_time(ctx, sd);
  sd->g = g;
  sd->has_grid = true;
  sd->ncells = ncells;
  sd->entries = c[SD_TOTAL];
  sd->ready = true;
  return SFMX_OK;
}

// points is a device pointer
int sd_query(sfmx_ctx* ctx, sfmx_sdist* sd, const double* points, int n, double* d2_out, int32_t* face_out) {
  hipStream_t s = ctx->stream;
  sd->last_us = 0.0;
  sd->kernel_us = 0.0;
  sd->tests = 0;
  if (n == 0) return SFMX_OK;
  const size_t nn = (size_t)n, nc1 = (size_t)sd->ncells + 1;
  const int max_items = (int)(nn / 64 + 1) + sd->ncells;  // sum of ceil(q_c / 64) <= n / 64 + cells with a query
  SFMX_HIP(ctx, sd->out_d2.ensure(nn * 8));
  SFMX_HIP(ctx, sd->out_f.ensure(nn * 4));
  SFMX_HIP(ctx, sd->qcells.ensure(4 * nc1 * 4));
  SFMX_HIP(ctx, sd->qwork.ensure(2 * nn * 4));
  SFMX_HIP(ctx, sd->aux.ensure(sfmx_scan_aux((int)nc1) * 4));
  int* qcnt = sd->qcells.as<int>();
  int* qoff = qcnt + nc1;
  int* icnt = qoff + nc1;
  int* ioff = icnt + nc1;
  int* qc = sd->qwork.as<int>();
  int* qidx = qc + nn;
  unsigned long long* counters = sd->counters.as<unsigned long long>();
  double* d2 = sd->out_d2.as<double>();
  int* face = sd->out_f.as<int>();
  const unsigned nbq = (unsigned)((nn + 255) / 256), nbc = (unsigned)((nc1 + 255) / 256);
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(sd->ev[0], s));
  SFMX_HIP(ctx, hipMemsetAsync(counters, 0, SD_COUNTERS * 8, s));
  SFMX_HIP(ctx, hipMemsetAsync(qcnt, 0, 4 * nc1 * 4, s));
  k_sd_qcell<<<nbq, 256, 0, s>>>(points, n, sd->g, sd->hi[0], sd->hi[1], sd->hi[2], sd->has_grid ? 1 : 0, sd->dm2, qc, qcnt, d2, face,
                                 counters);
  int items = 0;
  unsigned long long c[SD_COUNTERS] = {};
  if (sd->has_grid) {
    k_sd_items<<<nbc, 256, 0, s>>>(qcnt, sd->ncells, icnt);
    sfmx_scan(qcnt, false, (int)nc1, qoff, sd->aux.as<int>(), s);
    sfmx_scan(icnt, false, (int)nc1, ioff, sd->aux.as<int>(), s);
    SFMX_HIP(ctx, hipMemcpyAsync(&items, ioff + sd->ncells, 4, hipMemcpyDeviceToHost, s));
  }
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, hipMemcpyAsync(c, counters, sizeof c, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  SFMX_REQUIRE(ctx, c[SD_FLAG] == 0);  // a non-finite coordinate in a query
  SFMX_REQUIRE(ctx, items >= 0 && items <= max_items);
  if (items > 0) {
    k_sd_qfill<<<nbq, 256, 0, s>>>(qc, n, qcnt, qoff, qidx);
    const int* coff = sd->cells.as<int>() + nc1;
    if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(sd->ev[2], s));
    k_sd_query<<<(unsigned)items, 64, 0, s>>>(points, sd->tv.as<double>(), sd->tf.as<int>(), ioff, sd->ncells, qoff, qidx, coff,
                                              sd->ent.as<int>(), sd->g.grow, sd->dm2, d2, face, counters);
    SFMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->timing) SFMX_HIP(ctx, hipEventRecord(sd->ev[1], s));  // straight after the last launch
  if (items > 0) SFMX_HIP(ctx, hipMemcpyAsync(&c[SD_TESTS], counters + SD_TESTS, 8, hipMemcpyDeviceToHost, s));
  if (d2_out) SFMX_HIP(ctx, hipMemcpyAsync(d2_out, d2, nn * 8, hipMemcpyDeviceToHost, s));
  if (face_out) SFMX_HIP(ctx, hipMemcpyAsync(face_out, face, nn * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  sd_time(ctx, sd);
  float kms = 0.f;
  if (ctx->timing && items > 0 && hipEventElapsedTime(&kms, sd->ev[2], sd->ev[1]) == hipSuccess) sd->kernel_us = (double)kms * 1000.0;
  sd->tests = c[SD_TESTS];
  return SFMX_OK;
}

}  // namespace

int sfmx_sdist_device_state(const sfmx_sdist* sd, const double** verts, const int32_t** faces, int* n_faces, const double** d2,
                            const int32_t** face) {
  const bool ok = sd && sd->ready;
  if (verts) *verts = ok ? sd->tv.as<double>() : nullptr;
  if (faces) *faces = ok ? sd->tf.as<int32_t>() : nullptr;
  if (n_faces) *n_faces = ok ? sd->m : 0;
  if (d2) *d2 = ok ? sd->out_d2.as<double>() : nullptr;
  if (face) *face = ok ? sd->out_f.as<int32_t>() : nullptr;
  return ok ? sd->nv : -1;
}

extern "C" {

void sfmx_sdist_default_params(sfmx_sdist_params* p) {
  if (!p) return;
  *p = sfmx_sdist_params{};
  p->d_max = 0.0;  // no default: it is a length in the caller's units
  p->cell = 0.0;
}

int sfmx_sdist_check_params(const sfmx_sdist_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  // 2^-500 .. 2^60 (NaN fails both): d_max * d_max neither underflows nor, with coordinates up to 2^40 d_max, does tri overflow
  if (!(p->d_max >= 0x1p-500) || !(p->d_max <= 0x1p60)) return SFMX_ERR_INVALID;
  if (!(p->cell >= 0.0) || !std::isfinite(p->cell)) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_sdist_create(sfmx_ctx* ctx, sfmx_sdist** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* sd = new sfmx_sdist;
  hipError_t e = hipEventCreate(&sd->ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&sd->ev[1]);
  if (e == hipSuccess) e = hipEventCreate(&sd->ev[2]);
  if (e != hipSuccess) {
    sfmx_sdist_destroy(ctx, sd);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_sdist_create", e);
  }
  *out = sd;
  return SFMX_OK;
}

void sfmx_sdist_destroy(sfmx_ctx* ctx, sfmx_sdist* sd) {
  if (!sd) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* b : {&sd->tv, &sd->tf, &sd->cells, &sd->ent, &sd->qcells, &sd->qwork, &sd->aux, &sd->counters, &sd->in_p, &sd->out_d2, &sd->out_f})
    b->release();
  for (hipEvent_t ev : sd->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete sd;
}

int sfmx_sdist_set_target(sfmx_ctx* ctx, sfmx_sdist* sd, const double* verts, int nv, const int32_t* faces, int m, int on_device,
                          const sfmx_sdist_params* p) {
  SFMX_REQUIRE(ctx, ctx && sd);
  sd->ready = false;  // every failure from here on leaves no target behind
  SFMX_REQUIRE(ctx, sfmx_sdist_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, nv >= 0 && m >= 0 && nv < (1 << 30) && m < (1 << 30) && (nv == 0 || verts) && (m == 0 || faces));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return sd_set_target(ctx, sd, verts, nv, faces, m, p);
  hipStream_t s = ctx->stream;
  SFMX_HIP(ctx, sd->tv.ensure((size_t)nv * 24));
  SFMX_HIP(ctx, sd->tf.ensure((size_t)m * 12));
  if (nv > 0) SFMX_HIP(ctx, hipMemcpyAsync(sd->tv.p, verts, (size_t)nv * 24, hipMemcpyHostToDevice, s));
  if (m > 0) SFMX_HIP(ctx, hipMemcpyAsync(sd->tf.p, faces, (size_t)m * 12, hipMemcpyHostToDevice, s));
  return sd_set_target(ctx, sd, sd->tv.as<double>(), nv, sd->tf.as<int32_t>(), m, p);
}

int sfmx_sdist_set_target_fusion(sfmx_ctx* ctx, sfmx_sdist* sd, const sfmx_fusion* fu, const sfmx_sdist_params* p) {
  SFMX_REQUIRE(ctx, ctx && sd);
  sd->ready = false;
  SFMX_REQUIRE(ctx, fu && sfmx_sdist_check_params(p) == SFMX_OK);
  const double *v = nullptr, *nr = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_fusion_device_mesh(fu, &v, &nr, &f, &m);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0);  // no current surface on the device
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sd_set_target(ctx, sd, v, n, f, m, p);
}

int sfmx_sdist_set_target_clean(sfmx_ctx* ctx, sfmx_sdist* sd, const sfmx_clean* cl, const sfmx_sdist_params* p) {
  SFMX_REQUIRE(ctx, ctx && sd);
  sd->ready = false;
  SFMX_REQUIRE(ctx, cl && sfmx_sdist_check_params(p) == SFMX_OK);
  const double* v = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_clean_device_mesh(cl, &v, &f, &m);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0);  // no successful run
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sd_set_target(ctx, sd, v, n, f, m, p);
}

int sfmx_sdist_query(sfmx_ctx* ctx, sfmx_sdist* sd, const double* points, int n, int on_device, double* d2_out, int32_t* face_out) {
  SFMX_REQUIRE(ctx, ctx && sd && sd->ready);
  SFMX_REQUIRE(ctx, n >= 0 && n < (1 << 30) && (n == 0 || points));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device || n == 0) return sd_query(ctx, sd, points, n, d2_out, face_out);
  SFMX_HIP(ctx, sd->in_p.ensure((size_t)n * 24));
  SFMX_HIP(ctx, hipMemcpyAsync(sd->in_p.p, points, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
  return sd_query(ctx, sd, sd->in_p.as<double>(), n, d2_out, face_out);
}

int sfmx_sdist_query_fusion(sfmx_ctx* ctx, sfmx_sdist* sd, const sfmx_fusion* fu, int cap, double* d2_out, int32_t* face_out, int* n_out) {
  if (n_out) *n_out = 0;
  SFMX_REQUIRE(ctx, ctx && sd && sd->ready && fu);
  const double *v = nullptr, *nr = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_fusion_device_mesh(fu, &v, &nr, &f, &m);
  SFMX_REQUIRE(ctx, n >= 0);  // no current surface on the device
  SFMX_REQUIRE(ctx, n <= cap || (!d2_out && !face_out));  // the host arrays are too short
  if (n_out) *n_out = n;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sd_query(ctx, sd, v, n, d2_out, face_out);
}

int sfmx_sdist_query_clean(sfmx_ctx* ctx, sfmx_sdist* sd, const sfmx_clean* cl, int cap, double* d2_out, int32_t* face_out, int* n_out) {
  if (n_out) *n_out = 0;
  SFMX_REQUIRE(ctx, ctx && sd && sd->ready && cl);
  const double* v = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_clean_device_mesh(cl, &v, &f, &m);
  SFMX_REQUIRE(ctx, n >= 0);  // no successful run
  SFMX_REQUIRE(ctx, n <= cap || (!d2_out && !face_out));  // the host arrays are too short
  if (n_out) *n_out = n;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sd_query(ctx, sd, v, n, d2_out, face_out);
}

int sfmx_sdist_stats(const sfmx_sdist* sd, int* dims3, int* entries, double* cell, uint64_t* tests, double* kernel_us) {
  if (kernel_us) *kernel_us = 0.0;
  if (dims3) dims3[0] = dims3[1] = dims3[2] = 0;
  if (entries) *entries = 0;
  if (cell) *cell = 0.0;
  if (tests) *tests = 0;
  if (!sd || !sd->ready) return SFMX_ERR_INVALID;
  if (dims3)
    for (int k = 0; k < 3; k++) dims3[k] = sd->g.n[k];
  if (entries) *entries = (int)sd->entries;
  if (cell) *cell = sd->g.cell;
  if (tests) *tests = sd->tests;
  if (kernel_us) *kernel_us = sd->kernel_us;
  return SFMX_OK;
}

double sfmx_sdist_last_us(const sfmx_sdist* sd) { return sd ? sd->last_us : 0.0; }

}  // extern "C"
