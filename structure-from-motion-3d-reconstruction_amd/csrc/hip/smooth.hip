// smooth.hip — exact Taubin lambda|mu smoothing of an indexed triangle mesh on the device.
//
// Exactness: a vertex's fixed-point position Q comes from one fixed sequence of IEEE double operations (-ffp-contract=off), a
// vertex's neighbours are the ends of its distinct undirected edges, and the sum over them is a 64-bit INTEGER sum: neither the
// order of a neighbour list nor the slot an edge lands in can show.  Each step is then one fixed expression per vertex.  Any
// schedule gives the same bytes; tests/smooth_ref.py restates it in NumPy and the tests compare bytes.
//
// Kernel layout, blocks of 256, all on the context's stream:
//   k_sm_quant    per vertex: Q = floor(q 2^20 + 0.5); a coordinate that is not finite or with |q| > 2^18 sets the flag (a plain
//                 same-value store) and gets Q = 0
//   k_sm_edges    per face: an index outside [0, n) sets the flag and the face is skipped; otherwise each directed edge with two
//                 different ends goes into an open-addressing table of uint64 keys lo << 32 | hi (all ones = empty, power-of-two
//                 size >= 4 m): a 64-bit CAS on an empty slot, or a match on the returned occupant, else the next slot of the
//                 key's probe sequence (et_slot, sfmx_edge_table.h); then an atomicAdd on the slot's fwd or bwd counter.  Slots are never emptied, no thread waits for another, and a probe
//                 sequence is bounded by the table size
//   k_sm_degree   a grid-stride loop over the slots, at most 1 024 blocks: an occupied slot adds 1 to cnt[lo] and cnt[hi]; one that
//                 is not regular stores the pinned byte of both ends (same value); the three edge counts are summed inside the
//                 block and stored as one partial per block
//   -- the host reads the flag and the partial counts (first synchronisation) and sizes the CSR columns --
//   k_scan_*      exclusive int32 scan of cnt (scan.hip): the CSR row starts
//   k_sm_fill     a grid-stride loop over the slots: each end of an occupied slot takes the next place of the other end's row
//                 (an atomicAdd cursor per row; the order inside a row depends on the schedule and cannot show)
//   k_sm_step     per vertex, 2 iters launches: a vertex that moves gathers the 3 x int64 of each neighbour from the Q array of
//                 the previous step and writes the other Q array; no atomics, no LDS.  |Q'| > 2^38 sets the diverged flag and
//                 keeps the old Q, so that every later sum stays below 2^62
//   k_sm_emit     a grid-stride loop over the vertices, at most 1 024 blocks: the output position (a moving vertex) or the input
//                 bytes, the flag byte, and one partial per block of the pinned and the isolated counts
//   -- the host reads the diverged flag and the partial counts (second synchronisation) --
// No kernel waits on another workgroup or spins on a memory word.
#include "sfmx_edge_table.h"
#include "sfmx_internal.h"

namespace {

constexpr double SM_SCALE = 1048576.0;            // 2^20: the fixed-point scale
constexpr double SM_MAX_Q = 262144.0;             // 2^18: the largest |q| of an input coordinate
constexpr long long SM_MAX_FIXED = 1ll << 38;     // the largest |Q| after a step
constexpr int SM_PART_BLOCKS = 1024;

// counters (int32 each): two flags, then the partial counts of k_sm_degree [SM_PART_BLOCKS][3] and of k_sm_emit [..][2]
enum { SM_FLAG = 0, SM_DIVERGED, SM_HEAD = 8 };
constexpr int SM_EDGE_PART = SM_HEAD;
constexpr int SM_VERT_PART = SM_EDGE_PART + 3 * SM_PART_BLOCKS;
constexpr int SM_COUNTERS = SM_VERT_PART + 2 * SM_PART_BLOCKS;

__global__ __launch_bounds__(256) void k_sm_quant(const double* __restrict__ verts, int n, double unit, double o0, double o1, double o2,
                                                  long long* __restrict__ Q, int* __restrict__ counters) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const double o[3] = {o0, o1, o2};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double q = (verts[3 * (size_t)v + k] - o[k]) / unit;
    long long r = 0;
    if (fabs(q) <= SM_MAX_Q) r = (long long)floor(q * SM_SCALE + 0.5);
    else counters[SM_FLAG] = 1;  // NaN and infinities included; the call fails
    Q[3 * (size_t)v + k] = r;
  }
}

__global__ __launch_bounds__(256) void k_sm_edges(const int* __restrict__ faces, int m, int n, unsigned long long* keys, int* uses,
                                                  unsigned long long mask, int nbits, int* __restrict__ counters) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  et_insert_face(faces, f, n, keys, uses, mask, nbits, counters + SM_FLAG);
}

__global__ __launch_bounds__(256) void k_sm_degree(const unsigned long long* __restrict__ keys, const int* __restrict__ uses, size_t slots,
                                                   int* cnt, unsigned char* pinned, int* __restrict__ counters) {
  int c[3] = {0, 0, 0};  // edges, boundary, irregular
  for (size_t h = (size_t)blockIdx.x * 256 + threadIdx.x; h < slots; h += (size_t)gridDim.x * 256) {
    const unsigned long long key = keys[h];
    if (key == ET_EMPTY) continue;
    const unsigned lo = (unsigned)(key >> 32), hi = (unsigned)key;
    const int fwd = uses[2 * h], bwd = uses[2 * h + 1];
    atomicAdd(&cnt[lo], 1);
    atomicAdd(&cnt[hi], 1);
    c[0]++;
    if (fwd == 1 && bwd == 1) continue;
    pinned[lo] = 1;
    pinned[hi] = 1;
    if (fwd + bwd == 1) c[1]++;
    else c[2]++;
  }
  const int s = sfmx_block_sums(c);
  if (threadIdx.x < 3) counters[SM_EDGE_PART + 3 * blockIdx.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_sm_fill(const unsigned long long* __restrict__ keys, size_t slots, const int* __restrict__ row,
                                                 int* cursor, int* __restrict__ col) {
  for (size_t h = (size_t)blockIdx.x * 256 + threadIdx.x; h < slots; h += (size_t)gridDim.x * 256) {
    const unsigned long long key = keys[h];
    if (key == ET_EMPTY) continue;
    const unsigned lo = (unsigned)(key >> 32), hi = (unsigned)key;
    col[(size_t)row[lo] + (size_t)atomicAdd(&cursor[lo], 1)] = (int)hi;
    col[(size_t)row[hi] + (size_t)atomicAdd(&cursor[hi], 1)] = (int)lo;
  }
}

__global__ __launch_bounds__(256) void k_sm_step(int n, const long long* __restrict__ Qin, long long* __restrict__ Qout,
                                                 const int* __restrict__ cnt, const int* __restrict__ row, const int* __restrict__ col,
                                                 const unsigned char* __restrict__ pinned, int pin, double f, int* __restrict__ counters) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const long long q0 = Qin[3 * (size_t)v], q1 = Qin[3 * (size_t)v + 1], q2 = Qin[3 * (size_t)v + 2];
  long long r0 = q0, r1 = q1, r2 = q2;
  const int c = cnt[v];
  if (c > 0 && !(pin && pinned[v])) {
    long long s0 = 0, s1 = 0, s2 = 0;  // |S| < 2^24 2^38
    const int* __restrict__ nb = col + row[v];
    for (int j = 0; j < c; j++) {
      const size_t u = (size_t)nb[j];
      s0 += Qin[3 * u];
      s1 += Qin[3 * u + 1];
      s2 += Qin[3 * u + 2];
    }
    const double k = (double)c;
    r0 = q0 + (long long)floor(f * ((double)s0 / k - (double)q0) + 0.5);
    r1 = q1 + (long long)floor(f * ((double)s1 / k - (double)q1) + 0.5);
    r2 = q2 + (long long)floor(f * ((double)s2 / k - (double)q2) + 0.5);
    if (llabs(r0) > SM_MAX_FIXED || llabs(r1) > SM_MAX_FIXED || llabs(r2) > SM_MAX_FIXED) {
      counters[SM_DIVERGED] = 1;  // the call fails; the vertex stays where it was, so every later sum is bounded too
      r0 = q0;
      r1 = q1;
      r2 = q2;
    }
  }
  Qout[3 * (size_t)v] = r0;
  Qout[3 * (size_t)v + 1] = r1;
  Qout[3 * (size_t)v + 2] = r2;
}

__global__ __launch_bounds__(256) void k_sm_emit(const double* __restrict__ verts, int n, const long long* __restrict__ Q,
                                                 const int* __restrict__ cnt, const unsigned char* __restrict__ pinned, int pin, double unit,
                                                 double o0, double o1, double o2, double* __restrict__ out, unsigned char* __restrict__ flags,
                                                 int* __restrict__ counters) {
  int c[2] = {0, 0};  // pinned, isolated
  const double o[3] = {o0, o1, o2};
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)n; v += (size_t)gridDim.x * 256) {
    const bool iso = cnt[v] == 0;
    const bool pnd = pin && pinned[v];
    c[0] += pnd ? 1 : 0;
    c[1] += iso ? 1 : 0;
    flags[v] = (unsigned char)((pnd ? 1 : 0) | (iso ? 2 : 0));
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double x = verts[3 * v + k];
      out[3 * v + k] = (iso || pnd) ? x : o[k] + ((double)Q[3 * v + k] * (1.0 / SM_SCALE)) * unit;
    }
  }
  const int s = sfmx_block_sums(c);
  if (threadIdx.x < 2) counters[SM_VERT_PART + 2 * blockIdx.x + threadIdx.x] = s;
}

}  // namespace

struct sfmx_smooth {
  // work: Q (two arrays), cnt, row starts, cursors, the scan's partials, the pinned bytes and the counters.  table: the keys and
  // the two use counters of every slot.  col: the CSR columns.
  DevBuf work, table, col;
  MeshInput in;  // host inputs, staged; in.in_f is also the faces _device_mesh hands out for them
  DevBuf out_v, flags;
  const int32_t* faces = nullptr;   // the faces of the last successful run, on the device
  const double* normals = nullptr;  // the normals its source carried on the device (_fusion, _clean), or null
  bool done = false;
  int n = 0, m = 0, counts[5] = {};
  StageTimer t;
};

namespace {

size_t sm_up8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

bool sm_finite(double x) { return x - x == 0.0; }

// verts / faces are device pointers
int sm_run(sfmx_ctx* ctx, sfmx_smooth* sm, const double* verts, int n, const int32_t* faces, int m, const sfmx_smooth_params* p) {
  hipStream_t s = ctx->stream;
  sm->done = false;
  sm->t.us = 0.0;
  const size_t nn = (size_t)n, mm = (size_t)m;
  const size_t aux = sfmx_scan_aux(n > 0 ? n : 1);
  // [cnt | cursor | pinned] is cleared in one memset
  const size_t b_q = 2 * 24 * nn, b_clear = sm_up8(8 * nn + nn), b_work = b_q + b_clear + sm_up8(4 * (nn + aux)) + SM_COUNTERS * 4;
  SFMX_HIP(ctx, sm->work.ensure(b_work));
  SFMX_HIP(ctx, sm->out_v.ensure(nn * 24));
  SFMX_HIP(ctx, sm->flags.ensure(nn));
  long long* Q0 = sm->work.as<long long>();
  long long* Q1 = Q0 + 3 * nn;
  int* cnt = reinterpret_cast<int*>(Q1 + 3 * nn);
  int* cursor = cnt + nn;
  unsigned char* pinned = reinterpret_cast<unsigned char*>(cursor + nn);
  int* row = reinterpret_cast<int*>(sm->work.as<char>() + b_q + b_clear);
  int* ax = row + nn;
  int* counters = reinterpret_cast<int*>(sm->work.as<char>() + b_work - SM_COUNTERS * 4);
  size_t slots = 0;
  if (m > 0) {
    slots = et_slots(mm);
    SFMX_HIP(ctx, sm->table.ensure(slots * 16));
  }
  unsigned long long* keys = sm->table.as<unsigned long long>();
  int* uses = reinterpret_cast<int*>(keys + slots);
  const unsigned nbv = (unsigned)((nn + 255) / 256), nbf = (unsigned)((mm + 255) / 256);
  const unsigned nbs = (unsigned)((slots + 255) / 256 < (size_t)SM_PART_BLOCKS ? (slots + 255) / 256 : (size_t)SM_PART_BLOCKS);
  const unsigned nbe = nbv < (unsigned)SM_PART_BLOCKS ? nbv : (unsigned)SM_PART_BLOCKS;
  SFMX_HIP(ctx, sm->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(counters, 0, SM_COUNTERS * 4, s));
  if (n > 0) {
    SFMX_HIP(ctx, hipMemsetAsync(cnt, 0, b_clear, s));
    k_sm_quant<<<nbv, 256, 0, s>>>(verts, n, p->unit, p->origin[0], p->origin[1], p->origin[2], Q0, counters);
  }
  if (m > 0) {
    SFMX_HIP(ctx, hipMemsetAsync(keys, 0xFF, slots * 8, s));
    SFMX_HIP(ctx, hipMemsetAsync(uses, 0, slots * 8, s));
    k_sm_edges<<<nbf, 256, 0, s>>>(faces, m, n, keys, uses, (unsigned long long)(slots - 1), et_nbits(n), counters);
    if (n > 0) k_sm_degree<<<nbs, 256, 0, s>>>(keys, uses, slots, cnt, pinned, counters);
  }
  SFMX_HIP(ctx, hipGetLastError());
  int c[SM_COUNTERS] = {};
  SFMX_HIP(ctx, hipMemcpyAsync(c, counters, (size_t)SM_VERT_PART * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  SFMX_REQUIRE(ctx, c[SM_FLAG] == 0);  // a coordinate that is not finite or beyond 2^18 units, or a face index outside [0, n)
  long long edges = 0, boundary = 0, irregular = 0;
  for (unsigned b = 0; b < nbs && m > 0 && n > 0; b++) {
    edges += c[SM_EDGE_PART + 3 * b];
    boundary += c[SM_EDGE_PART + 3 * b + 1];
    irregular += c[SM_EDGE_PART + 3 * b + 2];
  }
  SFMX_REQUIRE(ctx, edges <= (1ll << 30) - 1024);  // the CSR row starts are int32
  const long long* Q = Q0;
  if (n > 0) {
    if (edges > 0) {
      SFMX_HIP(ctx, sm->col.ensure((size_t)edges * 8));
      sfmx_scan(cnt, false, n, row, ax, s);
      k_sm_fill<<<nbs, 256, 0, s>>>(keys, slots, row, cursor, sm->col.as<int>());
      long long* Qa = Q0;
      long long* Qb = Q1;
      for (int step = 0; step < 2 * p->iters; step++) {
        k_sm_step<<<nbv, 256, 0, s>>>(n, Qa, Qb, cnt, row, sm->col.as<int>(), pinned, p->pin, (step & 1) ? p->mu : p->lambda, counters);
        long long* t = Qa;
        Qa = Qb;
        Qb = t;
      }
      Q = Qa;
    }
    k_sm_emit<<<nbe, 256, 0, s>>>(verts, n, Q, cnt, pinned, p->pin, p->unit, p->origin[0], p->origin[1], p->origin[2],
                                  sm->out_v.as<double>(), sm->flags.as<unsigned char>(), counters);
  }
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, sm->t.end(ctx));
  SFMX_HIP(ctx, hipMemcpyAsync(c, counters, sizeof c, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  sm->t.collect(ctx);
  SFMX_REQUIRE(ctx, c[SM_DIVERGED] == 0);  // a fixed-point coordinate beyond 2^38 at some step
  long long npin = 0, niso = 0;
  for (unsigned b = 0; b < nbe; b++) {
    npin += c[SM_VERT_PART + 2 * b];
    niso += c[SM_VERT_PART + 2 * b + 1];
  }
  sm->n = n;
  sm->m = m;
  sm->faces = faces;
  sm->normals = nullptr;
  sm->counts[0] = (int)edges;
  sm->counts[1] = (int)boundary;
  sm->counts[2] = (int)irregular;
  sm->counts[3] = (int)npin;
  sm->counts[4] = (int)niso;
  sm->done = true;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_smooth_default_params(sfmx_smooth_params* p) {
  if (!p) return;
  *p = sfmx_smooth_params{};  // unit has no default: 0 is refused
  p->lambda = 0.5;
  p->mu = -0.53;
  p->iters = 10;
  p->pin = 1;
}

int sfmx_smooth_check_params(const sfmx_smooth_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!sm_finite(p->unit) || !(p->unit > 0.0)) return SFMX_ERR_INVALID;
  for (double o : p->origin)
    if (!sm_finite(o)) return SFMX_ERR_INVALID;
  if (!(p->lambda > 0.0 && p->lambda <= 1.0) || !(p->mu >= -1.0 && p->mu <= 0.0)) return SFMX_ERR_INVALID;  // NaN included
  if (p->iters < 1 || p->iters > 64 || (p->pin != 0 && p->pin != 1)) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_smooth_create(sfmx_ctx* ctx, sfmx_smooth** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* sm = new sfmx_smooth;
  const hipError_t e = sm->t.create();
  if (e != hipSuccess) {
    sfmx_smooth_destroy(ctx, sm);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_smooth_create", e);
  }
  *out = sm;
  return SFMX_OK;
}

void sfmx_smooth_destroy(sfmx_ctx* ctx, sfmx_smooth* sm) {
  if (!sm) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  sm->in.release();
  for (DevBuf* b : {&sm->work, &sm->table, &sm->col, &sm->out_v, &sm->flags}) b->release();
  sm->t.destroy();
  delete sm;
}

int sfmx_smooth_run(sfmx_ctx* ctx, sfmx_smooth* sm, const double* verts, int n, const int32_t* faces, int m, int on_device,
                    const sfmx_smooth_params* p) {
  SFMX_REQUIRE(ctx, ctx && sm);
  sm->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, sfmx_smooth_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && n < (1 << 24) && m < (1 << 30) && (n == 0 || verts) && (m == 0 || faces));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return sm_run(ctx, sm, verts, n, faces, m, p);
  MeshDev d;
  SFMX_HIP(ctx, sm->in.stage(verts, nullptr, n, faces, m, ctx->stream, d));
  return sm_run(ctx, sm, d.verts, n, d.faces, m, p);
}

int sfmx_smooth_fusion(sfmx_ctx* ctx, sfmx_smooth* sm, const sfmx_fusion* fu, const sfmx_smooth_params* p) {
  SFMX_REQUIRE(ctx, ctx && sm);
  sm->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, fu && sfmx_smooth_check_params(p) == SFMX_OK);
  const double *v = nullptr, *nr = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_fusion_device_mesh(fu, &v, &nr, &f, &m);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && n < (1 << 24));  // no current surface on the device, or too many vertices
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = sm_run(ctx, sm, v, n, f, m, p);
  if (rc == SFMX_OK) sm->normals = nr;
  return rc;
}

int sfmx_smooth_clean(sfmx_ctx* ctx, sfmx_smooth* sm, const sfmx_clean* cl, const sfmx_smooth_params* p) {
  SFMX_REQUIRE(ctx, ctx && sm);
  sm->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, cl && sfmx_smooth_check_params(p) == SFMX_OK);
  const double *v = nullptr, *v2 = nullptr, *nr = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_clean_device_mesh(cl, &v, &f, &m);
  // no cleaned surface on the device, or too many vertices
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && n < (1 << 24) && sfmx_clean_device_surface(cl, &v2, &nr) == n);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = sm_run(ctx, sm, v, n, f, m, p);
  if (rc == SFMX_OK) sm->normals = nr;
  return rc;
}

int sfmx_smooth_read(sfmx_ctx* ctx, sfmx_smooth* sm, double* verts_out, uint8_t* flags_out) {
  SFMX_REQUIRE(ctx, ctx && sm && sm->done);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t n = (size_t)sm->n;
  if (verts_out && n) SFMX_HIP(ctx, hipMemcpyAsync(verts_out, sm->out_v.p, n * 24, hipMemcpyDeviceToHost, s));
  if (flags_out && n) SFMX_HIP(ctx, hipMemcpyAsync(flags_out, sm->flags.p, n, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

int sfmx_smooth_sizes(const sfmx_smooth* sm, int* n, int* m) {
  if (n) *n = 0;
  if (m) *m = 0;
  if (!sm || !sm->done) return SFMX_ERR_INVALID;
  if (n) *n = sm->n;
  if (m) *m = sm->m;
  return SFMX_OK;
}

int sfmx_smooth_counts(const sfmx_smooth* sm, int* edges, int* boundary_edges, int* irregular_edges, int* pinned, int* isolated) {
  int* out[5] = {edges, boundary_edges, irregular_edges, pinned, isolated};
  for (int k = 0; k < 5; k++)
    if (out[k]) *out[k] = sm && sm->done ? sm->counts[k] : 0;
  return sm && sm->done ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_smooth_device_mesh(const sfmx_smooth* sm, const double** verts, const int32_t** faces, int* n_faces) {
  if (verts) *verts = nullptr;
  if (faces) *faces = nullptr;
  if (n_faces) *n_faces = 0;
  if (!sm || !sm->done) return -1;
  if (verts) *verts = sm->out_v.as<double>();
  if (faces) *faces = sm->faces;
  if (n_faces) *n_faces = sm->m;
  return sm->n;
}

int sfmx_smooth_device_surface(const sfmx_smooth* sm, const double** verts, const double** normals) {
  if (verts) *verts = nullptr;
  if (normals) *normals = nullptr;
  if (!sm || !sm->done) return -1;
  if (verts) *verts = sm->out_v.as<double>();
  if (normals) *normals = sm->normals;
  return sm->n;
}

double sfmx_smooth_last_us(const sfmx_smooth* sm) { return sm ? sm->t.us : 0.0; }

}  // extern "C"
