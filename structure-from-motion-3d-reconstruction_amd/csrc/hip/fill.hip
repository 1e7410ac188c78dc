// fill.hip — exact filling of the small holes of an indexed triangle mesh by centroid fans on the device.
//
// Exactness: the edge table gives every undirected edge its two use counts whatever the schedule; a vertex's gap counts are
// integer sums over the boundary edges; a loop is found from its smallest vertex alone and walked in one fixed order; its
// centroid is a 64-bit INTEGER sum of fixed-point positions and its normal a sequential double sum in that order.  The offsets
// of the new vertices and faces are exclusive scans over the vertex index, so the loops come out in ascending leader order.  Any
// schedule gives the same bytes; tests/fill_ref.py restates it in NumPy and the tests compare bytes.
//
// Kernel layout, blocks of 256, all on the context's stream:
//   k_fl_check    per vertex: a coordinate that is not finite or with |q| > 2^18 sets the flag (a plain same-value store)
//   k_fl_edges    per face: an index outside [0, n) sets the flag and the face is skipped; otherwise each directed edge goes into
//                 the edge table (sfmx_edge_table.h: smooth's insert, with the same key, probe sequence and counters)
//   k_fl_gaps     a grid-stride loop over the slots, at most 1 024 blocks: a boundary slot adds 1 to out[tail] and in[head] of its
//                 gap half-edge and stores next[tail] = head (a plain store: next is read only where out == 1, where one slot
//                 wrote it); an irregular slot stores a same-value byte on both ends; the three edge counts are one partial
//                 per block
//   k_fl_class    a grid-stride loop over the vertices, at most 1 024 blocks: a vertex that is not simple gets next = -1, so
//                 that next >= 0 says simple from here on; the complex vertices are one partial per block
//   k_fl_walk     a grid-stride loop over the vertices, at most 1 024 blocks: a simple vertex follows next for at most max_edges
//                 steps and gives up on a vertex that is not simple or smaller than itself, so only a loop's leader comes
//                 back to itself; it writes its new-vertex count (0 or 1) and its new-face count (1 or L) at its own index;
//                 the filled loops are one partial per block
//   k_scan_*      exclusive int32 scans of the two count arrays (scan.hip) and their totals
//   -- the host reads the flag, the partials and the two totals (the one synchronisation before the result) and sizes the outputs --
//   device-to-device copies of the input rows
//   k_fl_emit     per vertex, a leader goes on: one lane walks its loop again, writes the faces, sums Q and the normals, and writes
//                 the centroid and its normal at the loop's offsets
// No kernel waits on another workgroup or spins on a memory word.
#include "sfmx_edge_table.h"
#include "sfmx_internal.h"

namespace {

constexpr double FL_SCALE = 1048576.0;  // 2^20: the fixed-point scale
constexpr double FL_MAX_Q = 262144.0;   // 2^18: the largest |q| of an input coordinate
constexpr int FL_MAX_EDGES = 1024;
constexpr int FL_PART_BLOCKS = 1024;

// counters (int32 each): the flag and the two scan totals, then the partial counts of k_fl_gaps [FL_PART_BLOCKS][3], of k_fl_class
// [..][1] and of k_fl_walk [..][1]
enum { FL_FLAG = 0, FL_NEW_VERTS, FL_NEW_FACES, FL_HEAD = 8 };
constexpr int FL_EDGE_PART = FL_HEAD;
constexpr int FL_CPLX_PART = FL_EDGE_PART + 3 * FL_PART_BLOCKS;
constexpr int FL_LOOP_PART = FL_CPLX_PART + FL_PART_BLOCKS;
constexpr int FL_COUNTERS = FL_LOOP_PART + FL_PART_BLOCKS;

__global__ __launch_bounds__(256) void k_fl_check(const double* __restrict__ verts, int n, double unit, double o0, double o1, double o2,
                                                  int* __restrict__ counters) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const double o[3] = {o0, o1, o2};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double q = (verts[3 * (size_t)v + k] - o[k]) / unit;
    if (!(fabs(q) <= FL_MAX_Q)) counters[FL_FLAG] = 1;  // NaN and infinities included; the call fails
  }
}

__global__ __launch_bounds__(256) void k_fl_edges(const int* __restrict__ faces, int m, int n, unsigned long long* keys, int* uses,
                                                  unsigned long long mask, int nbits, int* __restrict__ counters) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  et_insert_face(faces, f, n, keys, uses, mask, nbits, counters + FL_FLAG);
}

__global__ __launch_bounds__(256) void k_fl_gaps(const unsigned long long* __restrict__ keys, const int* __restrict__ uses, size_t slots,
                                                 int* outc, int* inc, int* next, unsigned char* irr, int* __restrict__ counters) {
  int c[3] = {0, 0, 0};  // edges, boundary, irregular
  for (size_t h = (size_t)blockIdx.x * 256 + threadIdx.x; h < slots; h += (size_t)gridDim.x * 256) {
    const unsigned long long key = keys[h];
    if (key == ET_EMPTY) continue;
    const unsigned lo = (unsigned)(key >> 32), hi = (unsigned)key;
    const int fwd = uses[2 * h], bwd = uses[2 * h + 1];
    c[0]++;
    if (fwd == 1 && bwd == 1) continue;
    if (fwd + bwd == 1) {
      // used as lo -> hi: the gap half-edge is hi -> lo, and the other way round
      const unsigned tail = fwd ? hi : lo, head = fwd ? lo : hi;
      atomicAdd(&outc[tail], 1);
      atomicAdd(&inc[head], 1);
      next[tail] = (int)head;
      c[1]++;
    } else {
      irr[lo] = 1;
      irr[hi] = 1;
      c[2]++;
    }
  }
  const int s = sfmx_block_sums(c);
  if (threadIdx.x < 3) counters[FL_EDGE_PART + 3 * blockIdx.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_fl_class(int n, const int* __restrict__ outc, const int* __restrict__ inc,
                                                  const unsigned char* __restrict__ irr, int* __restrict__ next, int* __restrict__ counters) {
  int c[1] = {0};  // complex vertices
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)n; v += (size_t)gridDim.x * 256) {
    const int o = outc[v], i = inc[v];
    if (o == 1 && i == 1 && !irr[v]) continue;
    next[v] = -1;
    c[0] += (o != 0 || i != 0) ? 1 : 0;
  }
  const int s = sfmx_block_sums(c);
  if (threadIdx.x == 0) counters[FL_CPLX_PART + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_fl_walk(int n, const int* __restrict__ next, int max_edges, int* __restrict__ kv, int* __restrict__ kf,
                                                 int* __restrict__ counters) {
  int c[1] = {0};  // filled loops
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
    const int v = (int)i;
    int L = 0, cur = next[v];
    if (cur >= 0) {
      for (int step = 1; step <= max_edges; step++) {
        if (cur == v) {
          L = step;
          break;
        }
        if (cur < v) break;  // a smaller vertex: v is not the leader
        cur = next[cur];
        if (cur < 0) break;  // a vertex that is not simple: a chain, not a loop
      }
    }
    kv[v] = L > 3 ? 1 : 0;
    kf[v] = L == 3 ? 1 : L;
    c[0] += L > 0 ? 1 : 0;
  }
  const int s = sfmx_block_sums(c);
  if (threadIdx.x == 0) counters[FL_LOOP_PART + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_fl_emit(const double* __restrict__ verts, const double* __restrict__ normals, int n, int m,
                                                 const int* __restrict__ next, const int* __restrict__ kf, const int* __restrict__ voff,
                                                 const int* __restrict__ foff, double unit, double o0, double o1, double o2,
                                                 double* __restrict__ out_v, double* __restrict__ out_n, int* __restrict__ out_f) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int F = kf[v];
  if (F == 0) return;
  int* __restrict__ fo = out_f + 3 * ((size_t)m + (size_t)foff[v]);
  if (F == 1) {  // a loop of three: one face, no vertex
    const int a = next[v];
    fo[0] = v;
    fo[1] = a;
    fo[2] = next[a];
    return;
  }
  const int L = F;
  const int c = n + voff[v];
  const double o[3] = {o0, o1, o2};
  long long S[3] = {0, 0, 0};      // |S| <= 2^10 2^38
  double s[3] = {0.0, 0.0, 0.0};
  int cur = v;
  for (int i = 0; i < L; i++) {
    const int nx = next[cur];
    fo[3 * (size_t)i] = cur;
    fo[3 * (size_t)i + 1] = nx;
    fo[3 * (size_t)i + 2] = c;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double q = (verts[3 * (size_t)cur + k] - o[k]) / unit;
      S[k] += (long long)floor(q * FL_SCALE + 0.5);
      if (normals) s[k] += normals[3 * (size_t)cur + k];
    }
    cur = nx;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const long long num = 2 * S[k] + L, den = 2 * (long long)L;
    long long q = num / den;
    if (num % den < 0) q--;  // a true floor: / truncates
    out_v[3 * (size_t)c + k] = o[k] + ((double)q * (1.0 / FL_SCALE)) * unit;
  }
  if (normals) {
    const double ln = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) out_n[3 * (size_t)c + k] = ln > 0.0 ? s[k] / ln : 0.0;
  }
}

}  // namespace

struct sfmx_fill {
  // work: the gap counts, next, the irregular bytes, the loop counts, their scans, the scan's partials and the counters.
  // table: the keys and the two use counters of every slot.
  DevBuf work, table;
  MeshInput in;  // host inputs, staged
  DevBuf out_v, out_n, out_f;
  bool done = false, has_normals = false;
  int n = 0, m = 0, n_out = 0, m_out = 0, counts[8] = {};
  StageTimer t;
};

namespace {

size_t fl_up8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

bool fl_finite(double x) { return x - x == 0.0; }

// verts / normals / faces are device pointers
int fl_run(sfmx_ctx* ctx, sfmx_fill* fl, const double* verts, const double* normals, int n, const int32_t* faces, int m,
           const sfmx_fill_params* p) {
  hipStream_t s = ctx->stream;
  fl->done = false;
  fl->t.us = 0.0;
  const size_t nn = (size_t)n, mm = (size_t)m;
  const size_t aux = sfmx_scan_aux(n > 0 ? n : 1);
  // [out | in | irr] is cleared in one memset; next is set to -1
  const size_t b_clear = fl_up8(8 * nn + nn), b_next = fl_up8(4 * nn), b_rest = fl_up8(4 * (4 * nn + aux));
  const size_t b_work = b_clear + b_next + b_rest + FL_COUNTERS * 4;
  SFMX_HIP(ctx, fl->work.ensure(b_work));
  int* outc = fl->work.as<int>();
  int* inc = outc + nn;
  unsigned char* irr = reinterpret_cast<unsigned char*>(inc + nn);
  int* next = reinterpret_cast<int*>(fl->work.as<char>() + b_clear);
  int* kv = reinterpret_cast<int*>(fl->work.as<char>() + b_clear + b_next);
  int* kf = kv + nn;
  int* voff = kf + nn;
  int* foff = voff + nn;
  int* ax = foff + nn;
  int* counters = reinterpret_cast<int*>(fl->work.as<char>() + b_work - FL_COUNTERS * 4);
  size_t slots = 0;
  if (m > 0) {
    slots = et_slots(mm);
    SFMX_HIP(ctx, fl->table.ensure(slots * 16));
  }
  unsigned long long* keys = fl->table.as<unsigned long long>();
  int* uses = reinterpret_cast<int*>(keys + slots);
  const unsigned nbv = (unsigned)((nn + 255) / 256), nbf = (unsigned)((mm + 255) / 256);
  const unsigned nbs = (unsigned)((slots + 255) / 256 < (size_t)FL_PART_BLOCKS ? (slots + 255) / 256 : (size_t)FL_PART_BLOCKS);
  const unsigned nbp = nbv < (unsigned)FL_PART_BLOCKS ? nbv : (unsigned)FL_PART_BLOCKS;
  const bool table = m > 0 && n > 0;
  SFMX_HIP(ctx, fl->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(counters, 0, FL_COUNTERS * 4, s));
  if (n > 0) {
    SFMX_HIP(ctx, hipMemsetAsync(outc, 0, b_clear, s));
    SFMX_HIP(ctx, hipMemsetAsync(next, 0xFF, 4 * nn, s));
    k_fl_check<<<nbv, 256, 0, s>>>(verts, n, p->unit, p->origin[0], p->origin[1], p->origin[2], counters);
  }
  if (m > 0) {
    SFMX_HIP(ctx, hipMemsetAsync(keys, 0xFF, slots * 8, s));
    SFMX_HIP(ctx, hipMemsetAsync(uses, 0, slots * 8, s));
    k_fl_edges<<<nbf, 256, 0, s>>>(faces, m, n, keys, uses, (unsigned long long)(slots - 1), et_nbits(n), counters);
    if (n > 0) k_fl_gaps<<<nbs, 256, 0, s>>>(keys, uses, slots, outc, inc, next, irr, counters);
  }
  if (n > 0) {
    k_fl_class<<<nbp, 256, 0, s>>>(n, outc, inc, irr, next, counters);
    k_fl_walk<<<nbp, 256, 0, s>>>(n, next, p->max_edges, kv, kf, counters);
    sfmx_scan(kv, false, n, voff, ax, s);
    sfmx_scan_total(kv, false, voff, n, counters + FL_NEW_VERTS, s);
    sfmx_scan(kf, false, n, foff, ax, s);
    sfmx_scan_total(kf, false, foff, n, counters + FL_NEW_FACES, s);
  }
  SFMX_HIP(ctx, hipGetLastError());
  int c[FL_COUNTERS] = {};
  SFMX_HIP(ctx, hipMemcpyAsync(c, counters, sizeof c, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  SFMX_REQUIRE(ctx, c[FL_FLAG] == 0);  // a coordinate that is not finite or beyond 2^18 units, or a face index outside [0, n)
  long long edges = 0, boundary = 0, irregular = 0, cplx = 0, loops = 0;
  for (unsigned b = 0; b < nbs && table; b++) {
    edges += c[FL_EDGE_PART + 3 * b];
    boundary += c[FL_EDGE_PART + 3 * b + 1];
    irregular += c[FL_EDGE_PART + 3 * b + 2];
  }
  for (unsigned b = 0; b < nbp; b++) {
    cplx += c[FL_CPLX_PART + b];
    loops += c[FL_LOOP_PART + b];
  }
  // the new faces are at most the boundary edges, and boundary <= 3 m < 2^32 could pass int32: the scans above are exact only
  // below 2^31, which this bound (smooth's) guarantees; their totals are not looked at before it
  SFMX_REQUIRE(ctx, edges <= (1ll << 30) - 1024);
  const long long K = c[FL_NEW_VERTS], F = c[FL_NEW_FACES];
  SFMX_REQUIRE(ctx, (long long)n + K < (1ll << 24) && (long long)m + F < (1ll << 30));
  const size_t n_out = nn + (size_t)K, m_out = mm + (size_t)F;
  SFMX_HIP(ctx, fl->out_v.ensure(n_out * 24));
  SFMX_HIP(ctx, fl->out_f.ensure(m_out * 12));
  if (normals) SFMX_HIP(ctx, fl->out_n.ensure(n_out * 24));
  if (n > 0) {
    SFMX_HIP(ctx, hipMemcpyAsync(fl->out_v.p, verts, nn * 24, hipMemcpyDeviceToDevice, s));
    if (normals) SFMX_HIP(ctx, hipMemcpyAsync(fl->out_n.p, normals, nn * 24, hipMemcpyDeviceToDevice, s));
  }
  if (m > 0) SFMX_HIP(ctx, hipMemcpyAsync(fl->out_f.p, faces, mm * 12, hipMemcpyDeviceToDevice, s));
  if (F > 0)
    k_fl_emit<<<nbv, 256, 0, s>>>(verts, normals, n, m, next, kf, voff, foff, p->unit, p->origin[0], p->origin[1], p->origin[2],
                                  fl->out_v.as<double>(), normals ? fl->out_n.as<double>() : nullptr, fl->out_f.as<int>());
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, fl->t.end(ctx));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  fl->t.collect(ctx);
  fl->n = n;
  fl->m = m;
  fl->n_out = (int)n_out;
  fl->m_out = (int)m_out;
  fl->has_normals = normals != nullptr;
  fl->counts[0] = (int)edges;
  fl->counts[1] = (int)boundary;
  fl->counts[2] = (int)irregular;
  fl->counts[3] = (int)cplx;
  fl->counts[4] = (int)loops;
  fl->counts[5] = (int)(F + 2 * (loops - K));  // a loop of three gives one face for three edges, a longer one a face per edge
  fl->counts[6] = (int)K;
  fl->counts[7] = (int)F;
  fl->done = true;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_fill_default_params(sfmx_fill_params* p) {
  if (!p) return;
  *p = sfmx_fill_params{};  // unit has no default: 0 is refused
  p->max_edges = 32;
}

int sfmx_fill_check_params(const sfmx_fill_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!fl_finite(p->unit) || !(p->unit > 0.0)) return SFMX_ERR_INVALID;
  for (double o : p->origin)
    if (!fl_finite(o)) return SFMX_ERR_INVALID;
  if (p->max_edges < 3 || p->max_edges > FL_MAX_EDGES) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_fill_create(sfmx_ctx* ctx, sfmx_fill** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* fl = new sfmx_fill;
  const hipError_t e = fl->t.create();
  if (e != hipSuccess) {
    sfmx_fill_destroy(ctx, fl);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_fill_create", e);
  }
  *out = fl;
  return SFMX_OK;
}

void sfmx_fill_destroy(sfmx_ctx* ctx, sfmx_fill* fl) {
  if (!fl) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  fl->in.release();
  for (DevBuf* b : {&fl->work, &fl->table, &fl->out_v, &fl->out_n, &fl->out_f}) b->release();
  fl->t.destroy();
  delete fl;
}

int sfmx_fill_run(sfmx_ctx* ctx, sfmx_fill* fl, const double* verts, const double* normals, int n, const int32_t* faces, int m,
                  int on_device, const sfmx_fill_params* p) {
  SFMX_REQUIRE(ctx, ctx && fl);
  fl->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, sfmx_fill_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && n < (1 << 24) && m < (1 << 30) && (n == 0 || verts) && (m == 0 || faces));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  const double* nrm = n > 0 ? normals : nullptr;  // an empty mesh passes no normals on, from the host or from the device
  if (on_device) return fl_run(ctx, fl, verts, nrm, n, faces, m, p);
  MeshDev d;
  SFMX_HIP(ctx, fl->in.stage(verts, nrm, n, faces, m, ctx->stream, d));
  return fl_run(ctx, fl, d.verts, d.normals, n, d.faces, m, p);
}

int sfmx_fill_fusion(sfmx_ctx* ctx, sfmx_fill* fl, const sfmx_fusion* fu, const sfmx_fill_params* p) {
  SFMX_REQUIRE(ctx, ctx && fl);
  fl->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, fu && sfmx_fill_check_params(p) == SFMX_OK);
  const double *v = nullptr, *nr = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_fusion_device_mesh(fu, &v, &nr, &f, &m);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && n < (1 << 24));  // no current surface on the device, or too many vertices
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return fl_run(ctx, fl, v, n > 0 ? nr : nullptr, n, f, m, p);
}

int sfmx_fill_clean(sfmx_ctx* ctx, sfmx_fill* fl, const sfmx_clean* cl, const sfmx_fill_params* p) {
  SFMX_REQUIRE(ctx, ctx && fl);
  fl->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, cl && sfmx_fill_check_params(p) == SFMX_OK);
  const double *v = nullptr, *v2 = nullptr, *nr = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_clean_device_mesh(cl, &v, &f, &m);
  // no cleaned surface on the device, or too many vertices
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && n < (1 << 24) && sfmx_clean_device_surface(cl, &v2, &nr) == n);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return fl_run(ctx, fl, v, n > 0 ? nr : nullptr, n, f, m, p);
}

int sfmx_fill_read(sfmx_ctx* ctx, sfmx_fill* fl, double* verts_out, double* normals_out, int32_t* faces_out) {
  SFMX_REQUIRE(ctx, ctx && fl && fl->done);
  SFMX_REQUIRE(ctx, !normals_out || fl->has_normals);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t n = (size_t)fl->n_out, m = (size_t)fl->m_out;
  if (verts_out && n) SFMX_HIP(ctx, hipMemcpyAsync(verts_out, fl->out_v.p, n * 24, hipMemcpyDeviceToHost, s));
  if (normals_out && n) SFMX_HIP(ctx, hipMemcpyAsync(normals_out, fl->out_n.p, n * 24, hipMemcpyDeviceToHost, s));
  if (faces_out && m) SFMX_HIP(ctx, hipMemcpyAsync(faces_out, fl->out_f.p, m * 12, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

int sfmx_fill_sizes(const sfmx_fill* fl, int* n, int* m, int* n_out, int* m_out) {
  int* out[4] = {n, m, n_out, m_out};
  const int val[4] = {fl ? fl->n : 0, fl ? fl->m : 0, fl ? fl->n_out : 0, fl ? fl->m_out : 0};
  for (int k = 0; k < 4; k++)
    if (out[k]) *out[k] = fl && fl->done ? val[k] : 0;
  return fl && fl->done ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_fill_counts(const sfmx_fill* fl, int* edges, int* boundary_edges, int* irregular_edges, int* complex_vertices, int* filled_loops,
                     int* filled_edges, int* new_verts, int* new_faces) {
  int* out[8] = {edges, boundary_edges, irregular_edges, complex_vertices, filled_loops, filled_edges, new_verts, new_faces};
  for (int k = 0; k < 8; k++)
    if (out[k]) *out[k] = fl && fl->done ? fl->counts[k] : 0;
  return fl && fl->done ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_fill_device_mesh(const sfmx_fill* fl, const double** verts, const int32_t** faces, int* n_verts, int* n_faces) {
  if (verts) *verts = nullptr;
  if (faces) *faces = nullptr;
  if (n_verts) *n_verts = 0;
  if (n_faces) *n_faces = 0;
  if (!fl || !fl->done) return -1;
  if (verts) *verts = fl->out_v.as<double>();
  if (faces) *faces = fl->out_f.as<int32_t>();
  if (n_verts) *n_verts = fl->n_out;
  if (n_faces) *n_faces = fl->m_out;
  return fl->n_out;
}

int sfmx_fill_device_surface(const sfmx_fill* fl, const double** verts, const double** normals) {
  if (verts) *verts = nullptr;
  if (normals) *normals = nullptr;
  if (!fl || !fl->done) return -1;
  if (verts) *verts = fl->out_v.as<double>();
  if (normals) *normals = fl->has_normals ? fl->out_n.as<double>() : nullptr;
  return fl->n_out;
}

double sfmx_fill_last_us(const sfmx_fill* fl) { return fl ? fl->t.us : 0.0; }

}  // extern "C"
