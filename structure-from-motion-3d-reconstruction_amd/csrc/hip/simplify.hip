// simplify.hip — exact vertex clustering of an indexed triangle mesh on a uniform grid, on the device.
//
// Exactness: a vertex's cell and its position inside the cell come from one fixed sequence of IEEE double operations
// (-ffp-contract=off), the position is quantised to 2^-30 of the cell, and a cluster's sums are 64-bit INTEGER sums: there is no
// order of additions to pin.  Cluster numbers, duplicate removal and the output offsets are integer scans and integer minima.
// Any schedule gives the same bytes; tests/simplify_ref.py restates it in NumPy and the tests compare bytes.
//
// Kernel layout, one thread per vertex, face or cluster, blocks of 256, all on the context's stream:
//   k_sp_box         a grid-stride loop over the vertices, at most 256 blocks: the three cell indices of each; a non-finite
//                    coordinate, a cell index beyond 2^30 or (with normals) a component that is not finite or beyond 4 sets the
//                    flag (atomicOr); the indices go into the block's box of occupied cells (registers, wave shuffles, 96 bytes
//                    of LDS), stored as one partial box per block
//   -- the host reads the flag and the partial boxes, joins them, sizes the grid and refuses more than 2^27 cells --
//   k_sp_occupy      per vertex: occ[cell] = 1 (a same-value store) and vcell[v] = cell
//   k_scan_*         exclusive int32 scan of occ (scan.hip): the cluster number of every occupied cell, and their count
//   k_sp_accum       per vertex: the cluster's number, then 64-bit integer atomicAdd of Q (and Qn) and a count.  Runs of equal
//                    clusters inside a wave are folded first (a segmented sum over the run, 6 shuffle steps): only the first
//                    lane of a run issues atomics
//   k_sp_faces       per face: an index outside [0, n) sets the flag and the face is skipped; otherwise the triple of its corners'
//                    clusters, dropped when two are equal, else rotated so that the smallest comes first; a flag per face says
//                    whether it has a triple
//   k_sp_dedup       per face with a triple: insertion into an open-addressing table of face indices (int32 slots, cleared to -1,
//                    power-of-two size >= 2 m).  CAS an empty slot; when the occupant's triple is equal, atomicMin the face index
//                    into the slot; otherwise the next slot.  Slots are never emptied, so a triple owns exactly one slot; a failed
//                    CAS hands back the occupant.  No thread waits for another, and a probe sequence is bounded by the table size
//   k_sp_mark        per face: kept iff its triple's slot holds its own index; a kept face flags its three clusters
//   k_scan_*         exclusive int32 scans of the face flags (kept, then has-a-triple, as one array: its two sums count the
//                    degenerate and the duplicate faces without an atomic) and of the cluster flags
//   k_sp_emit_verts  per used cluster: its position (and normal) from the integer sums, its member count
//   k_sp_vert_dst    per input vertex: the output vertex of its cluster, or -1
//   k_mesh_emit_faces  per kept face: its renumbered canonical triple, its input index (sfmx_mesh_dev.h, as clean.hip's)
// No kernel waits on another workgroup or spins on a memory word.  A face with an index out of range is skipped by every per-face
// kernel (they all run before the host reads the flag), so nothing is ever accessed through such an index.
#include <climits>

#include "sfmx_internal.h"
#include "sfmx_mesh_dev.h"

namespace {

constexpr long long SP_MAX_CELLS = 1ll << 27;  // the fusion volume's own limit
constexpr double SP_ONE = 1073741824.0;        // 2^30: the fixed-point scale, and the largest cell index

// counters (int32 each), followed in memory by the partial boxes of k_sp_box: [SP_BOX_BLOCKS][6], min then max per axis
enum { SP_FLAG = 0, SP_NCLUST, SP_NF_OUT, SP_NF_VALID, SP_NV_OUT, SP_COUNTERS = 8 };
constexpr int SP_BOX_BLOCKS = 256;
constexpr int SP_TAIL = SP_COUNTERS + 6 * SP_BOX_BLOCKS;  // ints at the end of the work buffer

struct SpGrid {
  double cell;
  double origin[3];
  int cmin[3];
  int dims[3];
};

// cell index c and fixed-point offset Q of one coordinate; false when x is not finite or |c| > 2^30
__device__ __forceinline__ bool sp_cell(double x, double o, double cell, int& c, long long& Q) {
  const double q = (x - o) / cell;
  const double cf = floor(q);
  if (!(fabs(cf) <= SP_ONE)) return false;  // NaN and infinities included
  const double t = q - cf;
  c = (int)cf;
  Q = (long long)floor(t * SP_ONE + 0.5);
  return true;
}

__device__ __forceinline__ unsigned sp_hash(int a, int b, int c) {
  unsigned h = (unsigned)a * 0x9E3779B1u ^ (unsigned)b * 0x85EBCA77u ^ (unsigned)c * 0xC2B2AE3Du;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}

// Partial boxes, one per block, reduced by the host after the read-back it makes anyway.  The launch is a grid-stride loop over
// at most SP_BOX_BLOCKS blocks and nothing goes through an atomic but the flag: with one thread per vertex and six atomicMin /
// atomicMax per wave (the k_sd_bbox pattern) this kernel took 649 us of a 1 070 us call at 256^3, six words serving 67 000
// atomics one after the other.
__global__ __launch_bounds__(256) void k_sp_box(const double* __restrict__ verts, const double* __restrict__ normals, int n, double cell,
                                                double o0, double o1, double o2, unsigned* __restrict__ counters, int* __restrict__ part) {
  __shared__ int red[4][6];
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  bool bad = false;
  const double o[3] = {o0, o1, o2};
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)n; v += (size_t)gridDim.x * 256) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      int c = 0;
      long long Q;
      if (!sp_cell(verts[3 * v + k], o[k], cell, c, Q)) bad = true;
      mn[k] = min(mn[k], c);
      mx[k] = max(mx[k], c);
      if (normals && !(fabs(normals[3 * v + k]) <= 4.0)) bad = true;  // NaN included
    }
  }
  if (bad) atomicOr(&counters[SP_FLAG], 1u);  // the call fails: the box is not used
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      mn[k] = min(mn[k], __shfl_xor(mn[k], s, 64));
      mx[k] = max(mx[k], __shfl_xor(mx[k], s, 64));
    }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      red[threadIdx.x >> 6][k] = mn[k];
      red[threadIdx.x >> 6][3 + k] = mx[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {  // every block of the launch holds at least one vertex
    const int k = threadIdx.x;
    int r = red[0][k];
    for (int w = 1; w < 4; w++) r = k < 3 ? min(r, red[w][k]) : max(r, red[w][k]);
    part[6 * blockIdx.x + k] = r;
  }
}

// the linear cell index of vertex v and its Q; every vertex has passed k_sp_box's checks and lies inside the box
__device__ __forceinline__ int sp_lin(const double* __restrict__ verts, int v, const SpGrid& g, long long* Q) {
  int c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c[k] = 0;
    sp_cell(verts[3 * (size_t)v + k], g.origin[k], g.cell, c[k], Q[k]);
    c[k] -= g.cmin[k];
  }
  return c[0] + g.dims[0] * (c[1] + g.dims[1] * c[2]);
}

__global__ __launch_bounds__(256) void k_sp_occupy(const double* __restrict__ verts, int n, SpGrid g, int* __restrict__ occ,
                                                   int* __restrict__ vcell) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  long long Q[3];
  const int lin = sp_lin(verts, v, g, Q);
  vcell[v] = lin;
  occ[lin] = 1;
}

template <bool NRM>
__global__ __launch_bounds__(256) void k_sp_accum(const double* __restrict__ verts, const double* __restrict__ normals, int n, SpGrid g,
                                                  const int* __restrict__ off, int* __restrict__ vclu, int* __restrict__ ccell,
                                                  unsigned long long* __restrict__ S, unsigned long long* __restrict__ Sn,
                                                  int* __restrict__ cnt) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  int id = -1, lin = 0;
  long long Q[NRM ? 6 : 3] = {};
  if (v < n) {
    lin = sp_lin(verts, v, g, Q);
    id = off[lin];
    vclu[v] = id;
    if (NRM) {
#pragma unroll
      for (int k = 0; k < 3; k++) Q[3 + k] = (long long)floor(normals[3 * (size_t)v + k] * SP_ONE + 0.5);
    }
  }
  // Fusion order puts neighbouring vertices into neighbouring threads, so a wave holds runs of equal clusters.  A run is
  // summed inside the wave and only its first lane goes to memory; integer sums, so the folding changes no bit.
  const int lane = threadIdx.x & 63;
#ifdef SFMX_SP_NO_FOLD  // diagnostic build for the A/B of DESIGN.md 20 (tools/bench_simplify.py --build-dir): every lane on its own
  const unsigned long long heads = ~0ull;
  const int end = lane + 1;
#else
  const int prev = __shfl_up(id, 1, 64);
  const unsigned long long heads = __ballot(lane == 0 || prev != id);
  const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int end = above ? lane + __ffsll(above) : 64;  // one past the last lane of this lane's run
#endif
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
    for (int k = 0; k < (NRM ? 6 : 3); k++) {
      const long long y = __shfl_down(Q[k], s, 64);
      if (lane + s < end) Q[k] += y;
    }
  }
  if (id >= 0 && ((heads >> lane) & 1)) {
#pragma unroll
    for (int k = 0; k < 3; k++) atomicAdd(&S[3 * (size_t)id + k], (unsigned long long)Q[k]);
    if (NRM) {
#pragma unroll
      for (int k = 0; k < 3; k++) atomicAdd(&Sn[3 * (size_t)id + k], (unsigned long long)Q[3 + k]);
    }
    atomicAdd(&cnt[id], end - lane);
    ccell[id] = lin;  // a same-value store
  }
}

__global__ __launch_bounds__(256) void k_sp_faces(const int* __restrict__ faces, int m, int n, const int* __restrict__ vclu,
                                                  int* __restrict__ tri, int* __restrict__ fvalid, unsigned* __restrict__ counters) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f < m) {
    const int v0 = faces[3 * (size_t)f], v1 = faces[3 * (size_t)f + 1], v2 = faces[3 * (size_t)f + 2];
    int a = -1, b = -1, c = -1;
    if ((unsigned)v0 < (unsigned)n && (unsigned)v1 < (unsigned)n && (unsigned)v2 < (unsigned)n) {
      a = vclu[v0];
      b = vclu[v1];
      c = vclu[v2];
      if (a == b || b == c || a == c) {
        a = -1;
      } else if (b < a && b < c) {  // rotated, never reflected
        const int t = a;
        a = b;
        b = c;
        c = t;
      } else if (c < a && c < b) {
        const int t = c;
        c = b;
        b = a;
        a = t;
      }
    } else {
      atomicOr(&counters[SP_FLAG], 1u);
    }
    tri[3 * (size_t)f] = a;  // -1: no triple
    tri[3 * (size_t)f + 1] = b;
    tri[3 * (size_t)f + 2] = c;
    fvalid[f] = a >= 0 ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_sp_dedup(const int* __restrict__ tri, int m, int* table, unsigned mask,
                                                  unsigned* __restrict__ fslot) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  const int a = tri[3 * (size_t)f];
  if (a < 0) return;
  const int b = tri[3 * (size_t)f + 1], c = tri[3 * (size_t)f + 2];
  unsigned h = sp_hash(a, b, c) & mask;
  // at most mask + 1 probes: the table has more slots than there are triples, and no slot is ever emptied
  for (unsigned probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
    const int cur = atomicCAS(&table[h], -1, f);
    if (cur == -1) {
      fslot[f] = h;
      return;
    }
    // the occupant may be replaced meanwhile, but only by a face of the same triple
    if (tri[3 * (size_t)cur] == a && tri[3 * (size_t)cur + 1] == b && tri[3 * (size_t)cur + 2] == c) {
      atomicMin(&table[h], f);
      fslot[f] = h;
      return;
    }
  }
  fslot[f] = 0;  // not reached: the table has at least twice as many slots as there are faces
}

__global__ __launch_bounds__(256) void k_sp_mark(const int* __restrict__ tri, int m, const int* __restrict__ table,
                                                 const unsigned* __restrict__ fslot, int* __restrict__ fkeep, int* used) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  const int a = tri[3 * (size_t)f];
  const bool keep = a >= 0 && table[fslot[f]] == f;
  fkeep[f] = keep ? 1 : 0;
  if (keep) {
    used[a] = 1;
    used[tri[3 * (size_t)f + 1]] = 1;
    used[tri[3 * (size_t)f + 2]] = 1;
  }
}

__global__ void k_sp_add(int* __restrict__ a, const int* __restrict__ b) {
  if (threadIdx.x == 0) *a += *b;
}

__global__ __launch_bounds__(256) void k_sp_emit_verts(int n, const unsigned* __restrict__ counters, const int* __restrict__ used,
                                                       const int* __restrict__ voff, const int* __restrict__ ccell,
                                                       const unsigned long long* __restrict__ S, const unsigned long long* __restrict__ Sn,
                                                       const int* __restrict__ cnt, SpGrid g, double* __restrict__ verts_out,
                                                       double* __restrict__ normals_out, int* __restrict__ members) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= n || (unsigned)id >= counters[SP_NCLUST] || !used[id]) return;
  const size_t o = (size_t)voff[id];
  const int lin = ccell[id], k = cnt[id];
  const int c[3] = {g.cmin[0] + lin % g.dims[0], g.cmin[1] + (lin / g.dims[0]) % g.dims[1], g.cmin[2] + lin / g.dims[0] / g.dims[1]};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double mean = (double)(long long)S[3 * (size_t)id + a] / (double)k;
    verts_out[3 * o + a] = g.origin[a] + ((double)c[a] + mean / SP_ONE) * g.cell;
  }
  if (Sn) {
    const double s0 = (double)(long long)Sn[3 * (size_t)id], s1 = (double)(long long)Sn[3 * (size_t)id + 1],
                 s2 = (double)(long long)Sn[3 * (size_t)id + 2];
    const double len = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
    normals_out[3 * o] = len == 0.0 ? 0.0 : s0 / len;
    normals_out[3 * o + 1] = len == 0.0 ? 0.0 : s1 / len;
    normals_out[3 * o + 2] = len == 0.0 ? 0.0 : s2 / len;
  }
  members[o] = k;
}

__global__ __launch_bounds__(256) void k_sp_vert_dst(int n, const int* __restrict__ vclu, const int* __restrict__ used,
                                                     const int* __restrict__ voff, int* __restrict__ vdst) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int id = vclu[v];
  vdst[v] = used[id] ? voff[id] : -1;
}

}  // namespace

struct sfmx_simplify {
  // work: per cluster (at most n) S, Sn, cnt, used, ccell, voff; per vertex vcell / vclu; per face tri, fslot, fkeep, fvalid and
  // two offsets; the scans' partials; the counters and the partial boxes.  grid: per cell occ, off and their scan partials.
  // table: the duplicate table.
  DevBuf work, grid, table;
  MeshInput in;  // host inputs, staged
  DevBuf out_v, out_n, out_f, vdst, fsrc, members;
  bool done = false, has_normals = false;
  int n = 0, m = 0, nv_out = 0, nf_out = 0, clusters = 0, degenerate = 0, duplicates = 0;
  StageTimer t;
};

namespace {

size_t sp_up8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

// verts / normals / faces are device pointers
int sp_run(sfmx_ctx* ctx, sfmx_simplify* sp, const double* verts, const double* normals, int n, const int32_t* faces, int m,
           const sfmx_simplify_params* p, int* n_verts_out, int* n_faces_out) {
  hipStream_t s = ctx->stream;
  sp->done = false;
  sp->t.us = 0.0;
  const size_t nn = (size_t)n, mm = (size_t)m;
  const size_t aux = sfmx_scan_aux(n > 2 * m ? n : 2 * m);
  // 64-bit sums first, then the ints; [S | Sn | cnt | used] is cleared in one memset
  const size_t b_sums = (normals ? 48 : 24) * nn, b_clear = b_sums + 8 * nn;
  const size_t b_work = sp_up8(b_clear + 4 * (4 * nn + 8 * mm + aux)) + SP_TAIL * 4;
  SFMX_HIP(ctx, sp->work.ensure(b_work));
  // the outputs are sized by the input: the counts are only known on the host after the launches
  SFMX_HIP(ctx, sp->out_v.ensure(nn * 24));
  if (normals) SFMX_HIP(ctx, sp->out_n.ensure(nn * 24));
  SFMX_HIP(ctx, sp->out_f.ensure(mm * 12));
  SFMX_HIP(ctx, sp->vdst.ensure(nn * 4));
  SFMX_HIP(ctx, sp->fsrc.ensure(mm * 4));
  SFMX_HIP(ctx, sp->members.ensure(nn * 4));
  unsigned long long* S = sp->work.as<unsigned long long>();
  unsigned long long* Sn = normals ? S + 3 * nn : nullptr;
  int* cnt = reinterpret_cast<int*>(S + (normals ? 6 : 3) * nn);
  int* used = cnt + nn;
  int* ccell = used + nn;
  int* voff = ccell + nn;
  int* vclu = voff + nn;  // first the cell of each vertex, then its cluster
  int* vend = vclu + nn;
  int* tri = vend;
  unsigned* fslot = reinterpret_cast<unsigned*>(tri + 3 * mm);
  // [fkeep | fvalid] is one array of 2 m flags under one scan: the sum of its first half is m', the sum of all of it m' plus
  // the faces with a triple.  Degenerate and duplicate faces are counted by these two sums, not by atomics on one word (in
  // k_sp_faces one atomicAdd per wave took 251 us at 256^3: nearly every wave holds a degenerate face)
  int* fkeep = reinterpret_cast<int*>(fslot + mm);
  int* fvalid = fkeep + mm;
  int* foff = fvalid + mm;
  int* ax = foff + 2 * mm;
  unsigned* counters = reinterpret_cast<unsigned*>(sp->work.as<char>() + b_work - SP_TAIL * 4);
  int* part = reinterpret_cast<int*>(counters) + SP_COUNTERS;
  const unsigned nbv = (unsigned)((nn + 255) / 256), nbf = (unsigned)((mm + 255) / 256);
  SFMX_HIP(ctx, sp->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(counters, 0, SP_COUNTERS * 4, s));
  SpGrid g{};
  g.cell = p->cell;
  for (int k = 0; k < 3; k++) g.origin[k] = p->origin[k];
  if (n > 0) {
    const unsigned nbb = nbv < (unsigned)SP_BOX_BLOCKS ? nbv : (unsigned)SP_BOX_BLOCKS;
    k_sp_box<<<nbb, 256, 0, s>>>(verts, normals, n, p->cell, p->origin[0], p->origin[1], p->origin[2], counters, part);
    SFMX_HIP(ctx, hipGetLastError());
    int c[SP_TAIL] = {};
    SFMX_HIP(ctx, hipMemcpyAsync(c, counters, (SP_COUNTERS + 6 * (size_t)nbb) * 4, hipMemcpyDeviceToHost, s));
    SFMX_HIP(ctx, hipStreamSynchronize(s));
    SFMX_REQUIRE(ctx, c[SP_FLAG] == 0);  // a non-finite coordinate, a cell index beyond 2^30, or a bad normal
    long long cells = 1;
    for (int k = 0; k < 3; k++) {
      long long lo = INT_MAX, hi = INT_MIN;
      for (unsigned b = 0; b < nbb; b++) {
        const int* q = c + SP_COUNTERS + 6 * b;
        lo = q[k] < lo ? q[k] : lo;
        hi = q[3 + k] > hi ? q[3 + k] : hi;
      }
      const long long d = hi - lo + 1;  // 1 .. 2^31 + 1
      SFMX_REQUIRE(ctx, d >= 1 && d <= SP_MAX_CELLS);
      g.cmin[k] = (int)lo;
      g.dims[k] = (int)d;
      cells *= d;  // three factors of at most 2^27 each
      SFMX_REQUIRE(ctx, cells <= SP_MAX_CELLS);  // the box of the occupied cells is too large
    }
    const int nc = (int)cells;
    const size_t caux = sfmx_scan_aux(nc);
    SFMX_HIP(ctx, sp->grid.ensure((2 * (size_t)nc + caux) * 4));
    int* occ = sp->grid.as<int>();
    int* off = occ + nc;
    int* cax = off + nc;
    SFMX_HIP(ctx, hipMemsetAsync(occ, 0, (size_t)nc * 4, s));
    SFMX_HIP(ctx, hipMemsetAsync(S, 0, b_clear, s));
    k_sp_occupy<<<nbv, 256, 0, s>>>(verts, n, g, occ, vclu);
    sfmx_scan(occ, false, nc, off, cax, s);
    sfmx_scan_total(occ, false, off, nc, reinterpret_cast<int*>(counters) + SP_NCLUST, s);
    if (normals) k_sp_accum<true><<<nbv, 256, 0, s>>>(verts, normals, n, g, off, vclu, ccell, S, Sn, cnt);
    else k_sp_accum<false><<<nbv, 256, 0, s>>>(verts, nullptr, n, g, off, vclu, ccell, S, nullptr, cnt);
  }
  if (m > 0) {
    size_t slots = 2;
    while (slots < 2 * mm) slots <<= 1;  // at most 2^31
    SFMX_HIP(ctx, sp->table.ensure(slots * 4));
    SFMX_HIP(ctx, hipMemsetAsync(sp->table.p, 0xFF, slots * 4, s));
    k_sp_faces<<<nbf, 256, 0, s>>>(faces, m, n, vclu, tri, fvalid, counters);
    k_sp_dedup<<<nbf, 256, 0, s>>>(tri, m, sp->table.as<int>(), (unsigned)(slots - 1), fslot);
    k_sp_mark<<<nbf, 256, 0, s>>>(tri, m, sp->table.as<int>(), fslot, fkeep, used);
    if (m <= (1 << 30) - 512) {  // 2 m + 1023 fits the scan's int
      sfmx_scan(fkeep, false, 2 * m, foff, ax, s);
      sfmx_scan_total(fkeep, false, foff, m, reinterpret_cast<int*>(counters) + SP_NF_OUT, s);
      sfmx_scan_total(fkeep, false, foff, 2 * m, reinterpret_cast<int*>(counters) + SP_NF_VALID, s);
    } else {  // the two halves on their own; SP_NF_VALID is still the sum of both
      sfmx_scan(fkeep, false, m, foff, ax, s);
      sfmx_scan_total(fkeep, false, foff, m, reinterpret_cast<int*>(counters) + SP_NF_OUT, s);
      sfmx_scan(fvalid, false, m, foff + mm, ax, s);
      sfmx_scan_total(fvalid, false, foff + mm, m, reinterpret_cast<int*>(counters) + SP_NF_VALID, s);
      k_sp_add<<<1, 64, 0, s>>>(reinterpret_cast<int*>(counters) + SP_NF_VALID, reinterpret_cast<const int*>(counters) + SP_NF_OUT);
    }
  }
  if (n > 0) {
    sfmx_scan(used, false, n, voff, ax, s);
    sfmx_scan_total(used, false, voff, n, reinterpret_cast<int*>(counters) + SP_NV_OUT, s);
    k_sp_emit_verts<<<nbv, 256, 0, s>>>(n, counters, used, voff, ccell, S, Sn, cnt, g, sp->out_v.as<double>(), sp->out_n.as<double>(),
                                        sp->members.as<int>());
    k_sp_vert_dst<<<nbv, 256, 0, s>>>(n, vclu, used, voff, sp->vdst.as<int>());
  }
  if (m > 0 && n > 0) sfmx_mesh_emit_faces(tri, m, fkeep, foff, voff, sp->out_f.as<int32_t>(), sp->fsrc.as<int>(), s);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, sp->t.end(ctx));
  unsigned c[SP_COUNTERS] = {};
  SFMX_HIP(ctx, hipMemcpyAsync(c, counters, sizeof c, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  sp->t.collect(ctx);
  SFMX_REQUIRE(ctx, c[SP_FLAG] == 0);  // a face index outside [0, n)
  sp->n = n;
  sp->m = m;
  sp->nv_out = (int)c[SP_NV_OUT];
  sp->nf_out = (int)c[SP_NF_OUT];
  sp->clusters = (int)c[SP_NCLUST];
  const int with_triple = (int)c[SP_NF_VALID] - (int)c[SP_NF_OUT];
  sp->degenerate = m - with_triple;
  sp->duplicates = with_triple - (int)c[SP_NF_OUT];
  sp->has_normals = normals != nullptr;
  sp->done = true;
  if (n_verts_out) *n_verts_out = sp->nv_out;
  if (n_faces_out) *n_faces_out = sp->nf_out;
  return SFMX_OK;
}

void sp_zero(int* a, int* b) {
  if (a) *a = 0;
  if (b) *b = 0;
}

bool sp_finite(double x) { return x - x == 0.0; }

}  // namespace

extern "C" {

void sfmx_simplify_default_params(sfmx_simplify_params* p) {
  if (!p) return;
  *p = sfmx_simplify_params{};  // cell has no default: 0 is refused
}

int sfmx_simplify_check_params(const sfmx_simplify_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!sp_finite(p->cell) || !(p->cell > 0.0)) return SFMX_ERR_INVALID;
  for (double o : p->origin)
    if (!sp_finite(o)) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_simplify_create(sfmx_ctx* ctx, sfmx_simplify** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* sp = new sfmx_simplify;
  const hipError_t e = sp->t.create();
  if (e != hipSuccess) {
    sfmx_simplify_destroy(ctx, sp);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_simplify_create", e);
  }
  *out = sp;
  return SFMX_OK;
}

void sfmx_simplify_destroy(sfmx_ctx* ctx, sfmx_simplify* sp) {
  if (!sp) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  sp->in.release();
  for (DevBuf* b : {&sp->work, &sp->grid, &sp->table, &sp->out_v, &sp->out_n, &sp->out_f, &sp->vdst, &sp->fsrc, &sp->members}) b->release();
  sp->t.destroy();
  delete sp;
}

int sfmx_simplify_run(sfmx_ctx* ctx, sfmx_simplify* sp, const double* verts, const double* normals, int n, const int32_t* faces, int m,
                      int on_device, const sfmx_simplify_params* p, int* n_verts_out, int* n_faces_out) {
  sp_zero(n_verts_out, n_faces_out);
  SFMX_REQUIRE(ctx, ctx && sp);
  sp->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, sfmx_simplify_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && n < (1 << 30) && m < (1 << 30) && (n == 0 || verts) && (m == 0 || faces));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return sp_run(ctx, sp, verts, normals, n, faces, m, p, n_verts_out, n_faces_out);
  MeshDev d;
  SFMX_HIP(ctx, sp->in.stage(verts, normals, n, faces, m, ctx->stream, d));
  return sp_run(ctx, sp, d.verts, d.normals, n, d.faces, m, p, n_verts_out, n_faces_out);
}

int sfmx_simplify_fusion(sfmx_ctx* ctx, sfmx_simplify* sp, const sfmx_fusion* fu, const sfmx_simplify_params* p, int* n_verts_out,
                         int* n_faces_out) {
  sp_zero(n_verts_out, n_faces_out);
  SFMX_REQUIRE(ctx, ctx && sp);
  sp->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, fu && sfmx_simplify_check_params(p) == SFMX_OK);
  const double *v = nullptr, *nr = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_fusion_device_mesh(fu, &v, &nr, &f, &m);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0);  // no current surface on the device
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sp_run(ctx, sp, v, nr, n, f, m, p, n_verts_out, n_faces_out);
}

int sfmx_simplify_clean(sfmx_ctx* ctx, sfmx_simplify* sp, const sfmx_clean* cl, const sfmx_simplify_params* p, int* n_verts_out,
                        int* n_faces_out) {
  sp_zero(n_verts_out, n_faces_out);
  SFMX_REQUIRE(ctx, ctx && sp);
  sp->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, cl && sfmx_simplify_check_params(p) == SFMX_OK);
  const double *v = nullptr, *v2 = nullptr, *nr = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_clean_device_mesh(cl, &v, &f, &m);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && sfmx_clean_device_surface(cl, &v2, &nr) == n);  // no cleaned surface on the device
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return sp_run(ctx, sp, v, nr, n, f, m, p, n_verts_out, n_faces_out);
}

int sfmx_simplify_read(sfmx_ctx* ctx, sfmx_simplify* sp, double* verts_out, double* normals_out, int32_t* faces_out, int32_t* vert_dst,
                       int32_t* face_src, int32_t* members) {
  SFMX_REQUIRE(ctx, ctx && sp && sp->done);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t nv = (size_t)sp->nv_out, nf = (size_t)sp->nf_out, n = (size_t)sp->n;
  if (verts_out && nv) SFMX_HIP(ctx, hipMemcpyAsync(verts_out, sp->out_v.p, nv * 24, hipMemcpyDeviceToHost, s));
  if (normals_out && nv && sp->has_normals) SFMX_HIP(ctx, hipMemcpyAsync(normals_out, sp->out_n.p, nv * 24, hipMemcpyDeviceToHost, s));
  if (faces_out && nf) SFMX_HIP(ctx, hipMemcpyAsync(faces_out, sp->out_f.p, nf * 12, hipMemcpyDeviceToHost, s));
  if (vert_dst && n) SFMX_HIP(ctx, hipMemcpyAsync(vert_dst, sp->vdst.p, n * 4, hipMemcpyDeviceToHost, s));
  if (face_src && nf) SFMX_HIP(ctx, hipMemcpyAsync(face_src, sp->fsrc.p, nf * 4, hipMemcpyDeviceToHost, s));
  if (members && nv) SFMX_HIP(ctx, hipMemcpyAsync(members, sp->members.p, nv * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

int sfmx_simplify_sizes(const sfmx_simplify* sp, int* n, int* m, int* n_verts_out, int* n_faces_out) {
  sp_zero(n, m);
  sp_zero(n_verts_out, n_faces_out);
  if (!sp || !sp->done) return SFMX_ERR_INVALID;
  if (n) *n = sp->n;
  if (m) *m = sp->m;
  if (n_verts_out) *n_verts_out = sp->nv_out;
  if (n_faces_out) *n_faces_out = sp->nf_out;
  return SFMX_OK;
}

int sfmx_simplify_counts(const sfmx_simplify* sp, int* clusters, int* degenerate, int* duplicates, int* n_verts_out, int* n_faces_out) {
  sp_zero(clusters, degenerate);
  sp_zero(duplicates, n_verts_out);
  sp_zero(n_faces_out, nullptr);
  if (!sp || !sp->done) return SFMX_ERR_INVALID;
  if (clusters) *clusters = sp->clusters;
  if (degenerate) *degenerate = sp->degenerate;
  if (duplicates) *duplicates = sp->duplicates;
  if (n_verts_out) *n_verts_out = sp->nv_out;
  if (n_faces_out) *n_faces_out = sp->nf_out;
  return SFMX_OK;
}

int sfmx_simplify_device_surface(const sfmx_simplify* sp, const double** verts, const double** normals) {
  if (verts) *verts = nullptr;
  if (normals) *normals = nullptr;
  if (!sp || !sp->done) return -1;
  if (verts) *verts = sp->out_v.as<double>();
  if (normals && sp->has_normals) *normals = sp->out_n.as<double>();
  return sp->nv_out;
}

int sfmx_simplify_device_mesh(const sfmx_simplify* sp, const double** verts, const int32_t** faces, int* n_faces) {
  if (verts) *verts = nullptr;
  if (faces) *faces = nullptr;
  if (n_faces) *n_faces = 0;
  if (!sp || !sp->done) return -1;
  if (verts) *verts = sp->out_v.as<double>();
  if (faces) *faces = sp->out_f.as<int32_t>();
  if (n_faces) *n_faces = sp->nf_out;
  return sp->nv_out;
}

double sfmx_simplify_last_us(const sfmx_simplify* sp) { return sp ? sp->t.us : 0.0; }

}  // extern "C"
