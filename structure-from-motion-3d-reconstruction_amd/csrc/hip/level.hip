// level.hip — levelling the seams of a texture atlas: exact per-view vertex offsets.
//
// A sfmx_level takes a mesh and the sfmx_texture whose last run was on it (texture.hip).  Every corner of a textured
// face belongs to the node (vertex, view of the face).  A node samples its view's image at its vertex, in 1/256 grey level.  A
// vertex with nodes of two or more views is a seam vertex: its nodes are pinned to the offset that brings them to the rounded
// mean of their samples.  Every other node is free and starts at 0.  T Jacobi sweeps give every free node the rounded mean of its
// neighbours (the nodes of the same view it shares a face edge with).  The levelled atlas is the texture's atlas with the
// barycentric blend of the three corner offsets added to every texel before the one rounding.
//
// Exactness: a node is a set member, a sample is a fixed sequence of double operations (built with -ffp-contract=off), the sums
// are integers and a sweep reads one buffer and writes the other; node numbers and the order of a row's neighbours depend on the
// schedule and no output depends on them.  tests/level_ref.py restates it in NumPy; the tests compare bytes.
//
// Kernel layout (blocks of 256, the context's stream, no inter-workgroup hand-off, no spinning, no scratch):
//   k_lv_insert   one thread per corner: the range check of the face's indices (the call's flag) and the node (v << 32 | k)
//                 into a lock-free open-addressing table; the thread that claims a slot numbers the node (one atomicAdd per
//                 wave), takes its sample and adds it to its vertex's view count and sample sum (integer atomics)
//   (one read-back: the flag and the number of nodes)
//   k_lv_edges    per textured face: its corners' node numbers, and its three node edges into the edge table (sfmx_edge_table.h)
//   k_lv_verts    per vertex: the seam vertices counted
//   k_lv_pin      per node: pinned with target - sample, or free with 0, into both buffers
//   k_lv_deg      per slot of the edge table: the degrees of both ends;  k_scan_*: the rows;  k_lv_fill: the rows' neighbours
//   k_lv_sweep    T launches: one thread per node gathers its row from one buffer and writes the other
//   k_lv_corners  per corner: corner_adj and corner_sample
//   k_lv_bake     k_tx_bake's body (sfmx_texture_dev.h: tx_bake<true>) with three more int32 per half cell in LDS: the levelled atlas
// Two host synchronisations per run: after the node count, and at the end (the counts).
#include <cmath>

#include "sfmx_edge_table.h"
#include "sfmx_internal.h"
#include "sfmx_texture_dev.h"

namespace {

constexpr int LV_ITER_MAX = 65536;

enum { LV_FLAG = 0, LV_NODES, LV_SEAM, LV_PINNED, LV_EDGES, LV_NWORDS = 8 };  // int32 words read back

// floor(a / b), b > 0
__device__ __forceinline__ long long lv_floordiv(long long a, long long b) {
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// adds the number of set predicates of the wave to *counter with one atomicAdd; every lane of the wave calls it
__device__ __forceinline__ void lv_count(bool pred, int* counter) {
  const unsigned long long b = __ballot(pred);
  if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(counter, __popcll(b));
}

__global__ __launch_bounds__(256) void k_lv_insert(const double* __restrict__ verts, const int* __restrict__ faces, long long corners,
                                                   int n, const int* __restrict__ fview, const RsSlot* __restrict__ slots,
                                                   const uint8_t* __restrict__ img, int L, int fill, unsigned long long* keys,
                                                   unsigned long long mask, int* __restrict__ ids, unsigned* __restrict__ cslot,
                                                   unsigned long long* __restrict__ nkey, int* __restrict__ nfx, int* vcnt,
                                                   unsigned long long* vsum, int* words) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  bool win = false;
  unsigned long long slot = 0, key = 0;
  if (t < corners) {
    const long long f = t / 3;
    const int c = (int)(t - 3 * f);
    int a0, a1, a2;
    const bool ok = mesh_face(faces, (int)f, n, a0, a1, a2);
    if (!ok && c == 0) atomicOr(&words[LV_FLAG], 1);  // the call fails; nothing is read through the index
    const int k = fview[f];
    if (ok && k >= 0) {
      const int v = c == 0 ? a0 : (c == 1 ? a1 : a2);
      key = (unsigned long long)(unsigned)v << 32 | (unsigned)k;
      const unsigned long long hk = et_hash(key);
      // a bounded number of probes: the table has more slots than there are corners, and no slot is ever emptied
      for (unsigned long long probe = 0; probe <= mask; probe++) {
        const unsigned long long h = (hk + probe) & mask;
        const unsigned long long cur = atomicCAS(&keys[h], ET_EMPTY, key);
        if (cur == ET_EMPTY || cur == key) {
          win = cur == ET_EMPTY;
          slot = h;
          break;
        }
      }
      cslot[t] = (unsigned)slot;
    }
  }
  // the wave's new nodes take consecutive numbers behind one atomicAdd
  const unsigned long long b = __ballot(win);
  int id = 0;
  if (b) {
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)b) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&words[LV_NODES], __popcll(b));
    base = __shfl(base, leader, 64);
    id = base + __popcll(b & ((1ull << lane) - 1ull));
  }
  if (!win) return;
  const int v = (int)(key >> 32), k = (int)(unsigned)key;
  const RsSlot& S = slots[k];
  const double dl = (double)L;
  const double X0 = (dl * verts[3 * (size_t)v]) / dl, X1 = (dl * verts[3 * (size_t)v + 1]) / dl, X2 = (dl * verts[3 * (size_t)v + 2]) / dl;
  int fx = 256 * fill;
  const TxSample sm = tx_sample(S.cam, S.img_off, img, X0, X1, X2);
  if (sm.ok) fx = (int)(long long)floor(sm.g * 256.0 + 0.5);
  ids[slot] = id;
  nkey[id] = key;
  nfx[id] = fx;
  atomicAdd(&vcnt[v], 1);  // integers: the order does not matter
  atomicAdd(&vsum[v], (unsigned long long)fx);
}

__global__ __launch_bounds__(256) void k_lv_edges(int m, const int* __restrict__ fview, const unsigned* __restrict__ cslot,
                                                  const int* __restrict__ ids, int* __restrict__ cnode, unsigned long long* ekeys,
                                                  int* euses, unsigned long long emask, int nbits) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m || fview[f] < 0) return;
  const int a = ids[cslot[3 * (size_t)f]], b = ids[cslot[3 * (size_t)f + 1]], c = ids[cslot[3 * (size_t)f + 2]];
  cnode[3 * (size_t)f] = a;
  cnode[3 * (size_t)f + 1] = b;
  cnode[3 * (size_t)f + 2] = c;
  et_insert(a, b, ekeys, euses, emask, nbits);  // an edge of two faces of one view is one key
  et_insert(b, c, ekeys, euses, emask, nbits);
  et_insert(c, a, ekeys, euses, emask, nbits);
}

__global__ __launch_bounds__(256) void k_lv_verts(int n, const int* __restrict__ vcnt, int* words) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  lv_count(v < n && vcnt[v] >= 2, &words[LV_SEAM]);
}

__global__ __launch_bounds__(256) void k_lv_pin(int nodes, const unsigned long long* __restrict__ nkey, const int* __restrict__ nfx,
                                                const int* __restrict__ vcnt, const unsigned long long* __restrict__ vsum,
                                                int* __restrict__ g0, int* __restrict__ g1, uint8_t* __restrict__ pin, int* words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool pinned = false;
  if (i < nodes) {
    const int v = (int)(nkey[i] >> 32);
    const long long c = vcnt[v];
    int g = 0;
    if (c >= 2) {
      pinned = true;
      g = (int)((2 * (long long)vsum[v] + c) / (2 * c) - (long long)nfx[i]);  // the numerator is not negative
    }
    g0[i] = g;
    g1[i] = g;
    pin[i] = pinned ? 1 : 0;
  }
  lv_count(pinned, &words[LV_PINNED]);
}

__global__ __launch_bounds__(256) void k_lv_deg(unsigned long long eslots, const unsigned long long* __restrict__ ekeys, int* deg, int* words) {
  const unsigned long long h = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long key = h < eslots ? ekeys[h] : ET_EMPTY;
  if (key != ET_EMPTY) {
    atomicAdd(&deg[(int)(key >> 32)], 1);
    atomicAdd(&deg[(int)(unsigned)key], 1);
  }
  lv_count(key != ET_EMPTY, &words[LV_EDGES]);
}

// row: the exclusive scan of deg, exact modulo 2^32 (it is below 2^32: at most 6 m entries)
__global__ __launch_bounds__(256) void k_lv_fill(unsigned long long eslots, const unsigned long long* __restrict__ ekeys,
                                                 const unsigned* __restrict__ row, int* cur, int* __restrict__ adj) {
  const unsigned long long h = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (h >= eslots) return;
  const unsigned long long key = ekeys[h];
  if (key == ET_EMPTY) return;
  const int lo = (int)(key >> 32), hi = (int)(unsigned)key;
  adj[(size_t)row[lo] + (size_t)atomicAdd(&cur[lo], 1)] = hi;  // the order inside a row does not matter: the sum is an integer
  adj[(size_t)row[hi] + (size_t)atomicAdd(&cur[hi], 1)] = lo;
}

__global__ __launch_bounds__(256) void k_lv_sweep(int nodes, const unsigned* __restrict__ row, const int* __restrict__ deg,
                                                  const int* __restrict__ adj, const uint8_t* __restrict__ pin,
                                                  const int* __restrict__ gin, int* __restrict__ gout) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nodes || pin[i]) return;  // a pinned node has its value in both buffers
  const int d = deg[i];
  if (d == 0) return;  // a free node has neighbours; one of a face with a repeated vertex stays at 0
  const int* a = adj + (size_t)row[i];
  long long sum = 0;
  for (int e = 0; e < d; e++) sum += gin[a[e]];
  gout[i] = (int)lv_floordiv(2 * sum + d, 2 * (long long)d);
}

__global__ __launch_bounds__(256) void k_lv_corners(long long corners, const int* __restrict__ fview, const int* __restrict__ cnode,
                                                    const int* __restrict__ g, const int* __restrict__ nfx, int* __restrict__ cadj,
                                                    int* __restrict__ csamp) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= corners) return;
  int ga = 0, s = 0;
  if (fview[t / 3] >= 0) {
    const int id = cnode[t];
    ga = g[id];
    s = nfx[id];
  }
  cadj[t] = ga;
  csamp[t] = s;
}

__global__ __launch_bounds__(256) void k_lv_bake(const double* __restrict__ verts, const int* __restrict__ faces,
                                                 const int* __restrict__ list, const int* __restrict__ fview,
                                                 const int* __restrict__ cadj, const RsSlot* __restrict__ slots,
                                                 const uint8_t* __restrict__ img, TxLayout lay, uint8_t* __restrict__ atlas) {
  tx_bake<true>(verts, faces, list, fview, cadj, slots, img, lay, atlas);
}

}  // namespace

struct sfmx_level {
  MeshInput in;                       // host inputs, staged
  DevBuf nkeys, ids;                  // the node table: keys and node numbers per slot
  DevBuf cslot, cnode;                // per corner: its node's slot, its node
  DevBuf nkey, nfx, g0, g1, pin;      // per node
  DevBuf deg, row, cur, adj, aux;     // the rows
  DevBuf ekeys, euses;                // the edge table
  DevBuf vsum, res;                   // per vertex: the sample sum; the words
  DevBuf vviews, cadj, csamp, atlas;  // the result
  bool done = false;
  int n = 0, m = 0, W = 0, H = 0;
  int32_t counts[6] = {};
  StageTimer t, ts, tb;  // the whole run, the sweeps alone, k_lv_bake alone
};

namespace {

// verts / faces are device pointers
int lv_run(sfmx_ctx* ctx, sfmx_level* lv, const sfmx_texture* tx, const double* verts, int n, const int32_t* faces, int m, int T) {
  hipStream_t s = ctx->stream;
  const TxLayout lay = tx->lay;
  const int L = lay.S - 2, V = tx->nviews;
  const size_t nn = (size_t)n, mm = (size_t)m, corners = 3 * mm;
  size_t bound = nn * (size_t)V;  // of the number of nodes
  bound = bound < corners ? bound : corners;
  size_t nslots = 4;
  while (nslots < 2 * corners) nslots <<= 1;  // at most 2^32: a slot number is an unsigned
  const size_t eslots = et_slots(mm);         // at most 3 m node edges in at least 4 m slots
  const unsigned nbc = (unsigned)((corners + 255) / 256), nbv = (unsigned)((nn + 255) / 256), nbf = (unsigned)((mm + 255) / 256);
  const int* fview = tx->fview.as<int>();
  const RsSlot* slots = tx->vs.d_slots.as<RsSlot>();
  const uint8_t* img = tx->vs.img.as<uint8_t>();

  SFMX_HIP(ctx, lv->res.ensure(LV_NWORDS * 4));
  SFMX_HIP(ctx, lv->vviews.ensure(nn * 4));
  SFMX_HIP(ctx, lv->vsum.ensure(nn * 8));
  SFMX_HIP(ctx, lv->cadj.ensure(corners * 4));
  SFMX_HIP(ctx, lv->csamp.ensure(corners * 4));
  SFMX_HIP(ctx, lv->atlas.ensure((size_t)lay.W * (size_t)lay.H));
  int* words = lv->res.as<int>();
  int w[LV_NWORDS] = {};

  SFMX_HIP(ctx, lv->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(words, 0, LV_NWORDS * 4, s));
  if (n > 0) SFMX_HIP(ctx, hipMemsetAsync(lv->vviews.p, 0, nn * 4, s));
  if (m > 0) {
    SFMX_HIP(ctx, lv->nkeys.ensure(nslots * 8));
    SFMX_HIP(ctx, lv->ids.ensure(nslots * 4));
    SFMX_HIP(ctx, lv->cslot.ensure(corners * 4));
    SFMX_HIP(ctx, lv->cnode.ensure(corners * 4));
    SFMX_HIP(ctx, lv->nkey.ensure(bound * 8));
    SFMX_HIP(ctx, lv->nfx.ensure(bound * 4));
    SFMX_HIP(ctx, hipMemsetAsync(lv->nkeys.p, 0xFF, nslots * 8, s));
    if (n > 0) SFMX_HIP(ctx, hipMemsetAsync(lv->vsum.p, 0, nn * 8, s));
    k_lv_insert<<<nbc, 256, 0, s>>>(verts, faces, (long long)corners, n, fview, slots, img, L, lay.fill, lv->nkeys.as<unsigned long long>(),
                                    (unsigned long long)nslots - 1, lv->ids.as<int>(), lv->cslot.as<unsigned>(),
                                    lv->nkey.as<unsigned long long>(), lv->nfx.as<int>(), lv->vviews.as<int>(),
                                    lv->vsum.as<unsigned long long>(), words);
    SFMX_HIP(ctx, hipGetLastError());
    SFMX_HIP(ctx, hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, s));
    SFMX_HIP(ctx, hipStreamSynchronize(s));
    SFMX_REQUIRE(ctx, w[LV_FLAG] == 0 && "a face index outside [0, n)");
  }
  const int nodes = w[LV_NODES];
  SFMX_REQUIRE(ctx, nodes >= 0 && (size_t)nodes <= bound);
  const int* gfinal = nullptr;
  if (nodes > 0) {
    const size_t nd = (size_t)nodes;
    const unsigned nbn = (unsigned)((nd + 255) / 256), nbe = (unsigned)((eslots + 255) / 256);
    SFMX_HIP(ctx, lv->g0.ensure(nd * 4));
    SFMX_HIP(ctx, lv->g1.ensure(nd * 4));
    SFMX_HIP(ctx, lv->pin.ensure(nd));
    SFMX_HIP(ctx, lv->deg.ensure(nd * 4));
    SFMX_HIP(ctx, lv->row.ensure(nd * 4));
    SFMX_HIP(ctx, lv->cur.ensure(nd * 4));
    SFMX_HIP(ctx, lv->aux.ensure(sfmx_scan_aux(nodes) * 4));
    SFMX_HIP(ctx, lv->adj.ensure(6 * mm * 4));
    SFMX_HIP(ctx, lv->ekeys.ensure(eslots * 8));
    SFMX_HIP(ctx, lv->euses.ensure(eslots * 8));
    SFMX_HIP(ctx, hipMemsetAsync(lv->ekeys.p, 0xFF, eslots * 8, s));
    SFMX_HIP(ctx, hipMemsetAsync(lv->deg.p, 0, nd * 4, s));
    SFMX_HIP(ctx, hipMemsetAsync(lv->cur.p, 0, nd * 4, s));
    k_lv_edges<<<nbf, 256, 0, s>>>(m, fview, lv->cslot.as<unsigned>(), lv->ids.as<int>(), lv->cnode.as<int>(), lv->ekeys.as<unsigned long long>(),
                                   lv->euses.as<int>(), (unsigned long long)eslots - 1, et_nbits(nodes));
    k_lv_verts<<<nbv, 256, 0, s>>>(n, lv->vviews.as<int>(), words);
    k_lv_pin<<<nbn, 256, 0, s>>>(nodes, lv->nkey.as<unsigned long long>(), lv->nfx.as<int>(), lv->vviews.as<int>(),
                                 lv->vsum.as<unsigned long long>(), lv->g0.as<int>(), lv->g1.as<int>(), lv->pin.as<uint8_t>(), words);
    k_lv_deg<<<nbe, 256, 0, s>>>((unsigned long long)eslots, lv->ekeys.as<unsigned long long>(), lv->deg.as<int>(), words);
    sfmx_scan(lv->deg.as<int>(), false, nodes, lv->row.as<int>(), lv->aux.as<int>(), s);
    k_lv_fill<<<nbe, 256, 0, s>>>((unsigned long long)eslots, lv->ekeys.as<unsigned long long>(), lv->row.as<unsigned>(), lv->cur.as<int>(),
                                  lv->adj.as<int>());
    SFMX_HIP(ctx, lv->ts.begin(ctx));
    int *gin = lv->g0.as<int>(), *gout = lv->g1.as<int>();
    for (int it = 0; it < T; it++) {  // one launch per sweep: the launch boundary is the only barrier
      k_lv_sweep<<<nbn, 256, 0, s>>>(nodes, lv->row.as<unsigned>(), lv->deg.as<int>(), lv->adj.as<int>(), lv->pin.as<uint8_t>(), gin, gout);
      int* x = gin;
      gin = gout;
      gout = x;
    }
    SFMX_HIP(ctx, lv->ts.end(ctx));
    gfinal = gin;
  }
  if (m > 0)
    k_lv_corners<<<nbc, 256, 0, s>>>((long long)corners, fview, lv->cnode.as<int>(), gfinal, lv->nfx.as<int>(), lv->cadj.as<int>(),
                                     lv->csamp.as<int>());
  if (lay.cells > 0) {
    const int rows = lay.H / lay.S;
    SFMX_HIP(ctx, lv->tb.begin(ctx));
    k_lv_bake<<<dim3((unsigned)rows, (unsigned)((lay.C + TX_GROUP - 1) / TX_GROUP)), 256, 0, s>>>(
        verts, faces, tx->list, fview, lv->cadj.as<int>(), slots, img, lay, lv->atlas.as<uint8_t>());
    SFMX_HIP(ctx, lv->tb.end(ctx));
  }
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, lv->t.end(ctx));
  SFMX_HIP(ctx, hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  lv->t.collect(ctx);
  if (nodes > 0) lv->ts.collect(ctx);
  if (lay.cells > 0) lv->tb.collect(ctx);
  lv->n = n;
  lv->m = m;
  lv->W = lay.W;
  lv->H = lay.H;
  lv->counts[0] = nodes;
  lv->counts[1] = w[LV_SEAM];
  lv->counts[2] = w[LV_PINNED];
  lv->counts[3] = nodes - w[LV_PINNED];
  lv->counts[4] = w[LV_EDGES];
  lv->counts[5] = T;
  lv->done = true;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_level_default_params(sfmx_level_params* p) {
  if (!p) return;
  *p = sfmx_level_params{};
  p->iterations = 64;
}

int sfmx_level_check_params(const sfmx_level_params* p) {
  if (!p || p->iterations < 0 || p->iterations > LV_ITER_MAX) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_level_create(sfmx_ctx* ctx, sfmx_level** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* lv = new sfmx_level;
  hipError_t e = lv->t.create();
  if (e == hipSuccess) e = lv->ts.create();
  if (e == hipSuccess) e = lv->tb.create();
  if (e != hipSuccess) {
    sfmx_level_destroy(ctx, lv);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_level_create", e);
  }
  *out = lv;
  return SFMX_OK;
}

void sfmx_level_destroy(sfmx_ctx* ctx, sfmx_level* lv) {
  if (!lv) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  lv->in.release();
  for (DevBuf* b : {&lv->nkeys, &lv->ids, &lv->cslot, &lv->cnode, &lv->nkey, &lv->nfx, &lv->g0, &lv->g1, &lv->pin, &lv->deg,
                    &lv->row, &lv->cur, &lv->adj, &lv->aux, &lv->ekeys, &lv->euses, &lv->vsum, &lv->res, &lv->vviews, &lv->cadj, &lv->csamp,
                    &lv->atlas})
    b->release();
  lv->t.destroy();
  lv->ts.destroy();
  lv->tb.destroy();
  delete lv;
}

int sfmx_level_run(sfmx_ctx* ctx, sfmx_level* lv, const sfmx_texture* tx, const double* verts, int n, const int32_t* faces, int m,
                   int on_device, const sfmx_level_params* p) {
  SFMX_REQUIRE(ctx, ctx && lv);
  lv->done = false;  // every failure from here on leaves no result behind
  lv->t.us = 0.0;
  lv->ts.us = 0.0;
  lv->tb.us = 0.0;
  SFMX_REQUIRE(ctx, sfmx_level_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, tx && tx->done && "the texture object needs a successful run");
  SFMX_REQUIRE(ctx, n == tx->n && m == tx->m && "the mesh of the texture object's last run");
  SFMX_REQUIRE(ctx, 3ll * m <= 2147483647ll);  // before any allocation
  SFMX_REQUIRE(ctx, (verts || n == 0) && (faces || m == 0));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return lv_run(ctx, lv, tx, verts, n, faces, m, p->iterations);
  MeshDev d;
  SFMX_HIP(ctx, lv->in.stage(verts, nullptr, n, faces, m, ctx->stream, d));
  return lv_run(ctx, lv, tx, d.verts, n, d.faces, m, p->iterations);
}

int sfmx_level_read(sfmx_ctx* ctx, sfmx_level* lv, uint8_t* atlas, int32_t* corner_adj, int32_t* corner_sample, int32_t* vertex_views) {
  SFMX_REQUIRE(ctx, ctx && lv && lv->done);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t n = (size_t)lv->n, m = (size_t)lv->m, px = (size_t)lv->W * (size_t)lv->H;
  if (atlas && px) SFMX_HIP(ctx, hipMemcpyAsync(atlas, lv->atlas.p, px, hipMemcpyDeviceToHost, s));
  if (corner_adj && m) SFMX_HIP(ctx, hipMemcpyAsync(corner_adj, lv->cadj.p, m * 12, hipMemcpyDeviceToHost, s));
  if (corner_sample && m) SFMX_HIP(ctx, hipMemcpyAsync(corner_sample, lv->csamp.p, m * 12, hipMemcpyDeviceToHost, s));
  if (vertex_views && n) SFMX_HIP(ctx, hipMemcpyAsync(vertex_views, lv->vviews.p, n * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

int sfmx_level_counts(const sfmx_level* lv, int32_t* counts6) {
  const bool have = lv && lv->done;
  if (counts6)
    for (int k = 0; k < 6; k++) counts6[k] = have ? lv->counts[k] : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_level_device_atlas(const sfmx_level* lv, const uint8_t** atlas, int* W, int* H) {
  const bool have = lv && lv->done;
  if (atlas) *atlas = have ? lv->atlas.as<uint8_t>() : nullptr;
  if (W) *W = have ? lv->W : 0;
  if (H) *H = have ? lv->H : 0;
  return have ? lv->W * lv->H : -1;
}

double sfmx_level_last_us(const sfmx_level* lv) { return lv ? lv->t.us : 0.0; }

double sfmx_level_last_sweeps_us(const sfmx_level* lv) { return lv ? lv->ts.us : 0.0; }

double sfmx_level_last_bake_us(const sfmx_level* lv) { return lv ? lv->tb.us : 0.0; }

}  // extern "C"
