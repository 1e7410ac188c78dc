// texture.hip — a texture atlas for a mesh from the cameras that see it: best view per face, one patch per face.
//
// A sfmx_texture keeps an ordered list of cameras with one u8 image each on the device.  A run builds the exact z-buffer of the
// whole mesh for every camera (as the visibility stage does), tests every vertex against the key
// image of every camera, gives every face the camera that sees it from the front with the largest integer area, lays the
// textured faces out two to a cell of (patch + 1) x patch texels in the order of their indices and bakes every texel of the
// atlas from the image of its face's camera, bilinearly, at the projection of the texel's point on the face.
//
// Exactness: the key image is the renderer's (sfmx_raster_dev.h: the same kernels).  The depth test is visib.hip's two lines,
// restated here.  The best view is a strict > on int64 areas over views in ascending order, so batches cannot change it; the
// ranks come from a scan; the layout is integer arithmetic on the host; a texel is a fixed sequence of double operations (built
// with -ffp-contract=off) on values that depend on (face, i, j) alone.  tests/texture_ref.py restates it in NumPy; the tests
// compare bytes.  The batch size, every grid size, TX_BUDGET and TX_GROUP change the speed only.
//
// Kernel layout (blocks of 256, the context's stream, no inter-workgroup hand-off, no spinning).  Per batch of at most 64 views,
// sized as visib.hip sizes it:
//   k_rs_project / k_rs_faces / k_rs_big <true>   the key images of the batch's views (sfmx_raster_dev.h)
//   k_tx_verts    one thread per vertex over the batch's views: one bit per view that sees the vertex
//   k_tx_faces    one thread per face: the AND of its corners' masks and, per set bit in ascending order, the area A of that
//                 view; -A > face_area replaces the face's view
// After the last batch:
//   k_tx_mark     per face: the range check of its indices (the call's flag) and the flag "textured"
//   k_scan_*      the exclusive scan of the flags: the ranks (scan.hip)
//   k_tx_list     rank -> face, and the histogram view_faces
//   (one read-back of the flag and the number of textured faces; the layout and its refusals on the host)
//   k_tx_bake     the hot path: one block per group of TX_GROUP cells of one cell row.  The block first stages, per half cell, the
//                 face's nine doubles and its view's camera, image offset and size in LDS (26 eight-byte words, loaded by 26
//                 threads each once), then walks the group's texels row by row, thread t on texel t, t + 256, ...: a wave
//                 stores 64 neighbouring bytes of one atlas row.  Every texel of the atlas is written exactly once, `fill`
//                 included (also the cells of a partial last row).
//   k_tx_uv       per face: its three corners in half-texels
// Two host synchronisations per run: after the counts, and at the end.
#include <cmath>
#include <vector>

#include "sfmx_internal.h"
#include "sfmx_raster_dev.h"
#include "sfmx_texture_dev.h"

namespace {

constexpr size_t TX_BUDGET = (size_t)256 << 20;  // bytes a batch's key slab, per-(view, vertex) records and big-face lists may take
constexpr int TX_MAX_BATCH = 64;                 // one bit per view in a vertex's mask
constexpr int TX_BIG_BLOCKS = 64;                // blocks of k_rs_big per view
constexpr int TX_SMALL = 64;                     // as raster.hip's RS_SMALL
constexpr int TX_GROUP = 16;                     // cells per block of k_tx_bake
constexpr int TX_REC = 26;                       // eight-byte words per half cell in LDS
constexpr int TX_PATCH_MIN = 3, TX_PATCH_MAX = 64, TX_W_MAX = 16384;
constexpr long long TX_TEXELS_MAX = 1ll << 28;

enum { TX_FLAG = 0, TX_NTEX, TX_NWORDS = 4 };  // int32 words read back

static_assert(sizeof(RsCam) == 16 * 8 && sizeof(RsSlot) == 18 * 8, "k_tx_bake copies a slot as eight-byte words");

__global__ __launch_bounds__(256) void k_tx_verts(const double* __restrict__ verts, int n, const RsSlot* __restrict__ slots, int nb,
                                                  const RsVert* __restrict__ pv, const uint8_t* __restrict__ fl,
                                                  const unsigned long long* __restrict__ keys, double depth_tol,
                                                  unsigned long long* __restrict__ mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double X0 = verts[3 * (size_t)i], X1 = verts[3 * (size_t)i + 1], X2 = verts[3 * (size_t)i + 2];
  unsigned long long mk = 0;
  for (int k = 0; k < nb; k++) {
    const RsSlot& S = slots[k];
    const size_t at = (size_t)k * (size_t)n + (size_t)i;
    if (!(fl[at] & 2u)) continue;  // not inband
    const RsVert P = pv[at];
    const int x = (P.U + 128) >> 8, y = (P.V + 128) >> 8;
    if (x < 0 || x >= S.cam.w || y < 0 || y >= S.cam.h) continue;
    const unsigned long long key = keys[S.key_off + ((long long)y * S.cam.w + x)];
    double p0, p1, p2;
    const double q2 = rs_depth(S.cam, X0, X1, X2, p0, p1, p2);
    bool visible = true;
    if (key != ~0ull) {
      const double D = (double)__uint_as_float((unsigned)(key >> 32));
      visible = q2 <= D + depth_tol;  // false for a NaN
    }
    if (visible) mk |= 1ull << k;
  }
  mask[i] = mk;
}

__device__ __forceinline__ bool tx_face(const int* __restrict__ faces, int f, int n, int& a, int& b, int& c) {
  a = faces[3 * (size_t)f];
  b = faces[3 * (size_t)f + 1];
  c = faces[3 * (size_t)f + 2];
  return (unsigned)a < (unsigned)n && (unsigned)b < (unsigned)n && (unsigned)c < (unsigned)n;
}

__global__ __launch_bounds__(256) void k_tx_faces(const int* __restrict__ faces, int m, int n, const RsVert* __restrict__ pv,
                                                  const unsigned long long* __restrict__ mask, int first, int* __restrict__ fview,
                                                  long long* __restrict__ farea) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int a, b, c;
  if (!tx_face(faces, f, n, a, b, c)) return;  // k_tx_mark fails the call; nothing is read through the index
  unsigned long long mk = mask[a] & mask[b] & mask[c];
  if (!mk) return;
  long long best = farea[f];
  int view = -1;
  while (mk) {
    const int k = __ffsll((long long)mk) - 1;
    mk &= mk - 1;
    const RsVert* q = pv + (size_t)k * (size_t)n;
    const RsVert P[3] = {q[a], q[b], q[c]};
    const long long A = rs_area(P);
    if (-A > best) {  // strict: a tie stays with the smaller view index
      best = -A;
      view = first + k;
    }
  }
  if (view >= 0) {
    farea[f] = best;
    fview[f] = view;
  }
}

__global__ __launch_bounds__(256) void k_tx_mark(const int* __restrict__ faces, int m, int n, const int* __restrict__ fview,
                                                 int* __restrict__ ftex, int* words) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int a, b, c;
  if (!tx_face(faces, f, n, a, b, c)) atomicOr(&words[TX_FLAG], 1);
  ftex[f] = fview[f] >= 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_tx_list(int m, const int* __restrict__ fview, const int* __restrict__ rank,
                                                 int* __restrict__ list, int* view_faces) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  const int k = fview[f];
  if (k < 0) return;
  list[rank[f]] = f;
  atomicAdd(&view_faces[k], 1);  // integers: the order does not matter
}

__global__ __launch_bounds__(256) void k_tx_bake(const double* __restrict__ verts, const int* __restrict__ faces,
                                                 const int* __restrict__ list, const int* __restrict__ fview,
                                                 const RsSlot* __restrict__ slots, const uint8_t* __restrict__ img, TxLayout lay,
                                                 uint8_t* __restrict__ atlas) {
  __shared__ double rec[2 * TX_GROUP][TX_REC];  // X a, b, c (9), the camera (16 words), the image's offset
  __shared__ int idx[2 * TX_GROUP][4];          // the face's corners and its view, -1: a half without a face
  const int S = lay.S, L = S - 2, row = blockIdx.x, g0 = blockIdx.y * TX_GROUP;
  const int gc = min(TX_GROUP, lay.C - g0);  // cells of this group
  if (threadIdx.x < 2 * TX_GROUP) {
    const int hl = threadIdx.x, c = row * lay.C + g0 + (hl >> 1);
    const long long r = 2ll * c + (hl & 1);
    int v = -1, a = 0, b = 0, cc = 0;
    if ((hl >> 1) < gc && c < lay.cells && c != lay.fill_cell && r < lay.n_tex) {
      const int f = list[r];
      v = fview[f];
      a = faces[3 * (size_t)f];  // a textured face has passed the range check
      b = faces[3 * (size_t)f + 1];
      cc = faces[3 * (size_t)f + 2];
    }
    idx[hl][0] = a;
    idx[hl][1] = b;
    idx[hl][2] = cc;
    idx[hl][3] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * TX_GROUP * TX_REC; e += 256) {
    const int hl = e / TX_REC, j = e % TX_REC, v = idx[hl][3];
    if (v < 0) continue;
    unsigned long long x;  // bits: the camera's last word is its two ints
    if (j < 9) {
      x = reinterpret_cast<const unsigned long long*>(verts)[3 * (size_t)idx[hl][j / 3] + (j % 3)];
    } else {
      const unsigned long long* s = reinterpret_cast<const unsigned long long*>(slots + v);  // words 0 .. 15 the camera, 16 key_off, 17 img_off
      x = s[j == TX_REC - 1 ? 17 : j - 9];
    }
    reinterpret_cast<unsigned long long*>(rec[hl])[j] = x;
  }
  __syncthreads();
  const int rw = gc * (S + 1), total = rw * S;
  const size_t base = (size_t)row * S * lay.W + (size_t)g0 * (S + 1);
  for (int t = threadIdx.x; t < total; t += 256) {
    const int ly = t / rw, x = t - ly * rw;
    const int cb = x / (S + 1), lx = x - cb * (S + 1);
    const int half = lx + ly >= S ? 1 : 0;
    const int i = half ? S - lx : lx, j = half ? S - 1 - ly : ly;
    const int hl = 2 * cb + half;
    int out = lay.fill;
    if (idx[hl][3] >= 0) {
      const double* r = rec[hl];
      const int i2 = min(i, L), j2 = min(j, L - i2);
      const double wa = (double)(L - i2 - j2), wb = (double)i2, wc = (double)j2, dl = (double)L;
      const double X0 = ((wa * r[0] + wb * r[3]) + wc * r[6]) / dl;
      const double X1 = ((wa * r[1] + wb * r[4]) + wc * r[7]) / dl;
      const double X2 = ((wa * r[2] + wb * r[5]) + wc * r[8]) / dl;
      const double* R = r + 9;  // R[0 .. 8], c = R[9 .. 11], f, cx, cy = R[12 .. 14]
      const double p0 = X0 - R[9], p1 = X1 - R[10], p2 = X2 - R[11];
      const double q0 = (R[0] * p0 + R[1] * p1) + R[2] * p2;
      const double q1 = (R[3] * p0 + R[4] * p1) + R[5] * p2;
      const double q2 = (R[6] * p0 + R[7] * p1) + R[8] * p2;
      const double u = (R[12] * q0) / q2 + R[13], v = (R[12] * q1) / q2 + R[14];
      if (q2 > 0.0 && isfinite(u) && isfinite(v)) {
        const int2 wh = *reinterpret_cast<const int2*>(r + 24);
        const long long off = *reinterpret_cast<const long long*>(r + 25);
        const int w = wh.x, h = wh.y;
        const double uc = fmin(fmax(u, -1.0), (double)w), vc = fmin(fmax(v, -1.0), (double)h);
        const double x0 = floor(uc), y0 = floor(vc);
        const double ax = uc - x0, ay = vc - y0;
        const int xi0 = min(max((int)x0, 0), w - 1), xi1 = min(max((int)x0 + 1, 0), w - 1);
        const int yi0 = min(max((int)y0, 0), h - 1), yi1 = min(max((int)y0 + 1, 0), h - 1);
        const uint8_t* I0 = img + off + (long long)yi0 * w;
        const uint8_t* I1 = img + off + (long long)yi1 * w;
        const double top = (1.0 - ax) * (double)I0[xi0] + ax * (double)I0[xi1];
        const double bot = (1.0 - ax) * (double)I1[xi0] + ax * (double)I1[xi1];
        const double g = (1.0 - ay) * top + ay * bot;
        out = (int)fmin(255.0, floor(g + 0.5));
      }
    }
    atlas[base + (size_t)ly * lay.W + x] = (uint8_t)out;
  }
}

__global__ __launch_bounds__(256) void k_tx_uv(int m, const int* __restrict__ fview, const int* __restrict__ rank, TxLayout lay,
                                               int* __restrict__ uvh) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  const int S = lay.S;
  const bool tex = fview[f] >= 0;
  const int r = tex ? rank[f] : 0;
  const int cell = tex ? r >> 1 : lay.fill_cell;
  const int x0 = 2 * ((cell % lay.C) * (S + 1)), y0 = 2 * ((cell / lay.C) * S);
  int c[3][2] = {{1, 1}, {2 * S - 3, 1}, {1, 2 * S - 3}};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int x = c[k][0], y = c[k][1];
    if (!tex) {
      x = S + 1;
      y = S;
    } else if (r & 1) {
      x = 2 * (S + 1) - x;
      y = 2 * S - y;
    }
    uvh[6 * (size_t)f + 2 * k] = x0 + x;
    uvh[6 * (size_t)f + 2 * k + 1] = y0 + y;
  }
}

struct TxBatch {
  int first, count;
};

}  // namespace

namespace {

std::vector<TxBatch> tx_plan(const sfmx_texture* tx, int n, int m, size_t& key_px, int& widest) {
  std::vector<TxBatch> out;
  const int V = (int)tx->views.size();
  key_px = 0;
  widest = 0;
  int k = 0;
  while (k < V) {
    size_t bytes = 0, px = 0;
    int c = 0;
    while (k + c < V && c < TX_MAX_BATCH) {
      const size_t p = (size_t)tx->views[k + c].w * (size_t)tx->views[k + c].h;
      const size_t one = p * 8 + (size_t)n * 17 + (size_t)m * 4;
      if (tx->forced_batch ? c >= tx->forced_batch : (c > 0 && bytes + one > TX_BUDGET)) break;
      bytes += one;
      px += p;
      c++;
    }
    out.push_back({k, c});
    key_px = px > key_px ? px : key_px;
    widest = c > widest ? c : widest;
    k += c;
  }
  return out;
}

// the layout from the counts; false when the atlas would be too wide or too large
bool tx_layout(int n_tex, int n_un, const sfmx_texture_params* p, TxLayout& lay) {
  const int S = p->patch;
  const long long cells = ((long long)n_tex + 1) / 2 + (n_un > 0 ? 1 : 0);
  long long C = p->cells_per_row;
  if (C == 0) {
    C = 1;
    while (C * C < cells) C++;
    const long long cap = TX_W_MAX / (S + 1);
    C = C > cap ? cap : C;
    C = C < 1 ? 1 : C;
  }
  lay = TxLayout{S, (int)C, (int)cells, n_tex, n_un > 0 ? (int)cells - 1 : -1, 0, 0, p->fill};
  if (cells == 0) return true;
  const long long W = C * (S + 1), H = ((cells + C - 1) / C) * S;
  if (W > TX_W_MAX || W * H > TX_TEXELS_MAX) return false;
  lay.W = (int)W;
  lay.H = (int)H;
  return true;
}

// verts / faces are device pointers
int tx_run(sfmx_ctx* ctx, sfmx_texture* tx, const double* verts, int n, const int32_t* faces, int m, const sfmx_texture_params* p) {
  hipStream_t s = ctx->stream;
  const int V = (int)tx->views.size();
  SFMX_REQUIRE(ctx, V >= 1);
  for (long long o : tx->img_off) SFMX_REQUIRE(ctx, o >= 0 && "every view needs an image");
  const size_t nn = (size_t)n, mm = (size_t)m;
  size_t key_px = 0;
  int widest = 0;
  const std::vector<TxBatch> plan = tx_plan(tx, n, m, key_px, widest);
  const unsigned nbv = (unsigned)((nn + 255) / 256), nbf = (unsigned)((mm + 255) / 256);
  const int fb = m > (RS_FACE_BLOCKS - 1) * 256 ? RS_FACE_BLOCKS : (m + 255) / 256;

  SFMX_HIP(ctx, tx->keys.ensure(key_px * 8));
  SFMX_HIP(ctx, tx->pv.ensure((size_t)widest * nn * sizeof(RsVert)));
  SFMX_HIP(ctx, tx->fl.ensure((size_t)widest * nn));
  SFMX_HIP(ctx, tx->big.ensure((size_t)widest * mm * 4));
  SFMX_HIP(ctx, tx->rcounters.ensure((size_t)TX_MAX_BATCH * RS_NWORDS * 4));
  // work: mask u64 [n], then int32: ftex, rank, list [m], the scan's aux
  const size_t aux = sfmx_scan_aux(m > 0 ? m : 1);
  SFMX_HIP(ctx, tx->work.ensure(nn * 8 + (3 * mm + aux) * 4));
  SFMX_HIP(ctx, tx->res.ensure(TX_NWORDS * 4));
  SFMX_HIP(ctx, tx->fview.ensure(mm * 4));
  SFMX_HIP(ctx, tx->farea.ensure(mm * 8));
  SFMX_HIP(ctx, tx->uvh.ensure(mm * 24));
  SFMX_HIP(ctx, tx->vfaces.ensure((size_t)V * 4));
  unsigned long long* mask = tx->work.as<unsigned long long>();
  int* ftex = reinterpret_cast<int*>(mask + nn);
  int* rank = ftex + mm;
  int* list = rank + mm;
  int* ax = list + mm;
  int* words = tx->res.as<int>();

  // the slots of all views: a batch's key images lie back to back in the key slab
  tx->slots.resize((size_t)V);
  for (const TxBatch& b : plan) {
    long long at = 0;
    for (int k = b.first; k < b.first + b.count; k++) {
      tx->slots[k].cam = rs_cam(&tx->views[k]);
      tx->slots[k].key_off = at;
      tx->slots[k].img_off = tx->img_off[k];
      at += (long long)tx->views[k].w * tx->views[k].h;
    }
  }
  SFMX_HIP(ctx, tx->d_slots.ensure(sizeof(RsSlot) * (size_t)V));
  SFMX_HIP(ctx, hipMemcpyAsync(tx->d_slots.p, tx->slots.data(), sizeof(RsSlot) * (size_t)V, hipMemcpyHostToDevice, s));
  const RsSlot* d_slots = tx->d_slots.as<RsSlot>();

  SFMX_HIP(ctx, tx->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(tx->res.p, 0, TX_NWORDS * 4, s));
  SFMX_HIP(ctx, hipMemsetAsync(tx->vfaces.p, 0, (size_t)V * 4, s));
  if (m > 0) {
    SFMX_HIP(ctx, hipMemsetAsync(tx->fview.p, 0xFF, mm * 4, s));
    SFMX_HIP(ctx, hipMemsetAsync(tx->farea.p, 0, mm * 8, s));
  }
  for (const TxBatch& b : plan) {
    if (n == 0 || m == 0) break;  // nothing to see; a face of a mesh without vertices fails in k_tx_mark
    size_t px = 0;
    for (int k = b.first; k < b.first + b.count; k++) px += (size_t)tx->views[k].w * (size_t)tx->views[k].h;
    const RsSlot* sl = d_slots + b.first;
    SFMX_HIP(ctx, hipMemsetAsync(tx->keys.p, 0xFF, px * 8, s));
    SFMX_HIP(ctx, hipMemsetAsync(tx->rcounters.p, 0, (size_t)b.count * RS_NWORDS * 4, s));
    k_rs_project<true><<<dim3(nbv, (unsigned)b.count), 256, 0, s>>>(verts, n, RsCam{}, sl, p->z_min, tx->pv.as<RsVert>(), tx->fl.as<uint8_t>());
    k_rs_faces<true, TX_SMALL><<<dim3((unsigned)fb, (unsigned)b.count), 256, 0, s>>>(faces, m, n, tx->pv.as<RsVert>(), tx->fl.as<uint8_t>(), 0, 0, 0,
                                                                           tx->keys.as<unsigned long long>(), tx->big.as<int>(),
                                                                           tx->rcounters.as<unsigned>(), nullptr, sl);
    k_rs_big<true><<<dim3(TX_BIG_BLOCKS, (unsigned)b.count), 256, 0, s>>>(faces, m, n, tx->pv.as<RsVert>(), 0, 0, tx->keys.as<unsigned long long>(),
                                                                          tx->big.as<int>(), tx->rcounters.as<unsigned>(), nullptr, sl);
    k_tx_verts<<<nbv, 256, 0, s>>>(verts, n, sl, b.count, tx->pv.as<RsVert>(), tx->fl.as<uint8_t>(), tx->keys.as<unsigned long long>(),
                                   p->depth_tol, mask);
    k_tx_faces<<<nbf, 256, 0, s>>>(faces, m, n, tx->pv.as<RsVert>(), mask, b.first, tx->fview.as<int>(), tx->farea.as<long long>());
  }
  if (m > 0) {
    k_tx_mark<<<nbf, 256, 0, s>>>(faces, m, n, tx->fview.as<int>(), ftex, words);
    sfmx_scan(ftex, false, m, rank, ax, s);
    sfmx_scan_total(ftex, false, rank, m, words + TX_NTEX, s);
    k_tx_list<<<nbf, 256, 0, s>>>(m, tx->fview.as<int>(), rank, list, tx->vfaces.as<int>());
  }
  SFMX_HIP(ctx, hipGetLastError());
  int w[TX_NWORDS];
  SFMX_HIP(ctx, hipMemcpyAsync(w, tx->res.p, sizeof w, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  SFMX_REQUIRE(ctx, w[TX_FLAG] == 0 && "a face index outside [0, n)");
  const int n_tex = w[TX_NTEX];
  SFMX_REQUIRE(ctx, n_tex >= 0 && n_tex <= m);
  TxLayout lay;
  SFMX_REQUIRE(ctx, tx_layout(n_tex, m - n_tex, p, lay) && "the atlas is wider than 16384 texels or larger than 2^28");
  SFMX_HIP(ctx, tx->atlas.ensure((size_t)lay.W * (size_t)lay.H));
  if (lay.cells > 0) {
    const int rows = lay.H / lay.S;
    SFMX_HIP(ctx, tx->tb.begin(ctx));
    k_tx_bake<<<dim3((unsigned)rows, (unsigned)((lay.C + TX_GROUP - 1) / TX_GROUP)), 256, 0, s>>>(verts, faces, list, tx->fview.as<int>(), d_slots,
                                                                                              tx->img.as<uint8_t>(), lay, tx->atlas.as<uint8_t>());
    SFMX_HIP(ctx, tx->tb.end(ctx));
    k_tx_uv<<<nbf, 256, 0, s>>>(m, tx->fview.as<int>(), rank, lay, tx->uvh.as<int>());
  }
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, tx->t.end(ctx));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  tx->t.collect(ctx);
  if (lay.cells > 0) tx->tb.collect(ctx);
  tx->n = n;
  tx->m = m;
  tx->nviews = V;
  tx->counts[0] = n_tex;
  tx->counts[1] = m - n_tex;
  tx->counts[2] = lay.cells;
  tx->counts[3] = lay.W;
  tx->counts[4] = lay.H;
  tx->counts[5] = lay.C;
  tx->lay = lay;
  tx->last_batch = widest;
  tx->done = true;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_texture_default_params(sfmx_texture_params* p) {
  if (!p) return;
  *p = sfmx_texture_params{};
  p->patch = 8;
  p->cells_per_row = 0;
  p->fill = 0;
}

int sfmx_texture_check_params(const sfmx_texture_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!std::isfinite(p->z_min) || !(p->z_min > 0.0) || !std::isfinite(p->depth_tol) || !(p->depth_tol >= 0.0)) return SFMX_ERR_INVALID;
  if (p->patch < TX_PATCH_MIN || p->patch > TX_PATCH_MAX || p->cells_per_row < 0 || p->fill < 0 || p->fill > 255) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_texture_create(sfmx_ctx* ctx, sfmx_texture** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* tx = new sfmx_texture;
  hipError_t e = tx->t.create();
  if (e == hipSuccess) e = tx->tb.create();
  if (e != hipSuccess) {
    sfmx_texture_destroy(ctx, tx);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_texture_create", e);
  }
  *out = tx;
  return SFMX_OK;
}

void sfmx_texture_destroy(sfmx_ctx* ctx, sfmx_texture* tx) {
  if (!tx) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* b : {&tx->img, &tx->d_slots, &tx->keys, &tx->pv, &tx->fl, &tx->big, &tx->rcounters, &tx->work, &tx->res, &tx->in_v, &tx->in_f,
                    &tx->fview, &tx->farea, &tx->uvh, &tx->vfaces, &tx->atlas})
    b->release();
  tx->t.destroy();
  tx->tb.destroy();
  delete tx;
}

int sfmx_texture_reset(sfmx_ctx* ctx, sfmx_texture* tx) {
  SFMX_REQUIRE(ctx, ctx && tx);
  tx->views.clear();
  tx->img_off.clear();
  tx->img_used = 0;
  return SFMX_OK;
}

int sfmx_texture_add_stereo_view(sfmx_ctx* ctx, sfmx_texture* tx, const sfmx_fusion_view* view, const sfmx_stereo* st) {
  SFMX_REQUIRE(ctx, ctx && tx && st && view);
  int w = 0, h = 0;
  const uint8_t* im = sfmx_stereo_device_rect_left(st, &w, &h);
  SFMX_REQUIRE(ctx, im && view->w == w && view->h == h);
  return sfmx_texture_add_view(ctx, tx, view, im, 1);
}

int sfmx_texture_add_view(sfmx_ctx* ctx, sfmx_texture* tx, const sfmx_fusion_view* view, const uint8_t* image, int on_device) {
  SFMX_REQUIRE(ctx, ctx && tx && rs_view_ok(view));
  long long off = -1;
  if (image) {
    SFMX_HIP(ctx, hipSetDevice(ctx->device));
    const long long px = (long long)view->w * view->h;
    SFMX_REQUIRE(ctx, tx->img_used + px < (1ll << 40));
    SFMX_HIP(ctx, sfmx_grow_keep(tx->img, (size_t)tx->img_used, (size_t)(tx->img_used + px), ctx->stream));
    SFMX_HIP(ctx, hipMemcpyAsync(tx->img.as<uint8_t>() + tx->img_used, image, (size_t)px,
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may reuse its buffer
    off = tx->img_used;
    tx->img_used += px;
  }
  tx->views.push_back(*view);
  tx->img_off.push_back(off);
  return SFMX_OK;
}

int sfmx_texture_view_count(const sfmx_texture* tx) { return tx ? (int)tx->views.size() : 0; }

int sfmx_texture_set_batch(sfmx_texture* tx, int k) {
  if (!tx || k < 0 || k > TX_MAX_BATCH) return SFMX_ERR_INVALID;
  tx->forced_batch = k;
  return SFMX_OK;
}

int sfmx_texture_run(sfmx_ctx* ctx, sfmx_texture* tx, const double* verts, int n, const int32_t* faces, int m, int on_device,
                     const sfmx_texture_params* p) {
  SFMX_REQUIRE(ctx, ctx && tx);
  tx->done = false;  // every failure from here on leaves no result behind
  tx->t.us = 0.0;
  tx->tb.us = 0.0;
  SFMX_REQUIRE(ctx, sfmx_texture_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, n >= 0 && n < SFMX_RASTER_MAX_VERTS && m >= 0 && m < SFMX_RASTER_MAX_FACES);
  SFMX_REQUIRE(ctx, (verts || n == 0) && (faces || m == 0));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return tx_run(ctx, tx, verts, n, faces, m, p);
  hipStream_t s = ctx->stream;
  const size_t vbytes = (size_t)n * 24, fbytes = (size_t)m * 12;
  SFMX_HIP(ctx, tx->in_v.ensure(vbytes));
  SFMX_HIP(ctx, tx->in_f.ensure(fbytes));
  if (n > 0) SFMX_HIP(ctx, hipMemcpyAsync(tx->in_v.p, verts, vbytes, hipMemcpyHostToDevice, s));
  if (m > 0) SFMX_HIP(ctx, hipMemcpyAsync(tx->in_f.p, faces, fbytes, hipMemcpyHostToDevice, s));
  return tx_run(ctx, tx, tx->in_v.as<double>(), n, tx->in_f.as<int32_t>(), m, p);
}

int sfmx_texture_read(sfmx_ctx* ctx, sfmx_texture* tx, uint8_t* atlas, int32_t* face_view, int64_t* face_area, int32_t* uv_half,
                      int32_t* view_faces) {
  SFMX_REQUIRE(ctx, ctx && tx && tx->done);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t m = (size_t)tx->m, px = (size_t)tx->counts[3] * (size_t)tx->counts[4];
  if (atlas && px) SFMX_HIP(ctx, hipMemcpyAsync(atlas, tx->atlas.p, px, hipMemcpyDeviceToHost, s));
  if (face_view && m) SFMX_HIP(ctx, hipMemcpyAsync(face_view, tx->fview.p, m * 4, hipMemcpyDeviceToHost, s));
  if (face_area && m) SFMX_HIP(ctx, hipMemcpyAsync(face_area, tx->farea.p, m * 8, hipMemcpyDeviceToHost, s));
  if (uv_half && m) SFMX_HIP(ctx, hipMemcpyAsync(uv_half, tx->uvh.p, m * 24, hipMemcpyDeviceToHost, s));
  if (view_faces && tx->nviews) SFMX_HIP(ctx, hipMemcpyAsync(view_faces, tx->vfaces.p, (size_t)tx->nviews * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

int sfmx_texture_sizes(const sfmx_texture* tx, int* n, int* m, int* n_views, int* W, int* H) {
  const bool have = tx && tx->done;
  if (n) *n = have ? tx->n : 0;
  if (m) *m = have ? tx->m : 0;
  if (n_views) *n_views = have ? tx->nviews : 0;
  if (W) *W = have ? tx->counts[3] : 0;
  if (H) *H = have ? tx->counts[4] : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_texture_counts(const sfmx_texture* tx, int32_t* counts6) {
  const bool have = tx && tx->done;
  if (counts6)
    for (int k = 0; k < 6; k++) counts6[k] = have ? tx->counts[k] : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_texture_device_atlas(const sfmx_texture* tx, const uint8_t** atlas, int* W, int* H) {
  const bool have = tx && tx->done;
  if (atlas) *atlas = have ? tx->atlas.as<uint8_t>() : nullptr;
  if (W) *W = have ? tx->counts[3] : 0;
  if (H) *H = have ? tx->counts[4] : 0;
  return have ? tx->counts[3] * tx->counts[4] : -1;
}

double sfmx_texture_last_us(const sfmx_texture* tx) { return tx ? tx->t.us : 0.0; }

double sfmx_texture_last_bake_us(const sfmx_texture* tx) { return tx ? tx->tb.us : 0.0; }

int sfmx_texture_last_batch(const sfmx_texture* tx) { return tx && tx->done ? tx->last_batch : 0; }

}  // extern "C"
