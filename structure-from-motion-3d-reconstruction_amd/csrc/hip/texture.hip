// texture.hip — a texture atlas for a mesh from the cameras that see it: best view per face, one patch per face.
//
// A sfmx_texture keeps an ordered list of cameras with one u8 image each on the device.  A run builds the exact z-buffer of the
// whole mesh for every camera (as the visibility stage does), tests every vertex against the key
// image of every camera, gives every face the camera that sees it from the front with the largest integer area, lays the
// textured faces out two to a cell of (patch + 1) x patch texels in the order of their indices and bakes every texel of the
// atlas from the image of its face's camera, bilinearly, at the projection of the texel's point on the face.
//
// Exactness: the key image is the renderer's (sfmx_raster_dev.h: the same kernels).  The depth test is visib.hip's: both call
// rs_vertex_sees.  The best view is a strict > on int64 areas over views in ascending order, so batches cannot change it; the
// ranks come from a scan; the layout is integer arithmetic on the host; a texel is a fixed sequence of double operations (built
// with -ffp-contract=off) on values that depend on (face, i, j) alone.  tests/texture_ref.py restates it in NumPy; the tests
// compare bytes.  The batch size, every grid size, RS_BATCH_BUDGET and TX_GROUP change the speed only.
//
// Kernel layout (blocks of 256, the context's stream, no inter-workgroup hand-off, no spinning).  Per batch of at most 64 views
// (sfmx_raster_dev.h: RsViewSet, as visib.hip):
//   k_rs_project / k_rs_faces / k_rs_big <true>   the key images of the batch's views (RsViewSet::zbuffer)
//   k_tx_verts    one thread per vertex over the batch's views: one bit per view that sees the vertex
//   k_tx_faces    one thread per face: the AND of its corners' masks and, per set bit in ascending order, the area A of that
//                 view; -A > face_area replaces the face's view
// After the last batch:
//   k_tx_mark     per face: the range check of its indices (the call's flag) and the flag "textured"
//   k_scan_*      the exclusive scan of the flags: the ranks (scan.hip)
//   k_tx_list     rank -> face, and the histogram view_faces
//   (one read-back of the flag and the number of textured faces; the layout and its refusals on the host)
//   k_tx_bake     the hot path: one block per group of TX_GROUP cells of one cell row (sfmx_texture_dev.h: tx_bake, shared with
//                 k_lv_bake).  Every texel of the atlas is written exactly once, `fill` included.
//   k_tx_uv       per face: its three corners in half-texels
// Two host synchronisations per run: after the counts, and at the end.
#include <cmath>
#include <vector>

#include "sfmx_internal.h"
#include "sfmx_raster_dev.h"
#include "sfmx_texture_dev.h"

namespace {

constexpr int TX_PATCH_MIN = 3, TX_PATCH_MAX = 64, TX_W_MAX = 16384;
constexpr long long TX_TEXELS_MAX = 1ll << 28;

enum { TX_FLAG = 0, TX_NTEX, TX_NWORDS = 4 };  // int32 words read back

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
    if (rs_vertex_sees(S, pv, fl, keys, at, X0, X1, X2, depth_tol).state == RS_SEES_VISIBLE) mk |= 1ull << k;
  }
  mask[i] = mk;
}

__global__ __launch_bounds__(256) void k_tx_faces(const int* __restrict__ faces, int m, int n, const RsVert* __restrict__ pv,
                                                  const unsigned long long* __restrict__ mask, int first, int* __restrict__ fview,
                                                  long long* __restrict__ farea) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int a, b, c;
  if (!mesh_face(faces, f, n, a, b, c)) return;  // k_tx_mark fails the call; nothing is read through the index
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
  if (!mesh_face(faces, f, n, a, b, c)) atomicOr(&words[TX_FLAG], 1);
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
  tx_bake<false>(verts, faces, list, fview, nullptr, slots, img, lay, atlas);
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
  RsViewSet& vs = tx->vs;
  const int V = vs.view_count();
  SFMX_REQUIRE(ctx, V >= 1);
  for (long long o : vs.img_off) SFMX_REQUIRE(ctx, o >= 0 && "every view needs an image");
  const size_t nn = (size_t)n, mm = (size_t)m;
  const unsigned nbv = (unsigned)((nn + 255) / 256), nbf = (unsigned)((mm + 255) / 256);

  if (const int rc = vs.prepare(ctx, n, m)) return rc;
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

  SFMX_HIP(ctx, tx->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(tx->res.p, 0, TX_NWORDS * 4, s));
  SFMX_HIP(ctx, hipMemsetAsync(tx->vfaces.p, 0, (size_t)V * 4, s));
  if (m > 0) {
    SFMX_HIP(ctx, hipMemsetAsync(tx->fview.p, 0xFF, mm * 4, s));
    SFMX_HIP(ctx, hipMemsetAsync(tx->farea.p, 0, mm * 8, s));
  }
  for (const RsBatch& b : vs.batches) {
    if (n == 0 || m == 0) break;  // nothing to see; a face of a mesh without vertices fails in k_tx_mark
    SFMX_HIP(ctx, vs.zbuffer(b, verts, n, faces, m, p->z_min, s));
    k_tx_verts<<<nbv, 256, 0, s>>>(verts, n, vs.batch_slots(b), b.count, vs.pv.as<RsVert>(), vs.fl.as<uint8_t>(),
                                   vs.keys.as<unsigned long long>(), p->depth_tol, mask);
    k_tx_faces<<<nbf, 256, 0, s>>>(faces, m, n, vs.pv.as<RsVert>(), mask, b.first, tx->fview.as<int>(), tx->farea.as<long long>());
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
    k_tx_bake<<<dim3((unsigned)rows, (unsigned)((lay.C + TX_GROUP - 1) / TX_GROUP)), 256, 0, s>>>(
        verts, faces, list, tx->fview.as<int>(), vs.d_slots.as<RsSlot>(), vs.img.as<uint8_t>(), lay, tx->atlas.as<uint8_t>());
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
  tx->list = list;
  vs.last_batch = vs.widest;
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
  tx->vs.release();
  tx->in.release();
  for (DevBuf* b : {&tx->work, &tx->res, &tx->fview, &tx->farea, &tx->uvh, &tx->vfaces, &tx->atlas}) b->release();
  tx->t.destroy();
  tx->tb.destroy();
  delete tx;
}

int sfmx_texture_reset(sfmx_ctx* ctx, sfmx_texture* tx) {
  SFMX_REQUIRE(ctx, ctx && tx);
  return tx->vs.reset();
}

int sfmx_texture_add_stereo_view(sfmx_ctx* ctx, sfmx_texture* tx, const sfmx_fusion_view* view, const sfmx_stereo* st) {
  SFMX_REQUIRE(ctx, ctx && tx);
  return tx->vs.add_stereo_view(ctx, view, st);
}

int sfmx_texture_add_view(sfmx_ctx* ctx, sfmx_texture* tx, const sfmx_fusion_view* view, const uint8_t* image, int on_device) {
  SFMX_REQUIRE(ctx, ctx && tx);
  return tx->vs.add_view(ctx, view, image, on_device);
}

int sfmx_texture_view_count(const sfmx_texture* tx) { return tx ? tx->vs.view_count() : 0; }

int sfmx_texture_set_batch(sfmx_texture* tx, int k) { return tx ? tx->vs.set_batch(k) : SFMX_ERR_INVALID; }

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
  MeshDev d;
  SFMX_HIP(ctx, tx->in.stage(verts, nullptr, n, faces, m, ctx->stream, d));
  return tx_run(ctx, tx, d.verts, n, d.faces, m, p);
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

int sfmx_texture_last_batch(const sfmx_texture* tx) { return tx && tx->done ? tx->vs.last_batch : 0; }

}  // extern "C"
