// photo.hip — the textured mesh rendered back into cameras and compared with their pictures: exact photometric error
// (DESIGN.md 27).
//
// A sfmx_photo keeps an ordered list of cameras, each with or without a u8 image and with the index of that camera in the
// texture object's list (or -1).  A run builds the exact z-buffer of the whole mesh for every camera (through
// RsViewSet as visib.hip and texture.hip do), then per pixel reads the winner's place in the atlas of a sfmx_texture (or the
// levelled atlas of a sfmx_level) bilinearly, at the perspective-correct blend of the face's three corners in half-texels, and
// where the view has an image adds |rendered - image| to the sums and the histogram of the pixel's class.
//
// Exactness: the key image is the renderer's (sfmx_raster_dev.h: the same kernels).  A pixel's rendered value is a fixed
// sequence of double operations (built with -ffp-contract=off) on values that depend on (face, pixel) alone, written by exactly
// one thread.  Every count, sum and histogram bin is an integer sum, and integer adds commute.  tests/photo_ref.py restates it
// in NumPy; the tests compare bytes.  The batch size, every grid size and RS_BATCH_BUDGET change the speed only.
//
// Kernel layout (blocks of 256, the context's stream, no inter-workgroup hand-off, no spinning, no float atomics):
//   k_ph_check    once per run, one thread per face: the range check of its indices (the call's flag)
// Per batch of at most 64 views (sfmx_raster_dev.h: RsViewSet):
//   k_rs_project / k_rs_faces / k_rs_big <true>   the key images of the batch's views (RsViewSet::zbuffer)
//   k_ph_resolve  the hot path: grid (16 x 16 tiles of the batch's largest view, views of the batch), one thread per pixel, a
//                 wave is an 8 x 8 tile (as k_rs_resolve).  It stores rendered, cls and face of every pixel, so the slabs need
//                 no memset.  Class counts: one ballot and at most one 64-bit atomicAdd per wave and class.  The six sums: a
//                 ballot (the count) and two wave reductions (the sums of d and d d fit 32 bits: 64 x 255^2 < 2^23), then one
//                 64-bit integer atomicAdd per wave and non-zero quantity.  The histogram: an LDS table of 2 x 256 words per
//                 block, LDS atomics, flushed as non-zero bins only with 64-bit integer atomics.
// One host synchronisation per run, at the end (the flag).
#include <cmath>
#include <vector>

#include "sfmx_internal.h"
#include "sfmx_raster_dev.h"
#include "sfmx_texture_dev.h"

namespace {

constexpr long long PH_PIXELS_MAX = 1ll << 28;  // the sum of w h over the views

// what the resolve needs of a view beyond its slot
struct PhView {
  long long out_off;  // of its pixels in the per-pixel outputs
  int tex_view;       // its index in the texture object's list, or -1
  int has_img;
};

struct PhArgs {
  const unsigned long long* keys;
  const int* faces;
  const RsVert* pv;
  int n;
  const RsSlot* slots;   // of the batch's first view
  const PhView* pviews;  // likewise
  const uint8_t* img;
  const int* fview;
  const int* uvh;
  const uint8_t* atlas;
  int W, H, fill, background;
  uint8_t* rendered;
  uint8_t* cls;
  int* face;
  unsigned long long *classes, *stats, *hist;  // of the batch's first view: [5], [2][3], [2][256] per view
};

__global__ __launch_bounds__(256) void k_ph_check(const int* __restrict__ faces, int m, int n, int* flag) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int a, b, c;
  if (!mesh_face(faces, f, n, a, b, c)) atomicOr(flag, 1);  // the call fails; nothing is read through the index
}

__device__ __forceinline__ unsigned ph_wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_ph_resolve(PhArgs a) {
  __shared__ unsigned bins[2 * 256];
  const int view = blockIdx.y;
  const RsSlot& S = a.slots[view];
  const int w = S.cam.w, h = S.cam.h;
  const int tw = (w + 15) >> 4, th = (h + 15) >> 4;  // tw <= 256 and w h <= 2^24, so tw th < 2^31
  if ((int)blockIdx.x >= tw * th) return;            // uniform over the block: a smaller view of the batch
  const PhView pw = a.pviews[view];
  bins[threadIdx.x] = 0;
  bins[threadIdx.x + 256] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = (int)(blockIdx.x % tw) * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = (int)(blockIdx.x / tw) * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool live = x < w && y < h;
  const size_t px = (size_t)y * w + x;
  const unsigned long long key = live ? a.keys[S.key_off + px] : ~0ull;
  int c = 0, fwin = -1, out = a.background;
  if (key != ~0ull) {
    fwin = (int)(unsigned)(key & 0xffffffffull);
    const RsVert* q = a.pv + (size_t)view * (size_t)a.n;
    const RsVert P[3] = {q[a.faces[3 * (size_t)fwin]], q[a.faces[3 * (size_t)fwin + 1]], q[a.faces[3 * (size_t)fwin + 2]]};  // checked by k_rs_faces
    RsFace F;
    rs_setup(P, F);
    const int k = a.fview[fwin];
    if (F.back) {
      c = 1;
    } else if (k < 0) {
      c = 2;
      out = a.fill;
    } else {
      c = k == pw.tex_view ? 3 : 4;
      const long long e0 = rs_edge(F, 0, x, y), e1 = rs_edge(F, 1, x, y), e2 = rs_edge(F, 2, x, y);
      const double s = rs_s(e0, e1, e2, P);
      const double t0 = (double)e0 * P[0].r, t1 = (double)e1 * P[1].r, t2 = (double)e2 * P[2].r;
      const int* hc = a.uvh + 6 * (size_t)fwin;
      const double hx = ((t0 * (double)hc[0] + t1 * (double)hc[2]) + t2 * (double)hc[4]) / s;
      const double hy = ((t0 * (double)hc[1] + t1 * (double)hc[3]) + t2 * (double)hc[5]) / s;
      const double ax = hx * 0.5 - 0.5, ay = hy * 0.5 - 0.5;
      const double acx = fmin(fmax(ax, 0.0), (double)(a.W - 1)), acy = fmin(fmax(ay, 0.0), (double)(a.H - 1));
      const double x0 = floor(acx), y0 = floor(acy);
      const double fx = acx - x0, fy = acy - y0;
      const int xi0 = (int)x0, xi1 = min(xi0 + 1, a.W - 1);
      const int yi0 = (int)y0, yi1 = min(yi0 + 1, a.H - 1);
      const uint8_t* A0 = a.atlas + (size_t)yi0 * a.W;
      const uint8_t* A1 = a.atlas + (size_t)yi1 * a.W;
      const double top = (1.0 - fx) * (double)A0[xi0] + fx * (double)A0[xi1];
      const double bot = (1.0 - fx) * (double)A1[xi0] + fx * (double)A1[xi1];
      const double g = (1.0 - fy) * top + fy * bot;
      out = (int)fmin(255.0, floor(g + 0.5));
    }
  }
  if (live) {
    const size_t o = (size_t)pw.out_off + px;
    a.rendered[o] = (uint8_t)out;
    a.cls[o] = (uint8_t)c;
    a.face[o] = fwin;
  }
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const unsigned long long b = __ballot(live && c == k);
    if (lane == 0 && b) atomicAdd(&a.classes[(size_t)view * 5 + k], (unsigned long long)__popcll(b));
  }
  if (!pw.has_img) return;  // uniform over the block: nothing was added to bins
  const bool scored = live && c >= 3;
  unsigned d = 0;
  if (scored) {
    const int di = out - (int)a.img[S.img_off + (long long)px];
    d = (unsigned)(di < 0 ? -di : di);
    atomicAdd(&bins[(c - 3) * 256 + (int)d], 1u);
  }
#pragma unroll
  for (int o = 0; o < 2; o++) {
    const bool mine = scored && c == 3 + o;
    const unsigned long long b = __ballot(mine);
    if (!b) continue;  // uniform over the wave
    const unsigned sd = ph_wave_sum(mine ? d : 0u), sd2 = ph_wave_sum(mine ? d * d : 0u);
    if (lane == 0) {
      unsigned long long* st = a.stats + (size_t)view * 6 + 3 * o;
      atomicAdd(&st[0], (unsigned long long)__popcll(b));
      if (sd) atomicAdd(&st[1], (unsigned long long)sd);
      if (sd2) atomicAdd(&st[2], (unsigned long long)sd2);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const unsigned v = bins[threadIdx.x + 256 * j];
    if (v) atomicAdd(&a.hist[(size_t)view * 512 + threadIdx.x + 256 * j], (unsigned long long)v);
  }
}

}  // namespace

struct sfmx_photo {
  RsViewSet vs;               // the cameras, their images and one batch's z-buffers
  std::vector<int> tex_view;  // per view
  MeshInput in;               // host inputs, staged
  DevBuf pviews, res;         // the PhView records; the flag
  DevBuf rendered, cls, face, sums;  // the result: per pixel, and int64 [Q][5], [Q][2][3], [Q][2][256]
  std::vector<StageTimer> tr;        // k_ph_resolve, one pair of events per batch
  bool done = false;
  int Q = 0;
  long long px = 0;
  double resolve_us = 0.0;
  StageTimer t;  // the whole run
};

namespace {

// verts / faces are device pointers
int ph_run(sfmx_ctx* ctx, sfmx_photo* ph, const sfmx_texture* tx, const uint8_t* atlas, const double* verts, int n, const int32_t* faces,
           int m, const sfmx_photo_params* p) {
  hipStream_t s = ctx->stream;
  RsViewSet& vs = ph->vs;
  const int Q = vs.view_count();
  long long total = 0;
  std::vector<PhView> pvs((size_t)Q);
  for (int q = 0; q < Q; q++) {
    pvs[q] = PhView{total, ph->tex_view[q], vs.img_off[q] >= 0 ? 1 : 0};
    total += (long long)vs.views[q].w * vs.views[q].h;
  }
  SFMX_REQUIRE(ctx, total <= PH_PIXELS_MAX && "the views have more than 2^28 pixels");  // before any allocation
  const size_t np = (size_t)total, QQ = (size_t)Q, nsums = QQ * (5 + 6 + 512);
  if (const int rc = vs.prepare(ctx, n, m)) return rc;
  SFMX_HIP(ctx, ph->rendered.ensure(np));
  SFMX_HIP(ctx, ph->cls.ensure(np));
  SFMX_HIP(ctx, ph->face.ensure(np * 4));
  SFMX_HIP(ctx, ph->sums.ensure(nsums * 8));
  SFMX_HIP(ctx, ph->pviews.ensure(QQ * sizeof(PhView)));
  SFMX_HIP(ctx, ph->res.ensure(4));
  if (ctx->timing) {
    while (ph->tr.size() < vs.batches.size()) {
      StageTimer st;
      const hipError_t e = st.create();
      if (e != hipSuccess) {
        st.destroy();
        return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_photo_run", e);
      }
      ph->tr.push_back(st);
    }
  }
  unsigned long long* classes = ph->sums.as<unsigned long long>();
  unsigned long long* stats = classes + QQ * 5;
  unsigned long long* hist = stats + QQ * 6;

  SFMX_HIP(ctx, ph->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(ph->res.p, 0, 4, s));
  if (Q > 0) {
    SFMX_HIP(ctx, hipMemsetAsync(ph->sums.p, 0, nsums * 8, s));
    SFMX_HIP(ctx, hipMemcpyAsync(ph->pviews.p, pvs.data(), QQ * sizeof(PhView), hipMemcpyHostToDevice, s));
  }
  if (m > 0) k_ph_check<<<(unsigned)(((size_t)m + 255) / 256), 256, 0, s>>>(faces, m, n, ph->res.as<int>());
  size_t nb = 0;
  for (const RsBatch& b : vs.batches) {
    if (n > 0 && m > 0) {
      SFMX_HIP(ctx, vs.zbuffer(b, verts, n, faces, m, p->z_min, s));
    } else {  // nothing to draw; a face of a mesh without vertices fails in k_ph_check
      SFMX_HIP(ctx, hipMemsetAsync(vs.keys.p, 0xFF, b.px * 8, s));
    }
    unsigned tiles = 0;
    for (int k = b.first; k < b.first + b.count; k++) {
      const unsigned t = (unsigned)((vs.views[k].w + 15) / 16) * (unsigned)((vs.views[k].h + 15) / 16);
      tiles = t > tiles ? t : tiles;
    }
    PhArgs a{vs.keys.as<unsigned long long>(), faces, vs.pv.as<RsVert>(), n, vs.batch_slots(b), ph->pviews.as<PhView>() + b.first,
             vs.img.as<uint8_t>(), tx->fview.as<int>(), tx->uvh.as<int>(), atlas, tx->lay.W, tx->lay.H, tx->lay.fill, (int)p->background,
             ph->rendered.as<uint8_t>(), ph->cls.as<uint8_t>(), ph->face.as<int>(), classes + (size_t)b.first * 5,
             stats + (size_t)b.first * 6, hist + (size_t)b.first * 512};
    if (ctx->timing) SFMX_HIP(ctx, ph->tr[nb].begin(ctx));
    k_ph_resolve<<<dim3(tiles, (unsigned)b.count), 256, 0, s>>>(a);
    if (ctx->timing) SFMX_HIP(ctx, ph->tr[nb].end(ctx));
    nb++;
  }
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, ph->t.end(ctx));
  int flag = 0;
  SFMX_HIP(ctx, hipMemcpyAsync(&flag, ph->res.p, 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));  // the caller may reuse its arrays
  SFMX_REQUIRE(ctx, flag == 0 && "a face index outside [0, n)");
  ph->t.collect(ctx);
  if (ctx->timing) {
    for (size_t k = 0; k < nb; k++) {
      ph->tr[k].us = 0.0;
      ph->tr[k].collect(ctx);
      ph->resolve_us += ph->tr[k].us;
    }
  }
  ph->Q = Q;
  ph->px = total;
  vs.last_batch = vs.widest;
  ph->done = true;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_photo_default_params(sfmx_photo_params* p) {
  if (!p) return;
  *p = sfmx_photo_params{};
}

int sfmx_photo_check_params(const sfmx_photo_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!(p->z_min > 0.0) || !std::isfinite(p->z_min)) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_photo_create(sfmx_ctx* ctx, sfmx_photo** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* ph = new sfmx_photo;
  const hipError_t e = ph->t.create();
  if (e != hipSuccess) {
    sfmx_photo_destroy(ctx, ph);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_photo_create", e);
  }
  *out = ph;
  return SFMX_OK;
}

void sfmx_photo_destroy(sfmx_ctx* ctx, sfmx_photo* ph) {
  if (!ph) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  ph->vs.release();
  ph->in.release();
  for (DevBuf* b : {&ph->pviews, &ph->res, &ph->rendered, &ph->cls, &ph->face, &ph->sums}) b->release();
  ph->t.destroy();
  for (StageTimer& st : ph->tr) st.destroy();
  delete ph;
}

int sfmx_photo_reset(sfmx_ctx* ctx, sfmx_photo* ph) {
  SFMX_REQUIRE(ctx, ctx && ph);
  ph->tex_view.clear();
  return ph->vs.reset();
}

int sfmx_photo_add_view(sfmx_ctx* ctx, sfmx_photo* ph, const sfmx_fusion_view* view, const uint8_t* image, int on_device, int tex_view) {
  SFMX_REQUIRE(ctx, ctx && ph);
  SFMX_REQUIRE(ctx, tex_view >= -1);
  if (const int rc = ph->vs.add_view(ctx, view, image, on_device)) return rc;
  ph->tex_view.push_back(tex_view);
  return SFMX_OK;
}

int sfmx_photo_add_texture_views(sfmx_ctx* ctx, sfmx_photo* ph, const sfmx_texture* tx) {
  SFMX_REQUIRE(ctx, ctx && ph && tx);
  const RsViewSet& src = tx->vs;
  for (int k = 0; k < src.view_count(); k++) {
    const uint8_t* im = src.img_off[k] >= 0 ? src.img.as<uint8_t>() + src.img_off[k] : nullptr;
    if (const int rc = ph->vs.add_view(ctx, &src.views[k], im, 1)) return rc;
    ph->tex_view.push_back(k);
  }
  return SFMX_OK;
}

int sfmx_photo_view_count(const sfmx_photo* ph) { return ph ? ph->vs.view_count() : 0; }

int sfmx_photo_set_batch(sfmx_photo* ph, int k) { return ph ? ph->vs.set_batch(k) : SFMX_ERR_INVALID; }

int sfmx_photo_run(sfmx_ctx* ctx, sfmx_photo* ph, const sfmx_texture* tx, const sfmx_level* lv, const double* verts, int n,
                   const int32_t* faces, int m, int on_device, const sfmx_photo_params* p) {
  SFMX_REQUIRE(ctx, ctx && ph);
  ph->done = false;  // every failure from here on leaves no result behind
  ph->t.us = 0.0;
  ph->resolve_us = 0.0;
  SFMX_REQUIRE(ctx, sfmx_photo_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, tx && tx->done && "the texture object needs a successful run");
  SFMX_REQUIRE(ctx, n == tx->n && m == tx->m && "the mesh of the texture object's last run");
  const uint8_t* atlas = tx->atlas.as<uint8_t>();
  if (lv) {
    int W = 0, H = 0;
    SFMX_REQUIRE(ctx, sfmx_level_device_atlas(lv, &atlas, &W, &H) >= 0 && "the level object needs a successful run");
    SFMX_REQUIRE(ctx, W == tx->lay.W && H == tx->lay.H && "the level object's atlas has the texture object's size");
  }
  for (int k : ph->tex_view) SFMX_REQUIRE(ctx, k >= -1 && k < tx->nviews && "tex_view is -1 or a view of the texture object");
  SFMX_REQUIRE(ctx, (verts || n == 0) && (faces || m == 0));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return ph_run(ctx, ph, tx, atlas, verts, n, faces, m, p);
  MeshDev d;
  SFMX_HIP(ctx, ph->in.stage(verts, nullptr, n, faces, m, ctx->stream, d));
  return ph_run(ctx, ph, tx, atlas, d.verts, n, d.faces, m, p);
}

int sfmx_photo_read(sfmx_ctx* ctx, sfmx_photo* ph, uint8_t* rendered, uint8_t* cls, int32_t* face, int64_t* classes, int64_t* stats,
                    int64_t* hist) {
  SFMX_REQUIRE(ctx, ctx && ph && ph->done);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t np = (size_t)ph->px, Q = (size_t)ph->Q;
  const unsigned long long* base = ph->sums.as<unsigned long long>();
  if (rendered && np) SFMX_HIP(ctx, hipMemcpyAsync(rendered, ph->rendered.p, np, hipMemcpyDeviceToHost, s));
  if (cls && np) SFMX_HIP(ctx, hipMemcpyAsync(cls, ph->cls.p, np, hipMemcpyDeviceToHost, s));
  if (face && np) SFMX_HIP(ctx, hipMemcpyAsync(face, ph->face.p, np * 4, hipMemcpyDeviceToHost, s));
  if (classes && Q) SFMX_HIP(ctx, hipMemcpyAsync(classes, base, Q * 5 * 8, hipMemcpyDeviceToHost, s));
  if (stats && Q) SFMX_HIP(ctx, hipMemcpyAsync(stats, base + Q * 5, Q * 6 * 8, hipMemcpyDeviceToHost, s));
  if (hist && Q) SFMX_HIP(ctx, hipMemcpyAsync(hist, base + Q * 11, Q * 512 * 8, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

int sfmx_photo_sizes(const sfmx_photo* ph, int* n_views, int* pixels) {
  const bool have = ph && ph->done;
  if (n_views) *n_views = have ? ph->Q : 0;
  if (pixels) *pixels = have ? (int)ph->px : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_photo_device_rendered(const sfmx_photo* ph, const uint8_t** rendered) {
  const bool have = ph && ph->done;
  if (rendered) *rendered = have ? ph->rendered.as<uint8_t>() : nullptr;
  return have ? (int)ph->px : -1;
}

double sfmx_photo_last_us(const sfmx_photo* ph) { return ph ? ph->t.us : 0.0; }

double sfmx_photo_last_resolve_us(const sfmx_photo* ph) { return ph ? ph->resolve_us : 0.0; }

int sfmx_photo_last_batch(const sfmx_photo* ph) { return ph && ph->done ? ph->vs.last_batch : 0; }

}  // extern "C"
