// raster.hip — a triangle mesh seen from any pinhole camera: an exact z-buffer.  Per pixel the visible face, its depth, point,
// normal, a head-light shade and (with per-vertex grey) an interpolated grey value.
//
// There is NO near-plane clipping and no guard-band clipping: a face with a vertex nearer than z_min (faces_behind) or with a
// vertex whose image position leaves the band |u|, |v| <= 16384 (faces_outside) is counted and dropped whole.
//
// Exactness: vertices are projected in IEEE double in the definition's expression order (built with -ffp-contract=off) and
// snapped to 1 / 256 pixel.  Coverage is three int64 edge functions on the snapped coordinates with a top-left rule, so it is
// integer.  A fragment's depth is one fixed double expression of (face, pixel); it is rounded to float only to form the key
// (bits((float)depth) << 32) | face, and the pixel's winner is the smallest key: one 64-bit atomicMin per fragment, and a
// minimum does not depend on the order of its candidates.  Everything a pixel reports is then recomputed in double from the
// winning face alone.  tests/raster_ref.py restates the definition in NumPy (every face against every pixel); the tests compare
// bytes.  RS_SMALL, the tile shape and every grid size below change the speed only.
//
// Kernel layout (blocks of 256, the context's stream, no LDS beyond the count reduction, no inter-workgroup hand-off):
//   k_rs_project  one thread per vertex: near / inband flags, U, V (int32: |U| <= 2^22) and r = 1 / q2, once per vertex
//   k_rs_faces    a grid-stride loop over the faces, at most RS_FACE_BLOCKS blocks.  An index outside [0, n) sets the flag and
//                 the face is skipped before anything is read through it.  Classification, then the box of pixel centres the
//                 face can cover (integer ceiling and floor of the snapped extremes, clamped to the image).  A box of at most
//                 RS_SMALL pixels is walked by the thread itself, the edge functions stepped by integer adds; a plain load of the
//                 current key skips an atomicMin that cannot win (keys only ever decrease, so a stale value only costs an
//                 atomic).  A larger box appends the face to the list of big faces with one atomicAdd per wave.  The counts are
//                 one partial per block (registers, wave shuffles, 72 bytes of LDS), never an atomic on a shared word.
//   k_rs_big      a fixed grid strides over that list, its length read from device memory.  One block per face, its four waves
//                 stride over the 8 x 8 tiles of the box, one pixel per lane.  A tile is skipped when one edge function's
//                 largest value over the tile (affine: base plus the positive steps) fails the edge's test, which is exact.
//   k_rs_sum      one block adds the partial counts
//   k_rs_resolve  one thread per pixel, a wave is an 8 x 8 tile (as k_rc_render): the winner's edge functions, depth, point,
//                 normal, shade and grey; hits and back_pixels are a ballot and one atomicAdd per wave each
// The first three kernels and the device helpers live in sfmx_raster_dev.h, which visib.hip and texture.hip share; this file uses their
// one-camera form (BATCH = false).
#include <cmath>

#include "sfmx_internal.h"
#include "sfmx_raster_dev.h"

namespace {

constexpr int RS_SMALL = 64;  // a box of at most this many pixel centres is walked by the face's own thread

__global__ __launch_bounds__(256) void k_rs_sum(const unsigned long long* __restrict__ parts, int nb, unsigned long long* __restrict__ totals) {
  unsigned long long cnt[RS_NPART] = {};
  for (int b = threadIdx.x; b < nb; b += 256) {
#pragma unroll
    for (int k = 0; k < RS_NPART; k++) cnt[k] += parts[(size_t)b * RS_NPART + k];
  }
  const unsigned long long sum = sfmx_block_sums(cnt);
  if (threadIdx.x < RS_NPART) totals[threadIdx.x] = sum;
}

__global__ __launch_bounds__(256) void k_rs_resolve(const unsigned long long* __restrict__ keys, const int* __restrict__ faces,
                                                    const RsVert* __restrict__ pv, const double* __restrict__ verts,
                                                    const double* __restrict__ vnormals, const uint8_t* __restrict__ vgrey, RsCam cam,
                                                    int background, double* __restrict__ depth, int* __restrict__ face,
                                                    double* __restrict__ points, double* __restrict__ normals, uint8_t* __restrict__ shaded,
                                                    uint8_t* __restrict__ grey, unsigned* counters) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool live = x < cam.w && y < cam.h;
  const size_t px = (size_t)y * cam.w + x;
  const unsigned long long key = live ? keys[px] : ~0ull;
  const bool hit = key != ~0ull;
  double d = 0.0, Pt[3] = {0.0, 0.0, 0.0}, nr[3] = {0.0, 0.0, 0.0};
  int fwin = -1, sh = background, gr = background;
  bool back = false;
  if (hit) {
    fwin = (int)(unsigned)(key & 0xffffffffull);
    const int id[3] = {faces[3 * (size_t)fwin], faces[3 * (size_t)fwin + 1], faces[3 * (size_t)fwin + 2]};
    const RsVert P[3] = {pv[id[0]], pv[id[1]], pv[id[2]]};
    RsFace F;
    rs_setup(P, F);
    back = F.back;
    const long long e0 = rs_edge(F, 0, x, y), e1 = rs_edge(F, 1, x, y), e2 = rs_edge(F, 2, x, y);
    const double s = rs_s(e0, e1, e2, P);
    d = (double)F.absA / s;
    const double dc0 = ((double)x - cam.cx) / cam.f, dc1 = ((double)y - cam.cy) / cam.f;
    double dw[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      dw[a] = (cam.R[a] * dc0 + cam.R[3 + a] * dc1) + cam.R[6 + a] * 1.0;
      Pt[a] = cam.c[a] + d * dw[a];
    }
    const double t0 = (double)e0 * P[0].r, t1 = (double)e1 * P[1].r, t2 = (double)e2 * P[2].r;
    double N[3];
    if (vnormals) {
#pragma unroll
      for (int a = 0; a < 3; a++)
        N[a] = (t0 * vnormals[3 * (size_t)id[0] + a] + t1 * vnormals[3 * (size_t)id[1] + a]) + t2 * vnormals[3 * (size_t)id[2] + a];
    } else {
      double A[3], B[3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double v0 = verts[3 * (size_t)id[0] + a];
        A[a] = verts[3 * (size_t)id[1] + a] - v0;
        B[a] = verts[3 * (size_t)id[2] + a] - v0;
      }
      N[0] = A[1] * B[2] - A[2] * B[1];
      N[1] = A[2] * B[0] - A[0] * B[2];
      N[2] = A[0] * B[1] - A[1] * B[0];
    }
    const double len = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
    const bool nz = len > 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) nr[a] = nz ? N[a] / len : 0.0;
    const double Ld = sqrt((dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2]);
    const double lam = -(((nr[0] * dw[0] + nr[1] * dw[1]) + nr[2] * dw[2]) / Ld);
    sh = lam > 0.0 ? (int)fmin(255.0, floor(lam * 255.0 + 0.5)) : 0;
    if (vgrey) {
      const double g = ((t0 * (double)vgrey[id[0]] + t1 * (double)vgrey[id[1]]) + t2 * (double)vgrey[id[2]]) / s;
      gr = (int)fmin(255.0, floor(g + 0.5));
    }
  }
  if (live) {
    depth[px] = d;
    face[px] = fwin;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      points[3 * px + a] = Pt[a];
      normals[3 * px + a] = nr[a];
    }
    shaded[px] = (uint8_t)sh;
    if (vgrey) grey[px] = (uint8_t)gr;
  }
  const unsigned long long hb = __ballot(hit), bb = __ballot(hit && back);
  if (lane == 0) {
    if (hb) atomicAdd(&counters[RS_HITS], (unsigned)__popcll(hb));
    if (bb) atomicAdd(&counters[RS_BACKPX], (unsigned)__popcll(bb));
  }
}

}  // namespace

struct sfmx_raster {
  DevBuf keys, depth, face, points, normals, shaded, grey;  // per pixel
  DevBuf pv, fl, big, parts, counters;                      // projected vertices and flags, the big faces, the counts
  DevBuf in_verts, in_normals, in_grey, in_faces;           // sfmx_raster_run's copy of host arrays
  int w = 0, h = 0;                                         // size of the last run; 0 before one
  bool has_grey = false;
  int32_t counts[8] = {};
  uint64_t fragments = 0;
  int big_faces = 0;
  StageTimer t;
};

extern "C" {

void sfmx_raster_default_params(sfmx_raster_params* p) {
  if (!p) return;
  *p = sfmx_raster_params{};
}

int sfmx_raster_check_params(const sfmx_raster_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!(p->z_min > 0.0) || !std::isfinite(p->z_min) || p->cull < 0 || p->cull > 2) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_raster_create(sfmx_ctx* ctx, sfmx_raster** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* rs = new sfmx_raster;
  const hipError_t e = rs->t.create();
  if (e != hipSuccess) {
    sfmx_raster_destroy(ctx, rs);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_raster_create", e);
  }
  *out = rs;
  return SFMX_OK;
}

void sfmx_raster_destroy(sfmx_ctx* ctx, sfmx_raster* rs) {
  if (!rs) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* b : {&rs->keys, &rs->depth, &rs->face, &rs->points, &rs->normals, &rs->shaded, &rs->grey, &rs->pv, &rs->fl, &rs->big,
                    &rs->parts, &rs->counters, &rs->in_verts, &rs->in_normals, &rs->in_grey, &rs->in_faces})
    b->release();
  rs->t.destroy();
  delete rs;
}

int sfmx_raster_run(sfmx_ctx* ctx, sfmx_raster* rs, const double* verts, const double* normals, const uint8_t* grey, int n,
                    const int32_t* faces, int m, int on_device, const sfmx_fusion_view* view, const sfmx_raster_params* p) {
  SFMX_REQUIRE(ctx, ctx && rs);
  rs->w = rs->h = 0;  // a failed run leaves no result
  rs->t.us = 0.0;
  SFMX_REQUIRE(ctx, rs_view_ok(view) && sfmx_raster_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, n >= 0 && n < SFMX_RASTER_MAX_VERTS && m >= 0 && m < SFMX_RASTER_MAX_FACES);
  SFMX_REQUIRE(ctx, (verts || n == 0) && (faces || m == 0));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (!on_device) {
    const size_t nv = (size_t)n, nf = (size_t)m;
    SFMX_HIP(ctx, rs->in_verts.ensure(nv * 24));
    SFMX_HIP(ctx, rs->in_faces.ensure(nf * 12));
    if (n) SFMX_HIP(ctx, hipMemcpyAsync(rs->in_verts.p, verts, nv * 24, hipMemcpyHostToDevice, s));
    if (m) SFMX_HIP(ctx, hipMemcpyAsync(rs->in_faces.p, faces, nf * 12, hipMemcpyHostToDevice, s));
    verts = rs->in_verts.as<double>();
    faces = rs->in_faces.as<int32_t>();
    if (normals) {
      SFMX_HIP(ctx, rs->in_normals.ensure(nv * 24 + 8));
      if (n) SFMX_HIP(ctx, hipMemcpyAsync(rs->in_normals.p, normals, nv * 24, hipMemcpyHostToDevice, s));
      normals = rs->in_normals.as<double>();
    }
    if (grey) {
      SFMX_HIP(ctx, rs->in_grey.ensure(nv + 8));
      if (n) SFMX_HIP(ctx, hipMemcpyAsync(rs->in_grey.p, grey, nv, hipMemcpyHostToDevice, s));
      grey = rs->in_grey.as<uint8_t>();
    }
  }
  const RsCam cam = rs_cam(view);
  const size_t np = (size_t)view->w * view->h;
  const int fb = m > (RS_FACE_BLOCKS - 1) * 256 ? RS_FACE_BLOCKS : (m + 255) / 256;
  const int nparts = m ? fb + RS_BIG_BLOCKS : 0;
  SFMX_HIP(ctx, rs->keys.ensure(np * 8));
  SFMX_HIP(ctx, rs->depth.ensure(np * 8));
  SFMX_HIP(ctx, rs->face.ensure(np * 4));
  SFMX_HIP(ctx, rs->points.ensure(np * 24));
  SFMX_HIP(ctx, rs->normals.ensure(np * 24));
  SFMX_HIP(ctx, rs->shaded.ensure(np));
  SFMX_HIP(ctx, rs->grey.ensure(np));
  SFMX_HIP(ctx, rs->pv.ensure((size_t)n * sizeof(RsVert)));
  SFMX_HIP(ctx, rs->fl.ensure((size_t)n));
  SFMX_HIP(ctx, rs->big.ensure((size_t)m * 4));
  SFMX_HIP(ctx, rs->parts.ensure((size_t)(RS_FACE_BLOCKS + RS_BIG_BLOCKS) * RS_NPART * 8));
  const size_t cbytes = RS_NWORDS * 4 + RS_NPART * 8;
  SFMX_HIP(ctx, rs->counters.ensure(cbytes));
  unsigned* counters = rs->counters.as<unsigned>();
  unsigned long long* totals = reinterpret_cast<unsigned long long*>(counters + RS_NWORDS);
  SFMX_HIP(ctx, rs->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(rs->counters.p, 0, cbytes, s));
  SFMX_HIP(ctx, hipMemsetAsync(rs->keys.p, 0xFF, np * 8, s));
  if (n)
    k_rs_project<false><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(verts, n, cam, nullptr, p->z_min, rs->pv.as<RsVert>(), rs->fl.as<uint8_t>());
  if (m) {
    k_rs_faces<false, RS_SMALL><<<(unsigned)fb, 256, 0, s>>>(faces, m, n, rs->pv.as<RsVert>(), rs->fl.as<uint8_t>(), cam.w, cam.h, p->cull,
                                                   rs->keys.as<unsigned long long>(), rs->big.as<int>(), counters,
                                                   rs->parts.as<unsigned long long>(), nullptr);
    k_rs_big<false><<<RS_BIG_BLOCKS, 256, 0, s>>>(faces, m, n, rs->pv.as<RsVert>(), cam.w, cam.h, rs->keys.as<unsigned long long>(),
                                                  rs->big.as<int>(), counters, rs->parts.as<unsigned long long>() + (size_t)fb * RS_NPART,
                                                  nullptr);
    k_rs_sum<<<1, 256, 0, s>>>(rs->parts.as<unsigned long long>(), nparts, totals);
  }
  // a face that k_rs_faces refused never enters the contest, so the resolve reads through checked indices only and can be
  // queued before the host has seen the flag
  k_rs_resolve<<<dim3((unsigned)((cam.w + 15) / 16), (unsigned)((cam.h + 15) / 16)), 256, 0, s>>>(
      rs->keys.as<unsigned long long>(), faces, rs->pv.as<RsVert>(), verts, normals, grey, cam, (int)p->background, rs->depth.as<double>(),
      rs->face.as<int>(), rs->points.as<double>(), rs->normals.as<double>(), rs->shaded.as<uint8_t>(), rs->grey.as<uint8_t>(), counters);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, rs->t.end(ctx));
  unsigned char back[RS_NWORDS * 4 + RS_NPART * 8];
  SFMX_HIP(ctx, hipMemcpyAsync(back, rs->counters.p, cbytes, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));  // the caller may reuse its arrays
  unsigned words[RS_NWORDS];
  unsigned long long tot[RS_NPART];
  std::memcpy(words, back, sizeof words);
  std::memcpy(tot, back + RS_NWORDS * 4, sizeof tot);
  SFMX_REQUIRE(ctx, words[RS_FLAG] == 0 && "a face index outside [0, n)");
  rs->counts[0] = (int32_t)tot[RS_BEHIND];
  rs->counts[1] = (int32_t)tot[RS_OUTSIDE];
  rs->counts[2] = (int32_t)tot[RS_DEGENERATE];
  rs->counts[3] = (int32_t)tot[RS_BACK];
  rs->counts[4] = (int32_t)tot[RS_CULLED];
  rs->counts[5] = (int32_t)tot[RS_DRAWN];
  rs->counts[6] = (int32_t)words[RS_HITS];
  rs->counts[7] = (int32_t)words[RS_BACKPX];
  rs->fragments = tot[RS_FRAGMENTS];
  rs->big_faces = (int)tot[RS_BIG];
  rs->has_grey = grey != nullptr;
  rs->w = view->w;
  rs->h = view->h;
  rs->t.collect(ctx);
  return SFMX_OK;
}

int sfmx_raster_read(sfmx_ctx* ctx, sfmx_raster* rs, double* depth, int32_t* face, double* points, double* normals, uint8_t* shaded,
                     uint8_t* grey) {
  SFMX_REQUIRE(ctx, ctx && rs && rs->w > 0);
  SFMX_REQUIRE(ctx, !grey || rs->has_grey);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)rs->w * rs->h;
  hipStream_t s = ctx->stream;
  if (depth) SFMX_HIP(ctx, hipMemcpyAsync(depth, rs->depth.p, n * 8, hipMemcpyDeviceToHost, s));
  if (face) SFMX_HIP(ctx, hipMemcpyAsync(face, rs->face.p, n * 4, hipMemcpyDeviceToHost, s));
  if (points) SFMX_HIP(ctx, hipMemcpyAsync(points, rs->points.p, n * 24, hipMemcpyDeviceToHost, s));
  if (normals) SFMX_HIP(ctx, hipMemcpyAsync(normals, rs->normals.p, n * 24, hipMemcpyDeviceToHost, s));
  if (shaded) SFMX_HIP(ctx, hipMemcpyAsync(shaded, rs->shaded.p, n, hipMemcpyDeviceToHost, s));
  if (grey) SFMX_HIP(ctx, hipMemcpyAsync(grey, rs->grey.p, n, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

int sfmx_raster_counts(const sfmx_raster* rs, int32_t* counts8, uint64_t* fragments) {
  const bool have = rs && rs->w > 0;
  if (counts8)
    for (int k = 0; k < 8; k++) counts8[k] = have ? rs->counts[k] : 0;
  if (fragments) *fragments = have ? rs->fragments : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_raster_device_surface(const sfmx_raster* rs, const double** points, const double** normals, int* n) {
  const bool have = rs && rs->w > 0;
  if (points) *points = have ? rs->points.as<double>() : nullptr;
  if (normals) *normals = have ? rs->normals.as<double>() : nullptr;
  if (n) *n = have ? rs->w * rs->h : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

double sfmx_raster_last_us(const sfmx_raster* rs) { return rs ? rs->t.us : 0.0; }

int sfmx_raster_last_big_faces(const sfmx_raster* rs) { return rs && rs->w > 0 ? rs->big_faces : 0; }

}  // extern "C"
