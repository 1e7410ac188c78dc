// visib.hip — which faces and vertices of a mesh a set of cameras really sees: exact multi-view visibility.
//
// A sfmx_visib keeps an ordered list of cameras (and, optionally, one u8 image per camera on the device).  A run builds the
// exact z-buffer of the whole mesh (no culling: back faces occlude too) for every camera, tests every vertex
// against the key image of every camera, tallies per face the cameras that see it from the front and from behind, drops the
// faces that fewer than min_views cameras see from the front, compacts the mesh as sfmx_clean does and, with images, averages
// per vertex the pixels of the cameras that see it.
//
// Exactness: the key image is the renderer's (sfmx_raster_dev.h: the same kernels, a minimum over fragments, so order-free).  A
// vertex is compared with one key through one double addition and one comparison (built with -ffp-contract=off); everything
// after that is an integer, and every output offset comes from a scan.  tests/visib_ref.py restates it in NumPy; the tests
// compare bytes.  The batch size, every grid size and RS_BATCH_BUDGET change the speed only.
//
// Kernel layout (blocks of 256, the context's stream, no inter-workgroup hand-off, no spinning).  The views are processed in
// batches of at most 64, the view being the grid's second dimension of the z-buffer kernels; a batch is sized so that its key
// images, projected vertices (16 + 1 bytes per view and vertex) and lists of big faces stay within RS_BATCH_BUDGET (sfmx_raster_dev.h: RsViewSet):
//   k_rs_project / k_rs_faces / k_rs_big <true>   the key images of the batch's views (RsViewSet::zbuffer)
//   k_vb_verts    one thread per vertex over the batch's views: the vertex's snapped pixel, the key there, the depth test
//                 (rs_vertex_sees, shared with k_tx_verts); the
//                 three pair counters, the number of seeing views and acc / cnt of the grey average stay in registers across the
//                 views (as k_sh_shade's do) and are added to the per-vertex arrays once per batch; the camera is read through a
//                 wave-uniform index.  It leaves one bit per view in a 64-bit mask per vertex and one partial of the pair
//                 counters per block.
//   k_vb_faces    one thread per face: the AND of its corners' masks, and per set bit the sign of the integer area A from the
//                 snapped corners of that view
//   k_vb_mark     after the last batch, per face: the range check of its indices (the call's flag), the keep rule, the keep
//                 flags of its corners, one partial of the three face counts per block
//   k_scan_*      exclusive scans of the face and vertex flags (scan.hip)
//   k_mesh_emit_* the kept vertices (bytes copied), normals, renumbered faces, vert_src and face_src (sfmx_mesh_dev.h: MeshCompact)
//   k_vb_grey     per vertex: the rounded average or `fill`
//   k_vb_sum      one block adds the partials
// One host synchronisation at the end of a run.
#include <cmath>
#include <vector>

#include "sfmx_internal.h"
#include "sfmx_raster_dev.h"

namespace {

enum { VB_SEEN = 0, VB_BACK_ONLY, VB_UNSEEN, VB_PAIRS_VISIBLE, VB_PAIRS_OCCLUDED, VB_PAIRS_OFF, VB_NTOT };  // uint64 totals
enum { VB_FLAG = 0, VB_NF_OUT, VB_NV_OUT, VB_NWORDS = 4 };                                                  // int32 words after them

template <bool IMG>
__global__ __launch_bounds__(256) void k_vb_verts(const double* __restrict__ verts, const double* __restrict__ normals, int n,
                                                  const RsSlot* __restrict__ slots, int nb, const RsVert* __restrict__ pv,
                                                  const uint8_t* __restrict__ fl, const unsigned long long* __restrict__ keys,
                                                  const uint8_t* __restrict__ img, double depth_tol, int cull,
                                                  unsigned long long* __restrict__ mask, int* __restrict__ vviews, int* __restrict__ acc,
                                                  int* __restrict__ cnt, unsigned long long* __restrict__ pair_parts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  unsigned long long vis = 0, occ = 0, off = 0;
  if (i < n) {
    const double X0 = verts[3 * (size_t)i], X1 = verts[3 * (size_t)i + 1], X2 = verts[3 * (size_t)i + 2];
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (IMG && cull) {
      n0 = normals[3 * (size_t)i];
      n1 = normals[3 * (size_t)i + 1];
      n2 = normals[3 * (size_t)i + 2];
    }
    unsigned long long mk = 0;
    int a = 0, c = 0;
    for (int k = 0; k < nb; k++) {
      const RsSlot& S = slots[k];
      const size_t at = (size_t)k * (size_t)n + (size_t)i;
      const RsSight r = rs_vertex_sees(S, pv, fl, keys, at, X0, X1, X2, depth_tol);
      if (r.state == RS_SEES_OFF) {
        off++;
        continue;
      }
      if (r.state == RS_SEES_OCCLUDED) {
        occ++;
        continue;
      }
      vis++;
      mk |= 1ull << k;
      if (IMG) {
        if (cull && !(((n0 * r.p0 + n1 * r.p1) + n2 * r.p2) < 0.0)) continue;
        a += (int)img[S.img_off + r.px];
        c += 1;
      }
    }
    mask[i] = mk;
    vviews[i] += (int)vis;
    if (IMG) {
      acc[i] += a;
      cnt[i] += c;
    }
  }
  unsigned long long pairs[3] = {vis, occ, off};
  const unsigned long long s = sfmx_block_sums(pairs);
  if (threadIdx.x < 3) pair_parts[3 * (size_t)blockIdx.x + threadIdx.x] += s;  // launches on one stream: no other writer
}

__global__ __launch_bounds__(256) void k_vb_faces(const int* __restrict__ faces, int m, int n, const RsVert* __restrict__ pv,
                                                  const unsigned long long* __restrict__ mask, int* __restrict__ fviews,
                                                  int* __restrict__ fback) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int a, b, c;
  if (!mesh_face(faces, f, n, a, b, c)) return;  // k_vb_mark fails the call; nothing is read through the index
  unsigned long long mk = mask[a] & mask[b] & mask[c];
  int front = 0, back = 0;
  while (mk) {
    const int k = __ffsll((long long)mk) - 1;
    mk &= mk - 1;
    const RsVert* q = pv + (size_t)k * (size_t)n;
    const RsVert P[3] = {q[a], q[b], q[c]};
    const long long A = rs_area(P);
    front += A < 0 ? 1 : 0;
    back += A > 0 ? 1 : 0;
  }
  if (front) fviews[f] += front;
  if (back) fback[f] += back;
}

__global__ __launch_bounds__(256) void k_vb_mark(const int* __restrict__ faces, int m, int n, const int* __restrict__ fviews,
                                                 const int* __restrict__ fback, int min_views, int* __restrict__ fkeep, int* vkeep,
                                                 int* words, int* __restrict__ count_parts) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  int seen = 0, back_only = 0, unseen = 0;
  if (f < m) {
    int a, b, c;
    bool keep = false;
    if (!mesh_face(faces, f, n, a, b, c)) {
      atomicOr(&words[VB_FLAG], 1);
    } else {
      const int fv = fviews[f], fb = fback[f];
      seen = fv >= 1;
      back_only = fv == 0 && fb >= 1;
      unseen = fv == 0 && fb == 0;
      keep = fv >= min_views;
      if (keep) {
        vkeep[a] = 1;
        vkeep[b] = 1;
        vkeep[c] = 1;
      }
    }
    fkeep[f] = keep ? 1 : 0;
  }
  int tally[3] = {seen, back_only, unseen};
  const int s = sfmx_block_sums(tally);
  if (threadIdx.x < 3) count_parts[3 * (size_t)blockIdx.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_vb_grey(int n, const int* __restrict__ acc, const int* __restrict__ cnt, int fill,
                                                 uint8_t* __restrict__ grey) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = acc[i], c = cnt[i];
  grey[i] = (uint8_t)(c ? (2 * a + c) / (2 * c) : fill);
}

// k_vb_sum's own block sums of three values, valid in thread 0 .. 2 as the return value: with sfmx_block_sums, whose shuffles run
// value by value, the kernel takes two more VGPRs
__device__ __forceinline__ unsigned long long vb_block_sum3(unsigned long long a, unsigned long long b, unsigned long long c) {
  __shared__ unsigned long long sh[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
    c += __shfl_xor(c, off, 64);
  }
  if (lane == 0) {
    sh[wave][0] = a;
    sh[wave][1] = b;
    sh[wave][2] = c;
  }
  __syncthreads();
  const int j = threadIdx.x < 3 ? threadIdx.x : 0;
  return (sh[0][j] + sh[1][j]) + (sh[2][j] + sh[3][j]);
}

__global__ __launch_bounds__(256) void k_vb_sum(const int* __restrict__ count_parts, int nbf, const unsigned long long* __restrict__ pair_parts,
                                                int nbv, unsigned long long* __restrict__ totals) {
  unsigned long long c[3] = {0, 0, 0}, p[3] = {0, 0, 0};
  for (int b = threadIdx.x; b < nbf; b += 256) {
#pragma unroll
    for (int j = 0; j < 3; j++) c[j] += (unsigned long long)count_parts[3 * (size_t)b + j];
  }
  for (int b = threadIdx.x; b < nbv; b += 256) {
#pragma unroll
    for (int j = 0; j < 3; j++) p[j] += pair_parts[3 * (size_t)b + j];
  }
  const unsigned long long sc = vb_block_sum3(c[0], c[1], c[2]);
  __syncthreads();  // the helper's LDS is used again
  const unsigned long long sp = vb_block_sum3(p[0], p[1], p[2]);
  if (threadIdx.x < 3) {
    totals[VB_SEEN + threadIdx.x] = sc;
    totals[VB_PAIRS_VISIBLE + threadIdx.x] = sp;
  }
}

}  // namespace

struct sfmx_visib {
  RsViewSet vs;                                  // the cameras, their images and one batch's z-buffers
  DevBuf work;                                   // masks, flags, offsets, scan partials, count partials
  DevBuf res;                                    // the totals and the words
  MeshInput in;                                  // host inputs, staged
  MeshCompact out;                               // the culled mesh
  DevBuf fviews, fback, vviews, acc, cnt, grey;  // per input element
  bool done = false, has_grey = false;
  int n = 0, m = 0;
  int32_t counts[5] = {};
  uint64_t pairs[3] = {};
  StageTimer t;
};

namespace {

// verts / normals / faces are device pointers
int vb_run(sfmx_ctx* ctx, sfmx_visib* vb, const double* verts, const double* normals, int n, const int32_t* faces, int m,
           const sfmx_visib_params* p) {
  hipStream_t s = ctx->stream;
  RsViewSet& vs = vb->vs;
  const int V = vs.view_count();
  int with_img = 0;
  for (long long o : vs.img_off) with_img += o >= 0 ? 1 : 0;
  SFMX_REQUIRE(ctx, with_img == 0 || with_img == V);  // every view has an image or none has
  const bool grey = with_img > 0;
  SFMX_REQUIRE(ctx, !(grey && p->cull == 1 && n > 0 && !normals));
  const size_t nn = (size_t)n, mm = (size_t)m;
  const unsigned nbv = (unsigned)((nn + 255) / 256), nbf = (unsigned)((mm + 255) / 256);

  if (const int rc = vs.prepare(ctx, n, m)) return rc;
  // work: mask u64 [n], pair_parts u64 [3 nbv], then int32: vkeep, voff [n], fkeep, foff [m], count_parts [3 nbf], the scans' aux
  const size_t aux = sfmx_scan_aux(n > m ? (n > 0 ? n : 1) : m);
  SFMX_HIP(ctx, vb->work.ensure((nn + 3 * (size_t)nbv) * 8 + (2 * nn + 2 * mm + 3 * (size_t)nbf + aux) * 4));
  SFMX_HIP(ctx, vb->res.ensure(VB_NTOT * 8 + VB_NWORDS * 4));
  SFMX_HIP(ctx, vb->out.ensure(nn, mm, normals != nullptr));
  SFMX_HIP(ctx, vb->fviews.ensure(mm * 4));
  SFMX_HIP(ctx, vb->fback.ensure(mm * 4));
  SFMX_HIP(ctx, vb->vviews.ensure(nn * 4));
  SFMX_HIP(ctx, vb->acc.ensure(nn * 4));
  SFMX_HIP(ctx, vb->cnt.ensure(nn * 4));
  SFMX_HIP(ctx, vb->grey.ensure(nn));
  unsigned long long* mask = vb->work.as<unsigned long long>();
  unsigned long long* pair_parts = mask + nn;
  int* vkeep = reinterpret_cast<int*>(pair_parts + 3 * (size_t)nbv);
  int* voff = vkeep + nn;
  int* fkeep = voff + nn;
  int* foff = fkeep + mm;
  int* count_parts = foff + mm;
  int* ax = count_parts + 3 * (size_t)nbf;
  unsigned long long* totals = vb->res.as<unsigned long long>();
  int* words = reinterpret_cast<int*>(totals + VB_NTOT);

  SFMX_HIP(ctx, vb->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(vb->res.p, 0, VB_NTOT * 8 + VB_NWORDS * 4, s));
  if (n > 0) {
    SFMX_HIP(ctx, hipMemsetAsync(pair_parts, 0, 3 * (size_t)nbv * 8, s));
    SFMX_HIP(ctx, hipMemsetAsync(vkeep, 0, nn * 4, s));
    SFMX_HIP(ctx, hipMemsetAsync(vb->vviews.p, 0, nn * 4, s));
    SFMX_HIP(ctx, hipMemsetAsync(vb->acc.p, 0, nn * 4, s));
    SFMX_HIP(ctx, hipMemsetAsync(vb->cnt.p, 0, nn * 4, s));
  }
  if (m > 0) {
    SFMX_HIP(ctx, hipMemsetAsync(vb->fviews.p, 0, mm * 4, s));
    SFMX_HIP(ctx, hipMemsetAsync(vb->fback.p, 0, mm * 4, s));
  }
  for (const RsBatch& b : vs.batches) {
    if (n == 0) break;  // nothing to project; a face of a mesh without vertices fails in k_vb_mark
    const RsSlot* sl = vs.batch_slots(b);
    SFMX_HIP(ctx, vs.zbuffer(b, verts, n, faces, m, p->z_min, s));  // without faces (m == 0) the key images stay empty
    if (grey)
      k_vb_verts<true><<<nbv, 256, 0, s>>>(verts, normals, n, sl, b.count, vs.pv.as<RsVert>(), vs.fl.as<uint8_t>(),
                                           vs.keys.as<unsigned long long>(), vs.img.as<uint8_t>(), p->depth_tol, p->cull, mask,
                                           vb->vviews.as<int>(), vb->acc.as<int>(), vb->cnt.as<int>(), pair_parts);
    else
      k_vb_verts<false><<<nbv, 256, 0, s>>>(verts, normals, n, sl, b.count, vs.pv.as<RsVert>(), vs.fl.as<uint8_t>(),
                                            vs.keys.as<unsigned long long>(), nullptr, p->depth_tol, 0, mask, vb->vviews.as<int>(),
                                            vb->acc.as<int>(), vb->cnt.as<int>(), pair_parts);
    if (m > 0) k_vb_faces<<<nbf, 256, 0, s>>>(faces, m, n, vs.pv.as<RsVert>(), mask, vb->fviews.as<int>(), vb->fback.as<int>());
  }
  if (m > 0) k_vb_mark<<<nbf, 256, 0, s>>>(faces, m, n, vb->fviews.as<int>(), vb->fback.as<int>(), p->min_views, fkeep, vkeep, words, count_parts);
  vb->out.launch(verts, normals, n, faces, m, fkeep, foff, vkeep, voff, ax, words + VB_NF_OUT, words + VB_NV_OUT, m > 0 && n > 0, s);
  if (n > 0 && grey) k_vb_grey<<<nbv, 256, 0, s>>>(n, vb->acc.as<int>(), vb->cnt.as<int>(), p->fill, vb->grey.as<uint8_t>());
  k_vb_sum<<<1, 256, 0, s>>>(count_parts, (int)nbf, pair_parts, (int)nbv, totals);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, vb->t.end(ctx));
  unsigned char back[VB_NTOT * 8 + VB_NWORDS * 4];
  SFMX_HIP(ctx, hipMemcpyAsync(back, vb->res.p, sizeof back, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  vb->t.collect(ctx);
  unsigned long long tot[VB_NTOT];
  int w[VB_NWORDS];
  std::memcpy(tot, back, sizeof tot);
  std::memcpy(w, back + VB_NTOT * 8, sizeof w);
  SFMX_REQUIRE(ctx, w[VB_FLAG] == 0 && "a face index outside [0, n)");
  vb->n = n;
  vb->m = m;
  vb->out.nv_out = w[VB_NV_OUT];
  vb->out.nf_out = w[VB_NF_OUT];
  vb->counts[0] = (int32_t)tot[VB_SEEN];
  vb->counts[1] = (int32_t)tot[VB_BACK_ONLY];
  vb->counts[2] = (int32_t)tot[VB_UNSEEN];
  vb->counts[3] = vb->out.nf_out;
  vb->counts[4] = vb->out.nv_out;
  // without a batch (V = 0) every pair count is 0; a view of a run counts every vertex once
  vb->pairs[0] = tot[VB_PAIRS_VISIBLE];
  vb->pairs[1] = tot[VB_PAIRS_OCCLUDED];
  vb->pairs[2] = tot[VB_PAIRS_OFF];
  vb->out.has_normals = normals != nullptr;
  vb->has_grey = grey;
  vs.last_batch = vs.widest;
  vb->done = true;
  return SFMX_OK;
}

}  // namespace

extern "C" {

void sfmx_visib_default_params(sfmx_visib_params* p) {
  if (!p) return;
  *p = sfmx_visib_params{};
  p->min_views = 1;
  p->cull = 1;
  p->fill = 0;
}

int sfmx_visib_check_params(const sfmx_visib_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (!std::isfinite(p->z_min) || !(p->z_min > 0.0) || !std::isfinite(p->depth_tol) || !(p->depth_tol >= 0.0)) return SFMX_ERR_INVALID;
  if (p->min_views < 0 || (p->cull != 0 && p->cull != 1) || p->fill < 0 || p->fill > 255) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_visib_create(sfmx_ctx* ctx, sfmx_visib** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* vb = new sfmx_visib;
  const hipError_t e = vb->t.create();
  if (e != hipSuccess) {
    sfmx_visib_destroy(ctx, vb);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_visib_create", e);
  }
  *out = vb;
  return SFMX_OK;
}

void sfmx_visib_destroy(sfmx_ctx* ctx, sfmx_visib* vb) {
  if (!vb) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  vb->vs.release();
  vb->in.release();
  vb->out.release();
  for (DevBuf* b : {&vb->work, &vb->res, &vb->fviews, &vb->fback, &vb->vviews, &vb->acc, &vb->cnt, &vb->grey}) b->release();
  vb->t.destroy();
  delete vb;
}

int sfmx_visib_reset(sfmx_ctx* ctx, sfmx_visib* vb) {
  SFMX_REQUIRE(ctx, ctx && vb);
  return vb->vs.reset();
}

int sfmx_visib_add_stereo_view(sfmx_ctx* ctx, sfmx_visib* vb, const sfmx_fusion_view* view, const sfmx_stereo* st) {
  SFMX_REQUIRE(ctx, ctx && vb);
  return vb->vs.add_stereo_view(ctx, view, st);
}

int sfmx_visib_add_view(sfmx_ctx* ctx, sfmx_visib* vb, const sfmx_fusion_view* view, const uint8_t* image, int on_device) {
  SFMX_REQUIRE(ctx, ctx && vb);
  return vb->vs.add_view(ctx, view, image, on_device);
}

int sfmx_visib_view_count(const sfmx_visib* vb) { return vb ? vb->vs.view_count() : 0; }

int sfmx_visib_set_batch(sfmx_visib* vb, int k) { return vb ? vb->vs.set_batch(k) : SFMX_ERR_INVALID; }

int sfmx_visib_run(sfmx_ctx* ctx, sfmx_visib* vb, const double* verts, const double* normals, int n, const int32_t* faces, int m,
                   int on_device, const sfmx_visib_params* p) {
  SFMX_REQUIRE(ctx, ctx && vb);
  vb->done = false;  // every failure from here on leaves no result behind
  vb->t.us = 0.0;
  SFMX_REQUIRE(ctx, sfmx_visib_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, n >= 0 && n < SFMX_RASTER_MAX_VERTS && m >= 0 && m < SFMX_RASTER_MAX_FACES);
  SFMX_REQUIRE(ctx, (verts || n == 0) && (faces || m == 0));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return vb_run(ctx, vb, verts, normals, n, faces, m, p);
  MeshDev d;
  SFMX_HIP(ctx, vb->in.stage(verts, normals, n, faces, m, ctx->stream, d, 8));  // padded: an empty mesh given with normals has normals
  return vb_run(ctx, vb, d.verts, d.normals, n, d.faces, m, p);
}

int sfmx_visib_read(sfmx_ctx* ctx, sfmx_visib* vb, double* verts_out, double* normals_out, int32_t* faces_out, int32_t* vert_src,
                    int32_t* face_src, int32_t* face_views, int32_t* face_back_views, int32_t* vert_views, uint8_t* grey,
                    int32_t* grey_views) {
  SFMX_REQUIRE(ctx, ctx && vb && vb->done);
  SFMX_REQUIRE(ctx, !normals_out || vb->out.has_normals);
  SFMX_REQUIRE(ctx, (!grey && !grey_views) || vb->has_grey);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t n = (size_t)vb->n, m = (size_t)vb->m;
  SFMX_HIP(ctx, vb->out.read(verts_out, normals_out, faces_out, vert_src, face_src, s));
  if (face_views && m) SFMX_HIP(ctx, hipMemcpyAsync(face_views, vb->fviews.p, m * 4, hipMemcpyDeviceToHost, s));
  if (face_back_views && m) SFMX_HIP(ctx, hipMemcpyAsync(face_back_views, vb->fback.p, m * 4, hipMemcpyDeviceToHost, s));
  if (vert_views && n) SFMX_HIP(ctx, hipMemcpyAsync(vert_views, vb->vviews.p, n * 4, hipMemcpyDeviceToHost, s));
  if (grey && n) SFMX_HIP(ctx, hipMemcpyAsync(grey, vb->grey.p, n, hipMemcpyDeviceToHost, s));
  if (grey_views && n) SFMX_HIP(ctx, hipMemcpyAsync(grey_views, vb->cnt.p, n * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

int sfmx_visib_sizes(const sfmx_visib* vb, int* n, int* m, int* n_verts_out, int* n_faces_out) {
  const bool have = vb && vb->done;
  if (n) *n = have ? vb->n : 0;
  if (m) *m = have ? vb->m : 0;
  if (n_verts_out) *n_verts_out = have ? vb->out.nv_out : 0;
  if (n_faces_out) *n_faces_out = have ? vb->out.nf_out : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_visib_counts(const sfmx_visib* vb, int32_t* counts5, uint64_t* pairs3) {
  const bool have = vb && vb->done;
  if (counts5)
    for (int k = 0; k < 5; k++) counts5[k] = have ? vb->counts[k] : 0;
  if (pairs3)
    for (int k = 0; k < 3; k++) pairs3[k] = have ? vb->pairs[k] : 0;
  return have ? SFMX_OK : SFMX_ERR_INVALID;
}

int sfmx_visib_device_mesh(const sfmx_visib* vb, const double** verts, const int32_t** faces, int* n_verts, int* n_faces) {
  return MeshCompact::device_mesh(vb && vb->done ? &vb->out : nullptr, verts, faces, n_verts, n_faces);
}

int sfmx_visib_device_surface(const sfmx_visib* vb, const double** verts, const double** normals) {
  return MeshCompact::device_surface(vb && vb->done ? &vb->out : nullptr, verts, normals);
}

double sfmx_visib_last_us(const sfmx_visib* vb) { return vb ? vb->t.us : 0.0; }

int sfmx_visib_last_batch(const sfmx_visib* vb) { return vb && vb->done ? vb->vs.last_batch : 0; }

}  // extern "C"
