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
// compare bytes.  The batch size, every grid size and VB_BUDGET change the speed only.
//
// Kernel layout (blocks of 256, the context's stream, no inter-workgroup hand-off, no spinning).  The views are processed in
// batches of at most 64, the view being the grid's second dimension of the z-buffer kernels; a batch is sized so that its key
// images, projected vertices (16 + 1 bytes per view and vertex) and lists of big faces stay within VB_BUDGET:
//   k_rs_project / k_rs_faces / k_rs_big <true>   the key images of the batch's views (sfmx_raster_dev.h)
//   k_vb_verts    one thread per vertex over the batch's views: the vertex's snapped pixel, the key there, the depth test; the
//                 three pair counters, the number of seeing views and acc / cnt of the grey average stay in registers across the
//                 views (as k_sh_shade's do) and are added to the per-vertex arrays once per batch; the camera is read through a
//                 wave-uniform index.  It leaves one bit per view in a 64-bit mask per vertex and one partial of the pair
//                 counters per block.
//   k_vb_faces    one thread per face: the AND of its corners' masks, and per set bit the sign of the integer area A from the
//                 snapped corners of that view
//   k_vb_mark     after the last batch, per face: the range check of its indices (the call's flag), the keep rule, the keep
//                 flags of its corners, one partial of the three face counts per block
//   k_scan_*      exclusive scans of the face and vertex flags (scan.hip)
//   k_vb_emit_*   the kept vertices (bytes copied), normals, renumbered faces, vert_src and face_src
//   k_vb_grey     per vertex: the rounded average or `fill`
//   k_vb_sum      one block adds the partials
// One host synchronisation at the end of a run.
#include <cmath>
#include <vector>

#include "sfmx_internal.h"
#include "sfmx_raster_dev.h"

namespace {

constexpr size_t VB_BUDGET = (size_t)256 << 20;  // bytes a batch's key slab, per-(view, vertex) records and big-face lists may take
constexpr int VB_MAX_BATCH = 64;                 // one bit per view in a vertex's mask
constexpr int VB_BIG_BLOCKS = 64;                // blocks of k_rs_big per view
constexpr int VB_SMALL = 64;                     // as raster.hip's RS_SMALL: a larger box of pixel centres goes to k_rs_big

enum { VB_SEEN = 0, VB_BACK_ONLY, VB_UNSEEN, VB_PAIRS_VISIBLE, VB_PAIRS_OCCLUDED, VB_PAIRS_OFF, VB_NTOT };  // uint64 totals
enum { VB_FLAG = 0, VB_NF_OUT, VB_NV_OUT, VB_NWORDS = 4 };                                                  // int32 words after them

// the block's sums of three values, valid in thread 0 .. 2 as the return value
template <class T> __device__ __forceinline__ T vb_block_sum3(T a, T b, T c) {
  __shared__ T sh[4][3];
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
      if (!(fl[at] & 2u)) {  // not inband
        off++;
        continue;
      }
      const RsVert P = pv[at];
      const int x = (P.U + 128) >> 8, y = (P.V + 128) >> 8;
      if (x < 0 || x >= S.cam.w || y < 0 || y >= S.cam.h) {
        off++;
        continue;
      }
      const long long px = (long long)y * S.cam.w + x;
      const unsigned long long key = keys[S.key_off + px];
      double p0, p1, p2;
      const double q2 = rs_depth(S.cam, X0, X1, X2, p0, p1, p2);
      bool visible = true;
      if (key != ~0ull) {
        const double D = (double)__uint_as_float((unsigned)(key >> 32));
        visible = q2 <= D + depth_tol;  // false for a NaN
      }
      if (!visible) {
        occ++;
        continue;
      }
      vis++;
      mk |= 1ull << k;
      if (IMG) {
        if (cull && !(((n0 * p0 + n1 * p1) + n2 * p2) < 0.0)) continue;
        a += (int)img[S.img_off + px];
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
  const unsigned long long s = vb_block_sum3(vis, occ, off);
  if (threadIdx.x < 3) pair_parts[3 * (size_t)blockIdx.x + threadIdx.x] += s;  // launches on one stream: no other writer
}

__device__ __forceinline__ bool vb_face(const int* __restrict__ faces, int f, int n, int& a, int& b, int& c) {
  a = faces[3 * (size_t)f];
  b = faces[3 * (size_t)f + 1];
  c = faces[3 * (size_t)f + 2];
  return (unsigned)a < (unsigned)n && (unsigned)b < (unsigned)n && (unsigned)c < (unsigned)n;
}

__global__ __launch_bounds__(256) void k_vb_faces(const int* __restrict__ faces, int m, int n, const RsVert* __restrict__ pv,
                                                  const unsigned long long* __restrict__ mask, int* __restrict__ fviews,
                                                  int* __restrict__ fback) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int a, b, c;
  if (!vb_face(faces, f, n, a, b, c)) return;  // k_vb_mark fails the call; nothing is read through the index
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
    if (!vb_face(faces, f, n, a, b, c)) {
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
  const int s = vb_block_sum3(seen, back_only, unseen);
  if (threadIdx.x < 3) count_parts[3 * (size_t)blockIdx.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_vb_emit_verts(int n, const int* __restrict__ vkeep, const int* __restrict__ voff,
                                                       const unsigned long long* __restrict__ verts,
                                                       const unsigned long long* __restrict__ normals,
                                                       unsigned long long* __restrict__ verts_out,
                                                       unsigned long long* __restrict__ normals_out, int* __restrict__ vsrc) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n || !vkeep[v]) return;
  const size_t o = (size_t)voff[v], i = (size_t)v;
#pragma unroll
  for (int a = 0; a < 3; a++) verts_out[3 * o + a] = verts[3 * i + a];
  if (normals) {
#pragma unroll
    for (int a = 0; a < 3; a++) normals_out[3 * o + a] = normals[3 * i + a];
  }
  vsrc[o] = v;
}

__global__ __launch_bounds__(256) void k_vb_emit_faces(const int* __restrict__ faces, int m, const int* __restrict__ fkeep,
                                                       const int* __restrict__ foff, const int* __restrict__ voff,
                                                       int* __restrict__ faces_out, int* __restrict__ fsrc) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m || !fkeep[f]) return;  // a kept face has passed the range check
  const size_t o = (size_t)foff[f];
#pragma unroll
  for (int a = 0; a < 3; a++) faces_out[3 * o + a] = voff[faces[3 * (size_t)f + a]];
  fsrc[o] = f;
}

__global__ __launch_bounds__(256) void k_vb_grey(int n, const int* __restrict__ acc, const int* __restrict__ cnt, int fill,
                                                 uint8_t* __restrict__ grey) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = acc[i], c = cnt[i];
  grey[i] = (uint8_t)(c ? (2 * a + c) / (2 * c) : fill);
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

struct VbBatch {
  int first, count;
};

}  // namespace

struct sfmx_visib {
  std::vector<sfmx_fusion_view> views;
  std::vector<long long> img_off;  // of a view's image in the image slab, -1 without one
  std::vector<RsSlot> slots;       // of the last run, as uploaded
  long long img_used = 0;
  int forced_batch = 0, last_batch = 0;
  DevBuf img, d_slots;
  DevBuf keys, pv, fl, big, rcounters;                                   // one batch's z-buffers
  DevBuf work;                                                           // masks, flags, offsets, scan partials, count partials
  DevBuf res;                                                            // the totals and the words
  DevBuf in_v, in_n, in_f;                                               // host inputs, staged
  DevBuf out_v, out_n, out_f, vsrc, fsrc;                                // the culled mesh
  DevBuf fviews, fback, vviews, acc, cnt, grey;                          // per input element
  bool done = false, has_normals = false, has_grey = false;
  int n = 0, m = 0, nv_out = 0, nf_out = 0;
  int32_t counts[5] = {};
  uint64_t pairs[3] = {};
  StageTimer t;
};

namespace {

std::vector<VbBatch> vb_plan(const sfmx_visib* vb, int n, int m, size_t& key_px, int& widest) {
  std::vector<VbBatch> out;
  const int V = (int)vb->views.size();
  key_px = 0;
  widest = 0;
  int k = 0;
  while (k < V) {
    size_t bytes = 0, px = 0;
    int c = 0;
    while (k + c < V && c < VB_MAX_BATCH) {
      const size_t p = (size_t)vb->views[k + c].w * (size_t)vb->views[k + c].h;
      const size_t one = p * 8 + (size_t)n * 17 + (size_t)m * 4;
      if (vb->forced_batch ? c >= vb->forced_batch : (c > 0 && bytes + one > VB_BUDGET)) break;
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

// verts / normals / faces are device pointers
int vb_run(sfmx_ctx* ctx, sfmx_visib* vb, const double* verts, const double* normals, int n, const int32_t* faces, int m,
           const sfmx_visib_params* p) {
  hipStream_t s = ctx->stream;
  const int V = (int)vb->views.size();
  int with_img = 0;
  for (long long o : vb->img_off) with_img += o >= 0 ? 1 : 0;
  SFMX_REQUIRE(ctx, with_img == 0 || with_img == V);  // every view has an image or none has
  const bool grey = with_img > 0;
  SFMX_REQUIRE(ctx, !(grey && p->cull == 1 && n > 0 && !normals));
  const size_t nn = (size_t)n, mm = (size_t)m;
  size_t key_px = 0;
  int widest = 0;
  const std::vector<VbBatch> plan = vb_plan(vb, n, m, key_px, widest);
  const unsigned nbv = (unsigned)((nn + 255) / 256), nbf = (unsigned)((mm + 255) / 256);
  const int fb = m > (RS_FACE_BLOCKS - 1) * 256 ? RS_FACE_BLOCKS : (m + 255) / 256;

  SFMX_HIP(ctx, vb->keys.ensure(key_px * 8));
  SFMX_HIP(ctx, vb->pv.ensure((size_t)widest * nn * sizeof(RsVert)));
  SFMX_HIP(ctx, vb->fl.ensure((size_t)widest * nn));
  SFMX_HIP(ctx, vb->big.ensure((size_t)widest * mm * 4));
  SFMX_HIP(ctx, vb->rcounters.ensure((size_t)VB_MAX_BATCH * RS_NWORDS * 4));
  // work: mask u64 [n], pair_parts u64 [3 nbv], then int32: vkeep, voff [n], fkeep, foff [m], count_parts [3 nbf], the scans' aux
  const size_t aux = sfmx_scan_aux(n > m ? (n > 0 ? n : 1) : m);
  SFMX_HIP(ctx, vb->work.ensure((nn + 3 * (size_t)nbv) * 8 + (2 * nn + 2 * mm + 3 * (size_t)nbf + aux) * 4));
  SFMX_HIP(ctx, vb->res.ensure(VB_NTOT * 8 + VB_NWORDS * 4));
  SFMX_HIP(ctx, vb->out_v.ensure(nn * 24));
  if (normals) SFMX_HIP(ctx, vb->out_n.ensure(nn * 24));
  SFMX_HIP(ctx, vb->out_f.ensure(mm * 12));
  SFMX_HIP(ctx, vb->vsrc.ensure(nn * 4));
  SFMX_HIP(ctx, vb->fsrc.ensure(mm * 4));
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

  // the slots of all views: a batch's key images lie back to back in the key slab
  vb->slots.resize((size_t)V);
  for (const VbBatch& b : plan) {
    long long at = 0;
    for (int k = b.first; k < b.first + b.count; k++) {
      vb->slots[k].cam = rs_cam(&vb->views[k]);
      vb->slots[k].key_off = at;
      vb->slots[k].img_off = vb->img_off[k] >= 0 ? vb->img_off[k] : 0;
      at += (long long)vb->views[k].w * vb->views[k].h;
    }
  }
  if (V > 0) {
    SFMX_HIP(ctx, vb->d_slots.ensure(sizeof(RsSlot) * (size_t)V));
    SFMX_HIP(ctx, hipMemcpyAsync(vb->d_slots.p, vb->slots.data(), sizeof(RsSlot) * (size_t)V, hipMemcpyHostToDevice, s));
  }
  const RsSlot* d_slots = vb->d_slots.as<RsSlot>();

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
  for (const VbBatch& b : plan) {
    if (n == 0) break;  // nothing to project; a face of a mesh without vertices fails in k_vb_mark
    size_t px = 0;
    for (int k = b.first; k < b.first + b.count; k++) px += (size_t)vb->views[k].w * (size_t)vb->views[k].h;
    const RsSlot* sl = d_slots + b.first;
    SFMX_HIP(ctx, hipMemsetAsync(vb->keys.p, 0xFF, px * 8, s));
    SFMX_HIP(ctx, hipMemsetAsync(vb->rcounters.p, 0, (size_t)b.count * RS_NWORDS * 4, s));
    k_rs_project<true><<<dim3(nbv, (unsigned)b.count), 256, 0, s>>>(verts, n, RsCam{}, sl, p->z_min, vb->pv.as<RsVert>(), vb->fl.as<uint8_t>());
    if (m > 0) {
      k_rs_faces<true, VB_SMALL><<<dim3((unsigned)fb, (unsigned)b.count), 256, 0, s>>>(faces, m, n, vb->pv.as<RsVert>(), vb->fl.as<uint8_t>(), 0, 0, 0,
                                                                             vb->keys.as<unsigned long long>(), vb->big.as<int>(),
                                                                             vb->rcounters.as<unsigned>(), nullptr, sl);
      k_rs_big<true><<<dim3(VB_BIG_BLOCKS, (unsigned)b.count), 256, 0, s>>>(faces, m, n, vb->pv.as<RsVert>(), 0, 0,
                                                                            vb->keys.as<unsigned long long>(), vb->big.as<int>(),
                                                                            vb->rcounters.as<unsigned>(), nullptr, sl);
    }
    if (grey)
      k_vb_verts<true><<<nbv, 256, 0, s>>>(verts, normals, n, sl, b.count, vb->pv.as<RsVert>(), vb->fl.as<uint8_t>(),
                                           vb->keys.as<unsigned long long>(), vb->img.as<uint8_t>(), p->depth_tol, p->cull, mask,
                                           vb->vviews.as<int>(), vb->acc.as<int>(), vb->cnt.as<int>(), pair_parts);
    else
      k_vb_verts<false><<<nbv, 256, 0, s>>>(verts, normals, n, sl, b.count, vb->pv.as<RsVert>(), vb->fl.as<uint8_t>(),
                                            vb->keys.as<unsigned long long>(), nullptr, p->depth_tol, 0, mask, vb->vviews.as<int>(),
                                            vb->acc.as<int>(), vb->cnt.as<int>(), pair_parts);
    if (m > 0) k_vb_faces<<<nbf, 256, 0, s>>>(faces, m, n, vb->pv.as<RsVert>(), mask, vb->fviews.as<int>(), vb->fback.as<int>());
  }
  if (m > 0) {
    k_vb_mark<<<nbf, 256, 0, s>>>(faces, m, n, vb->fviews.as<int>(), vb->fback.as<int>(), p->min_views, fkeep, vkeep, words, count_parts);
    sfmx_scan(fkeep, false, m, foff, ax, s);
    sfmx_scan_total(fkeep, false, foff, m, words + VB_NF_OUT, s);
  }
  if (n > 0) {
    sfmx_scan(vkeep, false, n, voff, ax, s);
    sfmx_scan_total(vkeep, false, voff, n, words + VB_NV_OUT, s);
    k_vb_emit_verts<<<nbv, 256, 0, s>>>(n, vkeep, voff, reinterpret_cast<const unsigned long long*>(verts),
                                        reinterpret_cast<const unsigned long long*>(normals), vb->out_v.as<unsigned long long>(),
                                        vb->out_n.as<unsigned long long>(), vb->vsrc.as<int>());
    if (grey) k_vb_grey<<<nbv, 256, 0, s>>>(n, vb->acc.as<int>(), vb->cnt.as<int>(), p->fill, vb->grey.as<uint8_t>());
  }
  if (m > 0 && n > 0) k_vb_emit_faces<<<nbf, 256, 0, s>>>(faces, m, fkeep, foff, voff, vb->out_f.as<int>(), vb->fsrc.as<int>());
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
  vb->nv_out = w[VB_NV_OUT];
  vb->nf_out = w[VB_NF_OUT];
  vb->counts[0] = (int32_t)tot[VB_SEEN];
  vb->counts[1] = (int32_t)tot[VB_BACK_ONLY];
  vb->counts[2] = (int32_t)tot[VB_UNSEEN];
  vb->counts[3] = vb->nf_out;
  vb->counts[4] = vb->nv_out;
  // without a batch (V = 0) every pair count is 0; a view of a run counts every vertex once
  vb->pairs[0] = tot[VB_PAIRS_VISIBLE];
  vb->pairs[1] = tot[VB_PAIRS_OCCLUDED];
  vb->pairs[2] = tot[VB_PAIRS_OFF];
  vb->has_normals = normals != nullptr;
  vb->has_grey = grey;
  vb->last_batch = widest;
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
  for (DevBuf* b : {&vb->img, &vb->d_slots, &vb->keys, &vb->pv, &vb->fl, &vb->big, &vb->rcounters, &vb->work, &vb->res, &vb->in_v, &vb->in_n,
                    &vb->in_f, &vb->out_v, &vb->out_n, &vb->out_f, &vb->vsrc, &vb->fsrc, &vb->fviews, &vb->fback, &vb->vviews, &vb->acc,
                    &vb->cnt, &vb->grey})
    b->release();
  vb->t.destroy();
  delete vb;
}

int sfmx_visib_reset(sfmx_ctx* ctx, sfmx_visib* vb) {
  SFMX_REQUIRE(ctx, ctx && vb);
  vb->views.clear();
  vb->img_off.clear();
  vb->img_used = 0;
  return SFMX_OK;
}

int sfmx_visib_add_stereo_view(sfmx_ctx* ctx, sfmx_visib* vb, const sfmx_fusion_view* view, const sfmx_stereo* st) {
  SFMX_REQUIRE(ctx, ctx && vb && st && view);
  int w = 0, h = 0;
  const uint8_t* im = sfmx_stereo_device_rect_left(st, &w, &h);
  SFMX_REQUIRE(ctx, im && view->w == w && view->h == h);
  return sfmx_visib_add_view(ctx, vb, view, im, 1);
}

int sfmx_visib_add_view(sfmx_ctx* ctx, sfmx_visib* vb, const sfmx_fusion_view* view, const uint8_t* image, int on_device) {
  SFMX_REQUIRE(ctx, ctx && vb && rs_view_ok(view));
  long long off = -1;
  if (image) {
    SFMX_HIP(ctx, hipSetDevice(ctx->device));
    const long long px = (long long)view->w * view->h;
    SFMX_REQUIRE(ctx, vb->img_used + px < (1ll << 40));
    SFMX_HIP(ctx, sfmx_grow_keep(vb->img, (size_t)vb->img_used, (size_t)(vb->img_used + px), ctx->stream));
    SFMX_HIP(ctx, hipMemcpyAsync(vb->img.as<uint8_t>() + vb->img_used, image, (size_t)px,
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    SFMX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may reuse its buffer
    off = vb->img_used;
    vb->img_used += px;
  }
  vb->views.push_back(*view);
  vb->img_off.push_back(off);
  return SFMX_OK;
}

int sfmx_visib_view_count(const sfmx_visib* vb) { return vb ? (int)vb->views.size() : 0; }

int sfmx_visib_set_batch(sfmx_visib* vb, int k) {
  if (!vb || k < 0 || k > VB_MAX_BATCH) return SFMX_ERR_INVALID;
  vb->forced_batch = k;
  return SFMX_OK;
}

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
  hipStream_t s = ctx->stream;
  const size_t vbytes = (size_t)n * 24, fbytes = (size_t)m * 12;
  SFMX_HIP(ctx, vb->in_v.ensure(vbytes));
  SFMX_HIP(ctx, vb->in_f.ensure(fbytes));
  if (n > 0) SFMX_HIP(ctx, hipMemcpyAsync(vb->in_v.p, verts, vbytes, hipMemcpyHostToDevice, s));
  if (m > 0) SFMX_HIP(ctx, hipMemcpyAsync(vb->in_f.p, faces, fbytes, hipMemcpyHostToDevice, s));
  if (normals) {
    SFMX_HIP(ctx, vb->in_n.ensure(vbytes + 8));
    if (n > 0) SFMX_HIP(ctx, hipMemcpyAsync(vb->in_n.p, normals, vbytes, hipMemcpyHostToDevice, s));
  }
  return vb_run(ctx, vb, vb->in_v.as<double>(), normals ? vb->in_n.as<double>() : nullptr, n, vb->in_f.as<int32_t>(), m, p);
}

int sfmx_visib_read(sfmx_ctx* ctx, sfmx_visib* vb, double* verts_out, double* normals_out, int32_t* faces_out, int32_t* vert_src,
                    int32_t* face_src, int32_t* face_views, int32_t* face_back_views, int32_t* vert_views, uint8_t* grey,
                    int32_t* grey_views) {
  SFMX_REQUIRE(ctx, ctx && vb && vb->done);
  SFMX_REQUIRE(ctx, !normals_out || vb->has_normals);
  SFMX_REQUIRE(ctx, (!grey && !grey_views) || vb->has_grey);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t nv = (size_t)vb->nv_out, nf = (size_t)vb->nf_out, n = (size_t)vb->n, m = (size_t)vb->m;
  if (verts_out && nv) SFMX_HIP(ctx, hipMemcpyAsync(verts_out, vb->out_v.p, nv * 24, hipMemcpyDeviceToHost, s));
  if (normals_out && nv) SFMX_HIP(ctx, hipMemcpyAsync(normals_out, vb->out_n.p, nv * 24, hipMemcpyDeviceToHost, s));
  if (faces_out && nf) SFMX_HIP(ctx, hipMemcpyAsync(faces_out, vb->out_f.p, nf * 12, hipMemcpyDeviceToHost, s));
  if (vert_src && nv) SFMX_HIP(ctx, hipMemcpyAsync(vert_src, vb->vsrc.p, nv * 4, hipMemcpyDeviceToHost, s));
  if (face_src && nf) SFMX_HIP(ctx, hipMemcpyAsync(face_src, vb->fsrc.p, nf * 4, hipMemcpyDeviceToHost, s));
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
  if (n_verts_out) *n_verts_out = have ? vb->nv_out : 0;
  if (n_faces_out) *n_faces_out = have ? vb->nf_out : 0;
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
  const bool have = vb && vb->done;
  if (verts) *verts = have ? vb->out_v.as<double>() : nullptr;
  if (faces) *faces = have ? vb->out_f.as<int32_t>() : nullptr;
  if (n_verts) *n_verts = have ? vb->nv_out : 0;
  if (n_faces) *n_faces = have ? vb->nf_out : 0;
  return have ? vb->nv_out : -1;
}

int sfmx_visib_device_surface(const sfmx_visib* vb, const double** verts, const double** normals) {
  const bool have = vb && vb->done;
  if (verts) *verts = have ? vb->out_v.as<double>() : nullptr;
  if (normals) *normals = have && vb->has_normals ? vb->out_n.as<double>() : nullptr;
  return have ? vb->nv_out : -1;
}

double sfmx_visib_last_us(const sfmx_visib* vb) { return vb ? vb->t.us : 0.0; }

int sfmx_visib_last_batch(const sfmx_visib* vb) { return vb && vb->done ? vb->last_batch : 0; }

}  // extern "C"
