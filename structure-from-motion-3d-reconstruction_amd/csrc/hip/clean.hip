// clean.hip — small connected components of an indexed triangle mesh, removed on the device.
//
// Exactness: everything is an integer or a byte copy.  Components are a set partition, the smallest index of a set does not
// depend on the order of the unions, the face counts are integer sums and the output offsets integer scans: any schedule gives
// the same bytes.  tests/clean_ref.py restates it in NumPy; the tests compare bytes.
//
// Kernel layout, one thread per vertex or per face, blocks of 256, all on the context's stream:
//   k_cl_init        lab[v] = v, cf[v] = 0, vkeep[v] = 0
//   k_cl_merge       per face: indices outside [0, n) set the flag (atomicOr) and the face is skipped; otherwise unite (v0, v1)
//                    and (v0, v2).  The union is the speckle filter's (stereo.hip, k_st_uf_*): find both roots, CAS the larger
//                    root onto the smaller, retry when the CAS fails.  A link only ever points to a smaller index, so there is
//                    no cycle; a failed CAS means another thread linked that root, so the loop is lock-free, not a wait.
//                    find halves its path with atomicMin (a label only ever decreases, and only to an ancestor).
//   k_cl_flatten     lab[v] = find(v)
//   k_cl_count       per face: cf[lab[v0]] += 1, as one atomicAdd per wave and distinct root (ballot / popcount)
//   k_cl_stats       per vertex: vcf[v] = cf[lab[v]]; per root with cf > 0 a wave-reduced atomicMax into `largest` and a
//                    ballot / popcount add into `n_components`
//   k_cl_mark        per face: the keep rule on cf[lab[v0]]; a kept face flags its three corners
//   k_scan_*         exclusive int32 scans of the face flags and the vertex flags, one launch per level (scan.hip: no
//                    hand-off between workgroups inside a launch)
//   k_mesh_emit_*    the kept vertices and the renumbered kept faces (sfmx_mesh_dev.h: MeshCompact, shared with visib.hip)
// No kernel waits on another workgroup or spins on a memory word.  A face with an index out of range is skipped by every
// per-face kernel (they all run before the host reads the flag), so nothing is ever accessed through such an index.
#include "sfmx_internal.h"
#include "sfmx_mesh_dev.h"

namespace {

enum { CL_FLAG = 0, CL_LARGEST, CL_NCOMP, CL_NF_OUT, CL_NV_OUT, CL_COUNTERS = 8 };

__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; every second node on the way is re-pointed at its grandparent
__device__ __forceinline__ int cl_find(int* lab, int x) {
  while (true) {
    const int p = cl_load(lab + x);
    if (p == x) return x;
    const int g = cl_load(lab + p);
    if (g == p) return p;
    atomicMin(&lab[x], g);
    x = g;
  }
}

__device__ __forceinline__ void cl_unite(int* lab, int a, int b) {
  while (true) {
    a = cl_find(lab, a);
    b = cl_find(lab, b);
    if (a == b) return;
    const int lo = min(a, b), hi = max(a, b);
    if (atomicCAS(&lab[hi], hi, lo) == hi) return;  // hi was still a root: linked
  }
}

__global__ __launch_bounds__(256) void k_cl_init(int n, int* __restrict__ lab, int* __restrict__ cf, int* __restrict__ vkeep) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  lab[v] = v;
  cf[v] = 0;
  vkeep[v] = 0;
}

__global__ __launch_bounds__(256) void k_cl_merge(const int* __restrict__ faces, int m, int n, int* lab, int* __restrict__ counters) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int v0, v1, v2;
  if (!mesh_face(faces, f, n, v0, v1, v2)) {
    atomicOr(&counters[CL_FLAG], 1);
    return;
  }
  cl_unite(lab, v0, v1);
  cl_unite(lab, v0, v2);
}

__global__ __launch_bounds__(256) void k_cl_flatten(int n, int* lab) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int r = cl_find(lab, v);
  atomicMin(&lab[v], r);
}

__global__ __launch_bounds__(256) void k_cl_count(const int* __restrict__ faces, int m, int n, const int* __restrict__ lab,
                                                  int* __restrict__ cf) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  int v0, v1, v2;
  const int r = f < m && mesh_face(faces, f, n, v0, v1, v2) ? lab[v0] : -1;
  // one atomicAdd per wave and root: nearly every face of a surface belongs to one component, and a million adds on one
  // word are served one after the other.  The loop runs on wave-uniform values; nothing is read from memory inside it.
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(r >= 0);
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const int rl = __shfl(r, leader, 64);
    const unsigned long long same = __ballot(r == rl);
    if (lane == leader) atomicAdd(&cf[rl], __popcll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(256) void k_cl_stats(int n, const int* __restrict__ lab, const int* __restrict__ cf, int* __restrict__ vcf,
                                                  int* __restrict__ counters) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  int c = 0;  // this thread's component size if it is the root of a component with faces, else 0
  if (v < n) {
    const int r = lab[v];
    const int x = cf[r];
    vcf[v] = x;
    if (r == v) c = x;
  }
  const unsigned long long roots = __ballot(c > 0);
  if (roots == 0) return;  // the whole wave
  int mx = c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&counters[CL_LARGEST], mx);
    atomicAdd(&counters[CL_NCOMP], __popcll(roots));
  }
}

__global__ __launch_bounds__(256) void k_cl_mark(const int* __restrict__ faces, int m, int n, const int* __restrict__ lab,
                                                 const int* __restrict__ cf, const int* __restrict__ counters, int min_faces,
                                                 int min_permille, int* __restrict__ fkeep, int* vkeep) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m) return;
  int v0, v1, v2;
  bool keep = false;
  if (mesh_face(faces, f, n, v0, v1, v2)) {
    const int c = cf[lab[v0]];
    keep = c >= 1 && c >= min_faces && (long long)c * 1000 >= (long long)counters[CL_LARGEST] * min_permille;
  }
  fkeep[f] = keep ? 1 : 0;
  if (keep) {
    vkeep[v0] = 1;
    vkeep[v1] = 1;
    vkeep[v2] = 1;
  }
}

}  // namespace

struct sfmx_clean {
  // per input vertex: lab, cf, vcf, vkeep, voff; per input face: fkeep, foff; then the scans' partials and the counters
  DevBuf work;
  MeshInput in;     // host inputs, staged
  MeshCompact out;  // the cleaned mesh
  int *lab = nullptr, *vcf = nullptr;  // into work, of the last successful run
  bool done = false;
  int n = 0, m = 0;
  StageTimer t;
};

namespace {

// verts / normals / faces are device pointers
int cl_run(sfmx_ctx* ctx, sfmx_clean* cl, const double* verts, const double* normals, int n, const int32_t* faces, int m,
           const sfmx_clean_params* p, int* n_verts_out, int* n_faces_out, int* n_components, int* largest) {
  hipStream_t s = ctx->stream;
  cl->done = false;
  cl->t.us = 0.0;
  const size_t nn = (size_t)n, mm = (size_t)m;
  const size_t aux = sfmx_scan_aux(n > m ? n : m);
  SFMX_HIP(ctx, cl->work.ensure((5 * nn + 2 * mm + aux + CL_COUNTERS) * 4));
  SFMX_HIP(ctx, cl->out.ensure(nn, mm, normals != nullptr));
  int* lab = cl->work.as<int>();
  int* cf = lab + nn;
  int* vcf = cf + nn;
  int* vkeep = vcf + nn;
  int* voff = vkeep + nn;
  int* fkeep = voff + nn;
  int* foff = fkeep + mm;
  int* ax = foff + mm;
  int* counters = ax + aux;
  const unsigned nbv = (unsigned)((nn + 255) / 256), nbf = (unsigned)((mm + 255) / 256);
  SFMX_HIP(ctx, cl->t.begin(ctx));
  SFMX_HIP(ctx, hipMemsetAsync(counters, 0, CL_COUNTERS * 4, s));
  if (n > 0) k_cl_init<<<nbv, 256, 0, s>>>(n, lab, cf, vkeep);
  if (m > 0) k_cl_merge<<<nbf, 256, 0, s>>>(faces, m, n, lab, counters);
  if (n > 0) k_cl_flatten<<<nbv, 256, 0, s>>>(n, lab);
  if (m > 0) k_cl_count<<<nbf, 256, 0, s>>>(faces, m, n, lab, cf);
  if (n > 0) k_cl_stats<<<nbv, 256, 0, s>>>(n, lab, cf, vcf, counters);
  if (m > 0) k_cl_mark<<<nbf, 256, 0, s>>>(faces, m, n, lab, cf, counters, p->min_faces, p->min_permille, fkeep, vkeep);
  cl->out.launch(verts, normals, n, faces, m, fkeep, foff, vkeep, voff, ax, counters + CL_NF_OUT, counters + CL_NV_OUT, m > 0, s);
  SFMX_HIP(ctx, hipGetLastError());
  SFMX_HIP(ctx, cl->t.end(ctx));
  int c[CL_COUNTERS] = {};
  SFMX_HIP(ctx, hipMemcpyAsync(c, counters, sizeof c, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  cl->t.collect(ctx);
  SFMX_REQUIRE(ctx, c[CL_FLAG] == 0);  // a face index outside [0, n)
  cl->lab = lab;
  cl->vcf = vcf;
  cl->n = n;
  cl->m = m;
  cl->out.nv_out = c[CL_NV_OUT];
  cl->out.nf_out = c[CL_NF_OUT];
  cl->out.has_normals = normals != nullptr;
  cl->done = true;
  if (n_verts_out) *n_verts_out = cl->out.nv_out;
  if (n_faces_out) *n_faces_out = cl->out.nf_out;
  if (n_components) *n_components = c[CL_NCOMP];
  if (largest) *largest = c[CL_LARGEST];
  return SFMX_OK;
}

void cl_zero(int* a, int* b, int* c, int* d) {
  for (int* q : {a, b, c, d})
    if (q) *q = 0;
}

}  // namespace

extern "C" {

void sfmx_clean_default_params(sfmx_clean_params* p) {
  if (!p) return;
  *p = sfmx_clean_params{};
  p->min_faces = 0;
  p->min_permille = 10;
}

int sfmx_clean_check_params(const sfmx_clean_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  if (p->min_faces < 0 || p->min_permille < 0 || p->min_permille > 1000) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

int sfmx_clean_create(sfmx_ctx* ctx, sfmx_clean** out) {
  SFMX_REQUIRE(ctx, ctx && out);
  *out = nullptr;
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  auto* cl = new sfmx_clean;
  const hipError_t e = cl->t.create();
  if (e != hipSuccess) {
    sfmx_clean_destroy(ctx, cl);
    return sfmx_fail(ctx, SFMX_ERR_HIP, "sfmx_clean_create", e);
  }
  *out = cl;
  return SFMX_OK;
}

void sfmx_clean_destroy(sfmx_ctx* ctx, sfmx_clean* cl) {
  if (!cl) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  cl->work.release();
  cl->in.release();
  cl->out.release();
  cl->t.destroy();
  delete cl;
}

int sfmx_clean_run(sfmx_ctx* ctx, sfmx_clean* cl, const double* verts, const double* normals, int n, const int32_t* faces, int m,
                   int on_device, const sfmx_clean_params* p, int* n_verts_out, int* n_faces_out, int* n_components, int* largest) {
  cl_zero(n_verts_out, n_faces_out, n_components, largest);
  SFMX_REQUIRE(ctx, ctx && cl);
  cl->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, sfmx_clean_check_params(p) == SFMX_OK);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0 && n < (1 << 30) && m < (1 << 30) && (n == 0 || verts) && (m == 0 || faces));
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return cl_run(ctx, cl, verts, normals, n, faces, m, p, n_verts_out, n_faces_out, n_components, largest);
  MeshDev d;
  SFMX_HIP(ctx, cl->in.stage(verts, normals, n, faces, m, ctx->stream, d));
  return cl_run(ctx, cl, d.verts, d.normals, n, d.faces, m, p, n_verts_out, n_faces_out, n_components, largest);
}

int sfmx_clean_fusion(sfmx_ctx* ctx, sfmx_clean* cl, const sfmx_fusion* fu, const sfmx_clean_params* p, int* n_verts_out,
                      int* n_faces_out, int* n_components, int* largest) {
  cl_zero(n_verts_out, n_faces_out, n_components, largest);
  SFMX_REQUIRE(ctx, ctx && cl);
  cl->done = false;  // every failure from here on leaves no result behind
  SFMX_REQUIRE(ctx, fu && sfmx_clean_check_params(p) == SFMX_OK);
  const double *v = nullptr, *nr = nullptr;
  const int32_t* f = nullptr;
  int m = 0;
  const int n = sfmx_fusion_device_mesh(fu, &v, &nr, &f, &m);
  SFMX_REQUIRE(ctx, n >= 0 && m >= 0);  // no current surface on the device
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  return cl_run(ctx, cl, v, nr, n, f, m, p, n_verts_out, n_faces_out, n_components, largest);
}

int sfmx_clean_read(sfmx_ctx* ctx, sfmx_clean* cl, double* verts_out, double* normals_out, int32_t* faces_out, int32_t* vert_src,
                    int32_t* face_src, int32_t* vert_label, int32_t* vert_comp_faces) {
  SFMX_REQUIRE(ctx, ctx && cl && cl->done);
  SFMX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t n = (size_t)cl->n;
  SFMX_HIP(ctx, cl->out.read(verts_out, normals_out, faces_out, vert_src, face_src, s));
  if (vert_label && n) SFMX_HIP(ctx, hipMemcpyAsync(vert_label, cl->lab, n * 4, hipMemcpyDeviceToHost, s));
  if (vert_comp_faces && n) SFMX_HIP(ctx, hipMemcpyAsync(vert_comp_faces, cl->vcf, n * 4, hipMemcpyDeviceToHost, s));
  SFMX_HIP(ctx, hipStreamSynchronize(s));
  return SFMX_OK;
}

int sfmx_clean_sizes(const sfmx_clean* cl, int* n, int* m, int* n_verts_out, int* n_faces_out) {
  cl_zero(n, m, n_verts_out, n_faces_out);
  if (!cl || !cl->done) return SFMX_ERR_INVALID;
  if (n) *n = cl->n;
  if (m) *m = cl->m;
  if (n_verts_out) *n_verts_out = cl->out.nv_out;
  if (n_faces_out) *n_faces_out = cl->out.nf_out;
  return SFMX_OK;
}

int sfmx_clean_device_surface(const sfmx_clean* cl, const double** verts, const double** normals) {
  return MeshCompact::device_surface(cl && cl->done ? &cl->out : nullptr, verts, normals);
}

double sfmx_clean_last_us(const sfmx_clean* cl) { return cl ? cl->t.us : 0.0; }

}  // extern "C"

int sfmx_clean_device_mesh(const sfmx_clean* cl, const double** verts, const int32_t** faces, int* n_faces) {
  return MeshCompact::device_mesh(cl && cl->done ? &cl->out : nullptr, verts, faces, nullptr, n_faces);
}
