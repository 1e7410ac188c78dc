// sfmx_internal.h — context, buffers and error plumbing behind include/sfmx.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../../include/sfmx.h"
#include "sfmx_math.h"

#define SFMX_MAX_LEVELS 8

// Grow-only device / pinned slabs.  Growing never frees: hipFree / hipHostFree wait for EVERY stream of the device, and a
// lane that waits there while another lane's RCCL collective is in flight (blocked on a peer whose own lane waits the same way)
// is a deadlock across ranks.  The outgrown block is parked and released with the buffer (growth is geometric, so the parked
// blocks add up to less than four times the final size).
#include <vector>
template <class Mem> struct Slab {
  void* p = nullptr;
  size_t cap = 0;
  std::vector<void*> parked;
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) parked.push_back(p);
    p = nullptr;
    cap = 0;
    size_t want = n < 4096 ? 4096 : n + n / 4;
    hipError_t e = Mem::alloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)Mem::free(p);
    for (void* q : parked) (void)Mem::free(q);
    parked.clear();
    p = nullptr;
    cap = 0;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};
struct DevMem {
  static hipError_t alloc(void** p, size_t n) { return hipMalloc(p, n); }
  static hipError_t free(void* p) { return hipFree(p); }
};
// Pinned host memory that kernels read and write directly (track positions, BA poses, polled result blocks): fine-grained
// coherent and mapped, requested explicitly rather than through the runtime's default for flags == 0.
struct PinMem {
  static hipError_t alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocCoherent | hipHostMallocMapped); }
  static hipError_t free(void* p) { return hipHostFree(p); }
};
using DevBuf = Slab<DevMem>;
using PinBuf = Slab<PinMem>;

// room for `bytes` in a device slab that already holds `used` bytes: a grown slab gets the old contents on stream s (the old
// block is parked, not freed, so it is still there to copy from)
static inline hipError_t sfmx_grow_keep(DevBuf& b, size_t used, size_t bytes, hipStream_t s) {
  if (bytes <= b.cap) return hipSuccess;
  const void* old = b.p;
  hipError_t e = b.ensure(bytes + bytes / 2);
  if (e == hipSuccess && old && used) e = hipMemcpyAsync(b.p, old, used, hipMemcpyDeviceToDevice, s);
  return e;
}

// per-kernel profile (only while ctx->timing): accumulated GPU time and launch count of the hot kernels, measured
// with HIP events recorded on the context's own stream around each launch
enum SfmxKid {
  KID_KLT = 0, KID_HYPOTHESES, KID_SCORE, KID_BA_POINTS, KID_BA_EXPAND, KID_BA_REDUCE, KID_SOLVE, KID_SHI_SCORE, KID_SHI_FIXPOINT,
  KID_PYRAMID, KID_COUNT
};
#define SFMX_PROF_PAIRS 12

struct sfmx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;  // speculative D2H that must not delay the compute stream
  int stream_prio = 0;                // HIP priority both streams are created with (sfmx_ctx_create_stream)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timing = false;
  double last_us = 0.0;
  hipEvent_t pev[SFMX_PROF_PAIRS][2] = {};
  int prof_kid[SFMX_PROF_PAIRS] = {};
  int prof_n = 0;
  bool prof_open = false;
  double kus[KID_COUNT] = {};
  unsigned long long kcalls[KID_COUNT] = {};
  std::string err;
  // reusable staging: a few independent device / pinned slabs
  DevBuf d[8];
  PinBuf h[5];
  unsigned long long klt_slow_steps = 0;  // lk_steps of the last sfmx_klt_track call that took the per-pixel path
  int resident_points = 0;  // #correspondences left in d[0]/d[1] by the last RANSAC call
  int shi_full_count = 0;   // #candidate scores left in d[6] by the last pruned Shi-Tomasi call
  bool shi_keys_in_flight = false;
  unsigned long long ba_seq = 0;      // sequence number of the last BA step result published into pinned memory
  bool ba_upload_in_flight = false;  // sfmx_ba_reset's transfer out of h[4] has not been waited for yet
  DevBuf wl[4];             // Shi-Tomasi work lists (2), sweep counters, disc offset table
  int wl_md = 0, wl_ntaps = 0;
};

struct sfmx_comm {
  void* nccl = nullptr;  // ncclComm_t; null when world == 1
  int rank = 0, world = 1, device = 0;
};
// comm.hip: in-place all-reduce of device memory on the context's stream (dtype 0 = f64, 1 = u64; op 0 = sum, 1 = max)
int sfmx_comm_allreduce_dev(sfmx_ctx* ctx, sfmx_comm* comm, void* dev, size_t count, int dtype, int op);

struct sfmx_pyramid {
  int w = 0, h = 0, levels = 0;
  uint8_t* base = nullptr;
  size_t off[SFMX_MAX_LEVELS] = {0};
  int lw[SFMX_MAX_LEVELS] = {0}, lh[SFMX_MAX_LEVELS] = {0};
  size_t bytes = 0;
  // sfmx_pyramid_set_device_async: built on the context's second stream; `ready` orders later users behind it
  hipEvent_t ready = nullptr;
  bool ready_pending = false;
  int fetched_level = -1;     // level whose pixels were copied to `fetched` (pinned host memory) by the same call
  PinBuf fetched;
};

// by-value kernel argument describing one pyramid
struct PyrDesc {
  const uint8_t* px[SFMX_MAX_LEVELS];
  int w[SFMX_MAX_LEVELS];
  int h[SFMX_MAX_LEVELS];
  int levels;
};
static inline PyrDesc make_desc(const sfmx_pyramid* p) {
  PyrDesc d;
  for (int l = 0; l < SFMX_MAX_LEVELS; l++) {
    d.px[l] = (l < p->levels) ? p->base + p->off[l] : nullptr;
    d.w[l] = (l < p->levels) ? p->lw[l] : 0;
    d.h[l] = (l < p->levels) ? p->lh[l] : 0;
  }
  d.levels = p->levels;
  return d;
}

int sfmx_fail(sfmx_ctx* ctx, int status, const char* what, hipError_t e);
int sfmx_pyramid_settle(sfmx_ctx* ctx, const sfmx_pyramid* pyr);  // image.hip: order the main stream behind an asynchronous build
extern "C" void sfmx_release_graphs(sfmx_ctx* ctx);  // image.hip: drop the hipGraph executables cached for this context
const int16_t* sfmx_stereo_device_disp16(const sfmx_stereo* st, int* w, int* h);  // stereo.hip: the last disparity map on the device
const uint8_t* sfmx_stereo_device_rect_left(const sfmx_stereo* st, int* w, int* h);  // stereo.hip: the last left rectified image, u8 [h][w]
// fusion.hip: vertices and normals (double [n][3] each) of the last sfmx_fusion_extract_normals on the device; returns n, or -1
// when there is none (never extracted, or the volume or the vertex buffer has changed since)
int sfmx_fusion_device_surface(const sfmx_fusion* fu, const double** verts, const double** normals);
// fusion.hip: the surface the last extraction with arrays left on the device (verts double [n][3], faces int32 [*n_faces][3],
// normals double [n][3] or NULL when that extraction made none); returns n, or -1 when there is none (never extracted, or the
// volume has changed since)
int sfmx_fusion_device_mesh(const sfmx_fusion* fu, const double** verts, const double** normals, const int32_t** faces, int* n_faces);
// fusion.hip: the integrated volume on the device (sum double / count int32 [nz][ny][nx]) and the parameters it was created
// with; returns the number of grid points, or -1 while views are pending (integrate first)
int sfmx_fusion_device_volume(const sfmx_fusion* fu, const double** sum, const int32_t** count, sfmx_fusion_params* p);
// fusion.hip: integrates the pending views, then hands out the volume for writing (sum double / count int32 [nz][ny][nx]) with
// the parameters it was created with; the surface cached on the device is dropped, as sfmx_fusion_reset drops it.  With sum or
// count NULL only *p is filled and the object is not touched (a caller checks the grid before it takes the arrays).
int sfmx_fusion_mutable_volume(sfmx_ctx* ctx, sfmx_fusion* fu, double** sum, int32_t** count, sfmx_fusion_params* p);
// carve.hip: the hull of the last successful run on the device (hull double / views int32 [nz][ny][nx]), its grid and the
// min_views that defines a point; returns the number of grid points, or -1 before a successful run
int sfmx_carve_device_volume(const sfmx_carve* cv, const double** hull, const int32_t** views, sfmx_carve_volume* vol, int* min_views);
// clean.hip: the cleaned mesh of the last successful run on the device (verts double [n'][3], faces int32 [*n_faces][3]);
// returns n', or -1 before a successful run
int sfmx_clean_device_mesh(const sfmx_clean* cl, const double** verts, const int32_t** faces, int* n_faces);
// sdist.hip: the target copy the object holds (verts double [nv][3], faces int32 [*n_faces][3]) and where the last query with
// n > 0 left its results on the device (d2 double [n], face int32 [n]); any pointer may be NULL.  Returns nv, or -1 without a
// target.  Valid until the next set_target / query on sd.
int sfmx_sdist_device_state(const sfmx_sdist* sd, const double** verts, const int32_t** faces, int* n_faces, const double** d2,
                            const int32_t** face);
// consist.hip: view i as it was added and its filtered map on the device; false without a current result or with i out of range
bool sfmx_consist_device_view(const sfmx_consist* cs, int i, sfmx_fusion_view* view, const int16_t** filtered);

#define SFMX_HIP(ctx, call)                                                         \
  do {                                                                              \
    hipError_t e__ = (call);                                                        \
    if (e__ != hipSuccess) return sfmx_fail((ctx), SFMX_ERR_HIP, #call, e__);       \
  } while (0)

#define SFMX_REQUIRE(ctx, cond)                                                     \
  do {                                                                              \
    if (!(cond)) return sfmx_fail((ctx), SFMX_ERR_INVALID, #cond, hipSuccess);      \
  } while (0)

static inline void prof_begin(sfmx_ctx* c, int kid) {
  c->prof_open = false;
  if (!c->timing || c->prof_n >= SFMX_PROF_PAIRS) return;
  hipEvent_t* e = c->pev[c->prof_n];
  if (!e[0] && (hipEventCreate(&e[0]) != hipSuccess || hipEventCreate(&e[1]) != hipSuccess)) return;
  if (hipEventRecord(e[0], c->stream) != hipSuccess) return;
  c->prof_kid[c->prof_n] = kid;
  c->prof_open = true;
}
static inline void prof_end(sfmx_ctx* c) {
  if (!c->prof_open) return;
  c->prof_open = false;
  if (hipEventRecord(c->pev[c->prof_n][1], c->stream) == hipSuccess) c->prof_n++;
}
static inline void prof_collect(sfmx_ctx* c) {  // after the stream has been synchronised
  for (int i = 0; i < c->prof_n; i++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->pev[i][0], c->pev[i][1]) == hipSuccess) {
      c->kus[c->prof_kid[i]] += (double)ms * 1000.0;
      c->kcalls[c->prof_kid[i]]++;
    }
  }
  c->prof_n = 0;
}
// SFMX_PROF(ctx, KID_x, kernel<<<...>>>(...));
#define SFMX_PROF(ctx, kid, launch) \
  do {                              \
    prof_begin((ctx), (kid));       \
    launch;                         \
    prof_end((ctx));                \
  } while (0)

// event timing of the dominant kernel of an API call (only when ctx->timing)
struct KernelTimer {
  sfmx_ctx* c;
  explicit KernelTimer(sfmx_ctx* ctx) : c(ctx) {}
  void start() {
    if (c->timing) (void)hipEventRecord(c->ev0, c->stream);
  }
  void stop() {
    if (c->timing) (void)hipEventRecord(c->ev1, c->stream);
  }
  void collect() {  // call after the stream has been synchronised
    if (c->timing) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->last_us = (double)ms * 1000.0;
      prof_collect(c);
    }
  }
};

// event timing of one stage object's launches (sfmx_*_last_us).  The owner zeroes `us` itself: where its call starts, except
// sfmx_stereo_disparity, which does so after its last synchronise (a failed call keeps the earlier value).  The events are
// recorded only while ctx->timing, and `us` is set after the stream has been synchronised, only if the query succeeds.
struct StageTimer {
  hipEvent_t ev[2] = {};
  double us = 0.0;
  hipError_t create() {
    hipError_t e = hipEventCreate(&ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&ev[1]);
    return e;
  }
  void destroy() {
    for (hipEvent_t& e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
  hipError_t begin(const sfmx_ctx* c) { return c->timing ? hipEventRecord(ev[0], c->stream) : hipSuccess; }
  hipError_t end(const sfmx_ctx* c) { return c->timing ? hipEventRecord(ev[1], c->stream) : hipSuccess; }
  void collect(const sfmx_ctx* c) {  // call after the stream has been synchronised
    float ms = 0.f;
    if (c->timing && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) us = (double)ms * 1000.0;
  }
};

// scan.hip: exclusive int32 scan of in[0..n), n >= 1, into out (in may equal out), or with popc of the popcounts of in.  One
// launch per level; aux holds the block sums of every level, sfmx_scan_aux(n) ints.  sfmx_scan_total stores
// out[n - 1] + value(in[n - 1]), the sum of all n, into *total (device memory) with one more launch.
size_t sfmx_scan_aux(int n);
void sfmx_scan(const int* in, bool popc, int n, int* out, int* aux, hipStream_t s);
void sfmx_scan_total(const int* in, bool popc, const int* out, int n, int* total, hipStream_t s);

// The sums of K integers over a block of 256 threads: thread j < K returns the block's sum of v[j] (the other threads that of
// v[0]).  Every thread of the block calls it; a kernel that calls it twice puts a __syncthreads() between the calls, since both
// use the same LDS.
template <class T, int K> __device__ __forceinline__ T sfmx_block_sums(T (&v)[K]) {
  __shared__ T sh[4][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) sh[wave][k] = v[k];
  }
  __syncthreads();
  const int j = threadIdx.x < K ? threadIdx.x : 0;
  return (sh[0][j] + sh[1][j]) + (sh[2][j] + sh[3][j]);
}
