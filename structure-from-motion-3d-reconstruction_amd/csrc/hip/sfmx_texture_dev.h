// sfmx_texture_dev.h — the texture object of texture.hip as the stages that build on its last run see it
// (level.hip): the layout, the views as they were uploaded, the images and the per-face arrays on the device; and
// the one bilinear sample and the one atlas bake that both stages use, so that levelling adds its offsets to exactly the grey
// value the texture was rounded from.
#pragma once
#include <vector>

#include "sfmx_internal.h"
#include "sfmx_mesh_dev.h"
#include "sfmx_raster_dev.h"

struct TxLayout {
  int S, C, cells, n_tex, fill_cell, W, H, fill;  // fill_cell: its index, or -1 without one
};

struct sfmx_texture {
  RsViewSet vs;                             // the cameras, their images and one batch's z-buffers
  DevBuf work;                              // masks, flags, ranks, the list, the scan's partials
  DevBuf res;                               // the words
  MeshInput in;                             // host inputs, staged
  DevBuf fview, farea, uvh, vfaces, atlas;  // the result
  const int* list = nullptr;                // into work, of the last successful run: rank -> face, int32 [n_tex]
  bool done = false;
  int n = 0, m = 0, nviews = 0;
  int32_t counts[6] = {};
  TxLayout lay{};    // of the last successful run
  StageTimer t, tb;  // the whole run, k_tx_bake alone
};

namespace {

constexpr int TX_GROUP = 16;  // cells per block of the bake
constexpr int TX_REC = 26;    // eight-byte words per half cell in LDS

static_assert(sizeof(RsCam) == 16 * 8 && sizeof(RsSlot) == 18 * 8, "tx_bake copies a slot as eight-byte words");

// DESIGN.md 25's bilinear g (not rounded) of a camera, whose image lies at img + off, at the point X; ok is false where the
// texel would be `fill`.  Returned by value: as an out-parameter it costs the bake two more VGPRs.
struct TxSample {
  bool ok;
  double g;
};
__device__ __forceinline__ TxSample tx_sample(const RsCam& cam, const long long& off, const uint8_t* __restrict__ img, double X0, double X1,
                                              double X2) {
  const double* R = cam.R;
  const double p0 = X0 - cam.c[0], p1 = X1 - cam.c[1], p2 = X2 - cam.c[2];
  const double q0 = (R[0] * p0 + R[1] * p1) + R[2] * p2;
  const double q1 = (R[3] * p0 + R[4] * p1) + R[5] * p2;
  const double q2 = (R[6] * p0 + R[7] * p1) + R[8] * p2;
  const double u = (cam.f * q0) / q2 + cam.cx, v = (cam.f * q1) / q2 + cam.cy;
  if (!(q2 > 0.0 && isfinite(u) && isfinite(v))) return {false, 0.0};
  const int w = cam.w, h = cam.h;
  const double uc = fmin(fmax(u, -1.0), (double)w), vc = fmin(fmax(v, -1.0), (double)h);
  const double x0 = floor(uc), y0 = floor(vc);
  const double ax = uc - x0, ay = vc - y0;
  const int xi0 = min(max((int)x0, 0), w - 1), xi1 = min(max((int)x0 + 1, 0), w - 1);
  const int yi0 = min(max((int)y0, 0), h - 1), yi1 = min(max((int)y0 + 1, 0), h - 1);
  const uint8_t* I0 = img + off + (long long)yi0 * w;
  const uint8_t* I1 = img + off + (long long)yi1 * w;
  const double top = (1.0 - ax) * (double)I0[xi0] + ax * (double)I0[xi1];
  const double bot = (1.0 - ax) * (double)I1[xi0] + ax * (double)I1[xi1];
  return {true, (1.0 - ay) * top + ay * bot};
}

// The body of k_tx_bake (LEVEL = false) and k_lv_bake (LEVEL = true): one block per group of TX_GROUP cells of one cell row.
// The block first stages, per half cell, the face's nine doubles and its view's camera, image offset and size in LDS (TX_REC
// eight-byte words, loaded by as many threads each once; with LEVEL three more int32, the corners' offsets from cadj), then
// walks the group's texels row by row, thread t on texel t, t + 256, ...: a wave stores 64 neighbouring bytes of one atlas row.
// Every texel of the atlas is written exactly once, `fill` included (also the cells of a partial last row).  The two differ in
// the one rounding: LEVEL adds the barycentric blend of the three offsets before it.
template <bool LEVEL>
__device__ __forceinline__ void tx_bake(const double* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ list,
                                        const int* __restrict__ fview, const int* __restrict__ cadj, const RsSlot* __restrict__ slots,
                                        const uint8_t* __restrict__ img, const TxLayout& lay, uint8_t* __restrict__ atlas) {
  __shared__ double rec[2 * TX_GROUP][TX_REC];  // X a, b, c (9), the camera (16 words), the image's offset
  __shared__ int idx[2 * TX_GROUP][4];          // the face's corners and its view, -1: a half without a face
  __shared__ int adj[2 * TX_GROUP][4];          // LEVEL: the corners' offsets
  const int S = lay.S, L = S - 2, row = blockIdx.x, g0 = blockIdx.y * TX_GROUP;
  const int gc = min(TX_GROUP, lay.C - g0);  // cells of this group
  if (threadIdx.x < 2 * TX_GROUP) {
    const int hl = threadIdx.x, c = row * lay.C + g0 + (hl >> 1);
    const long long r = 2ll * c + (hl & 1);
    int v = -1, a = 0, b = 0, cc = 0, ga = 0, gb = 0, gcc = 0;
    if ((hl >> 1) < gc && c < lay.cells && c != lay.fill_cell && r < lay.n_tex) {
      const int f = list[r];
      v = fview[f];
      a = faces[3 * (size_t)f];  // a textured face has passed the range check
      b = faces[3 * (size_t)f + 1];
      cc = faces[3 * (size_t)f + 2];
      if (LEVEL) {
        ga = cadj[3 * (size_t)f];
        gb = cadj[3 * (size_t)f + 1];
        gcc = cadj[3 * (size_t)f + 2];
      }
    }
    idx[hl][0] = a;
    idx[hl][1] = b;
    idx[hl][2] = cc;
    idx[hl][3] = v;
    if (LEVEL) {
      adj[hl][0] = ga;
      adj[hl][1] = gb;
      adj[hl][2] = gcc;
    }
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
      const TxSample sm = tx_sample(*reinterpret_cast<const RsCam*>(r + 9), *reinterpret_cast<const long long*>(r + 25), img, X0, X1, X2);
      if (sm.ok) {
        if (LEVEL) {
          const long long N = ((long long)(L - i2 - j2) * adj[hl][0] + (long long)i2 * adj[hl][1]) + (long long)j2 * adj[hl][2];
          out = (int)fmin(255.0, fmax(0.0, floor((sm.g + (double)N / (double)(256 * L)) + 0.5)));
        } else {
          out = (int)fmin(255.0, floor(sm.g + 0.5));
        }
      }
    }
    atlas[base + (size_t)ly * lay.W + x] = (uint8_t)out;
  }
}

}  // namespace
