// sfmx_view.h - the rectified view as the device kernels read it: the camera and where its int16 map lies in a stage's slab,
// the projection of a world point onto its nearest pixel, the depth the map holds there, and the lift of a pixel back to its
// 3-D point.  Shared by fusion.hip (integration), shade.hip (visibility) and consist.hip (filtering), so that
// all three evaluate the same expressions in the same order: maps filtered under consist's projection are integrated under
// fusion's (sfmx_fusion_add_consist_view), which only means something if the two are one.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../../include/sfmx.h"

namespace {

struct DevView {
  double R[9], c[3], f, cx, cy, fB;
  long long off;  // first element of the view in the stage's slab(s)
  int w, h;
};

// what every stage that keeps views accepts
inline bool sfmx_view_ok(const sfmx_fusion_view* v) {
  if (!v || v->w <= 0 || v->h <= 0 || v->w > 4096 || (long long)v->w * v->h >= (1ll << 30)) return false;
  for (double x : v->R_rw)
    if (!std::isfinite(x)) return false;
  for (double x : v->c_left)
    if (!std::isfinite(x)) return false;
  return std::isfinite(v->f) && std::isfinite(v->cx) && std::isfinite(v->cy) && std::isfinite(v->B);
}

inline DevView sfmx_dev_view(const sfmx_fusion_view* v, long long off) {
  DevView d{};
  std::memcpy(d.R, v->R_rw, sizeof d.R);
  std::memcpy(d.c, v->c_left, sizeof d.c);
  d.f = v->f;
  d.cx = v->cx;
  d.cy = v->cy;
  d.fB = v->f * v->B;
  d.off = off;
  d.w = v->w;
  d.h = v->h;
  return d;
}

// camera-frame depth of the world point X; p = X - c comes back too (the projection goes on from it)
__device__ __forceinline__ double dv_depth(const DevView& V, double X0, double X1, double X2, double& p0, double& p1, double& p2) {
  p0 = X0 - V.c[0];
  p1 = X1 - V.c[1];
  p2 = X2 - V.c[2];
  return (V.R[6] * p0 + V.R[7] * p1) + V.R[8] * p2;
}

// image position of the point with offset p and depth q2 > 0
__device__ __forceinline__ void dv_project(const DevView& V, double p0, double p1, double p2, double q2, double& u, double& v) {
  const double q0 = (V.R[0] * p0 + V.R[1] * p1) + V.R[2] * p2;
  const double q1 = (V.R[3] * p0 + V.R[4] * p1) + V.R[5] * p2;
  u = (V.f * q0) / q2 + V.cx;
  v = (V.f * q1) / q2 + V.cy;
}

// its nearest pixel, kept as doubles; false outside the image
__device__ __forceinline__ bool dv_pixel(const DevView& V, double p0, double p1, double p2, double q2, double& x, double& y) {
  double u, v;
  dv_project(V, p0, p1, p2, q2, u, v);
  x = floor(u + 0.5);
  y = floor(v + 0.5);
  return x >= 0.0 && x < (double)V.w && y >= 0.0 && y < (double)V.h;
}

// pixel (x, y) of the view in a slab
__device__ __forceinline__ long long dv_index(const DevView& V, double x, double y) { return V.off + (long long)(int)y * V.w + (int)x; }

// a disparity d (1 / 16 px) counts unless it is the invalid mark or below disp_min
__device__ __forceinline__ bool dv_disp_ok(int d, double disp_min) { return d != -16 && (double)d / 16.0 >= disp_min; }

// the depth it stands for
__device__ __forceinline__ double dv_disp_depth(const DevView& V, int d) { return V.fB / ((double)d / 16.0); }

// the world point of pixel (x, y) at depth Z
__device__ __forceinline__ void dv_lift(const DevView& V, double x, double y, double Z, double& X0, double& X1, double& X2) {
  const double l0 = ((x - V.cx) * Z) / V.f, l1 = ((y - V.cy) * Z) / V.f;
  X0 = V.c[0] + ((V.R[0] * l0 + V.R[3] * l1) + V.R[6] * Z);
  X1 = V.c[1] + ((V.R[1] * l0 + V.R[4] * l1) + V.R[7] * Z);
  X2 = V.c[2] + ((V.R[2] * l0 + V.R[5] * l1) + V.R[8] * Z);
}

}  // namespace
