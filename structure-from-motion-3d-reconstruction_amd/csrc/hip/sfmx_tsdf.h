// sfmx_tsdf.h - the TSDF volume as the device kernels read it: the grid, s(g) = sum / count and "defined"  and
// the gradient G of s, and their trilinear interpolation inside a cell.  Shared by fusion.hip
// (extraction, normals), raycast.hip (rendering) and align.hip (registration), so that all evaluate the same expressions.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct FuGrid {
  double ox, oy, oz, vs;
  int nx, ny, nz;
  int minw;
};

__device__ __forceinline__ bool fu_value(const double* __restrict__ sum, const int* __restrict__ cnt, size_t L, int minw, double& s) {
  const int c = cnt[L];
  s = sum[L] / (double)c;
  return c >= minw;
}

// one axis of the gradient at a defined grid point with value s: central where both neighbours are defined, one-sided where
// one is, 0 where neither (a neighbour outside the grid is undefined)
__device__ __forceinline__ double fu_grad_axis(const double* __restrict__ sum, const int* __restrict__ cnt, int minw, double s, size_t L,
                                               size_t stride, bool in_p, bool in_m) {
  double sp = 0.0, sm = 0.0;
  const bool dp = in_p && fu_value(sum, cnt, L + stride, minw, sp);
  const bool dm = in_m && fu_value(sum, cnt, L - stride, minw, sm);
  return dp && dm ? (sp - sm) * 0.5 : dp ? sp - s : dm ? s - sm : 0.0;
}

__device__ __forceinline__ void fu_grad(const double* __restrict__ sum, const int* __restrict__ cnt, const FuGrid& g, int i, int j, int k,
                                        size_t L, double s, double& G0, double& G1, double& G2) {
  const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
  G0 = fu_grad_axis(sum, cnt, g.minw, s, L, 1, i + 1 < g.nx, i > 0);
  G1 = fu_grad_axis(sum, cnt, g.minw, s, L, sy, j + 1 < g.ny, j > 0);
  G2 = fu_grad_axis(sum, cnt, g.minw, s, L, sz, k + 1 < g.nz, k > 0);
}

__device__ __forceinline__ double fu_lerp(double p, double q, double t) { return p + t * (q - p); }

// trilinear interpolation of the 8 corner values of a cell (corner b = bx + 2 by + 4 bz) at the fractions (fx, fy, fz):
// along x, then y, then z
__device__ __forceinline__ double fu_trilerp(const double* s, double fx, double fy, double fz) {
  const double c00 = fu_lerp(s[0], s[1], fx), c10 = fu_lerp(s[2], s[3], fx);
  const double c01 = fu_lerp(s[4], s[5], fx), c11 = fu_lerp(s[6], s[7], fx);
  return fu_lerp(fu_lerp(c00, c10, fy), fu_lerp(c01, c11, fy), fz);
}

// the gradient interpolated the same way in the cell (i, j, k) (lower corner L), whose 8 corners are all defined
__device__ __forceinline__ void fu_grad_trilerp(const double* __restrict__ sum, const int* __restrict__ cnt, const FuGrid& g, int i, int j,
                                                int k, size_t L, double fx, double fy, double fz, double* N) {
  const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
  double cy[2][3];  // after the lerps along x and y, per z
#pragma unroll
  for (int bz = 0; bz < 2; bz++) {
    double cx[2][3];
#pragma unroll
    for (int by = 0; by < 2; by++) {
      double G[2][3];
#pragma unroll
      for (int bx = 0; bx < 2; bx++) {
        const size_t Lq = L + bx + by * sy + bz * sz;
        double sq;
        (void)fu_value(sum, cnt, Lq, g.minw, sq);
        fu_grad(sum, cnt, g, i + bx, j + by, k + bz, Lq, sq, G[bx][0], G[bx][1], G[bx][2]);
      }
#pragma unroll
      for (int a = 0; a < 3; a++) cx[by][a] = fu_lerp(G[0][a], G[1][a], fx);
    }
#pragma unroll
    for (int a = 0; a < 3; a++) cy[bz][a] = fu_lerp(cx[0][a], cx[1][a], fy);
  }
#pragma unroll
  for (int a = 0; a < 3; a++) N[a] = fu_lerp(cy[0][a], cy[1][a], fz);
}

}  // namespace
