// sfmx_tsdf.h - the TSDF volume as the device kernels read it: the grid, s(g) = sum / count and "defined"  and
// the gradient G of s.  Shared by fusion.hip (extraction, normals) and raycast.hip (rendering), so that both
// evaluate the same expressions.
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

}  // namespace
