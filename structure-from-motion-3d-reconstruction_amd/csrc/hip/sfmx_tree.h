// sfmx_tree.h — the fixed summation tree of DESIGN.md 19, shared by align.hip (rows of 28) and register.hip (rows of 37).
// A block of 256 threads sums one value per thread: the thread (lane, wave) sits at TREE INDEX t = 4 lane + wave, the halving tree
// over t (offsets 128 .. 4) is __shfl_xor over the lane (offsets 32 .. 1), and its last two levels (offsets 2 and 1) combine the
// four waves' partials: (p0 + p2) + (p1 + p3).  No floating-point atomics; no workgroup waits on another inside a launch.
#pragma once
#include <hip/hip_runtime.h>

// sum of v over the 64 lanes: the tree levels with offsets 128 .. 4 (t = 4 lane + wave); every lane gets the result
__device__ __forceinline__ double al_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// the last two levels (offsets 2 and 1) over the four waves' partials of one term
__device__ __forceinline__ double al_cross(const double* q) { return (q[0] + q[2]) + (q[1] + q[3]); }

// one level of the tree over rows of TERMS: group = blockIdx.x takes rows [256 group, 256 group + 256), missing rows are +0.0
template <int TERMS> __global__ __launch_bounds__(256) void k_al_tree(const double* __restrict__ in, int rows, double* __restrict__ out) {
  __shared__ double part[TERMS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * 256 + (4 * lane + wave);
  const bool have = r < (long long)rows;
#pragma unroll 4
  for (int t = 0; t < TERMS; t++) {
    const double v = al_wave_sum(have ? in[(size_t)r * TERMS + t] : 0.0);
    if (lane == 0) part[t][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < TERMS) out[(size_t)blockIdx.x * TERMS + threadIdx.x] = al_cross(part[threadIdx.x]);
}
