// scan.hip — the exclusive int32 scan of the surface stages: fusion's triangle counts and slot popcounts,
// clean's keep flags, sdist's cell and work-item counts.
//
// One launch per level and no hand-off between workgroups inside a launch: k_scan_local scans 1 024-element chunks and leaves
// one sum per chunk, the sums are scanned the same way (recursively, a third level from 1 024^2 + 1 elements on), and
// k_scan_add adds each chunk's offset.  Everything is an integer, so the result does not depend on the schedule.
//
// A file of its own rather than a header: the stages need the three entry points, not the kernels, and one object holds the
// one copy of them (a header would compile the same kernels, under the same names, into three objects).
#include "sfmx_internal.h"

namespace {

// exclusive scan of one 1024-element chunk per block (4 per thread); POPC: scan popcount(in) instead of in.
// in may equal out (every element is read before its block writes).
template <bool POPC>
__global__ __launch_bounds__(256) void k_scan_local(const int* in, int n, int* out, int* __restrict__ bsum) {
  __shared__ int wsum[4];
  const int base = blockIdx.x * 1024 + threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int q = 0; q < 4; q++) v[q] = base + q < n ? in[base + q] : 0;
  if (POPC) {
    // The empty statements keep the popcounts behind all four loads.  Without them the compiler moves each one into its
    // load's bounds branch, with a wait of its own, and the loads go out one at a time: the 256^3 extraction is slower
    // than with the run-time flag this parameter replaces (profiles/surface_shared_ab.json, `plain_popc_scan`).
#pragma unroll
    for (int q = 0; q < 4; q++) asm volatile("" : "+v"(v[q]));
#pragma unroll
    for (int q = 0; q < 4; q++) v[q] = __popc((unsigned)v[q]);
  }
  const int tsum = v[0] + v[1] + v[2] + v[3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = tsum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int pre = incl - tsum;
  for (int w = 0; w < wave; w++) pre += wsum[w];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    if (base + q < n) out[base + q] = pre;
    pre += v[q];
  }
  if (threadIdx.x == 255) bsum[blockIdx.x] = pre;
}

__global__ __launch_bounds__(256) void k_scan_add(int* out, int n, const int* __restrict__ offs) {
  const int base = blockIdx.x * 1024 + threadIdx.x * 4;
  const int o = offs[blockIdx.x];
#pragma unroll
  for (int q = 0; q < 4; q++)
    if (base + q < n) out[base + q] += o;
}

// *total = out[n - 1] + value(in[n - 1])
template <bool POPC>
__global__ void k_scan_total(const int* __restrict__ in, const int* __restrict__ out, int n, int* __restrict__ total) {
  if (threadIdx.x != 0) return;
  const int x = in[n - 1];
  *total = out[n - 1] + (POPC ? __popc((unsigned)x) : x);
}

}  // namespace

size_t sfmx_scan_aux(int n) {
  size_t a = 0;
  while (n > 1) {
    n = (n + 1023) / 1024;
    a += (size_t)n;
  }
  return a + 1;
}

void sfmx_scan(const int* in, bool popc, int n, int* out, int* aux, hipStream_t s) {
  const int nb = (n + 1023) / 1024;
  if (popc) k_scan_local<true><<<nb, 256, 0, s>>>(in, n, out, aux);
  else k_scan_local<false><<<nb, 256, 0, s>>>(in, n, out, aux);
  if (nb > 1) {
    sfmx_scan(aux, false, nb, aux, aux + nb, s);
    k_scan_add<<<nb, 256, 0, s>>>(out, n, aux);
  }
}

void sfmx_scan_total(const int* in, bool popc, const int* out, int n, int* total, hipStream_t s) {
  if (popc) k_scan_total<true><<<1, 64, 0, s>>>(in, out, n, total);
  else k_scan_total<false><<<1, 64, 0, s>>>(in, out, n, total);
}
