// mesh.hip — the two kernels that emit a mesh compacted by keep flags (sfmx_mesh_dev.h: MeshCompact).
//
// A file of its own rather than kernels in the header, as scan.hip: clean, simplify and visib need the two entry points, and one
// object holds the one copy of the kernels (every mesh stage includes the header, most of them for mesh_face and MeshInput alone).
// Bytes are copied and indices looked up; nothing is computed, so any schedule gives the same output.
#include "sfmx_mesh_dev.h"

namespace {

// per kept vertex: its 24 bytes (and its normal's), its input index
__global__ __launch_bounds__(256) void k_mesh_emit_verts(int n, const int* __restrict__ vkeep, const int* __restrict__ voff,
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

// per kept face: its indices renumbered through voff, its input index
__global__ __launch_bounds__(256) void k_mesh_emit_faces(const int* __restrict__ faces, int m, const int* __restrict__ fkeep,
                                                         const int* __restrict__ foff, const int* __restrict__ voff,
                                                         int* __restrict__ faces_out, int* __restrict__ fsrc) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= m || !fkeep[f]) return;  // a kept face has indices that voff covers
  const size_t o = (size_t)foff[f];
#pragma unroll
  for (int a = 0; a < 3; a++) faces_out[3 * o + a] = voff[faces[3 * (size_t)f + a]];
  fsrc[o] = f;
}

}  // namespace

void sfmx_mesh_emit_verts(int n, const int* vkeep, const int* voff, const double* verts, const double* normals, double* verts_out,
                          double* normals_out, int* vsrc, hipStream_t s) {
  k_mesh_emit_verts<<<(unsigned)(((size_t)n + 255) / 256), 256, 0, s>>>(
      n, vkeep, voff, reinterpret_cast<const unsigned long long*>(verts), reinterpret_cast<const unsigned long long*>(normals),
      reinterpret_cast<unsigned long long*>(verts_out), reinterpret_cast<unsigned long long*>(normals_out), vsrc);
}

void sfmx_mesh_emit_faces(const int32_t* faces, int m, const int* fkeep, const int* foff, const int* voff, int32_t* faces_out, int* fsrc,
                          hipStream_t s) {
  k_mesh_emit_faces<<<(unsigned)(((size_t)m + 255) / 256), 256, 0, s>>>(faces, m, fkeep, foff, voff, faces_out, fsrc);
}
