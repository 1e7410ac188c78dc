// sfmx_mesh_dev.h — what the mesh stages share: the range-checked load of a face, the staging of a host
// mesh, and the compaction of a mesh by keep flags (scan, scan, emit, emit) with its five output slabs.  clean.hip and visib.hip
// compact through the same kernels (mesh.hip) in the same order, so that their outputs agree byte for byte wherever their flags do.
#pragma once
#include "sfmx_internal.h"

namespace {

// the three indices of face f; false when one lies outside [0, n): nothing may then be read through them
__device__ __forceinline__ bool mesh_face(const int* __restrict__ faces, int f, int n, int& a, int& b, int& c) {
  a = faces[3 * (size_t)f];
  b = faces[3 * (size_t)f + 1];
  c = faces[3 * (size_t)f + 2];
  return (unsigned)a < (unsigned)n && (unsigned)b < (unsigned)n && (unsigned)c < (unsigned)n;
}

}  // namespace

// mesh.hip: the kept vertices (their 24 bytes, their normals' unless normals is null, their input indices) and the kept faces
// (their indices renumbered through voff, their input indices), one launch each on stream s; n > 0, m > 0
void sfmx_mesh_emit_verts(int n, const int* vkeep, const int* voff, const double* verts, const double* normals, double* verts_out,
                          double* normals_out, int* vsrc, hipStream_t s);
void sfmx_mesh_emit_faces(const int32_t* faces, int m, const int* fkeep, const int* foff, const int* voff, int32_t* faces_out, int* fsrc,
                          hipStream_t s);

// device pointers of a mesh; normals is null without them
struct MeshDev {
  const double *verts = nullptr, *normals = nullptr;
  const int32_t* faces = nullptr;
};

// a host mesh staged on the device
struct MeshInput {
  DevBuf in_v, in_n, in_f;
  // Copies the host arrays (normals may be null) and sets d to the device copies.  normals_pad > 0 sizes in_n so that normals
  // given with an empty mesh still come back non-null.
  hipError_t stage(const double* verts, const double* normals, int n, const int32_t* faces, int m, hipStream_t s, MeshDev& d,
                   size_t normals_pad = 0) {
    const size_t vb = (size_t)n * 24, fb = (size_t)m * 12;
    hipError_t e = in_v.ensure(vb);
    if (e == hipSuccess) e = in_f.ensure(fb);
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(in_v.p, verts, vb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && m > 0) e = hipMemcpyAsync(in_f.p, faces, fb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && normals) e = in_n.ensure(vb + normals_pad);
    if (e == hipSuccess && normals && n > 0) e = hipMemcpyAsync(in_n.p, normals, vb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) d = MeshDev{in_v.as<double>(), normals ? in_n.as<double>() : nullptr, in_f.as<int32_t>()};
    return e;
  }
  void release() {
    for (DevBuf* b : {&in_v, &in_n, &in_f}) b->release();
  }
};

// a mesh compacted by keep flags: the kept vertices (bytes copied), normals, renumbered faces and the input index of each
struct MeshCompact {
  DevBuf out_v, out_n, out_f, vsrc, fsrc;
  int nv_out = 0, nf_out = 0;  // the owner sets them from the two device words once it has read them back
  bool has_normals = false;

  // the outputs are sized by the input: the kept counts are only known on the host after the launches
  hipError_t ensure(size_t n, size_t m, bool normals) {
    hipError_t e = out_v.ensure(n * 24);
    if (e == hipSuccess && normals) e = out_n.ensure(n * 24);
    if (e == hipSuccess) e = out_f.ensure(m * 12);
    if (e == hipSuccess) e = vsrc.ensure(n * 4);
    if (e == hipSuccess) e = fsrc.ensure(m * 4);
    return e;
  }

  // fkeep [m] and vkeep [n] are the flags, foff / voff receive their exclusive scans, aux is the scans' (sfmx_scan_aux of the
  // larger), *nf_word / *nv_word (device) the kept counts.  The caller says whether the faces are emitted.
  void launch(const double* verts, const double* normals, int n, const int32_t* faces, int m, const int* fkeep, int* foff,
              const int* vkeep, int* voff, int* aux, int* nf_word, int* nv_word, bool emit_faces, hipStream_t s) {
    if (m > 0) {
      sfmx_scan(fkeep, false, m, foff, aux, s);
      sfmx_scan_total(fkeep, false, foff, m, nf_word, s);
    }
    if (n > 0) {
      sfmx_scan(vkeep, false, n, voff, aux, s);
      sfmx_scan_total(vkeep, false, voff, n, nv_word, s);
      sfmx_mesh_emit_verts(n, vkeep, voff, verts, normals, out_v.as<double>(), out_n.as<double>(), vsrc.as<int>(), s);
    }
    if (emit_faces) sfmx_mesh_emit_faces(faces, m, fkeep, foff, voff, out_f.as<int32_t>(), fsrc.as<int>(), s);
  }

  // queues the copies of the arrays asked for; the caller synchronises
  hipError_t read(double* verts_out, double* normals_out, int32_t* faces_out, int32_t* vert_src, int32_t* face_src, hipStream_t s) const {
    const size_t nv = (size_t)nv_out, nf = (size_t)nf_out;
    hipError_t e = hipSuccess;
    if (verts_out && nv) e = hipMemcpyAsync(verts_out, out_v.p, nv * 24, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && normals_out && nv && has_normals) e = hipMemcpyAsync(normals_out, out_n.p, nv * 24, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && faces_out && nf) e = hipMemcpyAsync(faces_out, out_f.p, nf * 12, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && vert_src && nv) e = hipMemcpyAsync(vert_src, vsrc.p, nv * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && face_src && nf) e = hipMemcpyAsync(face_src, fsrc.p, nf * 4, hipMemcpyDeviceToHost, s);
    return e;
  }

  // the compacted mesh on the device; mc is null while its owner has no result.  Return the number of vertices, or -1 without
  // a result.
  static int device_mesh(const MeshCompact* mc, const double** verts, const int32_t** faces, int* n_verts, int* n_faces) {
    if (verts) *verts = mc ? mc->out_v.as<double>() : nullptr;
    if (faces) *faces = mc ? mc->out_f.as<int32_t>() : nullptr;
    if (n_verts) *n_verts = mc ? mc->nv_out : 0;
    if (n_faces) *n_faces = mc ? mc->nf_out : 0;
    return mc ? mc->nv_out : -1;
  }
  static int device_surface(const MeshCompact* mc, const double** verts, const double** normals) {
    if (verts) *verts = mc ? mc->out_v.as<double>() : nullptr;
    if (normals) *normals = mc && mc->has_normals ? mc->out_n.as<double>() : nullptr;
    return mc ? mc->nv_out : -1;
  }

  void release() {
    for (DevBuf* b : {&out_v, &out_n, &out_f, &vsrc, &fsrc}) b->release();
  }
};
