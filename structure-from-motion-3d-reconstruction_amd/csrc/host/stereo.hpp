// stereo.hpp — host side of the keyframe-pair stereo mesh (stereo.cpp): rectification of a posed pair, the grid mesh of a
// disparity map, and the whole pair on top of sfmx_stereo_disparity.  C structs: bound by pipeline.py through ctypes.
#pragma once
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/sfmx.h"

extern "C" {

// rectified frame of a pair: rows of R_rw are the rectified axes in world coordinates; the left view is the one whose
// camera lies on the -x side of the other; H_* map a rectified pixel to a source pixel of that view
struct sfmx_stereo_rect {
  double R_rw[9], c_left[3], c_right[3];
  double f, cx, cy, B;
  double H_l[9], H_r[9];
  int swapped;  // 1: view b is the left one
};
struct sfmx_stereo_mesh_params {
  int step;
  double disp_min, disp_jump, z_max_percentile;
};
// one pair of a pipeline run (sfmx_pipeline_run_ex): keyframe indices + the disparity and mesh parameters
struct sfmx_stereo_request {
  int kf_a, kf_b;
  sfmx_stereo_params params;
  sfmx_stereo_mesh_params mesh;
};
// caller-owned outputs of a pair: verts [verts_cap][3], faces [faces_cap][3], disp16 [h][w] (optional)
struct sfmx_stereo_result {
  double* verts;
  int verts_cap;
  int* faces;
  int faces_cap;
  int16_t* disp16;
  int n_verts, n_faces;
  sfmx_stereo_rect rect;
};

// pose12: camera->world R (row-major) + camera centre.  SFMX_ERR_INVALID for a zero baseline.
int sfmx_host_stereo_rectify(const double* K9, const double* pose_a12, const double* pose_b12, int w, int h, sfmx_stereo_rect* out);
// grid mesh of disp16 [h][w]; returns the number of vertices (0 = skipped, the reason in warn), < 0 = -status
int sfmx_host_stereo_grid_mesh(const int16_t* disp16, int w, int h, const sfmx_stereo_rect* r, const sfmx_stereo_mesh_params* mp,
                               double* verts_out, int verts_cap, int* faces_out, int faces_cap, int* n_faces, char* warn, int warn_cap);
// rectify -> sfmx_stereo_disparity -> grid mesh (images u8 [h][w], host or on_device); res->n_verts == 0: skipped (warn)
int sfmx_host_stereo_mesh(sfmx_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int on_device, int w, int h, const double* K9,
                          const double* pose_a12, const double* pose_b12, const sfmx_stereo_params* p, const sfmx_stereo_mesh_params* mp,
                          sfmx_stereo_result* res, char* warn, int warn_cap);
}

namespace sfmx_host {
// the grid mesh on std containers; returns "" or the reason the export is skipped
std::string stereo_grid_mesh(const int16_t* disp16, int w, int h, const sfmx_stereo_rect& r, const sfmx_stereo_mesh_params& mp,
                             std::vector<double>& verts, std::vector<std::array<int, 3>>& faces);
}  // namespace sfmx_host
