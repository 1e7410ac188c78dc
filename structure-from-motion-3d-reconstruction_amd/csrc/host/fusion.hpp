// fusion.hpp — host side of multi-pair depth fusion (fusion.cpp): every listed keyframe pair through rectification and the
// device disparity into one TSDF volume (sfmx_fusion_*), then one surface.  C structs: bound by pipeline.py through ctypes.
#pragma once
#include <cstdint>

#include "../../../include/sfmx.h"

extern "C" {

// outputs of sfmx_host_fusion_mesh, allocated by the library (release with sfmx_host_fusion_free):
// verts double [n_verts][3], faces int32 [n_faces][3]; n_views = pairs integrated (skipped ones not counted)
struct sfmx_fusion_result {
  double* verts;
  int32_t* faces;
  int n_verts, n_faces, n_views;
};

// images: n pointers to u8 [h][w] (host, or device with on_device = 1); poses12 [n][12] camera->world R (row-major) + centre;
// pairs [m][2] indices into images.  A pair out of range or that cannot be rectified (zero baseline, degenerate
// rectified axes) is skipped with one WARN line in warn.
// ply_path (optional): the surface as PLY (not written when it has no faces; a WARN line says so).
int sfmx_host_fusion_mesh(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                          const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp, const sfmx_fusion_params* fp,
                          sfmx_fusion_result* res, const char* ply_path, char* warn, int warn_cap);
void sfmx_host_fusion_free(sfmx_fusion_result* res);

// sfmx_host_fusion_mesh with appearance.  app = NULL: exactly sfmx_host_fusion_mesh (normals / grey / views stay
// NULL, the PLY is the same file).  Otherwise every integrated pair is also kept as a shade view, the surface is extracted with
// normals and shaded on the device: normals double [n_verts][3], grey u8 [n_verts], views int32 [n_verts] (views that saw the
// vertex).  app->depth_tol = 0 means the volume's resolved trunc.  The PLY then carries nx ny nz (float) and red green blue
// (uchar, the grey three times) per vertex.  Release with sfmx_host_fusion_free_ex.
struct sfmx_fusion_result_ex {
  double* verts;
  int32_t* faces;
  int n_verts, n_faces, n_views;
  double* normals;
  uint8_t* grey;
  int32_t* views;
};
int sfmx_host_fusion_mesh_ex(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, sfmx_fusion_result_ex* res, const char* ply_path,
                             char* warn, int warn_cap);
void sfmx_host_fusion_free_ex(sfmx_fusion_result_ex* res);

// sfmx_host_fusion_mesh_ex with multi-view consistency filtering.  cs = NULL: exactly sfmx_host_fusion_mesh_ex
// (pair_counts is not touched).  Otherwise each pair's view is kept in a consist object instead of being queued into the
// volume; after the last pair one sfmx_consist_filter runs over all of them and the filtered maps are queued in the same
// order.  cs->disp_min is used as given (pipeline.fuse passes the fusion's).  pair_counts (optional) int32 [m][2]: the valid and
// the kept pixels of each listed pair's view, -1 -1 for a skipped pair.  The shade views of app keep the unfiltered maps.
int sfmx_host_fusion_mesh_cs(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_cs with the small connected components of the surface removed.  clean = NULL: exactly
// sfmx_host_fusion_mesh_cs (clean_counts is not touched).  Otherwise the surface is extracted (with normals when app is given),
// cleaned on the device (sfmx_clean_fusion), and with app the CLEANED device vertices and normals are shaded; the result arrays
// and the PLY are the cleaned mesh.  clean_counts (optional) int32 [4]: components, faces of the largest, vertices removed,
// faces removed.  A surface whose every component falls below min_faces has no faces left (the PLY is then skipped with its
// WARN line).
int sfmx_host_fusion_mesh_cl(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap);

// Surface accuracy and completeness, host arithmetic on squared distances from the device (sfmx_sdist_*).  Both
// sample at the vertices a face uses.  Accuracy: dist = sqrt(d2) from each reconstruction vertex to the ground-truth mesh, a
// clipped distance counting as d_max; accuracy = sorted(dist)[ceil(percentile / 100 n) - 1] (nearest rank), acc_within = the
// count with dist <= tau, acc_mean = one sequential sum in index order / n, acc_max.  Completeness: comp_within = the count of
// ground-truth vertices with dist <= tau to the reconstruction, completeness = comp_within / n_gt.  With no vertices on a side
// its doubles are NaN.  d_max > 0 and 0 <= tau <= d_max have no defaults; 0 < percentile <= 100; cell as sfmx_sdist_params.
struct sfmx_surface_eval_params {
  double d_max, tau, percentile, cell;
};
struct sfmx_surface_eval_result {
  double accuracy, acc_mean, acc_max, completeness;
  int acc_within, n_rec, comp_within, n_gt;
};
// every array is a host pointer; SFMX_ERR_INVALID for a face index out of range or a non-finite used coordinate
int sfmx_host_surface_eval(sfmx_ctx* ctx, const double* rec_verts, int n_rec_verts, const int32_t* rec_faces, int n_rec_faces,
                           const double* gt_verts, int n_gt_verts, const int32_t* gt_faces, int n_gt_faces,
                           const sfmx_surface_eval_params* p, sfmx_surface_eval_result* out);

// sfmx_host_fusion_mesh_cl with the final mesh (the cleaned one when clean is given) evaluated against a ground-truth mesh on
// the host; the final mesh is taken from the device where the last stage left it.  gt = NULL: exactly
// sfmx_host_fusion_mesh_cl (ev is not touched).  A surface without faces has n_rec = 0.
struct sfmx_surface_gt {
  const double* verts;
  int n_verts;
  const int32_t* faces;
  int n_faces;
  sfmx_surface_eval_params params;
};
int sfmx_host_fusion_mesh_ev(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_ev with the integrated volume rendered from further cameras by ray casting.  render =
// NULL: exactly sfmx_host_fusion_mesh_ev.  Otherwise each camera (R_rw, c_left, f, cx, cy, w, h of a sfmx_fusion_view; B is not
// used) is rendered with params after the surface has been made, and the arrays of out[i] that are not NULL are filled (caller
// allocated: depth double [h][w], normals / points double [h][w][3], shaded u8 [h][w]).  With app, grey u8 [h][w] and views
// int32 [h][w] are the shade stage over the render's device points and normals from the retained (unfiltered) shade views,
// pixels without a hit getting params.background and 0; without app they are left alone.  The mesh, the PLY and every other
// output are what they are without render.
struct sfmx_render_out {
  double* depth;
  double* normals;
  double* points;
  uint8_t* shaded;
  uint8_t* grey;
  int32_t* views;
  int32_t hits;
};
struct sfmx_render_request {
  const sfmx_fusion_view* cameras;
  int n_cameras;
  sfmx_raycast_params params;
  sfmx_render_out* out;  // [n_cameras]
};
int sfmx_host_fusion_mesh_rc(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_rc with each later pair's view registered to the volume before it enters it.  align =
// NULL: exactly sfmx_host_fusion_mesh_rc.  Otherwise the pairs are processed in list order: the first `seed` (>= 1) integrated
// pairs (skipped ones do not count) enter at their given views; each later pair's view is aligned against the volume integrated
// so far (sfmx_align_stereo_view, which integrates what is pending) with params, and it is the refined view that is queued into
// the volume and, with app, retained as the shade view.  out[q] (caller allocated, [m]) is the result of listed pair q; its
// status is -1 for a pair that was not aligned (a seed pair or a skipped one).  On SFMX_ALIGN_TOO_FEW or _DEGENERATE the pair
// keeps its given view and one WARN line says so.  align together with cs is refused with SFMX_ERR_INVALID: the filter needs
// every pose before anything is integrated.
struct sfmx_align_request {
  int seed;
  sfmx_align_params params;
  sfmx_align_result* out;  // [m]
};
int sfmx_host_fusion_mesh_al(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_al with the final surface simplified by exact vertex clustering.  simplify = NULL: exactly
// sfmx_host_fusion_mesh_al (simplify_counts is not touched).  Otherwise the order is: extract (with normals when app is given) ->
// clean (when given) -> simplify on the device (sfmx_simplify_clean, or sfmx_simplify_fusion without clean) -> with app the
// SIMPLIFIED device vertices are shaded with their own normals -> with gt the simplified mesh is evaluated from where it lies on
// the device -> the result arrays and the PLY are the simplified mesh.  simplify_counts (optional) int32 [5]: clusters,
// degenerate faces, duplicate faces, and the vertices and faces that went into the stage (zeros when the surface had no faces
// before it).  A surface that falls into one cell has no faces left (the PLY is then skipped with its WARN line).
int sfmx_host_fusion_mesh_sp(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_sp with the surface smoothed by the exact Taubin lambda|mu filter between cleaning and
// simplifying.  smooth = NULL: exactly sfmx_host_fusion_mesh_sp (smooth_counts is not touched).  Otherwise the order is: extract
// (with normals when app is given) -> clean (when given) -> smooth on the device (sfmx_smooth_clean, or sfmx_smooth_fusion
// without clean) -> simplify (when given; sfmx_simplify_run on the smooth object's device mesh with the normals of the stage
// before) -> with app the final device vertices are shaded (a smoothed vertex with the normal it had) -> with gt the final mesh
// is evaluated from where it lies on the device -> the result arrays and the PLY are the final mesh.  smooth->unit and origin are
// used as given (pipeline.fuse passes the voxel and the volume's origin).  smooth_counts (optional) int32 [5]: edges, boundary
// edges, irregular edges, pinned and isolated vertices (zeros when the surface had no faces before the stage).
int sfmx_host_fusion_mesh_sm(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_sm with the small holes of the surface filled by exact centroid fans between cleaning and
// smoothing.  fill = NULL: exactly sfmx_host_fusion_mesh_sm (fill_counts is not touched).  Otherwise the order is: extract (with
// normals when app is given) -> clean (when given) -> fill on the device (sfmx_fill_clean, or sfmx_fill_fusion without clean) ->
// smooth (when given; sfmx_smooth_run on the fill object's device mesh) -> simplify (when given; sfmx_simplify_run) -> with app
// the final device vertices are shaded -> with gt the final mesh is evaluated from where it lies on the device -> the result
// arrays and the PLY are the final mesh.  After a fill the vertex count differs from the stage before, so every later stage takes
// its faces and normals from the fill object.  fill->unit and origin are used as given (pipeline.fuse passes the voxel and the
// volume's origin).  fill_counts (optional) int32 [8]: edges, boundary edges, irregular edges and complex vertices of the surface
// that went in, the loops filled, their edges, and the new vertices and faces (zeros when the surface had no faces before the
// stage).
int sfmx_host_fusion_mesh_fl(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_fl with the final mesh rendered from further cameras by the exact z-buffer.  raster = NULL:
// exactly sfmx_host_fusion_mesh_fl.  Otherwise, after every other stage, each camera (R_rw, c_left, f, cx, cy, w, h of a
// sfmx_fusion_view; B is not used) renders the mesh that goes into the result arrays and the PLY (a surface without faces renders
// the background), with the appearance normals and grey per vertex when app is given, and the arrays of out[i] that are not NULL
// are filled (caller allocated: depth double [h][w], face int32 [h][w], points / normals double [h][w][3], shaded u8 [h][w], and
// with app grey u8 [h][w]; without app grey is left alone).  counts and fragments are sfmx_raster_counts'.  The mesh, the PLY,
// the ray-cast renders and every other output are what they are without raster.
struct sfmx_raster_out {
  double* depth;
  int32_t* face;
  double* points;
  double* normals;
  uint8_t* shaded;
  uint8_t* grey;
  int32_t counts[8];
  uint64_t fragments;
};
struct sfmx_raster_request {
  const sfmx_fusion_view* cameras;
  int n_cameras;
  sfmx_raster_params params;
  sfmx_raster_out* out;  // [n_cameras]
};
int sfmx_host_fusion_mesh_rs(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_rs with the faces no camera sees from the front removed from the final mesh.  visib =
// NULL: exactly sfmx_host_fusion_mesh_rs.  Otherwise the views are the integrated pairs' left rectified cameras at the image
// size (the refined ones with align), the stage runs on the final mesh after simplifying, and the shading's result arrays, the
// evaluation, the z-buffer renders and the PLY all take the culled mesh; the grey and views of a kept vertex are those it had.
// params.depth_tol == 0 stands for the voxel.  colour = 1 (needs app) replaces grey and views by this stage's grey and
// grey_views, from the pairs' left rectified images.  The request's outputs are filled: the counts, the sizes before culling and
// face_views / face_back_views [m_in], vert_views [n_in] (malloc'ed here, NULL for an empty surface; release them with
// sfmx_host_visib_free).  A surface with nothing left is no error: the result then has no arrays, as a volume without a surface.
struct sfmx_visib_request {
  sfmx_visib_params params;
  int colour;
  int32_t counts[5];   // faces_seen, faces_back_only, faces_unseen, faces_kept, verts_kept
  uint64_t pairs[3];   // pairs_visible, pairs_occluded, pairs_off
  int32_t n_in, m_in;  // vertices and faces of the mesh that entered the stage
  int32_t* face_views;
  int32_t* face_back_views;
  int32_t* vert_views;
};
void sfmx_host_visib_free(sfmx_visib_request* visib);
int sfmx_host_fusion_mesh_vs(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_vs with a texture atlas for the final mesh.  texture = NULL: exactly
// sfmx_host_fusion_mesh_vs.  Otherwise the views are the integrated pairs' left rectified cameras and images (the refined cameras
// with align), and the stage runs on the final mesh, after the visibility culling when that is asked for; the mesh, every other
// output and the PLY are what they are without it.  params.depth_tol == 0 stands for the voxel.  The request's outputs are filled:
// the counts, the faces and views of the run, and atlas u8 [H][W], face_view [n_faces], face_area [n_faces], uv_half
// [n_faces][3][2], view_faces [n_views] (malloc'ed here, NULL for an empty surface; release them with sfmx_host_texture_free).
struct sfmx_texture_request {
  sfmx_texture_params params;
  int32_t counts[6];  // faces_textured, faces_untextured, cells, W, H, cells_per_row
  int32_t n_faces, n_views;
  uint8_t* atlas;
  int32_t* face_view;
  int64_t* face_area;
  int32_t* uv_half;
  int32_t* view_faces;
};
void sfmx_host_texture_free(sfmx_texture_request* texture);
int sfmx_host_fusion_mesh_tx(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_texture_request* texture, sfmx_fusion_result_ex* res, const char* ply_path,
                             char* warn, int warn_cap);

// sfmx_host_fusion_mesh_tx with the atlas's seams levelled.  level = NULL: exactly sfmx_host_fusion_mesh_tx.
// Otherwise a texture request is required (SFMX_ERR_INVALID without one); the level stage runs after the texture stage on the
// same final mesh, and the mesh, the texture request's outputs, every other output and the PLY are what they are without it.
// The request's outputs are filled: the counts, the faces and vertices of the run, and atlas u8 [H][W] (the texture request's W
// and H), corner_adj [n_faces][3], corner_sample [n_faces][3], vertex_views [n_verts] (malloc'ed here, NULL for an empty
// surface; release them with sfmx_host_level_free).
struct sfmx_level_request {
  sfmx_level_params params;
  int32_t counts[6];  // nodes, seam_vertices, pinned_nodes, free_nodes, node_edges, iterations
  int32_t n_faces, n_verts;
  uint8_t* atlas;
  int32_t* corner_adj;
  int32_t* corner_sample;
  int32_t* vertex_views;
};
void sfmx_host_level_free(sfmx_level_request* level);
int sfmx_host_fusion_mesh_lv(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_texture_request* texture, sfmx_level_request* level, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_lv with the textured mesh rendered back into the texture's own views.  photo = NULL:
// exactly sfmx_host_fusion_mesh_lv.  Otherwise a texture request is required (SFMX_ERR_INVALID without one); the photo stage runs
// last on the same final mesh, over the texture object's views with their images (view k with tex_view = k), at the texture's
// z_min, from the levelled atlas with a level request; the mesh, the other requests' outputs and the PLY are what they are without
// it.  The request's outputs are filled: the views (each w x h, view q's pixels at q w h) and rendered u8, cls u8, face int32
// [n_views w h], classes int64 [n_views][5], stats int64 [n_views][2][3], hist int64 [n_views][2][256] (malloc'ed here, NULL for
// an empty surface; release them with sfmx_host_photo_free).
struct sfmx_photo_request {
  sfmx_photo_params params;  // z_min is not used: the texture's
  int32_t n_views, w, h;
  uint8_t* rendered;
  uint8_t* cls;
  int32_t* face;
  int64_t* classes;
  int64_t* stats;
  int64_t* hist;
};
void sfmx_host_photo_free(sfmx_photo_request* photo);
int sfmx_host_fusion_mesh_ph(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_texture_request* texture, sfmx_level_request* level, sfmx_photo_request* photo,
                             sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap);

// sfmx_host_fusion_mesh_ph with the volume carved by the pairs' silhouettes.  carve = NULL: exactly
// sfmx_host_fusion_mesh_ph.  Otherwise the silhouette of every integrated pair is its left rectified picture at `threshold` under
// the pair's left rectified camera (the refined one with align), kept as a signed squared distance map at params.cap; after the
// last integration and before the extraction the hull of all of them is computed on the volume's grid (params.trunc == 0 stands
// for the volume's resolved trunc) and the volume is carved with it (sfmx_carve_apply: params.margin, params.mode), so that the
// surface, the normals, the ray-cast renders and every later stage see the carved volume.  hull_only = 1 skips the disparities
// and the integration: each pair is only rectified, the hull is stored into the empty volume (sfmx_carve_store) and the rest of
// the chain runs on it; it is refused (SFMX_ERR_INVALID) together with cs, align and app, which need the disparity maps.  The
// request's outputs are filled: counts (defined, outside, changed; with hull_only the mode is not used, changed is 0 and the result's n_views, the pairs
// integrated, is 0), n_views and inside_pixels
// [n_views], the inside pixels of each view (malloc'ed here, NULL without a view; release it with sfmx_host_carve_free).
// Without an integrated pair nothing is carved.
struct sfmx_carve_request {
  sfmx_carve_params params;
  int threshold;  // 1 .. 255
  int hull_only;  // 0 or 1
  int32_t counts[3];
  int32_t n_views;
  int32_t* inside_pixels;
};
void sfmx_host_carve_free(sfmx_carve_request* carve);
int sfmx_host_fusion_mesh_cv(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_texture_request* texture, sfmx_level_request* level, sfmx_photo_request* photo,
                             sfmx_carve_request* carve, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap);
}
