// fusion.cpp — multi-pair depth fusion on the host: for each pair, rectify (host), disparity (device) and queue the left
// rectified view with its device disparity map; then one integration and one extraction.
#include "fusion.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "pipeline.hpp"
#include "stereo.hpp"

// Weak: a libsfmx.so without the device stages (tests/fake_sfmx, the CPU stand-in of the sanitizer builds) still links;
// sfmx_host_fusion_mesh then reports SFMX_ERR_UNSUPPORTED.
#pragma weak sfmx_stereo_check_params
#pragma weak sfmx_stereo_create
#pragma weak sfmx_stereo_destroy
#pragma weak sfmx_stereo_disparity
#pragma weak sfmx_fusion_check_params
#pragma weak sfmx_fusion_create
#pragma weak sfmx_fusion_destroy
#pragma weak sfmx_fusion_add_stereo_view
#pragma weak sfmx_fusion_integrate
#pragma weak sfmx_fusion_extract
#pragma weak sfmx_fusion_extract_normals
#pragma weak sfmx_shade_check_params
#pragma weak sfmx_shade_create
#pragma weak sfmx_shade_destroy
#pragma weak sfmx_shade_add_stereo_view
#pragma weak sfmx_shade_fusion
#pragma weak sfmx_consist_check_params
#pragma weak sfmx_consist_create
#pragma weak sfmx_consist_destroy
#pragma weak sfmx_consist_add_stereo_view
#pragma weak sfmx_consist_view_count
#pragma weak sfmx_consist_filter
#pragma weak sfmx_consist_counts
#pragma weak sfmx_fusion_add_consist_view
#pragma weak sfmx_clean_check_params
#pragma weak sfmx_clean_create
#pragma weak sfmx_clean_destroy
#pragma weak sfmx_clean_fusion
#pragma weak sfmx_clean_read
#pragma weak sfmx_clean_device_surface
#pragma weak sfmx_shade_vertices
#pragma weak sfmx_sdist_check_params
#pragma weak sfmx_sdist_create
#pragma weak sfmx_sdist_destroy
#pragma weak sfmx_sdist_set_target
#pragma weak sfmx_sdist_set_target_fusion
#pragma weak sfmx_sdist_set_target_clean
#pragma weak sfmx_sdist_query
#pragma weak sfmx_sdist_query_fusion
#pragma weak sfmx_sdist_query_clean
#pragma weak sfmx_raycast_check_params
#pragma weak sfmx_raycast_create
#pragma weak sfmx_raycast_destroy
#pragma weak sfmx_raycast_render
#pragma weak sfmx_raycast_read
#pragma weak sfmx_raycast_shade
#pragma weak sfmx_align_check_params
#pragma weak sfmx_align_create
#pragma weak sfmx_align_destroy
#pragma weak sfmx_align_stereo_view
#pragma weak sfmx_simplify_check_params
#pragma weak sfmx_simplify_create
#pragma weak sfmx_simplify_destroy
#pragma weak sfmx_simplify_fusion
#pragma weak sfmx_simplify_clean
#pragma weak sfmx_simplify_read
#pragma weak sfmx_simplify_counts
#pragma weak sfmx_simplify_device_surface
#pragma weak sfmx_simplify_device_mesh
#pragma weak sfmx_simplify_run
#pragma weak sfmx_smooth_check_params
#pragma weak sfmx_smooth_create
#pragma weak sfmx_smooth_destroy
#pragma weak sfmx_smooth_fusion
#pragma weak sfmx_smooth_clean
#pragma weak sfmx_smooth_read
#pragma weak sfmx_smooth_counts
#pragma weak sfmx_smooth_device_mesh
#pragma weak sfmx_smooth_device_surface
#pragma weak sfmx_smooth_run
#pragma weak sfmx_fill_check_params
#pragma weak sfmx_fill_create
#pragma weak sfmx_fill_destroy
#pragma weak sfmx_fill_fusion
#pragma weak sfmx_fill_clean
#pragma weak sfmx_fill_read
#pragma weak sfmx_fill_counts
#pragma weak sfmx_fill_device_mesh
#pragma weak sfmx_fill_device_surface
#pragma weak sfmx_raster_check_params
#pragma weak sfmx_raster_create
#pragma weak sfmx_raster_destroy
#pragma weak sfmx_raster_run
#pragma weak sfmx_raster_read
#pragma weak sfmx_raster_counts
#pragma weak sfmx_visib_check_params
#pragma weak sfmx_visib_create
#pragma weak sfmx_visib_destroy
#pragma weak sfmx_visib_add_view
#pragma weak sfmx_visib_add_stereo_view
#pragma weak sfmx_visib_run
#pragma weak sfmx_visib_read
#pragma weak sfmx_visib_sizes
#pragma weak sfmx_visib_counts
#pragma weak sfmx_visib_device_mesh
#pragma weak sfmx_texture_check_params
#pragma weak sfmx_texture_create
#pragma weak sfmx_texture_destroy
#pragma weak sfmx_texture_add_stereo_view
#pragma weak sfmx_texture_run
#pragma weak sfmx_texture_read
#pragma weak sfmx_texture_sizes
#pragma weak sfmx_texture_counts
#pragma weak sfmx_level_check_params
#pragma weak sfmx_level_create
#pragma weak sfmx_level_destroy
#pragma weak sfmx_level_run
#pragma weak sfmx_level_read
#pragma weak sfmx_level_counts
#pragma weak sfmx_photo_check_params
#pragma weak sfmx_photo_create
#pragma weak sfmx_photo_destroy
#pragma weak sfmx_photo_add_texture_views
#pragma weak sfmx_photo_run
#pragma weak sfmx_photo_read
#pragma weak sfmx_photo_sizes
#pragma weak sfmx_stereo_rectify
#pragma weak sfmx_carve_check_params
#pragma weak sfmx_carve_create
#pragma weak sfmx_carve_destroy
#pragma weak sfmx_carve_add_stereo_view
#pragma weak sfmx_carve_view_count
#pragma weak sfmx_carve_inside_pixels
#pragma weak sfmx_carve_run
#pragma weak sfmx_carve_apply
#pragma weak sfmx_carve_store
#pragma weak sfmx_carve_count

namespace {

struct Guard {
  sfmx_ctx* ctx;
  sfmx_stereo* st = nullptr;
  sfmx_fusion* fu = nullptr;
  sfmx_shade* sh = nullptr;
  sfmx_consist* cs = nullptr;
  sfmx_clean* cl = nullptr;
  sfmx_sdist* sd = nullptr;
  sfmx_raycast* rc = nullptr;
  sfmx_align* al = nullptr;
  sfmx_simplify* sm = nullptr;
  sfmx_smooth* ta = nullptr;
  sfmx_fill* fl = nullptr;
  sfmx_raster* rs = nullptr;
  sfmx_visib* vb = nullptr;
  sfmx_texture* tx = nullptr;
  sfmx_level* lv = nullptr;
  sfmx_photo* ph = nullptr;
  sfmx_carve* cv = nullptr;
  ~Guard() {
    if (cv) sfmx_carve_destroy(ctx, cv);
    if (ph) sfmx_photo_destroy(ctx, ph);
    if (lv) sfmx_level_destroy(ctx, lv);
    if (tx) sfmx_texture_destroy(ctx, tx);
    if (vb) sfmx_visib_destroy(ctx, vb);
    if (rs) sfmx_raster_destroy(ctx, rs);
    if (fl) sfmx_fill_destroy(ctx, fl);
    if (ta) sfmx_smooth_destroy(ctx, ta);
    if (sm) sfmx_simplify_destroy(ctx, sm);
    if (al) sfmx_align_destroy(ctx, al);
    if (rc) sfmx_raycast_destroy(ctx, rc);
    if (sd) sfmx_sdist_destroy(ctx, sd);
    if (cl) sfmx_clean_destroy(ctx, cl);
    if (cs) sfmx_consist_destroy(ctx, cs);
    if (st) sfmx_stereo_destroy(ctx, st);
    if (fu) sfmx_fusion_destroy(ctx, fu);
    if (sh) sfmx_shade_destroy(ctx, sh);
  }
};

// write_mesh_ply's file with nx ny nz (float) and red green blue (uchar, the grey three times) after x y z, which are printed
// exactly as write_mesh_ply prints them; the normals with 9 significant digits, enough to give back the same float
void write_mesh_ply_appearance(const std::string& path, const sfmx_fusion_result_ex& r) {
  std::ofstream f(path);
  if (!f) throw std::runtime_error("Failed to write: " + path);
  f << "ply\nformat ascii 1.0\n"
    << "element vertex " << r.n_verts << "\n"
    << "property float x\nproperty float y\nproperty float z\n"
    << "property float nx\nproperty float ny\nproperty float nz\n"
    << "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    << "element face " << r.n_faces << "\n"
    << "property list uchar int vertex_indices\n"
    << "end_header\n";
  const auto prec = f.precision();
  for (int i = 0; i < r.n_verts; i++) {
    const double* p = r.verts + 3 * (size_t)i;
    const double* n = r.normals + 3 * (size_t)i;
    const int g = r.grey[i];
    f << p[0] << " " << p[1] << " " << p[2] << " ";
    f.precision(9);
    f << (float)n[0] << " " << (float)n[1] << " " << (float)n[2];
    f.precision(prec);
    f << " " << g << " " << g << " " << g << "\n";
  }
  for (int i = 0; i < r.n_faces; i++) f << "3 " << r.faces[3 * i] << " " << r.faces[3 * i + 1] << " " << r.faces[3 * i + 2] << "\n";
}

bool sdist_linked() {
  return &sfmx_sdist_check_params && &sfmx_sdist_create && &sfmx_sdist_destroy && &sfmx_sdist_set_target && &sfmx_sdist_set_target_fusion &&
         &sfmx_sdist_set_target_clean && &sfmx_sdist_query && &sfmx_sdist_query_fusion && &sfmx_sdist_query_clean;
}

int check_eval_params(const sfmx_surface_eval_params* p) {
  if (!p) return SFMX_ERR_INVALID;
  const sfmx_sdist_params sp{p->d_max, p->cell};
  if (sfmx_sdist_check_params(&sp) != SFMX_OK) return SFMX_ERR_INVALID;
  if (!(p->tau >= 0.0) || !(p->tau <= p->d_max)) return SFMX_ERR_INVALID;
  if (!(p->percentile > 0.0) || !(p->percentile <= 100.0)) return SFMX_ERR_INVALID;
  return SFMX_OK;
}

// 1 per vertex that a face uses; false when a face index is outside [0, nv)
bool used_mask(const int32_t* faces, int m, int nv, std::vector<uint8_t>& used) {
  used.assign((size_t)nv, 0);
  for (size_t q = 0; q < (size_t)m * 3; q++) {
    if (faces[q] < 0 || faces[q] >= nv) return false;
    used[(size_t)faces[q]] = 1;
  }
  return true;
}

// the statistics of one direction from the squared distances of the used vertices, in index order
void eval_side(const std::vector<double>& d2, const std::vector<uint8_t>* used, const sfmx_surface_eval_params& p, int* n_out, int* within,
               double* rank, double* mean, double* mx) {
  std::vector<double> d;
  d.reserve(d2.size());
  for (size_t i = 0; i < d2.size(); i++)
    if (!used || (*used)[i]) d.push_back(std::sqrt(d2[i]));
  const long long n = (long long)d.size();
  int w = 0;
  double sum = 0.0, top = 0.0;
  for (double x : d) {  // one sequential sum in index order
    w += x <= p.tau ? 1 : 0;
    sum += x;
    top = x > top ? x : top;
  }
  *n_out = (int)n;
  *within = w;
  if (!rank) return;
  const double nan = std::nan("");
  *rank = *mean = *mx = nan;
  if (n == 0) return;
  *mean = sum / (double)n;
  *mx = top;
  // nearest rank, as the stereo mesh's depth cap: sorted(d)[ceil(p/100 n) - 1]
  const long long k = std::min(std::max((long long)std::ceil(p.percentile / 100.0 * (double)n), 1LL), n);
  std::nth_element(d.begin(), d.begin() + (k - 1), d.end());
  *rank = d[(size_t)(k - 1)];
}

void eval_finish(sfmx_surface_eval_result* r) {
  r->completeness = r->n_gt > 0 ? (double)r->comp_within / (double)r->n_gt : std::nan("");
}

std::vector<double> compact(const double* v, const std::vector<uint8_t>& used) {
  std::vector<double> out;
  for (size_t i = 0; i < used.size(); i++)
    if (used[i]) out.insert(out.end(), v + 3 * i, v + 3 * i + 3);
  return out;
}

}  // namespace

extern "C" {

int sfmx_host_surface_eval(sfmx_ctx* ctx, const double* rec_verts, int n_rec_verts, const int32_t* rec_faces, int n_rec_faces,
                           const double* gt_verts, int n_gt_verts, const int32_t* gt_faces, int n_gt_faces,
                           const sfmx_surface_eval_params* p, sfmx_surface_eval_result* out) {
  if (!ctx || !out || n_rec_verts < 0 || n_rec_faces < 0 || n_gt_verts < 0 || n_gt_faces < 0 || (n_rec_verts > 0 && !rec_verts) ||
      (n_rec_faces > 0 && !rec_faces) || (n_gt_verts > 0 && !gt_verts) || (n_gt_faces > 0 && !gt_faces))
    return SFMX_ERR_INVALID;
  *out = sfmx_surface_eval_result{};
  if (!sdist_linked()) return SFMX_ERR_UNSUPPORTED;
  int rc = check_eval_params(p);
  if (rc != SFMX_OK) return rc;
  std::vector<uint8_t> ru, gu;
  if (!used_mask(rec_faces, n_rec_faces, n_rec_verts, ru) || !used_mask(gt_faces, n_gt_faces, n_gt_verts, gu)) return SFMX_ERR_INVALID;
  const std::vector<double> rq = compact(rec_verts, ru), gq = compact(gt_verts, gu);
  const sfmx_sdist_params sp{p->d_max, p->cell};
  Guard g{ctx};
  rc = sfmx_sdist_create(ctx, &g.sd);
  if (rc != SFMX_OK) return rc;
  std::vector<double> d2(rq.size() / 3);
  rc = sfmx_sdist_set_target(ctx, g.sd, gt_verts, n_gt_verts, gt_faces, n_gt_faces, 0, &sp);
  if (rc == SFMX_OK) rc = sfmx_sdist_query(ctx, g.sd, rq.data(), (int)d2.size(), 0, d2.data(), nullptr);
  if (rc != SFMX_OK) return rc;
  eval_side(d2, nullptr, *p, &out->n_rec, &out->acc_within, &out->accuracy, &out->acc_mean, &out->acc_max);
  d2.assign(gq.size() / 3, 0.0);
  rc = sfmx_sdist_set_target(ctx, g.sd, rec_verts, n_rec_verts, rec_faces, n_rec_faces, 0, &sp);
  if (rc == SFMX_OK) rc = sfmx_sdist_query(ctx, g.sd, gq.data(), (int)d2.size(), 0, d2.data(), nullptr);
  if (rc != SFMX_OK) {
    *out = sfmx_surface_eval_result{};
    return rc;
  }
  eval_side(d2, nullptr, *p, &out->n_gt, &out->comp_within, nullptr, nullptr, nullptr);
  eval_finish(out);
  return SFMX_OK;
}

void sfmx_host_fusion_free_ex(sfmx_fusion_result_ex* res) {
  if (!res) return;
  std::free(res->verts);
  std::free(res->faces);
  std::free(res->normals);
  std::free(res->grey);
  std::free(res->views);
  *res = sfmx_fusion_result_ex{};
}

void sfmx_host_fusion_free(sfmx_fusion_result* res) {
  if (!res) return;
  std::free(res->verts);
  std::free(res->faces);
  res->verts = nullptr;
  res->faces = nullptr;
  res->n_verts = res->n_faces = 0;
}

int sfmx_host_fusion_mesh(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                          const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp, const sfmx_fusion_params* fp,
                          sfmx_fusion_result* res, const char* ply_path, char* warn, int warn_cap) {
  if (!res) return SFMX_ERR_INVALID;
  sfmx_fusion_result_ex ex{};
  const int rc = sfmx_host_fusion_mesh_ex(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, nullptr, &ex, ply_path, warn, warn_cap);
  *res = sfmx_fusion_result{ex.verts, ex.faces, ex.n_verts, ex.n_faces, ex.n_views};
  return rc;
}

int sfmx_host_fusion_mesh_ex(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, sfmx_fusion_result_ex* res, const char* ply_path,
                             char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_cs(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, nullptr, nullptr, res, ply_path,
                                  warn, warn_cap);
}

int sfmx_host_fusion_mesh_cs(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_cl(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, nullptr, nullptr,
                                  res, ply_path, warn, warn_cap);
}

int sfmx_host_fusion_mesh_cl(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_ev(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts,
                                  nullptr, nullptr, res, ply_path, warn, warn_cap);
}

int sfmx_host_fusion_mesh_ev(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_rc(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, nullptr, res, ply_path, warn, warn_cap);
}

int sfmx_host_fusion_mesh_rc(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_al(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, nullptr, res, ply_path, warn, warn_cap);
}

int sfmx_host_fusion_mesh_al(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_sp(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, align, nullptr, nullptr, res, ply_path, warn, warn_cap);
}

int sfmx_host_fusion_mesh_sp(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_sm(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, align, simplify, simplify_counts, nullptr, nullptr, res, ply_path, warn, warn_cap);
}

int sfmx_host_fusion_mesh_sm(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_fl(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, align, simplify, simplify_counts, smooth, smooth_counts, nullptr, nullptr, res, ply_path, warn,
                                  warn_cap);
}

int sfmx_host_fusion_mesh_fl(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_rs(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, align, simplify, simplify_counts, smooth, smooth_counts, fill, fill_counts, nullptr, res, ply_path,
                                  warn, warn_cap);
}

int sfmx_host_fusion_mesh_rs(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_vs(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, align, simplify, simplify_counts, smooth, smooth_counts, fill, fill_counts, raster, nullptr, res,
                                  ply_path, warn, warn_cap);
}

void sfmx_host_visib_free(sfmx_visib_request* visib) {
  if (!visib) return;
  std::free(visib->face_views);
  std::free(visib->face_back_views);
  std::free(visib->vert_views);
  visib->face_views = visib->face_back_views = visib->vert_views = nullptr;
}

int sfmx_host_fusion_mesh_vs(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_tx(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, align, simplify, simplify_counts, smooth, smooth_counts, fill, fill_counts, raster, visib, nullptr,
                                  res, ply_path, warn, warn_cap);
}

void sfmx_host_texture_free(sfmx_texture_request* texture) {
  if (!texture) return;
  std::free(texture->atlas);
  std::free(texture->face_view);
  std::free(texture->face_area);
  std::free(texture->uv_half);
  std::free(texture->view_faces);
  texture->atlas = nullptr;
  texture->face_view = texture->uv_half = texture->view_faces = nullptr;
  texture->face_area = nullptr;
}

int sfmx_host_fusion_mesh_tx(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_texture_request* texture, sfmx_fusion_result_ex* res, const char* ply_path,
                             char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_lv(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, align, simplify, simplify_counts, smooth, smooth_counts, fill, fill_counts, raster, visib, texture,
                                  nullptr, res, ply_path, warn, warn_cap);
}

void sfmx_host_level_free(sfmx_level_request* level) {
  if (!level) return;
  std::free(level->atlas);
  std::free(level->corner_adj);
  std::free(level->corner_sample);
  std::free(level->vertex_views);
  level->atlas = nullptr;
  level->corner_adj = level->corner_sample = level->vertex_views = nullptr;
}

int sfmx_host_fusion_mesh_lv(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_texture_request* texture, sfmx_level_request* level, sfmx_fusion_result_ex* res,
                             const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_ph(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, align, simplify, simplify_counts, smooth, smooth_counts, fill, fill_counts, raster, visib, texture,
                                  level, nullptr, res, ply_path, warn, warn_cap);
}

void sfmx_host_photo_free(sfmx_photo_request* photo) {
  if (!photo) return;
  std::free(photo->rendered);
  std::free(photo->cls);
  std::free(photo->face);
  std::free(photo->classes);
  std::free(photo->stats);
  std::free(photo->hist);
  photo->rendered = photo->cls = nullptr;
  photo->face = nullptr;
  photo->classes = photo->stats = photo->hist = nullptr;
}

int sfmx_host_fusion_mesh_ph(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_texture_request* texture, sfmx_level_request* level, sfmx_photo_request* photo,
                             sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap) {
  return sfmx_host_fusion_mesh_cv(ctx, images, on_device, n, w, h, K9, poses12, pairs, m, sp, fp, app, cs, pair_counts, clean, clean_counts, gt,
                                  ev, render, align, simplify, simplify_counts, smooth, smooth_counts, fill, fill_counts, raster, visib, texture,
                                  level, photo, nullptr, res, ply_path, warn, warn_cap);
}

void sfmx_host_carve_free(sfmx_carve_request* carve) {
  if (!carve) return;
  std::free(carve->inside_pixels);
  carve->inside_pixels = nullptr;
}

int sfmx_host_fusion_mesh_cv(sfmx_ctx* ctx, const uint8_t* const* images, int on_device, int n, int w, int h, const double* K9,
                             const double* poses12, const int32_t* pairs, int m, const sfmx_stereo_params* sp,
                             const sfmx_fusion_params* fp, const sfmx_shade_params* app, const sfmx_consist_params* cs,
                             int32_t* pair_counts, const sfmx_clean_params* clean, int32_t* clean_counts, const sfmx_surface_gt* gt,
                             sfmx_surface_eval_result* ev, const sfmx_render_request* render, const sfmx_align_request* align,
                             const sfmx_simplify_params* simplify, int32_t* simplify_counts, const sfmx_smooth_params* smooth,
                             int32_t* smooth_counts, const sfmx_fill_params* fill, int32_t* fill_counts, const sfmx_raster_request* raster,
                             sfmx_visib_request* visib, sfmx_texture_request* texture, sfmx_level_request* level, sfmx_photo_request* photo,
                             sfmx_carve_request* carve, sfmx_fusion_result_ex* res, const char* ply_path, char* warn, int warn_cap) {
  if (!ctx || (n > 0 && (!images || !poses12)) || n < 0 || m < 0 || (m > 0 && !pairs) || !K9 || !sp || !fp || !res)
    return SFMX_ERR_INVALID;
  *res = sfmx_fusion_result_ex{};
  if (warn && warn_cap > 0) warn[0] = 0;
  sfmx_visib_params vp{};
  if (visib) {
    for (int32_t& c : visib->counts) c = 0;
    for (uint64_t& c : visib->pairs) c = 0;
    visib->n_in = visib->m_in = 0;
    visib->face_views = visib->face_back_views = visib->vert_views = nullptr;
    if (!&sfmx_visib_check_params || !&sfmx_visib_create || !&sfmx_visib_destroy || !&sfmx_visib_add_view || !&sfmx_visib_add_stereo_view ||
        !&sfmx_visib_run || !&sfmx_visib_read || !&sfmx_visib_sizes || !&sfmx_visib_counts || !&sfmx_visib_device_mesh)
      return SFMX_ERR_UNSUPPORTED;
    vp = visib->params;
    if (vp.depth_tol == 0.0) vp.depth_tol = fp->voxel;
    if (sfmx_visib_check_params(&vp) != SFMX_OK || (visib->colour != 0 && visib->colour != 1) || (visib->colour && !app)) return SFMX_ERR_INVALID;
  }
  sfmx_texture_params xp{};
  if (texture) {
    for (int32_t& c : texture->counts) c = 0;
    texture->n_faces = texture->n_views = 0;
    texture->atlas = nullptr;
    texture->face_view = texture->uv_half = texture->view_faces = nullptr;
    texture->face_area = nullptr;
    if (!&sfmx_texture_check_params || !&sfmx_texture_create || !&sfmx_texture_destroy || !&sfmx_texture_add_stereo_view || !&sfmx_texture_run ||
        !&sfmx_texture_read || !&sfmx_texture_sizes || !&sfmx_texture_counts)
      return SFMX_ERR_UNSUPPORTED;
    xp = texture->params;
    if (xp.depth_tol == 0.0) xp.depth_tol = fp->voxel;
    if (sfmx_texture_check_params(&xp) != SFMX_OK) return SFMX_ERR_INVALID;
  }
  if (level) {
    for (int32_t& c : level->counts) c = 0;
    level->n_faces = level->n_verts = 0;
    level->atlas = nullptr;
    level->corner_adj = level->corner_sample = level->vertex_views = nullptr;
    if (!&sfmx_level_check_params || !&sfmx_level_create || !&sfmx_level_destroy || !&sfmx_level_run || !&sfmx_level_read || !&sfmx_level_counts)
      return SFMX_ERR_UNSUPPORTED;
    if (!texture || sfmx_level_check_params(&level->params) != SFMX_OK) return SFMX_ERR_INVALID;
  }
  sfmx_photo_params pp{};
  if (photo) {
    photo->n_views = photo->w = photo->h = 0;
    photo->rendered = photo->cls = nullptr;
    photo->face = nullptr;
    photo->classes = photo->stats = photo->hist = nullptr;
    if (!&sfmx_photo_check_params || !&sfmx_photo_create || !&sfmx_photo_destroy || !&sfmx_photo_add_texture_views || !&sfmx_photo_run ||
        !&sfmx_photo_read || !&sfmx_photo_sizes)
      return SFMX_ERR_UNSUPPORTED;
    if (!texture) return SFMX_ERR_INVALID;
    pp = photo->params;
    pp.z_min = xp.z_min;
    if (sfmx_photo_check_params(&pp) != SFMX_OK) return SFMX_ERR_INVALID;
  }
  sfmx_carve_params kp{};
  if (carve) {
    for (int32_t& c : carve->counts) c = 0;
    carve->n_views = 0;
    carve->inside_pixels = nullptr;
    if (!&sfmx_carve_check_params || !&sfmx_carve_create || !&sfmx_carve_destroy || !&sfmx_carve_add_stereo_view || !&sfmx_carve_view_count ||
        !&sfmx_carve_inside_pixels || !&sfmx_carve_run || !&sfmx_carve_apply || !&sfmx_carve_store || !&sfmx_carve_count || !&sfmx_stereo_rectify)
      return SFMX_ERR_UNSUPPORTED;
    kp = carve->params;
    if (kp.trunc == 0.0) kp.trunc = fp->trunc == 0.0 ? 4.0 * fp->voxel : fp->trunc;  // the volume's resolved trunc
    if (sfmx_carve_check_params(&kp) != SFMX_OK || carve->threshold < 1 || carve->threshold > 255 ||
        (carve->hull_only != 0 && carve->hull_only != 1))
      return SFMX_ERR_INVALID;
    if (carve->hull_only && (cs || align || app)) return SFMX_ERR_INVALID;  // they need the disparity maps
  }
  const bool hull_only = carve && carve->hull_only;
  if (!&sfmx_fusion_create || !&sfmx_stereo_disparity) return SFMX_ERR_UNSUPPORTED;
  if (app && (!&sfmx_shade_create || !&sfmx_fusion_extract_normals)) return SFMX_ERR_UNSUPPORTED;
  if (cs && (!&sfmx_consist_create || !&sfmx_fusion_add_consist_view)) return SFMX_ERR_UNSUPPORTED;
  if (clean && (!&sfmx_clean_create || !&sfmx_clean_fusion || !&sfmx_clean_read || !&sfmx_clean_device_surface || !&sfmx_shade_vertices))
    return SFMX_ERR_UNSUPPORTED;
  if (gt && !sdist_linked()) return SFMX_ERR_UNSUPPORTED;
  if (render && (!&sfmx_raycast_check_params || !&sfmx_raycast_create || !&sfmx_raycast_destroy || !&sfmx_raycast_render ||
                 !&sfmx_raycast_read || !&sfmx_raycast_shade))
    return SFMX_ERR_UNSUPPORTED;
  if (align && (!&sfmx_align_check_params || !&sfmx_align_create || !&sfmx_align_destroy || !&sfmx_align_stereo_view)) return SFMX_ERR_UNSUPPORTED;
  if (simplify && (!&sfmx_simplify_check_params || !&sfmx_simplify_create || !&sfmx_simplify_destroy || !&sfmx_simplify_fusion ||
                   !&sfmx_simplify_clean || !&sfmx_simplify_read || !&sfmx_simplify_counts || !&sfmx_simplify_device_surface ||
                   !&sfmx_simplify_device_mesh || !&sfmx_shade_vertices || !sdist_linked()))
    return SFMX_ERR_UNSUPPORTED;
  if (smooth && (!&sfmx_smooth_check_params || !&sfmx_smooth_create || !&sfmx_smooth_destroy || !&sfmx_smooth_fusion || !&sfmx_smooth_clean ||
                 !&sfmx_smooth_read || !&sfmx_smooth_counts || !&sfmx_smooth_device_mesh || !&sfmx_smooth_device_surface || !&sfmx_clean_read ||
                 !&sfmx_shade_vertices || !&sfmx_simplify_run || !sdist_linked()))
    return SFMX_ERR_UNSUPPORTED;
  if (fill && (!&sfmx_fill_check_params || !&sfmx_fill_create || !&sfmx_fill_destroy || !&sfmx_fill_fusion || !&sfmx_fill_clean ||
               !&sfmx_fill_read || !&sfmx_fill_counts || !&sfmx_fill_device_mesh || !&sfmx_fill_device_surface || !&sfmx_smooth_run ||
               !&sfmx_shade_vertices || !&sfmx_simplify_run || !sdist_linked()))
    return SFMX_ERR_UNSUPPORTED;
  if (raster && (!&sfmx_raster_check_params || !&sfmx_raster_create || !&sfmx_raster_destroy || !&sfmx_raster_run || !&sfmx_raster_read ||
                 !&sfmx_raster_counts))
    return SFMX_ERR_UNSUPPORTED;
  int rc = sfmx_stereo_check_params(w, h, sp);
  if (rc != SFMX_OK) return rc;
  rc = sfmx_fusion_check_params(fp);
  if (rc != SFMX_OK) return rc;
  std::vector<uint8_t> gt_used;
  if (gt) {
    if (!ev || gt->n_verts < 0 || gt->n_faces < 0 || (gt->n_verts > 0 && !gt->verts) || (gt->n_faces > 0 && !gt->faces)) return SFMX_ERR_INVALID;
    *ev = sfmx_surface_eval_result{};
    rc = check_eval_params(&gt->params);
    if (rc != SFMX_OK) return rc;
    if (!used_mask(gt->faces, gt->n_faces, gt->n_verts, gt_used)) return SFMX_ERR_INVALID;
  }
  sfmx_shade_params ap{};
  if (app) {
    ap = *app;
    if (ap.depth_tol == 0.0) ap.depth_tol = fp->trunc == 0.0 ? 4.0 * fp->voxel : fp->trunc;  // the volume's resolved trunc
    rc = sfmx_shade_check_params(&ap);
    if (rc != SFMX_OK) return rc;
  }
  if (cs) {
    rc = sfmx_consist_check_params(cs);
    if (rc != SFMX_OK) return rc;
    if (pair_counts)
      for (int q = 0; q < 2 * m; q++) pair_counts[q] = -1;
  }
  if (clean) {
    rc = sfmx_clean_check_params(clean);
    if (rc != SFMX_OK) return rc;
    if (clean_counts)
      for (int q = 0; q < 4; q++) clean_counts[q] = 0;
  }
  if (simplify) {
    rc = sfmx_simplify_check_params(simplify);
    if (rc != SFMX_OK) return rc;
    if (simplify_counts)
      for (int q = 0; q < 5; q++) simplify_counts[q] = 0;
  }
  if (smooth) {
    rc = sfmx_smooth_check_params(smooth);
    if (rc != SFMX_OK) return rc;
    if (smooth_counts)
      for (int q = 0; q < 5; q++) smooth_counts[q] = 0;
  }
  if (fill) {
    rc = sfmx_fill_check_params(fill);
    if (rc != SFMX_OK) return rc;
    if (fill_counts)
      for (int q = 0; q < 8; q++) fill_counts[q] = 0;
  }
  if (render) {
    if (render->n_cameras < 0 || (render->n_cameras > 0 && (!render->cameras || !render->out))) return SFMX_ERR_INVALID;
    rc = sfmx_raycast_check_params(&render->params);
    if (rc != SFMX_OK) return rc;
    for (int q = 0; q < render->n_cameras; q++) render->out[q].hits = 0;
  }
  if (raster) {
    if (raster->n_cameras < 0 || (raster->n_cameras > 0 && (!raster->cameras || !raster->out))) return SFMX_ERR_INVALID;
    rc = sfmx_raster_check_params(&raster->params);
    if (rc != SFMX_OK) return rc;
    for (int q = 0; q < raster->n_cameras; q++) {
      for (int32_t& c : raster->out[q].counts) c = 0;
      raster->out[q].fragments = 0;
    }
  }
  if (align) {
    // the filter needs every pose before anything is integrated
    if (cs || align->seed < 1 || (m > 0 && !align->out)) return SFMX_ERR_INVALID;
    rc = sfmx_align_check_params(&align->params);
    if (rc != SFMX_OK) return rc;
    for (int q = 0; q < m; q++) {
      align->out[q] = sfmx_align_result{};
      align->out[q].status = -1;
    }
  }
  std::string log;
  Guard g{ctx};
  rc = sfmx_fusion_create(ctx, fp, &g.fu);
  if (rc != SFMX_OK) return rc;
  if (align) {
    rc = sfmx_align_create(ctx, &g.al);
    if (rc != SFMX_OK) return rc;
  }
  if (cs) {
    rc = sfmx_consist_create(ctx, &g.cs);
    if (rc != SFMX_OK) return rc;
  }
  std::vector<int> listed;  // with cs: the listed pair behind each consist view
  if (app) {
    rc = sfmx_shade_create(ctx, &g.sh);
    if (rc != SFMX_OK) return rc;
  }
  if (visib) {
    rc = sfmx_visib_create(ctx, &g.vb);
    if (rc != SFMX_OK) return rc;
  }
  if (texture) {
    rc = sfmx_texture_create(ctx, &g.tx);
    if (rc != SFMX_OK) return rc;
  }
  if (level) {
    rc = sfmx_level_create(ctx, &g.lv);
    if (rc != SFMX_OK) return rc;
  }
  if (photo) {
    rc = sfmx_photo_create(ctx, &g.ph);
    if (rc != SFMX_OK) return rc;
  }
  if (carve) {
    rc = sfmx_carve_create(ctx, &g.cv);
    if (rc != SFMX_OK) return rc;
  }
  std::vector<int16_t> d16((size_t)w * h);  // sfmx_stereo_disparity always returns the map to the host
  for (int q = 0; q < m; q++) {
    const int a = pairs[2 * q], b = pairs[2 * q + 1];
    const std::string tag = "(" + std::to_string(a) + ", " + std::to_string(b) + ")";
    if (a < 0 || a >= n || b < 0 || b >= n) {
      log += "WARN: fusion pair " + tag + " skipped (out of range, images=" + std::to_string(n) + ")\n";
      continue;
    }
    sfmx_stereo_rect r{};
    if (sfmx_host_stereo_rectify(K9, poses12 + 12 * a, poses12 + 12 * b, w, h, &r) != SFMX_OK) {
      // rectification fails on a zero (or non-finite) baseline, or when the rectified y axis degenerates (both optical
      // axes parallel to the baseline)
      const double* ca = poses12 + 12 * a + 9;
      const double* cb = poses12 + 12 * b + 9;
      const bool same = ca[0] == cb[0] && ca[1] == cb[1] && ca[2] == cb[2];
      log += "WARN: fusion pair " + tag + (same ? " skipped (zero baseline)\n" : " skipped (degenerate rectification)\n");
      continue;
    }
    if (!g.st) {
      rc = sfmx_stereo_create(ctx, w, h, sp, &g.st);
      if (rc != SFMX_OK) return rc;
    }
    const uint8_t* il = r.swapped ? images[b] : images[a];
    const uint8_t* ir = r.swapped ? images[a] : images[b];
    rc = hull_only ? sfmx_stereo_rectify(ctx, g.st, il, ir, on_device, r.H_l, r.H_r)
                   : sfmx_stereo_disparity(ctx, g.st, il, ir, on_device, r.H_l, r.H_r, d16.data(), nullptr, nullptr);
    if (rc != SFMX_OK) return rc;
    sfmx_fusion_view v{};
    std::memcpy(v.R_rw, r.R_rw, sizeof v.R_rw);
    std::memcpy(v.c_left, r.c_left, sizeof v.c_left);
    v.f = r.f;
    v.cx = r.cx;
    v.cy = r.cy;
    v.B = r.B;
    v.w = w;
    v.h = h;
    if (align && res->n_views >= align->seed) {
      // against the volume integrated so far (the call integrates what is pending); the refined view enters it
      sfmx_align_result& ar = align->out[q];
      rc = sfmx_align_stereo_view(ctx, g.al, g.fu, &v, g.st, &align->params, &ar);
      if (rc != SFMX_OK) return rc;
      if (ar.status == SFMX_ALIGN_TOO_FEW || ar.status == SFMX_ALIGN_DEGENERATE)
        log += "WARN: fusion pair " + tag + " not aligned (" + (ar.status == SFMX_ALIGN_TOO_FEW ? "too few samples" : "degenerate system") +
               "), given view kept\n";
      else
        v = ar.view;
    }
    // with cs the view waits in the consist object: its filtered map is queued after the loop
    rc = hull_only ? SFMX_OK : cs ? sfmx_consist_add_stereo_view(ctx, g.cs, &v, g.st) : sfmx_fusion_add_stereo_view(ctx, g.fu, &v, g.st);
    if (rc != SFMX_OK) return rc;
    if (carve) {  // the silhouette of the view as it entered the volume
      rc = sfmx_carve_add_stereo_view(ctx, g.cv, &v, g.st, carve->threshold, kp.cap);
      if (rc != SFMX_OK) return rc;
    }
    if (cs) listed.push_back(q);
    if (app) {
      rc = sfmx_shade_add_stereo_view(ctx, g.sh, &v, g.st);
      if (rc != SFMX_OK) return rc;
    }
    if (visib) {  // the view as it entered the volume; its left rectified image only when the stage colours
      rc = visib->colour ? sfmx_visib_add_stereo_view(ctx, g.vb, &v, g.st) : sfmx_visib_add_view(ctx, g.vb, &v, nullptr, 0);
      if (rc != SFMX_OK) return rc;
    }
    if (texture) {  // the view as it entered the volume, with its left rectified image
      rc = sfmx_texture_add_stereo_view(ctx, g.tx, &v, g.st);
      if (rc != SFMX_OK) return rc;
    }
    if (!hull_only) res->n_views++;  // pairs integrated: none with hull_only (carve->n_views counts its silhouettes)
  }
  if (cs) {
    rc = sfmx_consist_filter(ctx, g.cs, cs);
    if (rc != SFMX_OK) return rc;
    const int nc = sfmx_consist_view_count(g.cs);
    for (int i = 0; i < nc; i++) {
      rc = sfmx_fusion_add_consist_view(ctx, g.fu, g.cs, i);
      if (rc != SFMX_OK) return rc;
    }
    if (pair_counts && nc > 0) {
      std::vector<int32_t> valid((size_t)nc), kept((size_t)nc);
      rc = sfmx_consist_counts(ctx, g.cs, valid.data(), kept.data());
      if (rc != SFMX_OK) return rc;
      for (int i = 0; i < nc; i++) {
        pair_counts[2 * listed[(size_t)i]] = valid[(size_t)i];
        pair_counts[2 * listed[(size_t)i] + 1] = kept[(size_t)i];
      }
    }
  }
  rc = sfmx_fusion_integrate(ctx, g.fu);
  if (rc != SFMX_OK) return rc;
  if (carve && sfmx_carve_view_count(g.cv) > 0) {
    const sfmx_carve_volume vol{{fp->origin[0], fp->origin[1], fp->origin[2]}, fp->voxel, fp->nx, fp->ny, fp->nz};
    rc = sfmx_carve_run(ctx, g.cv, &vol, &kp);
    // hull_only: the counters come from the hull alone (changed stays 0: there was no volume to change), then the hull is stored
    if (rc == SFMX_OK) rc = hull_only ? sfmx_carve_count(ctx, g.cv, &kp, carve->counts) : sfmx_carve_apply(ctx, g.cv, g.fu, &kp, carve->counts);
    if (rc == SFMX_OK && hull_only) rc = sfmx_carve_store(ctx, g.cv, g.fu);
    if (rc != SFMX_OK) return rc;
    carve->n_views = sfmx_carve_view_count(g.cv);
    carve->inside_pixels = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (size_t)carve->n_views));
    if (!carve->inside_pixels) return SFMX_ERR_INVALID;
    rc = sfmx_carve_inside_pixels(g.cv, carve->inside_pixels);
    if (rc != SFMX_OK) return rc;
  }
  int nv = 0, nf = 0;
  rc = sfmx_fusion_extract(ctx, g.fu, nullptr, 0, nullptr, 0, &nv, &nf);
  if (rc != SFMX_OK) return rc;
  if (clean && nf > 0) {
    // the extraction always returns its arrays to the host; the cleaning reads the copy it left on the device
    const int nv0 = nv, nf0 = nf;
    std::vector<double> tv((size_t)nv * 3), tn(app ? (size_t)nv * 3 : 0);
    std::vector<int32_t> tf((size_t)nf * 3);
    rc = app ? sfmx_fusion_extract_normals(ctx, g.fu, tv.data(), nv, tf.data(), nf, tn.data(), &nv, &nf)
             : sfmx_fusion_extract(ctx, g.fu, tv.data(), nv, tf.data(), nf, &nv, &nf);
    if (rc == SFMX_OK) rc = sfmx_clean_create(ctx, &g.cl);
    int ncomp = 0, largest = 0;
    if (rc == SFMX_OK) rc = sfmx_clean_fusion(ctx, g.cl, g.fu, clean, &nv, &nf, &ncomp, &largest);
    if (rc != SFMX_OK) return rc;
    if (clean_counts) {
      clean_counts[0] = ncomp;
      clean_counts[1] = largest;
      clean_counts[2] = nv0 - nv;
      clean_counts[3] = nf0 - nf;
    }
  }
  // filling adds vertices and faces: the mesh that leaves it lies inside the fill object (fdv, fdn, fdf), and every later stage
  // takes its faces and normals from there, not from the clean object or the extraction
  const double *fdv = nullptr, *fdn = nullptr;
  const int32_t* fdf = nullptr;
  if (fill && nf > 0) {
    if (!clean) {  // an uncleaned surface is extracted with its arrays so that it lies inside the volume object
      std::vector<double> tv((size_t)nv * 3), tn(app ? (size_t)nv * 3 : 0);
      std::vector<int32_t> tf((size_t)nf * 3);
      rc = app ? sfmx_fusion_extract_normals(ctx, g.fu, tv.data(), nv, tf.data(), nf, tn.data(), &nv, &nf)
               : sfmx_fusion_extract(ctx, g.fu, tv.data(), nv, tf.data(), nf, &nv, &nf);
      if (rc != SFMX_OK) return rc;
    }
    rc = sfmx_fill_create(ctx, &g.fl);
    if (rc == SFMX_OK) rc = clean ? sfmx_fill_clean(ctx, g.fl, g.cl, fill) : sfmx_fill_fusion(ctx, g.fl, g.fu, fill);
    int counts[8] = {};
    if (rc == SFMX_OK)
      rc = sfmx_fill_counts(g.fl, &counts[0], &counts[1], &counts[2], &counts[3], &counts[4], &counts[5], &counts[6], &counts[7]);
    if (rc == SFMX_OK && (sfmx_fill_device_mesh(g.fl, &fdv, &fdf, &nv, &nf) < 0 || nf <= 0)) rc = SFMX_ERR_INVALID;
    if (rc == SFMX_OK && app) {
      const double* tmp = nullptr;
      if (sfmx_fill_device_surface(g.fl, &tmp, &fdn) != nv || !fdn) rc = SFMX_ERR_INVALID;
    }
    if (rc != SFMX_OK) return rc;
    if (fill_counts)
      for (int q = 0; q < 8; q++) fill_counts[q] = counts[q];
  }
  const bool filled = g.fl != nullptr;
  // smoothing moves vertices only: the faces and the normals of the mesh that leaves it are those of the stage before, on the
  // device (sdf, sdn) and, for an uncleaned surface, in the host arrays of the extraction that put it there (sv, sf, sn)
  std::vector<double> sv, sn;
  std::vector<int32_t> sf;
  const double *sdv = nullptr, *sdn = nullptr;
  const int32_t* sdf = nullptr;
  if (smooth && nf > 0 && filled) {
    rc = sfmx_smooth_create(ctx, &g.ta);
    if (rc == SFMX_OK) rc = sfmx_smooth_run(ctx, g.ta, fdv, nv, fdf, nf, 1, smooth);
    int counts[5] = {};
    if (rc == SFMX_OK) rc = sfmx_smooth_counts(g.ta, &counts[0], &counts[1], &counts[2], &counts[3], &counts[4]);
    int snf = 0;
    if (rc == SFMX_OK && (sfmx_smooth_device_mesh(g.ta, &sdv, &sdf, &snf) != nv || snf != nf)) rc = SFMX_ERR_INVALID;
    if (rc != SFMX_OK) return rc;
    sdn = fdn;
    if (smooth_counts)
      for (int q = 0; q < 5; q++) smooth_counts[q] = counts[q];
  } else if (smooth && nf > 0) {
    if (!clean) {
      sv.resize((size_t)nv * 3);
      sn.resize(app ? (size_t)nv * 3 : 0);
      sf.resize((size_t)nf * 3);
      rc = app ? sfmx_fusion_extract_normals(ctx, g.fu, sv.data(), nv, sf.data(), nf, sn.data(), &nv, &nf)
               : sfmx_fusion_extract(ctx, g.fu, sv.data(), nv, sf.data(), nf, &nv, &nf);
      if (rc != SFMX_OK) return rc;
    }
    rc = sfmx_smooth_create(ctx, &g.ta);
    if (rc == SFMX_OK) rc = clean ? sfmx_smooth_clean(ctx, g.ta, g.cl, smooth) : sfmx_smooth_fusion(ctx, g.ta, g.fu, smooth);
    int counts[5] = {};
    if (rc == SFMX_OK) rc = sfmx_smooth_counts(g.ta, &counts[0], &counts[1], &counts[2], &counts[3], &counts[4]);
    int snf = 0;
    if (rc == SFMX_OK && (sfmx_smooth_device_mesh(g.ta, &sdv, &sdf, &snf) != nv || snf != nf)) rc = SFMX_ERR_INVALID;
    if (rc == SFMX_OK && app) {
      const double* tmp = nullptr;
      if (sfmx_smooth_device_surface(g.ta, &tmp, &sdn) != nv || !sdn) rc = SFMX_ERR_INVALID;
    }
    if (rc != SFMX_OK) return rc;
    if (smooth_counts)
      for (int q = 0; q < 5; q++) smooth_counts[q] = counts[q];
  }
  const bool smoothed = g.ta != nullptr;
  if (simplify && nf > 0) {
    // the cleaned surface lies inside the clean object; an uncleaned one is extracted with its arrays so that it lies inside
    // the volume object (the extraction always returns them to the host as well); a smoothed one lies inside the smooth object
    const int nv0 = nv, nf0 = nf;
    if (!clean && !smoothed && !filled) {
      std::vector<double> tv((size_t)nv * 3), tn(app ? (size_t)nv * 3 : 0);
      std::vector<int32_t> tf((size_t)nf * 3);
      rc = app ? sfmx_fusion_extract_normals(ctx, g.fu, tv.data(), nv, tf.data(), nf, tn.data(), &nv, &nf)
               : sfmx_fusion_extract(ctx, g.fu, tv.data(), nv, tf.data(), nf, &nv, &nf);
      if (rc != SFMX_OK) return rc;
    }
    rc = sfmx_simplify_create(ctx, &g.sm);
    if (rc == SFMX_OK)
      rc = smoothed ? sfmx_simplify_run(ctx, g.sm, sdv, sdn, nv0, sdf, nf0, 1, simplify, &nv, &nf)
           : filled ? sfmx_simplify_run(ctx, g.sm, fdv, fdn, nv0, fdf, nf0, 1, simplify, &nv, &nf)
           : clean  ? sfmx_simplify_clean(ctx, g.sm, g.cl, simplify, &nv, &nf)
                    : sfmx_simplify_fusion(ctx, g.sm, g.fu, simplify, &nv, &nf);
    int counts[3] = {};
    if (rc == SFMX_OK) rc = sfmx_simplify_counts(g.sm, &counts[0], &counts[1], &counts[2], nullptr, nullptr);
    if (rc != SFMX_OK) return rc;
    if (simplify_counts) {
      for (int q = 0; q < 3; q++) simplify_counts[q] = counts[q];
      simplify_counts[3] = nv0;
      simplify_counts[4] = nf0;
    }
  }
  const bool simplified = g.sm != nullptr;
  if (nf > 0) {
    res->verts = static_cast<double*>(std::malloc((size_t)nv * 3 * sizeof(double)));
    res->faces = static_cast<int32_t*>(std::malloc((size_t)nf * 3 * sizeof(int32_t)));
    if (app) {
      res->normals = static_cast<double*>(std::malloc((size_t)nv * 3 * sizeof(double)));
      res->grey = static_cast<uint8_t*>(std::malloc((size_t)nv));
      res->views = static_cast<int32_t*>(std::malloc((size_t)nv * sizeof(int32_t)));
    }
    if (!res->verts || !res->faces || (app && (!res->normals || !res->grey || !res->views))) {
      const int keep = res->n_views;
      sfmx_host_fusion_free_ex(res);
      res->n_views = keep;
      return SFMX_ERR_INVALID;
    }
    if (simplified) {
      rc = sfmx_simplify_read(ctx, g.sm, res->verts, res->normals, res->faces, nullptr, nullptr, nullptr);
      if (rc == SFMX_OK && app) {  // the simplified vertices are shaded with their own normals
        const double *dv = nullptr, *dn = nullptr;
        rc = sfmx_simplify_device_surface(g.sm, &dv, &dn) == nv && dn ? SFMX_OK : SFMX_ERR_INVALID;
        if (rc == SFMX_OK) rc = sfmx_shade_vertices(ctx, g.sh, dv, dn, nv, 1, &ap, res->grey, res->views);
      }
    } else if (smoothed) {
      rc = sfmx_smooth_read(ctx, g.ta, res->verts, nullptr);
      if (rc == SFMX_OK && filled) rc = sfmx_fill_read(ctx, g.fl, nullptr, res->normals, res->faces);
      if (rc == SFMX_OK && !filled && clean) rc = sfmx_clean_read(ctx, g.cl, nullptr, res->normals, res->faces, nullptr, nullptr, nullptr, nullptr);
      if (rc == SFMX_OK && !filled && !clean) {
        std::memcpy(res->faces, sf.data(), (size_t)nf * 3 * sizeof(int32_t));
        if (app) std::memcpy(res->normals, sn.data(), (size_t)nv * 3 * sizeof(double));
      }
      // the smoothed vertices are shaded with the normals they had
      if (rc == SFMX_OK && app) rc = sfmx_shade_vertices(ctx, g.sh, sdv, sdn, nv, 1, &ap, res->grey, res->views);
    } else if (filled) {
      rc = sfmx_fill_read(ctx, g.fl, res->verts, res->normals, res->faces);
      // the filled vertices are shaded with the fill object's normals: a new vertex with the normal its loop gave it
      if (rc == SFMX_OK && app) rc = sfmx_shade_vertices(ctx, g.sh, fdv, fdn, nv, 1, &ap, res->grey, res->views);
    } else if (clean) {
      rc = sfmx_clean_read(ctx, g.cl, res->verts, res->normals, res->faces, nullptr, nullptr, nullptr, nullptr);
      if (rc == SFMX_OK && app) {  // per vertex: the uncleaned shading gathered by vert_src
        const double *dv = nullptr, *dn = nullptr;
        rc = sfmx_clean_device_surface(g.cl, &dv, &dn) == nv ? SFMX_OK : SFMX_ERR_INVALID;
        if (rc == SFMX_OK) rc = sfmx_shade_vertices(ctx, g.sh, dv, dn, nv, 1, &ap, res->grey, res->views);
      }
    } else if (app) {
      rc = sfmx_fusion_extract_normals(ctx, g.fu, res->verts, nv, res->faces, nf, res->normals, &nv, &nf);
      if (rc == SFMX_OK) rc = sfmx_shade_fusion(ctx, g.sh, g.fu, &ap, res->grey, res->views);
    } else {
      rc = sfmx_fusion_extract(ctx, g.fu, res->verts, nv, res->faces, nf, &nv, &nf);
    }
    if (rc != SFMX_OK) {
      const int keep = res->n_views;
      sfmx_host_fusion_free_ex(res);
      res->n_views = keep;
      return rc;
    }
    res->n_verts = nv;
    res->n_faces = nf;
  }
  // visibility runs on the final mesh, fed from the result arrays (the same bytes as the device copy the last stage left: a run
  // takes its arrays from one side, and a smoothed mesh keeps its normals in another object than its vertices).  The culled mesh
  // replaces the result arrays in place and lies inside the visib object for the evaluation below.
  bool culled = false;
  if (visib && nf > 0) {
    const int nv0 = nv, nf0 = nf;
    visib->n_in = nv0;
    visib->m_in = nf0;
    rc = sfmx_visib_run(ctx, g.vb, res->verts, app ? res->normals : nullptr, nv0, res->faces, nf0, 0, &vp);
    if (rc == SFMX_OK) rc = sfmx_visib_sizes(g.vb, nullptr, nullptr, &nv, &nf);
    if (rc == SFMX_OK) rc = sfmx_visib_counts(g.vb, visib->counts, visib->pairs);
    std::vector<double> cv, cn;
    std::vector<int32_t> cf, vsrc, vc;
    std::vector<uint8_t> vg;
    if (rc == SFMX_OK) {
      visib->face_views = static_cast<int32_t*>(std::malloc((size_t)nf0 * sizeof(int32_t)));
      visib->face_back_views = static_cast<int32_t*>(std::malloc((size_t)nf0 * sizeof(int32_t)));
      visib->vert_views = static_cast<int32_t*>(std::malloc((size_t)nv0 * sizeof(int32_t)));
      if (!visib->face_views || !visib->face_back_views || !visib->vert_views) rc = SFMX_ERR_INVALID;
    }
    if (rc == SFMX_OK) {
      cv.resize((size_t)nv * 3);
      cn.resize(app ? (size_t)nv * 3 : 0);
      cf.resize((size_t)nf * 3);
      vsrc.resize((size_t)nv);
      if (visib->colour) {
        vg.resize((size_t)nv0);
        vc.resize((size_t)nv0);
      }
      rc = sfmx_visib_read(ctx, g.vb, cv.data(), app ? cn.data() : nullptr, cf.data(), vsrc.data(), nullptr, visib->face_views,
                           visib->face_back_views, visib->vert_views, visib->colour ? vg.data() : nullptr,
                           visib->colour ? vc.data() : nullptr);
    }
    if (rc != SFMX_OK) {
      const int keep = res->n_views;
      sfmx_host_fusion_free_ex(res);
      res->n_views = keep;
      sfmx_host_visib_free(visib);
      sfmx_host_texture_free(texture);
      sfmx_host_level_free(level);
      sfmx_host_photo_free(photo);
      return rc;
    }
    if (nf == 0) {  // nothing left: as a volume without a surface
      const int keep = res->n_views;
      sfmx_host_fusion_free_ex(res);
      res->n_views = keep;
      nv = 0;
    } else {
      std::memcpy(res->verts, cv.data(), (size_t)nv * 3 * sizeof(double));
      std::memcpy(res->faces, cf.data(), (size_t)nf * 3 * sizeof(int32_t));
      if (app) {
        std::memcpy(res->normals, cn.data(), (size_t)nv * 3 * sizeof(double));
        // vert_src ascends and vert_src[i] >= i: the gather can run in place
        for (int i = 0; i < nv; i++) {
          const size_t s = (size_t)vsrc[(size_t)i];
          res->grey[i] = visib->colour ? vg[s] : res->grey[s];
          res->views[i] = visib->colour ? vc[s] : res->views[s];
        }
      }
      res->n_verts = nv;
      res->n_faces = nf;
    }
    culled = true;
  }
  // the texture is baked for the final mesh, the one in the result arrays and the PLY, fed from those arrays
  if (texture && nf > 0) {
    rc = sfmx_texture_run(ctx, g.tx, res->verts, nv, res->faces, nf, 0, &xp);
    int W = 0, H = 0, V = 0;
    if (rc == SFMX_OK) rc = sfmx_texture_sizes(g.tx, nullptr, nullptr, &V, &W, &H);
    if (rc == SFMX_OK) rc = sfmx_texture_counts(g.tx, texture->counts);
    if (rc == SFMX_OK) {
      texture->n_faces = nf;
      texture->n_views = V;
      texture->atlas = static_cast<uint8_t*>(std::malloc((size_t)W * (size_t)H + 1));
      texture->face_view = static_cast<int32_t*>(std::malloc((size_t)nf * sizeof(int32_t)));
      texture->face_area = static_cast<int64_t*>(std::malloc((size_t)nf * sizeof(int64_t)));
      texture->uv_half = static_cast<int32_t*>(std::malloc((size_t)nf * 6 * sizeof(int32_t)));
      texture->view_faces = static_cast<int32_t*>(std::malloc((size_t)(V > 0 ? V : 1) * sizeof(int32_t)));
      if (!texture->atlas || !texture->face_view || !texture->face_area || !texture->uv_half || !texture->view_faces) rc = SFMX_ERR_INVALID;
    }
    if (rc == SFMX_OK)
      rc = sfmx_texture_read(ctx, g.tx, texture->atlas, texture->face_view, texture->face_area, texture->uv_half, texture->view_faces);
    // the seams are levelled on the same mesh, from the texture object as the run left it
    if (rc == SFMX_OK && level) {
      rc = sfmx_level_run(ctx, g.lv, g.tx, res->verts, nv, res->faces, nf, 0, &level->params);
      if (rc == SFMX_OK) rc = sfmx_level_counts(g.lv, level->counts);
      if (rc == SFMX_OK) {
        level->n_faces = nf;
        level->n_verts = nv;
        level->atlas = static_cast<uint8_t*>(std::malloc((size_t)W * (size_t)H + 1));
        level->corner_adj = static_cast<int32_t*>(std::malloc((size_t)nf * 3 * sizeof(int32_t)));
        level->corner_sample = static_cast<int32_t*>(std::malloc((size_t)nf * 3 * sizeof(int32_t)));
        level->vertex_views = static_cast<int32_t*>(std::malloc((size_t)(nv > 0 ? nv : 1) * sizeof(int32_t)));
        if (!level->atlas || !level->corner_adj || !level->corner_sample || !level->vertex_views) rc = SFMX_ERR_INVALID;
      }
      if (rc == SFMX_OK) rc = sfmx_level_read(ctx, g.lv, level->atlas, level->corner_adj, level->corner_sample, level->vertex_views);
    }
    // the textured mesh is rendered back into the texture's own views, from the atlas the caller will see
    if (rc == SFMX_OK && photo) {
      int Q = 0, px = 0;
      rc = sfmx_photo_add_texture_views(ctx, g.ph, g.tx);
      if (rc == SFMX_OK) rc = sfmx_photo_run(ctx, g.ph, g.tx, level ? g.lv : nullptr, res->verts, nv, res->faces, nf, 0, &pp);
      if (rc == SFMX_OK) rc = sfmx_photo_sizes(g.ph, &Q, &px);
      if (rc == SFMX_OK && (Q != V || (long long)px != (long long)Q * w * h)) rc = SFMX_ERR_INVALID;
      if (rc == SFMX_OK) {
        const size_t np = (size_t)px + 1, nq = (size_t)(Q > 0 ? Q : 1);
        photo->n_views = Q;
        photo->w = w;
        photo->h = h;
        photo->rendered = static_cast<uint8_t*>(std::malloc(np));
        photo->cls = static_cast<uint8_t*>(std::malloc(np));
        photo->face = static_cast<int32_t*>(std::malloc(np * sizeof(int32_t)));
        photo->classes = static_cast<int64_t*>(std::malloc(nq * 5 * sizeof(int64_t)));
        photo->stats = static_cast<int64_t*>(std::malloc(nq * 6 * sizeof(int64_t)));
        photo->hist = static_cast<int64_t*>(std::malloc(nq * 512 * sizeof(int64_t)));
        if (!photo->rendered || !photo->cls || !photo->face || !photo->classes || !photo->stats || !photo->hist) rc = SFMX_ERR_INVALID;
      }
      if (rc == SFMX_OK) rc = sfmx_photo_read(ctx, g.ph, photo->rendered, photo->cls, photo->face, photo->classes, photo->stats, photo->hist);
    }
    if (rc != SFMX_OK) {
      const int keep = res->n_views;
      sfmx_host_fusion_free_ex(res);
      res->n_views = keep;
      sfmx_host_visib_free(visib);
      sfmx_host_texture_free(texture);
      sfmx_host_level_free(level);
      sfmx_host_photo_free(photo);
      return rc;
    }
  }
  if (gt) {
    // the final mesh is still on the device (inside the simplify or the clean object, or inside the volume after the last
    // extraction): it is the query set of the accuracy and the target of the completeness, with no host round trip
    const double* mv = nullptr;
    const int32_t* mf = nullptr;
    int mnf = 0;
    const sfmx_sdist_params dp{gt->params.d_max, gt->params.cell};
    const std::vector<double> gq = compact(gt->verts, gt_used);
    std::vector<uint8_t> used;
    std::vector<double> d2((size_t)(nf > 0 ? nv : 0));
    rc = sfmx_sdist_create(ctx, &g.sd);
    if (rc == SFMX_OK && !culled && simplified && nf > 0 && (sfmx_simplify_device_mesh(g.sm, &mv, &mf, &mnf) != nv || mnf != nf))
      rc = SFMX_ERR_INVALID;
    const bool own = culled || simplified || smoothed || filled;  // the final mesh is handed over as device pointers
    if (culled) {  // the culled mesh lies inside the visib object
      int cnv = 0;
      if (rc == SFMX_OK && nf > 0 && (sfmx_visib_device_mesh(g.vb, &mv, &mf, &cnv, &mnf) != nv || mnf != nf)) rc = SFMX_ERR_INVALID;
    } else if (!simplified && smoothed) {
      mv = sdv;
      mf = sdf;
    } else if (!simplified && filled) {
      mv = fdv;
      mf = fdf;
    }
    if (rc == SFMX_OK) rc = sfmx_sdist_set_target(ctx, g.sd, gt->verts, gt->n_verts, gt->faces, gt->n_faces, 0, &dp);
    if (rc == SFMX_OK && nf > 0) {
      rc = used_mask(res->faces, nf, nv, used) ? SFMX_OK : SFMX_ERR_INVALID;
      if (rc == SFMX_OK)
        rc = own ? sfmx_sdist_query(ctx, g.sd, mv, nv, 1, d2.data(), nullptr)
             : clean    ? sfmx_sdist_query_clean(ctx, g.sd, g.cl, nv, d2.data(), nullptr, nullptr)
                        : sfmx_sdist_query_fusion(ctx, g.sd, g.fu, nv, d2.data(), nullptr, nullptr);
    }
    if (rc == SFMX_OK) {
      eval_side(d2, &used, gt->params, &ev->n_rec, &ev->acc_within, &ev->accuracy, &ev->acc_mean, &ev->acc_max);
      d2.assign(gq.size() / 3, 0.0);
      if (nf == 0)
        rc = sfmx_sdist_set_target(ctx, g.sd, nullptr, 0, nullptr, 0, 0, &dp);
      else
        rc = own ? sfmx_sdist_set_target(ctx, g.sd, mv, nv, mf, nf, 1, &dp)
             : clean    ? sfmx_sdist_set_target_clean(ctx, g.sd, g.cl, &dp)
                        : sfmx_sdist_set_target_fusion(ctx, g.sd, g.fu, &dp);
    }
    if (rc == SFMX_OK) rc = sfmx_sdist_query(ctx, g.sd, gq.data(), (int)d2.size(), 0, d2.data(), nullptr);
    if (rc != SFMX_OK) {
      const int keep = res->n_views;
      sfmx_host_fusion_free_ex(res);
      res->n_views = keep;
      *ev = sfmx_surface_eval_result{};
      sfmx_host_visib_free(visib);
      sfmx_host_texture_free(texture);
      sfmx_host_level_free(level);
      sfmx_host_photo_free(photo);
      return rc;
    }
    eval_side(d2, nullptr, gt->params, &ev->n_gt, &ev->comp_within, nullptr, nullptr, nullptr);
    eval_finish(ev);
  }
  if (render && render->n_cameras > 0) {
    // the volume is untouched by the stages above; a failed render frees the mesh like any other failure
    rc = sfmx_raycast_create(ctx, &g.rc);
    for (int q = 0; rc == SFMX_OK && q < render->n_cameras; q++) {
      sfmx_render_out& o = render->out[q];
      rc = sfmx_raycast_render(ctx, g.rc, g.fu, &render->cameras[q], &render->params);
      if (rc == SFMX_OK) rc = sfmx_raycast_read(ctx, g.rc, o.depth, o.normals, o.points, o.shaded, &o.hits);
      if (rc == SFMX_OK && app && (o.grey || o.views)) rc = sfmx_raycast_shade(ctx, g.rc, g.sh, &ap, o.grey, o.views);
    }
    if (rc != SFMX_OK) {
      const int keep = res->n_views;
      sfmx_host_fusion_free_ex(res);
      res->n_views = keep;
      if (gt) *ev = sfmx_surface_eval_result{};
      sfmx_host_visib_free(visib);
      sfmx_host_texture_free(texture);
      sfmx_host_level_free(level);
      sfmx_host_photo_free(photo);
      return rc;
    }
  }
  if (raster && raster->n_cameras > 0) {
    // the final mesh, the one in the result arrays and the PLY, with the appearance normals and grey when they were made.  The
    // grey exists on the host only (the shade stage returns it there) and a run takes its arrays from one side, so the mesh is
    // fed from the result arrays: the same bytes as the device copy the last stage left.  A surface without faces renders the
    // background.
    rc = sfmx_raster_create(ctx, &g.rs);
    for (int q = 0; rc == SFMX_OK && q < raster->n_cameras; q++) {
      sfmx_raster_out& o = raster->out[q];
      const bool attrs = app && nf > 0;  // a surface without faces has no appearance arrays: its grey image is the background
      rc = sfmx_raster_run(ctx, g.rs, res->verts, attrs ? res->normals : nullptr, attrs ? res->grey : nullptr, res->n_verts, res->faces,
                           res->n_faces, 0, &raster->cameras[q], &raster->params);
      if (rc == SFMX_OK) rc = sfmx_raster_read(ctx, g.rs, o.depth, o.face, o.points, o.normals, o.shaded, attrs ? o.grey : nullptr);
      if (rc == SFMX_OK && app && !attrs && o.grey)
        std::memset(o.grey, raster->params.background, (size_t)raster->cameras[q].w * (size_t)raster->cameras[q].h);
      if (rc == SFMX_OK) rc = sfmx_raster_counts(g.rs, o.counts, &o.fragments);
    }
    if (rc != SFMX_OK) {
      const int keep = res->n_views;
      sfmx_host_fusion_free_ex(res);
      res->n_views = keep;
      if (gt) *ev = sfmx_surface_eval_result{};
      sfmx_host_visib_free(visib);
      sfmx_host_texture_free(texture);
      sfmx_host_level_free(level);
      sfmx_host_photo_free(photo);
      return rc;
    }
  }
  if (ply_path) {
    if (nf == 0) {
      log += "WARN: fused mesh export skipped (no faces)\n";
    } else if (app) {
      try {
        write_mesh_ply_appearance(ply_path, *res);
      } catch (const std::exception& e) {
        log += std::string("WARN: fused mesh export failed (") + e.what() + ")\n";
      }
    } else {
      std::vector<sfmx_host::V3> vv((size_t)nv);
      for (int i = 0; i < nv; i++) vv[(size_t)i] = sfmx_host::V3{res->verts[3 * i], res->verts[3 * i + 1], res->verts[3 * i + 2]};
      std::vector<std::array<int, 3>> ff((size_t)nf);
      for (int i = 0; i < nf; i++) ff[(size_t)i] = {res->faces[3 * i], res->faces[3 * i + 1], res->faces[3 * i + 2]};
      try {
        sfmx_host::write_mesh_ply(ply_path, vv, ff);
      } catch (const std::exception& e) {
        log += std::string("WARN: fused mesh export failed (") + e.what() + ")\n";
      }
    }
  }
  if (warn && warn_cap > 0) std::snprintf(warn, (size_t)warn_cap, "%s", log.c_str());
  return SFMX_OK;
}

}  // extern "C"
