// fusion.cpp — multi-pair depth fusion on the host: for each pair, rectify (host), disparity (device) and queue the left
// rectified view with its device disparity map; then one integration and one extraction.
#include "fusion.hpp"

#include <array>
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

namespace {

struct Guard {
  sfmx_ctx* ctx;
  sfmx_stereo* st = nullptr;
  sfmx_fusion* fu = nullptr;
  sfmx_shade* sh = nullptr;
  sfmx_consist* cs = nullptr;
  sfmx_clean* cl = nullptr;
  ~Guard() {
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

}  // namespace

extern "C" {

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
  if (!ctx || (n > 0 && (!images || !poses12)) || n < 0 || m < 0 || (m > 0 && !pairs) || !K9 || !sp || !fp || !res)
    return SFMX_ERR_INVALID;
  *res = sfmx_fusion_result_ex{};
  if (warn && warn_cap > 0) warn[0] = 0;
  if (!&sfmx_fusion_create || !&sfmx_stereo_disparity) return SFMX_ERR_UNSUPPORTED;
  if (app && (!&sfmx_shade_create || !&sfmx_fusion_extract_normals)) return SFMX_ERR_UNSUPPORTED;
  if (cs && (!&sfmx_consist_create || !&sfmx_fusion_add_consist_view)) return SFMX_ERR_UNSUPPORTED;
  if (clean && (!&sfmx_clean_create || !&sfmx_clean_fusion || !&sfmx_clean_read || !&sfmx_clean_device_surface || !&sfmx_shade_vertices))
    return SFMX_ERR_UNSUPPORTED;
  int rc = sfmx_stereo_check_params(w, h, sp);
  if (rc != SFMX_OK) return rc;
  rc = sfmx_fusion_check_params(fp);
  if (rc != SFMX_OK) return rc;
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
  std::string log;
  Guard g{ctx};
  rc = sfmx_fusion_create(ctx, fp, &g.fu);
  if (rc != SFMX_OK) return rc;
  if (cs) {
    rc = sfmx_consist_create(ctx, &g.cs);
    if (rc != SFMX_OK) return rc;
  }
  std::vector<int> listed;  // with cs: the listed pair behind each consist view
  if (app) {
    rc = sfmx_shade_create(ctx, &g.sh);
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
    rc = sfmx_stereo_disparity(ctx, g.st, il, ir, on_device, r.H_l, r.H_r, d16.data(), nullptr, nullptr);
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
    // with cs the view waits in the consist object: its filtered map is queued after the loop
    rc = cs ? sfmx_consist_add_stereo_view(ctx, g.cs, &v, g.st) : sfmx_fusion_add_stereo_view(ctx, g.fu, &v, g.st);
    if (rc != SFMX_OK) return rc;
    if (cs) listed.push_back(q);
    if (app) {
      rc = sfmx_shade_add_stereo_view(ctx, g.sh, &v, g.st);
      if (rc != SFMX_OK) return rc;
    }
    res->n_views++;
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
    if (clean) {
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
