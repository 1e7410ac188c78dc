// stereo.cpp — keyframe-pair stereo mesh on the host: rectification of a posed pair (double, host), the device disparity
// (sfmx_stereo_disparity) and the grid mesh of the Python reference's export_stereo_grid_mesh with an exactly defined depth
// cap.  Not in the reference's C++ (it aliases mesh_stereo to the sparse mesh); DESIGN.md 12 defines every step.
#include "stereo.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

// Weak: a libsfmx.so without the stereo stage (tests/fake_sfmx, the CPU stand-in of the sanitizer builds) still links;
// sfmx_host_stereo_mesh then reports SFMX_ERR_UNSUPPORTED.
#pragma weak sfmx_stereo_check_params
#pragma weak sfmx_stereo_create
#pragma weak sfmx_stereo_destroy
#pragma weak sfmx_stereo_disparity

namespace sfmx_host {
namespace {

void cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
double norm3(const double* a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
// c = a * b (3x3 row-major)
void mul3(const double* a, const double* b, double* c) {
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) c[3 * r + k] = a[3 * r] * b[k] + a[3 * r + 1] * b[3 + k] + a[3 * r + 2] * b[6 + k];
}
void transpose3(const double* a, double* t) {
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) t[3 * k + r] = a[3 * r + k];
}

}  // namespace

std::string stereo_grid_mesh(const int16_t* disp16, int w, int h, const sfmx_stereo_rect& r, const sfmx_stereo_mesh_params& mp,
                             std::vector<double>& verts, std::vector<std::array<int, 3>>& faces) {
  verts.clear();
  faces.clear();
  const size_t n = (size_t)w * h;
  const double fB = r.f * r.B;
  std::vector<double> Z(n, 0.0);
  std::vector<char> ok(n, 0);
  std::vector<double> zs;
  for (size_t p = 0; p < n; p++) {
    const double d = (double)disp16[p] / 16.0;
    if (disp16[p] == -16 || !(d >= mp.disp_min)) continue;
    Z[p] = fB / d;
    ok[p] = 1;
    zs.push_back(Z[p]);
  }
  if (zs.empty()) return "no valid disparity/depth";
  // nearest-rank depth cap: sorted(Z)[ceil(p/100 n) - 1]
  const long long m = (long long)zs.size();
  const long long k = std::min(std::max((long long)std::ceil(mp.z_max_percentile / 100.0 * (double)m), 1LL), m);
  std::nth_element(zs.begin(), zs.begin() + (k - 1), zs.end());
  const double zcap = zs[(size_t)(k - 1)];
  const int step = std::max(1, mp.step);
  const int gw = (w + step - 1) / step, gh = (h + step - 1) / step;
  std::vector<int> vid((size_t)gw * gh, -1);
  for (int yi = 0; yi < gh; yi++)
    for (int xi = 0; xi < gw; xi++) {
      const int x = xi * step, y = yi * step;
      const size_t p = (size_t)y * w + x;
      if (!ok[p] || !(Z[p] <= zcap)) continue;
      const double z = Z[p];
      const double X = (((double)x - r.cx) * z) / r.f;
      const double Y = (((double)y - r.cy) * z) / r.f;
      vid[(size_t)yi * gw + xi] = (int)(verts.size() / 3);
      for (int i = 0; i < 3; i++) verts.push_back(r.R_rw[i] * X + r.R_rw[3 + i] * Y + r.R_rw[6 + i] * z + r.c_left[i]);
    }
  if (verts.size() < 9) {
    verts.clear();
    return "insufficient valid vertices";
  }
  auto disp = [&](int x, int y) { return (double)disp16[(size_t)y * w + x] / 16.0; };
  const double dj = mp.disp_jump;
  for (int yi = 0; yi + 1 < gh; yi++)
    for (int xi = 0; xi + 1 < gw; xi++) {
      const int v00 = vid[(size_t)yi * gw + xi], v01 = vid[(size_t)yi * gw + xi + 1];
      const int v10 = vid[(size_t)(yi + 1) * gw + xi], v11 = vid[(size_t)(yi + 1) * gw + xi + 1];
      if (v00 < 0 || v01 < 0 || v10 < 0 || v11 < 0) continue;
      const int x0 = xi * step, x1 = (xi + 1) * step, y0 = yi * step, y1 = (yi + 1) * step;
      const double d00 = disp(x0, y0), d01 = disp(x1, y0), d10 = disp(x0, y1), d11 = disp(x1, y1);
      if (std::fabs(d00 - d01) > dj || std::fabs(d00 - d10) > dj || std::fabs(d11 - d01) > dj || std::fabs(d11 - d10) > dj) continue;
      faces.push_back({v00, v01, v11});
      faces.push_back({v00, v11, v10});
    }
  if (faces.empty()) {
    verts.clear();
    return "no faces survived filtering";
  }
  return "";
}

}  // namespace sfmx_host

extern "C" {

int sfmx_host_stereo_rectify(const double* K9, const double* pose_a12, const double* pose_b12, int w, int h, sfmx_stereo_rect* out) {
  using namespace sfmx_host;
  if (!K9 || !pose_a12 || !pose_b12 || !out || w <= 0 || h <= 0) return SFMX_ERR_INVALID;
  const double* pa = pose_a12;
  const double* pb = pose_b12;
  double base[3] = {pb[9] - pa[9], pb[10] - pa[10], pb[11] - pa[11]};
  double len = norm3(base);
  if (!(len > 0.0) || !std::isfinite(len)) return SFMX_ERR_INVALID;
  double x[3] = {base[0] / len, base[1] / len, base[2] / len};
  // camera a's x axis in the world is column 0 of its camera->world R
  const bool swapped = x[0] * pa[0] + x[1] * pa[3] + x[2] * pa[6] < 0.0;
  if (swapped) {
    std::swap(pa, pb);
    for (int i = 0; i < 3; i++) base[i] = pb[9 + i] - pa[9 + i];
    len = norm3(base);
    for (int i = 0; i < 3; i++) x[i] = base[i] / len;
  }
  const double zsum[3] = {pa[2] + pb[2], pa[5] + pb[5], pa[8] + pb[8]};  // R_a e_z + R_b e_z
  double y[3], z[3];
  cross(zsum, x, y);
  const double ny = norm3(y);
  if (!(ny > 0.0)) return SFMX_ERR_INVALID;
  for (double& v : y) v /= ny;
  cross(x, y, z);
  sfmx_stereo_rect r{};
  for (int i = 0; i < 3; i++) {
    r.R_rw[i] = x[i];
    r.R_rw[3 + i] = y[i];
    r.R_rw[6 + i] = z[i];
    r.c_left[i] = pa[9 + i];
    r.c_right[i] = pb[9 + i];
  }
  r.f = (K9[0] + K9[4]) / 2.0;
  r.cx = K9[2];
  r.cy = K9[5];
  r.B = len;
  r.swapped = swapped ? 1 : 0;
  const double Kr_inv[9] = {1.0 / r.f, 0.0, -r.cx / r.f, 0.0, 1.0 / r.f, -r.cy / r.f, 0.0, 0.0, 1.0};
  double Rwr[9];  // R_rw^T: rectified -> world
  transpose3(r.R_rw, Rwr);
  double tail[9];
  mul3(Rwr, Kr_inv, tail);
  for (int v = 0; v < 2; v++) {
    const double* pv = v ? pb : pa;
    double Rcw[9], A[9], Kd[9];
    transpose3(pv, Rcw);  // R_v^T: world -> camera
    mul3(Rcw, tail, A);
    std::memcpy(Kd, K9, sizeof Kd);
    mul3(Kd, A, v ? r.H_r : r.H_l);
  }
  *out = r;
  return SFMX_OK;
}

int sfmx_host_stereo_grid_mesh(const int16_t* disp16, int w, int h, const sfmx_stereo_rect* r, const sfmx_stereo_mesh_params* mp,
                               double* verts_out, int verts_cap, int* faces_out, int faces_cap, int* n_faces, char* warn, int warn_cap) {
  if (!disp16 || !r || !mp || w <= 0 || h <= 0) return -SFMX_ERR_INVALID;
  std::vector<double> v;
  std::vector<std::array<int, 3>> f;
  const std::string why = sfmx_host::stereo_grid_mesh(disp16, w, h, *r, *mp, v, f);
  const int nv = (int)(v.size() / 3);
  if (nv > verts_cap || (int)f.size() > faces_cap) return -SFMX_ERR_INVALID;
  if (nv) std::memcpy(verts_out, v.data(), v.size() * sizeof(double));
  for (size_t i = 0; i < f.size(); i++)
    for (int k = 0; k < 3; k++) faces_out[3 * i + k] = f[i][(size_t)k];
  if (n_faces) *n_faces = (int)f.size();
  if (warn && warn_cap > 0) std::snprintf(warn, (size_t)warn_cap, "%s", why.c_str());
  return nv;
}

int sfmx_host_stereo_mesh(sfmx_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int on_device, int w, int h, const double* K9,
                          const double* pose_a12, const double* pose_b12, const sfmx_stereo_params* p, const sfmx_stereo_mesh_params* mp,
                          sfmx_stereo_result* res, char* warn, int warn_cap) {
  if (!ctx || !img_a || !img_b || !p || !mp || !res) return SFMX_ERR_INVALID;
  if (!&sfmx_stereo_disparity) return SFMX_ERR_UNSUPPORTED;
  int rc = sfmx_stereo_check_params(w, h, p);
  if (rc != SFMX_OK) return rc;
  rc = sfmx_host_stereo_rectify(K9, pose_a12, pose_b12, w, h, &res->rect);
  if (rc != SFMX_OK) return rc;
  sfmx_stereo* st = nullptr;
  rc = sfmx_stereo_create(ctx, w, h, p, &st);
  if (rc != SFMX_OK) return rc;
  std::vector<int16_t> own;
  int16_t* d16 = res->disp16;
  if (!d16) {
    own.resize((size_t)w * h);
    d16 = own.data();
  }
  const uint8_t* il = res->rect.swapped ? img_b : img_a;
  const uint8_t* ir = res->rect.swapped ? img_a : img_b;
  rc = sfmx_stereo_disparity(ctx, st, il, ir, on_device, res->rect.H_l, res->rect.H_r, d16, nullptr, nullptr);
  sfmx_stereo_destroy(ctx, st);
  if (rc != SFMX_OK) return rc;
  int nf = 0;
  const int nv = sfmx_host_stereo_grid_mesh(d16, w, h, &res->rect, mp, res->verts, res->verts_cap, res->faces, res->faces_cap, &nf, warn,
                                            warn_cap);
  if (nv < 0) return -nv;
  res->n_verts = nv;
  res->n_faces = nf;
  return SFMX_OK;
}

}  // extern "C"
