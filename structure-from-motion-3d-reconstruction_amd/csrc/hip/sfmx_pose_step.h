// sfmx_pose_step.h — the host side of a Gauss-Newton pose step, shared by align.hip (a view against the volume)
// and palign.hip (a view against the textured mesh): the 6 x 6 Cholesky solve of the 28 ordered sums, the rational (Cayley)
// update of a view about a pivot and the norm of a half of the step.  Host code only; IEEE double in one written order (the
// files that include it are built with -ffp-contract=off); the only library function is sqrt.
#pragma once
#include <cmath>

#include "../../../include/sfmx.h"

namespace {

// (A + damping I) delta = -b by Cholesky, one written order; false when a pivot is <= 0 or not finite
inline bool al_solve(const double* sums, double damping, double* delta) {
  double M[6][6], L[6][6] = {};
  int t = 0;
  for (int m = 0; m < 6; m++)
    for (int n = m; n < 6; n++) M[m][n] = M[n][m] = sums[t++];
  for (int m = 0; m < 6; m++) M[m][m] = M[m][m] + damping;
  const double* b = sums + 21;
  for (int j = 0; j < 6; j++) {
    double d = M[j][j];
    for (int k = 0; k < j; k++) d = d - L[j][k] * L[j][k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < 6; i++) {
      double v = M[i][j];
      for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; i++) {
    double v = -b[i];
    for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {
    double v = y[i];
    for (int k = i + 1; k < 6; k++) v = v - L[k][i] * delta[k];
    delta[i] = v / L[i][i];
  }
  return true;
}

// the Cayley update of the pose about the pivot p
inline void al_update(sfmx_fusion_view* v, const double* p, const double* delta) {
  const double a0 = 0.5 * delta[0], a1 = 0.5 * delta[1], a2 = 0.5 * delta[2];
  const double k = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2));
  double D[3][3];
  D[0][0] = 1.0 - k * (a1 * a1 + a2 * a2);
  D[0][1] = k * (a0 * a1 - a2);
  D[0][2] = k * (a0 * a2 + a1);
  D[1][0] = k * (a0 * a1 + a2);
  D[1][1] = 1.0 - k * (a0 * a0 + a2 * a2);
  D[1][2] = k * (a1 * a2 - a0);
  D[2][0] = k * (a0 * a2 - a1);
  D[2][1] = k * (a1 * a2 + a0);
  D[2][2] = 1.0 - k * (a0 * a0 + a1 * a1);
  for (int r = 0; r < 3; r++) {
    const double r0 = v->R_rw[3 * r], r1 = v->R_rw[3 * r + 1], r2 = v->R_rw[3 * r + 2];
    for (int a = 0; a < 3; a++) v->R_rw[3 * r + a] = (D[a][0] * r0 + D[a][1] * r1) + D[a][2] * r2;
  }
  const double u0 = v->c_left[0] - p[0], u1 = v->c_left[1] - p[1], u2 = v->c_left[2] - p[2];
  for (int a = 0; a < 3; a++) v->c_left[a] = (p[a] + ((D[a][0] * u0 + D[a][1] * u1) + D[a][2] * u2)) + delta[3 + a];
}

// |omega| (d = delta) or |v| (d = delta + 3)
inline double al_norm3(const double* d) { return sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]); }

}  // namespace
