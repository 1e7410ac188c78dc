// sfmx_sdist_math.h — squared point-segment and point-triangle distance, one fixed sequence of IEEE double
// operations shared by the device kernel and any host check.  Compile with -ffp-contract=off.  tests/sdist_ref.py restates
// every line in NumPy; the tests compare bits.
#pragma once
#include "sfmx_math.h"

namespace sfmx {

SFMX_HD double sd_dot(double x0, double x1, double x2, double y0, double y1, double y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }

// seg(p, a, b): the squared distance from p to the segment a b (a == b: to the point)
SFMX_HD double sd_seg(const double* p, const double* a, const double* b) {
  const double ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
  const double ap0 = p[0] - a[0], ap1 = p[1] - a[1], ap2 = p[2] - a[2];
  const double den = sd_dot(ab0, ab1, ab2, ab0, ab1, ab2);
  const double num = sd_dot(ap0, ap1, ap2, ab0, ab1, ab2);
  const double t = !(num > 0.0) ? 0.0 : (num >= den ? 1.0 : num / den);
  const double e0 = p[0] - (a[0] + t * ab0), e1 = p[1] - (a[1] + t * ab1), e2 = p[2] - (a[2] + t * ab2);
  return sd_dot(e0, e1, e2, e0, e1, e2);
}

// tri(p, a, b, c): the squared distance from p to the triangle a b c; a degenerate triangle (nn == 0) is its segments
SFMX_HD double sd_tri(const double* p, const double* a, const double* b, const double* c) {
  const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];  // b - a
  const double v0 = c[0] - a[0], v1 = c[1] - a[1], v2 = c[2] - a[2];  // c - a
  const double n0 = u1 * v2 - u2 * v1, n1 = u2 * v0 - u0 * v2, n2 = u0 * v1 - u1 * v0;
  const double nn = sd_dot(n0, n1, n2, n0, n1, n2);
  const double pa0 = p[0] - a[0], pa1 = p[1] - a[1], pa2 = p[2] - a[2];
  if (nn > 0.0) {
    const double s1 = sd_dot(u1 * pa2 - u2 * pa1, u2 * pa0 - u0 * pa2, u0 * pa1 - u1 * pa0, n0, n1, n2);
    const double w0 = c[0] - b[0], w1 = c[1] - b[1], w2 = c[2] - b[2];  // c - b
    const double pb0 = p[0] - b[0], pb1 = p[1] - b[1], pb2 = p[2] - b[2];
    const double s2 = sd_dot(w1 * pb2 - w2 * pb1, w2 * pb0 - w0 * pb2, w0 * pb1 - w1 * pb0, n0, n1, n2);
    const double x0 = a[0] - c[0], x1 = a[1] - c[1], x2 = a[2] - c[2];  // a - c
    const double pc0 = p[0] - c[0], pc1 = p[1] - c[1], pc2 = p[2] - c[2];
    const double s3 = sd_dot(x1 * pc2 - x2 * pc1, x2 * pc0 - x0 * pc2, x0 * pc1 - x1 * pc0, n0, n1, n2);
    if (s1 >= 0.0 && s2 >= 0.0 && s3 >= 0.0) {
      const double h = sd_dot(pa0, pa1, pa2, n0, n1, n2);
      return (h * h) / nn;
    }
  }
  const double d1 = sd_seg(p, a, b), d2 = sd_seg(p, b, c), d3 = sd_seg(p, c, a);
  const double m = d2 < d1 ? d2 : d1;  // min(min(d1, d2), d3); no operand is ever NaN
  return d3 < m ? d3 : m;
}

}  // namespace sfmx
