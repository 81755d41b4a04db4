/* nvbx_align_math.h -- the f64 arithmetic of one Gauss-Newton step of the pose alignment (SEMANTICS.md "Pose alignment"):
 * the damped 6 x 6 Cholesky solve with its pivot rule, the exponential map of se(3) and the pose update.  Plain C, host and device: the
 * solve launch of align.hip calls these functions, tests/cpp/align_math_check.cpp compiles them with g++.
 *
 * Conventions: a pose is R[9] (row-major 3 x 3) and t[3]; a step is xi = (v, omega); H[21] is the upper triangle of the symmetric 6 x 6
 * normal matrix stored row by row (H[0] = H00 .. H[5] = H05, H[6] = H11 ..), b[6] the gradient; the step solves (H + damping diag(H)) xi = -b. */
#ifndef NVBX_ALIGN_MATH_H_
#define NVBX_ALIGN_MATH_H_
#include <math.h>
#include <stdint.h>

#ifndef NVBX_HD
#if defined(__HIPCC__)
#define NVBX_HD __host__ __device__ inline
#else
#define NVBX_HD static inline
#endif
#endif

#define NVBX_ALIGN_SERIES_BELOW 1e-8      /* theta below this: the series instead of the closed forms */

/* position of entry (i, j), i <= j, in the packed upper triangle */
NVBX_HD int nvbx_align_tri(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

/* Solves (H + damping diag(H)) x = -b by Cholesky (A = L L^T, row by row).  Returns 1, or 0 when a pivot is <= min_pivot_ratio x the
 * largest diagonal entry of H (or is not a number): the problem is degenerate and x is left as it was.  *worst_pivot_ratio (may be
 * NULL) = the smallest pivot met / that largest entry. */
NVBX_HD int nvbx_align_solve6(const double H[21], const double b[6], double damping, double min_pivot_ratio, double x[6], double* worst_pivot_ratio) {
  double A[6][6], L[6][6], y[6];
  double dmax = 0.0;
  for (int i = 0; i < 6; i++) {
    for (int j = i; j < 6; j++) { A[i][j] = H[nvbx_align_tri(i, j)]; A[j][i] = A[i][j]; }
    const double d = A[i][i];
    if (d > dmax) dmax = d;
    A[i][i] = d + damping * d;
  }
  const double floor_ = min_pivot_ratio * dmax;
  double worst = INFINITY;
  int ok = 1;
  for (int k = 0; k < 6 && ok; k++) {
    double p = A[k][k];
    for (int j = 0; j < k; j++) p = p - L[k][j] * L[k][j];
    if (!(p > floor_) || !(p > 0.0)) { ok = 0; worst = (dmax > 0.0 && p == p) ? p / dmax : 0.0; break; }
    if (p / dmax < worst) worst = p / dmax;
    const double l = sqrt(p);
    L[k][k] = l;
    for (int i = k + 1; i < 6; i++) {
      double s = A[i][k];
      for (int j = 0; j < k; j++) s = s - L[i][j] * L[k][j];
      L[i][k] = s / l;
    }
  }
  if (worst_pivot_ratio) *worst_pivot_ratio = worst;
  if (!ok) return 0;
  for (int i = 0; i < 6; i++) {                 /* L y = -b */
    double s = -b[i];
    for (int j = 0; j < i; j++) s = s - L[i][j] * y[j];
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {                /* L^T x = y */
    double s = y[i];
    for (int j = i + 1; j < 6; j++) s = s - L[j][i] * x[j];
    x[i] = s / L[i][i];
  }
  return 1;
}

/* R = exp([w]x) = I + A K + B K^2 (Rodrigues) and V = I + B K + C K^2 with K = [w]x, theta = |w|, A = sin(theta) / theta,
 * B = (1 - cos(theta)) / theta^2 (evaluated as 2 sin^2(theta / 2) / theta^2: no cancellation), C = (theta - sin(theta)) / theta^3;
 * below NVBX_ALIGN_SERIES_BELOW the first two terms of each series. */
NVBX_HD void nvbx_align_exp(const double w[3], double R[9], double V[9]) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double th = sqrt(t2);
  double A, B, Cc;
  if (th < NVBX_ALIGN_SERIES_BELOW) {
    A = 1.0 - t2 / 6.0; B = 0.5 - t2 / 24.0; Cc = 1.0 / 6.0 - t2 / 120.0;
  } else {
    const double s = sin(th), h = sin(0.5 * th);
    A = s / th; B = 2.0 * h * h / t2; Cc = (th - s) / (t2 * th);
  }
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double k2 = w[i] * w[j] - (i == j ? t2 : 0.0);      /* K^2 = w w^T - theta^2 I */
      const double e = i == j ? 1.0 : 0.0;
      R[3 * i + j] = e + A * K[3 * i + j] + B * k2;
      V[3 * i + j] = e + B * K[3 * i + j] + Cc * k2;
    }
}

/* the update of one step xi = (v, omega): R <- exp([omega]x) R, t <- t + V(omega) v */
NVBX_HD void nvbx_align_apply(double R[9], double t[3], const double xi[6]) {
  double E[9], V[9], Rn[9];
  nvbx_align_exp(xi + 3, E, V);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Rn[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
  for (int i = 0; i < 9; i++) R[i] = Rn[i];
  for (int i = 0; i < 3; i++) t[i] = t[i] + ((V[3 * i] * xi[0] + V[3 * i + 1] * xi[1]) + V[3 * i + 2] * xi[2]);
}

#endif /* NVBX_ALIGN_MATH_H_ */
