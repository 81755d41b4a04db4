/* nvbx_merge_math.h -- the host/device arithmetic of map merging that is not per-voxel (SEMANTICS.md "Map merging"): the
 * rotation check, the inverse of T_D_S (f64, rounded to f32 once) and the candidate-block box of one source block.  Plain C, host and
 * device: merge.hip calls these functions on both sides, tests/cpp/merge_math_check.cpp compiles them with g++.
 *
 * Conventions: T is a row-major 4 x 4 (the rigid part is used), R[9] a row-major 3 x 3, p_D = R_DS p_S + t_DS, p_S = R_SD p_D + t_SD.
 * Every expression is evaluated left to right as written, in f64, without contraction. */
#ifndef NVBX_MERGE_MATH_H_
#define NVBX_MERGE_MATH_H_
#include <math.h>
#include <stdint.h>

#ifndef NVBX_HD
#if defined(__HIPCC__)
#define NVBX_HD __host__ __device__ inline
#else
#define NVBX_HD static inline
#endif
#endif

#define NVBX_MERGE_ROTATION_TOL 1e-5      /* largest |R^T R - I| entry a pose may have */
#define NVBX_MERGE_MARGIN_VOX 0.01        /* padding of the candidate box, in voxels */

/* 1 iff the upper-left 3 x 3 of T is a rotation: every entry of R^T R - I within NVBX_MERGE_ROTATION_TOL and det R > 0.  *err (may be
 * NULL) = the largest |entry|, *det (may be NULL) = the determinant. */
NVBX_HD int nvbx_merge_rotation_ok(const float T[16], double* err, double* det) {
  double R[9];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * i + j] = (double)T[4 * i + j];
  double worst = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = R[0 + i] * R[0 + j];
      s = s + R[3 + i] * R[3 + j];
      s = s + R[6 + i] * R[6 + j];
      const double e = fabs(s - (i == j ? 1.0 : 0.0));
      if (!(e <= worst)) worst = e;          /* (a NaN sticks) */
    }
  double d = R[0] * (R[4] * R[8] - R[5] * R[7]);
  d = d - R[1] * (R[3] * R[8] - R[5] * R[6]);
  d = d + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (err) *err = worst;
  if (det) *det = d;
  return worst <= NVBX_MERGE_ROTATION_TOL && d > 0.0;
}

/* T_D_S -> the f32 forward pair {R_DS, t_DS} (the entries of T as they are) and the f32 inverse pair {R_SD, t_SD}: R_SD = R_DS^T (exact),
 * t_SD = -(R_DS^T t_DS) summed in f64 and rounded to f32 once. */
NVBX_HD void nvbx_merge_transforms(const float T[16], float R_DS[9], float t_DS[3], float R_SD[9], float t_SD[3]) {
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) { R_DS[3 * i + j] = T[4 * i + j]; R_SD[3 * j + i] = T[4 * i + j]; } t_DS[i] = T[4 * i + 3]; }
  for (int i = 0; i < 3; i++) {
    double s = (double)R_SD[3 * i + 0] * (double)t_DS[0];
    s = s + (double)R_SD[3 * i + 1] * (double)t_DS[1];
    s = s + (double)R_SD[3 * i + 2] * (double)t_DS[2];
    t_SD[i] = (float)(-s);
  }
}

/* Candidate blocks of source block s[3] in the destination: lo[a] .. hi[a] per axis, at most three blocks each.  The cube of sample
 * positions whose base voxel lies in s is [(8 s + 0.5) vs, (8 s + 8.5) vs) per axis; its eight corners go through {R_DS, t_DS} in f64, their
 * axis-aligned box is padded by NVBX_MERGE_MARGIN_VOX voxels, and a block is a candidate iff one of its voxel centres (k + 0.5) vs lies
 * inside: k from ceil(min / vs - 0.5) to floor(max / vs - 0.5), block = k >> 3.  Returns 0 (and an empty range) if an index leaves the
 * addressable range [-2^20, 2^20) or is not a number. */
NVBX_HD int nvbx_merge_candidate_box(const float R_DS[9], const float t_DS[3], const int32_t s[3], float voxel_size, int32_t lo[3], int32_t hi[3]) {
  const double vs = (double)voxel_size, pad = NVBX_MERGE_MARGIN_VOX * vs;
  double c0[3], c1[3];
  for (int a = 0; a < 3; a++) { c0[a] = (8.0 * (double)s[a] + 0.5) * vs; c1[a] = (8.0 * (double)s[a] + 8.5) * vs; }
  int ok = 1;
  for (int a = 0; a < 3; a++) {
    double mn = INFINITY, mx = -INFINITY;
    for (int q = 0; q < 8; q++) {
      const double x = (q & 1) ? c1[0] : c0[0], y = (q & 2) ? c1[1] : c0[1], z = (q & 4) ? c1[2] : c0[2];
      double v = (double)R_DS[3 * a + 0] * x;
      v = v + (double)R_DS[3 * a + 1] * y;
      v = v + (double)R_DS[3 * a + 2] * z;
      v = v + (double)t_DS[a];
      if (v < mn) mn = v;
      if (v > mx) mx = v;
    }
    const double kl = ceil((mn - pad) / vs - 0.5), kh = floor((mx + pad) / vs - 0.5);
    if (!(kl >= -8388608.0 && kh <= 8388607.0 && kl <= kh)) { ok = 0; lo[a] = 0; hi[a] = -1; continue; }
    lo[a] = (int32_t)kl >> 3; hi[a] = (int32_t)kh >> 3;
  }
  if (!ok) for (int a = 0; a < 3; a++) { lo[a] = 0; hi[a] = -1; }
  return ok;
}

#endif  /* NVBX_MERGE_MATH_H_ */
