/* nvbx_feature_merge_math.h -- the candidate-block box of feature merging (SEMANTICS.md "Feature merging"), beside the
 * merge's (nvbx_merge_math.h), whose transforms, rotation check and margin it shares.  Plain C, host and device: feature_merge.hip calls it
 * on the device, tests/cpp/feature_merge_math_check.cpp compiles it with g++.  Every expression is evaluated left to right as written, in
 * f64, without contraction. */
#ifndef NVBX_FEATURE_MERGE_MATH_H_
#define NVBX_FEATURE_MERGE_MATH_H_
#include "nvbx_merge_math.h"

/* Candidate blocks of source block s[3] in the destination: lo[a] .. hi[a] per axis, at most three blocks each.  The cube of positions whose
 * CONTAINING voxel lies in s is [8 s vs, (8 s + 8) vs) per axis (the sample is the nearest voxel, floor(p / vs): not the merge's cube, which is
 * half a voxel on); its eight corners go through {R_DS, t_DS} in f64, their axis-aligned box is padded by NVBX_MERGE_MARGIN_VOX voxels, and a
 * block is a candidate iff one of its voxel centres (k + 0.5) vs lies inside: k from ceil(min / vs - 0.5) to floor(max / vs - 0.5),
 * block = k >> 3.  The box is at most 8 sqrt(3) + 0.02 voxels wide: at most 14 values of k, three blocks.  Returns 0 (and an empty range) if
 * an index leaves the addressable range [-2^20, 2^20) or is not a number. */
NVBX_HD int nvbx_feature_merge_candidate_box(const float R_DS[9], const float t_DS[3], const int32_t s[3], float voxel_size, int32_t lo[3], int32_t hi[3]) {
  const double vs = (double)voxel_size, pad = NVBX_MERGE_MARGIN_VOX * vs;
  double c0[3], c1[3];
  for (int a = 0; a < 3; a++) { c0[a] = (8.0 * (double)s[a]) * vs; c1[a] = (8.0 * (double)s[a] + 8.0) * vs; }
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

#endif  /* NVBX_FEATURE_MERGE_MATH_H_ */
