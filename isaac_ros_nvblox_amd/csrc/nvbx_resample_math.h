/* nvbx_resample_math.h -- the host/device arithmetic of map resampling that is not per-voxel (SEMANTICS.md "Resampling"): the
 * ratio of the two voxel sizes, the tap count and tap offsets, the reach of one destination block in source blocks and the candidate-block
 * box of one source block.  Plain C, host and device: resample.hip calls these functions on both sides,
 * tests/cpp/resample_math_check.cpp compiles them with g++.  The transforms and the rotation check are the merge's (nvbx_merge_math.h).
 *
 * Every expression is evaluated left to right as written, without contraction; f64 unless a cast says otherwise. */
#ifndef NVBX_RESAMPLE_MATH_H_
#define NVBX_RESAMPLE_MATH_H_
#include "nvbx_merge_math.h"

#define NVBX_RESAMPLE_MAX_RATIO 4.0       /* largest voxel_size(dst) / voxel_size(src) */
#define NVBX_RESAMPLE_MAX_TAPS 4          /* sub-samples per axis */

/* r = (double)vs_d / (double)vs_s; 1 iff 1 <= r <= NVBX_RESAMPLE_MAX_RATIO (a NaN or a voxel size <= 0 fails) */
NVBX_HD int nvbx_resample_ratio(float vs_d, float vs_s, double* r) {
  const double q = (double)vs_d / (double)vs_s;
  if (r) *r = q;
  return vs_s > 0.0f && vs_d > 0.0f && q >= 1.0 && q <= NVBX_RESAMPLE_MAX_RATIO;
}

/* sub-samples per axis: `taps` as it is in 1 .. 4; 0 = min(4, ceil(r)); anything else: 0 (refused) */
NVBX_HD int nvbx_resample_taps(double r, int32_t taps) {
  if (taps < 0 || taps > NVBX_RESAMPLE_MAX_TAPS) return 0;
  if (taps) return (int)taps;
  const double c = ceil(r);
  return c >= (double)NVBX_RESAMPLE_MAX_TAPS ? NVBX_RESAMPLE_MAX_TAPS : (c <= 1.0 ? 1 : (int)c);
}

/* offset of tap i of n along one axis, in destination voxels (f32): symmetric about 0, exactly +0 for n = 1 */
NVBX_HD float nvbx_resample_tap_offset(int i, int n) { return ((float)i + 0.5f) / (float)n - 0.5f; }

/* N: source blocks per axis that the corners of one destination block's taps can lie in.  The tap positions span (8 - 1/n) vs_d per axis,
 * under a rotation at most L = sqrt(3) (8 - 1/n) r source voxels; base voxels then differ by at most floor(L) + 1, corners by floor(L) + 2,
 * and voxel indices D apart lie in at most ceil(D / 8) + 1 blocks. */
NVBX_HD int nvbx_resample_reach(double r, int n) {
  const double L = sqrt(3.0) * (8.0 - 1.0 / (double)n) * r;
  return (int)ceil((floor(L) + 2.0) / 8.0) + 1;
}

/* Candidate blocks of source block s[3] in the destination: lo[a] .. hi[a] per axis, at most three blocks each.  nvbx_merge_candidate_box
 * with two voxel sizes: the cube [(8 s + 0.5) vs_s, (8 s + 8.5) vs_s) of the sample positions whose base voxel lies in s goes through
 * {R_DS, t_DS}; the box is padded by NVBX_MERGE_MARGIN_VOX vs_s + 0.5 vs_d (1 - 1/n) -- the second term is how far a tap lies from its
 * voxel's centre -- and a block is a candidate iff one of its voxel centres (k + 0.5) vs_d lies inside.  For vs_d == vs_s, n = 1 every
 * intermediate value is the merge's.  Returns 0 (and an empty range) if an index leaves the addressable range or is not a number. */
NVBX_HD int nvbx_resample_candidate_box(const float R_DS[9], const float t_DS[3], const int32_t s[3], float vs_src, float vs_dst, int n, int32_t lo[3],
                                        int32_t hi[3]) {
  const double vs = (double)vs_src, vd = (double)vs_dst;
  const double pad = NVBX_MERGE_MARGIN_VOX * vs + 0.5 * vd * (1.0 - 1.0 / (double)n);
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
    const double kl = ceil((mn - pad) / vd - 0.5), kh = floor((mx + pad) / vd - 0.5);
    if (!(kl >= -8388608.0 && kh <= 8388607.0 && kl <= kh)) { ok = 0; lo[a] = 0; hi[a] = -1; continue; }
    lo[a] = (int32_t)kl >> 3; hi[a] = (int32_t)kh >> 3;
  }
  if (!ok) for (int a = 0; a < 3; a++) { lo[a] = 0; hi[a] = -1; }
  return ok;
}

#endif  /* NVBX_RESAMPLE_MATH_H_ */
