// nvbx_feature.h -- what the feature layer's sources share (features.hip: integration and readers; feature_match.hip: scoring): the 16-byte
// chunk type of the value pool and the point -> voxel rule of its readers.  Device code only.
#pragma once
#include "nvbx_projective.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));      // one chunk: 8 channels, 16 bytes

// voxel that contains p: voxel_floor per axis (the renderer's colour rule, nvbx_projective.h); false: not finite / outside the addressable range
__device__ inline bool feature_voxel_of(float px, float py, float pz, float vs, int32_t* g) {
  const float fx = nvbx::voxel_floor(px, vs), fy = nvbx::voxel_floor(py, vs), fz = nvbx::voxel_floor(pz, vs);
  const float L = 8388608.0f;      // 2^20 blocks x 8 voxels
  if (!(fx >= -L && fx < L && fy >= -L && fy < L && fz >= -L && fz < L)) return false;      // (a NaN fails every comparison)
  g[0] = (int32_t)fx; g[1] = (int32_t)fy; g[2] = (int32_t)fz;
  return true;
}
