// nvbx_relocalize_math.h -- the search lattice of nvbx_relocalize_* (include/nvblox_hip.h, SEMANTICS.md "Relocalisation"): its checks, its
// tables and its poses.  Host code, plain C++, no HIP: relocalize.hip makes the tables with it and uploads them, nvbx_search_lattice_poses
// is nvbx_lattice_pose in a loop, and tests/cpp/relocalize_math_check.cpp compiles it with g++ against the numpy tables.
// Everything that involves a cosine is computed here, once, in f64 and rounded once to f32; the device only picks table entries and adds
// three f32 offsets, so a model that follows the header's formulas reproduces every hypothesis bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/nvblox_hip.h"

constexpr int NVBX_LATTICE_MAX_STEPS = 64;
constexpr int64_t NVBX_LATTICE_MAX_POSES = 1 << 20;

// off[a][i]: the offset of step i along axis a (x, y, z), metres; R[w]: Rz(yaw[w]) R0, row-major 3 x 3.  (One upload: the layout is the device's.)
struct nvbx_lattice_tables {
  float off[3][NVBX_LATTICE_MAX_STEPS];
  float R[NVBX_LATTICE_MAX_STEPS][9];
};

// steps 1 .. 64 each (so the product is at most 2^24: no overflow), product <= 2^20, half-extents finite and >= 0
inline bool nvbx_lattice_ok(const nvbx_search_lattice* l) {
  if (!l) return false;
  int64_t k = 1;
  for (int a = 0; a < 4; a++) {
    if (l->steps[a] < 1 || l->steps[a] > NVBX_LATTICE_MAX_STEPS) return false;
    k *= l->steps[a];
  }
  if (k > NVBX_LATTICE_MAX_POSES) return false;
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(l->half_extent_m[a]) || !(l->half_extent_m[a] >= 0.0f)) return false;
  return std::isfinite(l->half_yaw_rad) && l->half_yaw_rad >= 0.0f;
}
inline int64_t nvbx_lattice_count(const nvbx_search_lattice* l) { return (int64_t)l->steps[0] * l->steps[1] * l->steps[2] * l->steps[3]; }

// offset i of s steps over +-half
inline double nvbx_lattice_offset(float half, int32_t i, int32_t s) {
  if (s == 1) return 0.0;
  const double h = (double)half;
  return -h + (2.0 * h * (double)i) / (double)(s - 1);
}

inline void nvbx_lattice_make_tables(const float T0[16], const nvbx_search_lattice* l, nvbx_lattice_tables* t) {
  for (int a = 0; a < 3; a++)
    for (int i = 0; i < NVBX_LATTICE_MAX_STEPS; i++) t->off[a][i] = i < l->steps[a] ? (float)nvbx_lattice_offset(l->half_extent_m[a], i, l->steps[a]) : 0.0f;
  for (int w = 0; w < NVBX_LATTICE_MAX_STEPS; w++) {
    const double yaw = w < l->steps[3] ? nvbx_lattice_offset(l->half_yaw_rad, w, l->steps[3]) : 0.0;
    const double c = std::cos(yaw), s = std::sin(yaw);
    for (int j = 0; j < 3; j++) {
      const double r0 = (double)T0[j], r1 = (double)T0[4 + j], r2 = (double)T0[8 + j];
      const double c0 = c * r0, s1 = s * r1, s0 = s * r0, c1 = c * r1;
      t->R[w][j] = (float)(c0 - s1);
      t->R[w][3 + j] = (float)(s0 + c1);
      t->R[w][6 + j] = (float)r2;
    }
  }
}

// hypothesis h = ((ix ny + iy) nz + iz) nyaw + iw as a row-major 4 x 4 pose
inline void nvbx_lattice_pose(const float T0[16], const nvbx_search_lattice* l, const nvbx_lattice_tables* t, int64_t h, float T[16]) {
  const int32_t iw = (int32_t)(h % l->steps[3]); h /= l->steps[3];
  const int32_t iz = (int32_t)(h % l->steps[2]); h /= l->steps[2];
  const int32_t iy = (int32_t)(h % l->steps[1]); h /= l->steps[1];
  const int32_t ix = (int32_t)h;
  const float o[3] = {t->off[0][ix], t->off[1][iy], t->off[2][iz]};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[4 * i + j] = t->R[iw][3 * i + j];
    T[4 * i + 3] = T0[4 * i + 3] + o[i];
    T[12 + i] = 0.0f;
  }
  T[15] = 1.0f;
}
