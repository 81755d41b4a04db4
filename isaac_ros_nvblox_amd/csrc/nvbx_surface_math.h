/* nvbx_surface_math.h -- the per-edge arithmetic of nvbx_surface_points (surface.hip; SEMANTICS.md "Surface points"), plain
 * inline functions for host and device: which voxel is observed, which edge crosses, where, which origin voxels the box and the stride keep.
 * Every operation is one correctly rounded f32 operation on both sides (nvbx_arith.h, -ffp-contract=off), so tests/cpp/surface_math_check.cpp
 * checks on the host what the kernels compute. */
#ifndef NVBX_SURFACE_MATH_H_
#define NVBX_SURFACE_MATH_H_
#include <stdint.h>
#include "nvbx_arith.h"

#if defined(__HIPCC__)
#define NVBX_SURF_FN __host__ __device__ static inline
#else
#define NVBX_SURF_FN static inline
#endif

/* a stored {d, w} counts: weight at or above the threshold, distance not a NaN (the block's existence is the caller's business) */
NVBX_SURF_FN int nvbx_surface_observed(float d, float w, float min_weight) { return w >= min_weight && d == d; }

/* the edge from an origin voxel {d0, w0} to its neighbour {d1, w1} crosses the surface: both observed, exactly one of them at or below zero */
NVBX_SURF_FN int nvbx_surface_crosses(float d0, float w0, float d1, float w1, float min_weight) {
  return nvbx_surface_observed(d0, w0, min_weight) && nvbx_surface_observed(d1, w1, min_weight) && ((d0 <= 0.0f) != (d1 <= 0.0f));
}

/* centre of voxel v (0 .. 7) of block b along one axis: nvbx_tsdf_zero_crossings' and nvbx_elevation_map's expression (voxel_center) */
NVBX_SURF_FN float nvbx_surface_center(int32_t b, int32_t v, float vs) { return ((float)b * (8.0f * vs) + (float)v * vs) + vs * 0.5f; }

/* the crossing's coordinate along the edge's own axis */
NVBX_SURF_FN float nvbx_surface_crossing(int32_t b, int32_t v, float vs, float d0, float d1) {
  return nvbx_surface_center(b, v, vs) + vs * NVBX_DIV(-d0, d1 - d0);
}

/* g modulo s (s >= 1) with the mathematical sign: 0 .. s - 1 for negative g too */
NVBX_SURF_FN int32_t nvbx_floor_mod(int32_t g, int32_t s) { const int32_t r = g % s; return r < 0 ? r + s : r; }

/* an origin voxel (global coordinates g) passes the filters: inside the inclusive box {min x y z, max x y z} where one is used, and every
 * coordinate a multiple of the stride */
NVBX_SURF_FN int nvbx_surface_origin_kept(int32_t gx, int32_t gy, int32_t gz, int32_t stride, int32_t use_box, const int32_t* box) {
  if (use_box && (gx < box[0] || gx > box[3] || gy < box[1] || gy > box[4] || gz < box[2] || gz > box[5])) return 0;
  if (stride > 1 && (nvbx_floor_mod(gx, stride) | nvbx_floor_mod(gy, stride) | nvbx_floor_mod(gz, stride)) != 0) return 0;
  return 1;
}

/* which endpoint's colour voxel an edge takes: 0 = the origin, 1 = the neighbour (the endpoint nearer the surface; ties: the origin) */
NVBX_SURF_FN int nvbx_surface_color_end(float d0, float d1) { return fabsf(d0) <= fabsf(d1) ? 0 : 1; }

#endif
