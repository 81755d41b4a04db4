/* nvbx_terrain_math.h -- the voxel test of the elevation scan, and the gradient selection and class tests of the traversability call
 * (SEMANTICS.md "Elevation and traversability"), one definition for the kernels of elevation.hip and for host code (plain C:
 * tests/test_elevation_model.py compiles THIS file with gcc and holds it against the model).  All f32 arithmetic is in the order written; the
 * library and the test build with -ffp-contract=off. */
#ifndef NVBX_TERRAIN_MATH_H_
#define NVBX_TERRAIN_MATH_H_
#include <math.h>
#include <stdint.h>
#include "../../include/nvblox_hip.h"
#include "nvbx_arith.h"

#ifdef __HIPCC__
#define NVBX_TERRAIN_HD __host__ __device__ static inline
#else
#define NVBX_TERRAIN_HD static inline
#endif

#define NVBX_ELEV_MAX_PIXELS (1 << 22)
#define NVBX_ELEV_MAX_BAND 1024            /* z_hi - z_lo is below it */
#define NVBX_ELEV_VOXEL_LIMIT (1 << 23)    /* global voxel coordinates: [-2^23, 2^23) = the addressable blocks times 8 */
#define NVBX_TERRAIN_MAX_RADIUS 32

/* a stored voxel {d, w} of an allocated TSDF block is OBSERVED (a NaN weight or distance is not) */
NVBX_TERRAIN_HD int nvbx_elev_observed(float d, float w, float min_weight) { return w >= min_weight && d == d; }

/* one component of the height gradient at a known pixel: hm / h / hp = the heights left of, at and right of it (above / at / below for
 * rows), km / kp = whether those two neighbours exist and are known */
NVBX_TERRAIN_HD float nvbx_terrain_grad(int km, int kp, float hm, float h, float hp, float vs) {
  if (km && kp) return NVBX_DIV(hp - hm, 2.0f * vs);
  if (kp) return NVBX_DIV(hp - h, vs);
  if (km) return NVBX_DIV(h - hm, vs);
  return 0.0f;
}

/* the class of a pixel with `status`; step, slope2 and n_known are read for a SURFACE pixel only */
NVBX_TERRAIN_HD uint8_t nvbx_terrain_class(uint8_t status, float step, float slope2, int n_known, const nvbx_terrain_options* o) {
  if (status == NVBX_ELEV_BLOCKED) return NVBX_TERRAIN_HAZARD;
  if (status == NVBX_ELEV_VOID) return o->void_is_hazard ? NVBX_TERRAIN_HAZARD : NVBX_TERRAIN_UNKNOWN;
  if (status != NVBX_ELEV_SURFACE) return NVBX_TERRAIN_UNKNOWN;
  if (!(step <= o->max_step_m) || !(slope2 <= o->max_slope_tan * o->max_slope_tan) || n_known < o->min_known) return NVBX_TERRAIN_HAZARD;
  return NVBX_TERRAIN_OK;
}

/* why a set of options is refused; NULL = they are fine */
NVBX_TERRAIN_HD const char* nvbx_terrain_options_problem(const nvbx_terrain_options* o) {
  if (!(o->max_step_m >= 0.0f) || !(o->max_slope_tan >= 0.0f)) return ": max_step_m and max_slope_tan must be numbers >= 0";
  if (o->unknown_value != o->unknown_value) return ": unknown_value is not a number";
  if (o->min_known < 1 || o->min_known > 9) return ": min_known must be 1 .. 9";
  if (o->distance_radius_px < 0 || o->distance_radius_px > NVBX_TERRAIN_MAX_RADIUS) return ": distance_radius_px must be 0 .. 32";
  return 0;
}
#endif
