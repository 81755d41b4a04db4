/* nvbx_plan_math.h -- the pixel classes, penalties and step costs of the cost field (SEMANTICS.md "Cost field and paths"), one definition for
 * the kernels of plan.hip and for host code (plain C: tests/test_plan_model.py compiles THIS file with gcc and holds it against the model).
 * All f32 arithmetic is in the order written; the library and the test build with -ffp-contract=off. */
#ifndef NVBX_PLAN_MATH_H_
#define NVBX_PLAN_MATH_H_
#include <math.h>
#include <stdint.h>
#include "../../include/nvblox_hip.h"

#ifdef __HIPCC__
#define NVBX_PLAN_HD __host__ __device__ static inline
#else
#define NVBX_PLAN_HD static inline
#endif

#define NVBX_PLAN_BLOCKED (-1)      /* the class word of a pixel that is not traversable; a traversable pixel's word is its penalty, 0 .. 200 */
#define NVBX_PLAN_MAX_PIXELS (1 << 22)
#define NVBX_PLAN_MAX_PENALTY 200

/* the class word of a pixel with stored value v: NVBX_PLAN_BLOCKED, or the penalty of a traversable pixel */
NVBX_PLAN_HD int32_t nvbx_plan_class(float v, const nvbx_cost_options* o) {
  if (fabsf(v - o->unknown_value) < 1e-2f) return o->allow_unknown ? o->unknown_penalty : NVBX_PLAN_BLOCKED;      /* UNKNOWN: nvbx_occupancy_grid_from_slice's test */
  if (!(v > 0.0f) || !(v >= o->robot_radius_m)) return NVBX_PLAN_BLOCKED;                                           /* (a NaN v fails the first test) */
  const float t = o->inflation_radius_m - v;
  if (!(t > 0.0f)) return 0;
  const float u = o->penalty_per_m * t;
  return !(u < (float)o->max_penalty) ? o->max_penalty : (int32_t)u;      /* (a NaN u, 0 x inf, counts as the largest penalty) */
}

/* the eight moves in the order the path rule tries them: (drow, dcol); the first four run along an axis */
#define NVBX_PLAN_MOVES {{0, 1}, {1, 0}, {0, -1}, {-1, 0}, {1, 1}, {1, -1}, {-1, -1}, {-1, 1}}
/* the cost of a move between two traversable pixels with class words kp and kq */
NVBX_PLAN_HD int32_t nvbx_plan_step(int diagonal, int32_t kp, int32_t kq) { return (diagonal ? 14 : 10) + kp + kq; }

/* why a set of options is refused; NULL = they are fine */
NVBX_PLAN_HD const char* nvbx_plan_options_problem(const nvbx_cost_options* o) {
  if (!(o->robot_radius_m >= 0.0f) || !(o->inflation_radius_m >= 0.0f) || !(o->penalty_per_m >= 0.0f))
    return ": robot_radius_m, inflation_radius_m and penalty_per_m must be numbers >= 0";
  if (o->unknown_value != o->unknown_value) return ": unknown_value is not a number";
  if (o->max_penalty < 0 || o->max_penalty > NVBX_PLAN_MAX_PENALTY || o->unknown_penalty < 0 || o->unknown_penalty > NVBX_PLAN_MAX_PENALTY)
    return ": max_penalty and unknown_penalty must be 0 .. 200";
  return 0;
}
#endif
