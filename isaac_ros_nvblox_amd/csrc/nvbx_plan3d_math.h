/* nvbx_plan3d_math.h -- the moves and step costs of the cost volume (SEMANTICS.md "Cost volume and 3-D paths"), one definition for the kernels of
 * plan3d.hip and for host code (plain C: tests/test_plan3d_model.py compiles THIS file with gcc and holds it against the model).  The voxel
 * classes, penalties and option checks are nvbx_plan_math.h's, unchanged. */
#ifndef NVBX_PLAN3D_MATH_H_
#define NVBX_PLAN3D_MATH_H_
#include "nvbx_plan_math.h"

#define NVBX_PLAN3D_MAX_VOXELS (1 << 22)

/* the 26 moves (dx, dy, dz) in the order the path rule tries them: by the number k of nonzero components, then lexicographically with each
 * component ordered +1, 0, -1.  Six along an axis, twelve face diagonals, eight space diagonals. */
#define NVBX_PLAN_MOVES_3D { \
  {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, -1}, {0, -1, 0}, {-1, 0, 0}, \
  {1, 1, 0}, {1, 0, 1}, {1, 0, -1}, {1, -1, 0}, {0, 1, 1}, {0, 1, -1}, {0, -1, 1}, {0, -1, -1}, {-1, 1, 0}, {-1, 0, 1}, {-1, 0, -1}, {-1, -1, 0}, \
  {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}, {-1, 1, 1}, {-1, 1, -1}, {-1, -1, 1}, {-1, -1, -1}}
#define NVBX_PLAN_MOVES_3D_AXIS 6        /* moves [0, 6) have k = 1 */
#define NVBX_PLAN_MOVES_3D_FACE 18       /* moves [6, 18) have k = 2, moves [18, 26) k = 3 */

/* B_k: the base cost of a move with k = 1, 2, 3 nonzero components */
NVBX_PLAN_HD int32_t nvbx_plan3d_base(int k) { return k == 1 ? 10 : k == 2 ? 14 : 17; }
/* the cost of a move with k nonzero components between two traversable voxels with class words kp and kq */
NVBX_PLAN_HD int32_t nvbx_plan3d_step(int k, int32_t kp, int32_t kq) { return nvbx_plan3d_base(k) + kp + kq; }
#endif
