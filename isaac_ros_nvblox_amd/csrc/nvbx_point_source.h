// nvbx_point_source.h -- the points of a call that reads a sensor cloud against the map (align.hip, relocalize.hip): either a
// cloud points_xyz_dev[n][3], or the pixels (r s, c s) of a depth image, back-projected inside the launch.  One struct, one host check, one fetch.
#pragma once
#include "nvbx_mapper.h"

namespace nvbx {

// n <= 2^30 in the depth form: image sides are 1 .. 32768 (image_dims_ok, refused below), so point_source_fetch indexes pixels in 32 bits (see pix())
struct PointSource {
  const float* pts;                                             // [n][3], or ...
  const float* depth; int32_t cols, cs, s; float fu, fv, cu, cv, max_d;      // ... the pixels (r s, c s): n = rs x cs of them
  int64_t n;
  const uint8_t* rgb;                                           // null, or the points' colours: [n][3] beside a cloud, [rows][cols][3] rgb8 beside a depth image
};

// The refusals of a point source, in their order; *out is filled where there is none.  depth != null or cam != null: the depth form (pts and n are not
// looked at), else the point form.
inline int point_source_check(const char* who, const float* pts, int64_t n, const float* depth, int32_t rows, int32_t cols, const nvbx_camera* cam,
                              int32_t subsampling, float max_depth_m, PointSource* out) {
  if (depth || cam) {
    if (!depth || !image_dims_ok(rows, cols) || !nvbx_camera_matches(cam, rows, cols)) return refuse(who, ": the depth image and a camera of its size are required");
    if (subsampling < 1) return refuse(who, ": subsampling must be >= 1");
    const int32_t rs = (rows + subsampling - 1) / subsampling, cs = (cols + subsampling - 1) / subsampling;
    out->depth = depth; out->cols = cols; out->cs = cs; out->s = subsampling;
    out->fu = cam->fu; out->fv = cam->fv; out->cu = cam->cu; out->cv = cam->cv; out->max_d = max_depth_m;
    out->n = (int64_t)rs * cs;
  } else {
    if (n < 0 || (n > 0 && !pts)) return refuse(who, ": n points need points_xyz_dev");
    out->pts = pts; out->n = n;
  }
  return NVBX_OK;
}
// what every _depth entry refuses first, ahead of the checks it shares with its _points sibling
inline int depth_entry_refused(const char* who, const void* m, const float* depth, const nvbx_camera* cam) {
  return m && (!depth || !cam) ? refuse(who, ": the depth image and the camera are required") : NVBX_OK;
}

// point i < s.n in the sensor frame -> x; false: a pixel the back-projection does not take (backproject_takes)
template <bool DEPTH>
__device__ inline bool point_source_fetch(const PointSource& s, int64_t i, float x[3]) {
  if (DEPTH) {
    const int32_t ii = (int32_t)i, r = ii / s.cs * s.s, c = ii % s.cs * s.s;
    const float d = s.depth[(int64_t)r * s.cols + c];
    if (!backproject_takes(d, s.max_d)) return false;
    backproject_pixel(r, c, d, s.fu, s.fv, s.cu, s.cv, x);
  } else {
    x[0] = s.pts[3 * i]; x[1] = s.pts[3 * i + 1]; x[2] = s.pts[3 * i + 2];
  }
  return true;
}
// the same with the point's colour (s.rgb must not be null): *ys = the luminance in levels of the point's rgb8 triple -- the depth's pixel in the depth form
template <bool DEPTH>
__device__ inline bool point_source_fetch(const PointSource& s, int64_t i, float x[3], float* ys) {
  if (!point_source_fetch<DEPTH>(s, i, x)) return false;
  int64_t at = i;
  if (DEPTH) { const int32_t ii = (int32_t)i; at = (int64_t)(ii / s.cs * s.s) * s.cols + ii % s.cs * s.s; }
  const uint8_t* c = s.rgb + 3 * at;
  *ys = luma_levels(c[0], c[1], c[2]);
  return true;
}

}  // namespace nvbx
