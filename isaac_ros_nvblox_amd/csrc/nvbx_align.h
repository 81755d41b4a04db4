// nvbx_align.h -- what align.hip shares with relocalize.hip, whose launches end in the alignment's: the device state record, the argument block of
// the two alignment kernels, and the three steps of a call over one checked AlignArgs.
#pragma once
#include "nvbx_point_source.h"

namespace nvbx {

struct AlignState { double R[9], t[3]; int32_t status, iterations; };      // 104 bytes, at the front of nvbx_mapper::align_buf; status 0 = running

struct AlignArgs {
  PointSource src;
  float R0[9], t0[3];                                           // the pose of iteration 0 ...
  int32_t from_state;                                           // ... unless set: then an earlier launch left it in *st (relocalize.hip), with the status to start from
  int32_t iter, max_iter, mode, min_valid, nblocks;
  float vs, min_weight;
  double huber, damping, min_pivot, stop_t, stop_r;
  AlignState* st; double* partial; nvbx_align_result* res;
  float* out_p; float* out_r; float* out_g; uint8_t* out_v;     // per-point outputs of nvbx_linearize_points (each may be null)
  // the colour term (nvbx_*_color).  terms = the doubles of a partial slot: 29, or 31 in a colour call (+ colour cost, colour count)
  int32_t color, terms;
  float min_color_weight, pad;
  double color_w, color_huber;                                  // lambda; the Huber threshold in levels (<= 0: none)
  nvbx_align_color_result* cres;
  float* out_cy; float* out_cg; uint8_t* out_cv;                // per-point outputs of nvbx_linearize_points_color (each may be null)
};

// The steps of a call.  nvbx_relocalize_* takes them one by one: its alignment is nvbx_align_points / nvbx_align_depth whose iteration 0 reads the pose
// -- and whether to run at all -- from the state record that a launch of relocalize.hip writes, and every refusal has to come before that launch.
// 1: every refusal of such an alignment; launches nothing, fills `a` but for the buffers
int align_check_from_state(const char* who, nvbx_mapper* m, const float* pts, int64_t n, const float* depth, int32_t rows, int32_t cols,
                           const nvbx_camera* cam, const nvbx_align_options* options, nvbx_align_result* res, AlignArgs& a);
int align_buffers(nvbx_mapper* m, AlignArgs& a);      // 2: a.st, a.partial.  (A growth waits for the stream: before the first launch of a call.)
int align_launch(nvbx_mapper* m, AlignArgs& a);       // 3: every launch of a checked call (it makes sure of the buffers itself)

// nvbx_align_map / nvbx_relocalize_map (surface.hip) have their points only after their first launches, and every refusal has to come before
// those: they make the point call twice.  check_only: the call's refusals for n = 0 (pts and rgb null), nothing is launched; then, with the
// points, the call itself.  who: the name the refusals carry.
// nvbx_align_points, or with `color` nvbx_align_points_color (rgb: the points' colours)
int align_points_call(const char* who, nvbx_mapper* m, const float* pts, const uint8_t* rgb, int64_t n, const float T[16], const nvbx_align_options* options,
                      bool color, const nvbx_align_color_options* color_options, nvbx_align_result* res, nvbx_align_color_result* cres, bool check_only);
// nvbx_relocalize_points (relocalize.hip)
int relocalize_points_call(const char* who, nvbx_mapper* m, const float* pts, int64_t n, const float T0[16], const nvbx_search_lattice* lattice,
                           const nvbx_score_options* score_options, int32_t min_inliers, const nvbx_align_options* align_options, nvbx_pose_score* scores,
                           nvbx_relocalize_result* res, bool check_only);

}  // namespace nvbx
