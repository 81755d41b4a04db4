// align.hip -- frame-to-model pose refinement against the TSDF (nvbx_align_points / nvbx_align_depth / nvbx_linearize_points;
// SEMANTICS.md "Pose alignment").  [U] KinectFusion's tracking step and voxblox's ICP refinement serve the same request;
// nothing of the kind is readable in the reference tree.
//
// An iteration is two launches in stream order, and nothing waits for another workgroup inside a launch:
//   k_align_accumulate  one lane = one sensor-frame point, grid-stride: transform (apply_rt, f32), the TSDF point query of k_query_points
//                       (q_point, nvbx_query_point.h: the same inline code), then 29 f64 products per valid lane -- 21 of H, 6 of b, the cost and
//                       the count -- summed in the lane, across the wavefront with shuffles, across the workgroup through LDS, all in a fixed
//                       order; one store of 29 doubles into partial slot blockIdx.x.  Grid = min(ceil(n / 256), 256) workgroups of 256: a
//                       function of n alone, so the sums are bit-identical from run to run.
//   k_align_solve       one workgroup: the partials are summed per entry in a fixed order (eight groups of lanes take every eighth slot, then
//                       the groups in order), lane 0 runs the Cholesky solve, the exponential map and the pose update (nvbx_align_math.h),
//                       writes the f64 pose state, the status word and the caller's result record.
// All max_iterations pairs are enqueued up front; the pose of iteration 0 and the options travel as kernel arguments, the pose of the later
// ones is the state the previous solve left.  Once the status is final the remaining launches read it and return at once.
// nvbx_relocalize_* (relocalize.hip) enqueues the same launches behind its selection, which leaves iteration 0's pose -- and a status that may
// already be final -- in the state (AlignArgs::from_state; nvbx_align.h).
// nvbx_align_points_color / nvbx_align_depth_color / nvbx_linearize_points_color (SEMANTICS.md "Colour alignment and colour queries", DESIGN.md
// 2.24) are the same launches with COLOR set: a point with a valid geometric term and a valid colour interpolant (q_color, over the slots q_point
// resolved) adds its colour products into the same H and b, the partial slots hold 31 doubles, and the solve writes the colour record as well.
#include <algorithm>
#include <cmath>
#include "nvbx_align.h"
#include "nvbx_query_point.h"
#include "nvbx_align_math.h"

using namespace nvbx;

constexpr int ALIGN_TERMS = 29;              // H 21, b 6, cost, n_valid
constexpr int ALIGN_COLOR_TERMS = 31;        // ... and in a colour call: colour cost, n_color
constexpr int ALIGN_MAX_WG = 256, ALIGN_TPB = 256;
enum { ALIGN_RUNNING = 0 };
enum { MODE_ALIGN = 0, MODE_LINEARIZE = 1 };

// (AlignState, AlignArgs: nvbx_align.h -- the state's 104 bytes at the front of nvbx_mapper::align_buf)
constexpr size_t ALIGN_PARTIAL_OFFSET = 128;
constexpr size_t ALIGN_BUF_BYTES = ALIGN_PARTIAL_OFFSET + (size_t)ALIGN_MAX_WG * ALIGN_COLOR_TERMS * sizeof(double);

// COLOR (nvbx_*_color): the colour term of a point rides on its geometric one -- q_color over the slots q_point resolved, 27 more
// products into the same H and b, and two further sums.  The COLOR = false instantiations are the plain calls'.
template <bool DEPTH, bool COLOR>
__global__ __launch_bounds__(ALIGN_TPB) void k_align_accumulate(DMap m, AlignArgs a) {
  constexpr int TERMS = COLOR ? ALIGN_COLOR_TERMS : ALIGN_TERMS;
  __shared__ double s_part[ALIGN_TPB / 64][TERMS];
  float R[9], t[3];
  if (a.iter == 0 && !a.from_state) {
    for (int k = 0; k < 9; k++) R[k] = a.R0[k];
    for (int k = 0; k < 3; k++) t[k] = a.t0[k];
  } else {
    if (a.st->status != ALIGN_RUNNING) return;                  // (uniform: the whole grid leaves)
    for (int k = 0; k < 9; k++) R[k] = (float)a.st->R[k];
    for (int k = 0; k < 3; k++) t[k] = (float)a.st->t[k];
  }
  const uint2* pool = reinterpret_cast<const uint2*>(m.tsdf);
  double acc[TERMS];
#pragma unroll
  for (int k = 0; k < TERMS; k++) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.src.n; i += (int64_t)gridDim.x * blockDim.x) {
    float x[3] = {0.0f, 0.0f, 0.0f};
    float ys = 0.0f;
    if (COLOR) { if (!point_source_fetch<DEPTH>(a.src, i, x, &ys)) continue; }
    else if (!point_source_fetch<DEPTH>(a.src, i, x)) continue;
    float p[3], g[3], d;
    uint32_t sl[8];
    apply_rt(R, t, x[0], x[1], x[2], p);
    const bool valid = q_point<Q_TSDF>(m, pool, p, a.vs, a.min_weight, 0.0f, 0, &d, g, nullptr, COLOR ? sl : nullptr);
    float yc = 0.0f, gc[3] = {0.0f, 0.0f, 0.0f};
    bool cvalid = false;
    if (COLOR) {
      // (a point without a geometric term has no colour term: its colour is looked up for the per-point outputs alone)
      if (valid || (!DEPTH && (a.out_cy || a.out_cg || a.out_cv))) cvalid = q_color<false>(m, p, a.vs, a.min_color_weight, sl, &yc, gc, nullptr);
      if (!DEPTH) {
        if (a.out_cy) a.out_cy[i] = yc;
        if (a.out_cg) { a.out_cg[3 * i] = gc[0]; a.out_cg[3 * i + 1] = gc[1]; a.out_cg[3 * i + 2] = gc[2]; }
        if (a.out_cv) a.out_cv[i] = cvalid ? 1 : 0;
      }
    }
    if (!DEPTH) {
      if (a.out_p) { a.out_p[3 * i] = p[0]; a.out_p[3 * i + 1] = p[1]; a.out_p[3 * i + 2] = p[2]; }
      if (a.out_r) a.out_r[i] = d;
      if (a.out_g) { a.out_g[3 * i] = g[0]; a.out_g[3 * i + 1] = g[1]; a.out_g[3 * i + 2] = g[2]; }
      if (a.out_v) a.out_v[i] = valid ? 1 : 0;
    }
    if (!valid) continue;
    const double r = (double)d;
    const double q[3] = {(double)p[0] - (double)t[0], (double)p[1] - (double)t[1], (double)p[2] - (double)t[2]};
    const double gd[3] = {(double)g[0], (double)g[1], (double)g[2]};
    const double J[6] = {gd[0], gd[1], gd[2], q[1] * gd[2] - q[2] * gd[1], q[2] * gd[0] - q[0] * gd[2], q[0] * gd[1] - q[1] * gd[0]};
    const double ar = fabs(r);
    const double w = (a.huber <= 0.0 || ar <= a.huber) ? 1.0 : a.huber / ar;
    double wJ[6];
#pragma unroll
    for (int k = 0; k < 6; k++) wJ[k] = w * J[k];
    int e = 0;
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
      for (int l = k; l < 6; l++) { acc[e] = acc[e] + wJ[k] * J[l]; e++; }
#pragma unroll
    for (int k = 0; k < 6; k++) acc[21 + k] = acc[21 + k] + wJ[k] * r;
    acc[27] = acc[27] + (w * r) * r;
    acc[28] = acc[28] + 1.0;
    if (COLOR && cvalid) {
      // e in levels; kappa = vs / 255 brings residual and Jacobian to the TSDF's scale (a full-range step across one voxel: |kappa gY| = 1)
      const double kappa = (double)a.vs / 255.0;
      const double e_c = (double)yc - (double)ys;
      const double gy[3] = {(double)gc[0], (double)gc[1], (double)gc[2]};
      const double Jr[6] = {gy[0], gy[1], gy[2], q[1] * gy[2] - q[2] * gy[1], q[2] * gy[0] - q[0] * gy[2], q[0] * gy[1] - q[1] * gy[0]};
      const double ae = fabs(e_c);
      const double wc = (a.color_huber <= 0.0 || ae <= a.color_huber) ? 1.0 : a.color_huber / ae;
      const double rc = kappa * e_c, lw = a.color_w * wc;
      double Jc[6], wJc[6];
#pragma unroll
      for (int k = 0; k < 6; k++) { Jc[k] = kappa * Jr[k]; wJc[k] = lw * Jc[k]; }
      int ec = 0;
#pragma unroll
      for (int k = 0; k < 6; k++)
#pragma unroll
        for (int l = k; l < 6; l++) { acc[ec] = acc[ec] + wJc[k] * Jc[l]; ec++; }
#pragma unroll
      for (int k = 0; k < 6; k++) acc[21 + k] = acc[21 + k] + wJc[k] * rc;
      acc[TERMS - 2] = acc[TERMS - 2] + (wc * e_c) * e_c;
      acc[TERMS - 1] = acc[TERMS - 1] + 1.0;
    }
  }
  // wavefront: lane l takes lane l + off, off = 32 .. 1; workgroup: the four wavefronts in order
#pragma unroll
  for (int k = 0; k < TERMS; k++) {
    double v = acc[k];
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
    acc[k] = v;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < TERMS; k++) s_part[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < TERMS) {
    double v = s_part[0][threadIdx.x];
    for (int wv = 1; wv < ALIGN_TPB / 64; wv++) v = v + s_part[wv][threadIdx.x];
    a.partial[(size_t)blockIdx.x * TERMS + threadIdx.x] = v;
  }
}

constexpr int SOLVE_TPB = 256, SOLVE_GROUPS = SOLVE_TPB / 32;
__global__ __launch_bounds__(SOLVE_TPB) void k_align_solve(AlignArgs a) {
  __shared__ double s_grp[SOLVE_GROUPS][32];
  __shared__ double s_sum[32];
  if ((a.iter > 0 || a.from_state) && a.st->status != ALIGN_RUNNING) return;
  // entry j of the partials: group g of 32 lanes takes the slots g, g + 8, .. in order (chains of at most 32 loads instead of one of 256), then the
  // eight groups in order -- a fixed order again
  const int j = threadIdx.x & 31, grp = threadIdx.x >> 5;
  double v = 0.0;
  if (j < a.terms)
    for (int32_t b = grp; b < a.nblocks; b += SOLVE_GROUPS) v = v + a.partial[(size_t)b * a.terms + j];
  s_grp[grp][j] = v;
  __syncthreads();
  if (threadIdx.x < a.terms) {
    double t = s_grp[0][threadIdx.x];
    for (int g = 1; g < SOLVE_GROUPS; g++) t = t + s_grp[g][threadIdx.x];
    s_sum[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double R[9], t[3];
  if (a.iter == 0 && !a.from_state) {
    for (int k = 0; k < 9; k++) R[k] = (double)a.R0[k];
    for (int k = 0; k < 3; k++) t[k] = (double)a.t0[k];
  } else {
    for (int k = 0; k < 9; k++) R[k] = a.st->R[k];
    for (int k = 0; k < 3; k++) t[k] = a.st->t[k];
  }
  nvbx_align_sums cur;
  for (int k = 0; k < 21; k++) cur.H[k] = s_sum[k];
  for (int k = 0; k < 6; k++) cur.b[k] = s_sum[21 + k];
  cur.cost = s_sum[27]; cur.n_valid = (int32_t)s_sum[28]; cur.pad = 0;
  double xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int32_t status = ALIGN_RUNNING;
  if (cur.n_valid < a.min_valid) status = NVBX_ALIGN_TOO_FEW;
  else if (!nvbx_align_solve6(cur.H, cur.b, a.damping, a.min_pivot, xi, nullptr)) { status = NVBX_ALIGN_DEGENERATE; for (int k = 0; k < 6; k++) xi[k] = 0.0; }
  else if (a.mode == MODE_LINEARIZE) status = NVBX_ALIGN_LINEARIZED;
  else {
    nvbx_align_apply(R, t, xi);
    const double nv = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]), nw = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
    if (nv <= a.stop_t && nw <= a.stop_r) status = NVBX_ALIGN_CONVERGED;
    else if (a.iter + 1 >= a.max_iter) status = NVBX_ALIGN_MAX_ITERATIONS;
  }
  for (int k = 0; k < 9; k++) a.st->R[k] = R[k];
  for (int k = 0; k < 3; k++) a.st->t[k] = t[k];
  a.st->status = status; a.st->iterations = a.iter + 1;
  nvbx_align_result* o = a.res;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) { o->T64[4 * i + j] = R[3 * i + j]; o->T_L_S[4 * i + j] = (float)R[3 * i + j]; }
    o->T64[4 * i + 3] = t[i]; o->T_L_S[4 * i + 3] = (float)t[i];
    o->T64[12 + i] = 0.0; o->T_L_S[12 + i] = 0.0f;
  }
  o->T64[15] = 1.0; o->T_L_S[15] = 1.0f;
  for (int k = 0; k < 6; k++) o->step[k] = xi[k];
  if (a.iter == 0) o->first = cur;
  o->last = cur;
  o->iterations = a.iter + 1; o->status = status;
  if (a.color) {
    nvbx_align_color_result* c = a.cres;
    if (a.iter == 0) { c->color_cost_first = s_sum[ALIGN_TERMS]; c->n_color_first = (int32_t)s_sum[ALIGN_TERMS + 1]; }
    c->color_cost_last = s_sum[ALIGN_TERMS]; c->n_color_last = (int32_t)s_sum[ALIGN_TERMS + 1];
  }
}

// the checks of the three entry points, which launch nothing: -> `a` filled but for the buffers.  depth != null: the depth form (pts null), else the
// point form.  T null (nvbx_relocalize_*): iteration 0 takes its pose and its status from the state record.
// what a colour call (nvbx_*_color) hands over beside the plain call's arguments; null: a plain call
struct AlignColorIn {
  const uint8_t* rgb; const nvbx_align_color_options* options; nvbx_align_color_result* res;
  float* out_y; float* out_g; uint8_t* out_v;
};

static int align_check(const char* who, nvbx_mapper* m, const float* pts, int64_t n, const float* depth, int32_t rows, int32_t cols, const nvbx_camera* cam,
                const float T[16], bool from_state, const nvbx_align_options* options, nvbx_align_result* res, int mode, float* out_p, float* out_r,
                float* out_g, uint8_t* out_v, AlignArgs& a, const AlignColorIn* color = nullptr) {
  if (!m) return NVBX_E_INVALID;
  nvbx_align_options o;
  if (options) o = *options; else nvbx_default_align_options(&o);
  if ((!T && !from_state) || !res) return refuse(who, ": the pose and result_dev are required");
  if ((uintptr_t)res & 7) return refuse(who, ": result_dev must be 8-byte aligned");
  if (tsdf_reader_refused(m, who)) return NVBX_E_INVALID;
  if (o.max_iterations < 1 || o.max_iterations > 64) return refuse(who, ": max_iterations must be 1 .. 64");
  if (o.min_valid < 1) return refuse(who, ": min_valid must be >= 1");
  if (!(o.damping >= 0.0) || !(o.min_pivot_ratio >= 0.0) || !(o.stop_translation_m >= 0.0) || !(o.stop_rotation_rad >= 0.0) ||
      !std::isfinite(o.damping) || !std::isfinite(o.min_pivot_ratio) || !std::isfinite(o.stop_translation_m) || !std::isfinite(o.stop_rotation_rad))
    return refuse(who, ": damping, min_pivot_ratio and the stop thresholds must be finite and >= 0");
  if (o.min_weight != o.min_weight || o.huber_delta_m != o.huber_delta_m || o.max_depth_m != o.max_depth_m)
    return refuse(who, ": min_weight / huber_delta_m / max_depth_m is not a number");
  if (!from_state && !nvbx_pose_in_range(T, m->p.voxel_size * 8.0f, 0.0f)) return refuse(who, ": the pose is not finite or out of range");
  a = AlignArgs{};
  if (point_source_check(who, pts, n, depth, rows, cols, cam, o.subsampling, o.max_depth_m, &a.src)) return NVBX_E_INVALID;
  a.from_state = from_state ? 1 : 0;
  if (!from_state) nvbx_pose_unpack(T, a.R0, a.t0);
  a.max_iter = mode == MODE_LINEARIZE ? 1 : o.max_iterations; a.mode = mode; a.min_valid = o.min_valid;
  a.nblocks = (int32_t)std::min<int64_t>((a.src.n + ALIGN_TPB - 1) / ALIGN_TPB, ALIGN_MAX_WG);
  a.vs = m->p.voxel_size; a.min_weight = o.min_weight;
  a.huber = (double)o.huber_delta_m; a.damping = o.damping; a.min_pivot = o.min_pivot_ratio; a.stop_t = o.stop_translation_m; a.stop_r = o.stop_rotation_rad;
  a.res = res; a.out_p = out_p; a.out_r = out_r; a.out_g = out_g; a.out_v = out_v;
  a.terms = ALIGN_TERMS;
  if (color) {
    nvbx_align_color_options c;
    if (color->options) c = *color->options; else nvbx_default_align_color_options(&c);
    if (!color->rgb && (a.src.depth || a.src.n > 0)) return refuse(who, ": the points' colours are required");
    if (!color->res) return refuse(who, ": color_result_dev is required");
    if ((uintptr_t)color->res & 7) return refuse(who, ": color_result_dev must be 8-byte aligned");
    if (!(c.color_weight >= 0.0f) || !std::isfinite(c.color_weight)) return refuse(who, ": color_weight must be finite and >= 0");
    if (c.min_color_weight != c.min_color_weight || c.color_huber_levels != c.color_huber_levels)
      return refuse(who, ": min_color_weight / color_huber_levels is not a number");
    a.src.rgb = color->rgb;
    a.color = 1; a.terms = ALIGN_COLOR_TERMS; a.min_color_weight = c.min_color_weight;
    a.color_w = (double)c.color_weight; a.color_huber = (double)c.color_huber_levels;
    a.cres = color->res; a.out_cy = color->out_y; a.out_cg = color->out_g; a.out_cv = color->out_v;
  }
  return NVBX_OK;
}

int nvbx::align_buffers(nvbx_mapper* m, AlignArgs& a) {
  if (m->align_buf.ensure(m->stream, ALIGN_BUF_BYTES)) return NVBX_E_DEVICE;
  a.st = reinterpret_cast<AlignState*>(m->align_buf.as<unsigned char>());
  a.partial = reinterpret_cast<double*>(m->align_buf.as<unsigned char>() + ALIGN_PARTIAL_OFFSET);
  return NVBX_OK;
}

int nvbx::align_launch(nvbx_mapper* m, AlignArgs& a) {
  NVBX_HIP(hipSetDevice(m->device));
  // reads TSDF voxels and the TSDF flags only: held-back work stays held back, as for the TSDF point query (query.hip).  A colour call reads the
  // colour layer, which a held-back integrateColor writes: that work is carried out first (as for nvbx_query_colors).
  if (a.color ? m->begin_call() : m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  if (align_buffers(m, a)) return NVBX_E_DEVICE;
  for (int32_t it = 0; it < a.max_iter; it++) {
    a.iter = it;
    if (a.nblocks > 0) {
      const dim3 grid((unsigned)a.nblocks), block(ALIGN_TPB);
      if (a.color) {
        if (a.src.depth) NVBX_LAUNCH(m, (k_align_accumulate<true, true>), grid, block, m->d, a);
        else NVBX_LAUNCH(m, (k_align_accumulate<false, true>), grid, block, m->d, a);
      } else if (a.src.depth) NVBX_LAUNCH(m, (k_align_accumulate<true, false>), grid, block, m->d, a);
      else NVBX_LAUNCH(m, (k_align_accumulate<false, false>), grid, block, m->d, a);
    }
    NVBX_LAUNCH(m, k_align_solve, dim3(1), dim3(SOLVE_TPB), a);
    if (a.nblocks == 0) break;      // (an empty cloud: the first solve says TOO_FEW)
  }
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

static int align_run(const char* who, nvbx_mapper* m, const float* pts, int64_t n, const float* depth, int32_t rows, int32_t cols, const nvbx_camera* cam,
              const float T[16], const nvbx_align_options* options, nvbx_align_result* res, int mode, float* out_p, float* out_r, float* out_g,
              uint8_t* out_v, const AlignColorIn* color = nullptr, bool check_only = false) {
  AlignArgs a;
  const int rc = align_check(who, m, pts, n, depth, rows, cols, cam, T, false, options, res, mode, out_p, out_r, out_g, out_v, a, color);
  return rc || check_only ? rc : align_launch(m, a);
}

// nvbx_align_map (surface.hip, described in nvbx_align.h)
int nvbx::align_points_call(const char* who, nvbx_mapper* m, const float* pts, const uint8_t* rgb, int64_t n, const float T[16], const nvbx_align_options* options,
                            bool color, const nvbx_align_color_options* color_options, nvbx_align_result* res, nvbx_align_color_result* cres, bool check_only) {
  const AlignColorIn c{rgb, color_options, cres, nullptr, nullptr, nullptr};
  return align_run(who, m, pts, n, nullptr, 0, 0, nullptr, T, options, res, MODE_ALIGN, nullptr, nullptr, nullptr, nullptr, color ? &c : nullptr, check_only);
}

// nvbx_relocalize_* (relocalize.hip, described in nvbx_align.h), which then calls align_buffers and align_launch itself
int nvbx::align_check_from_state(const char* who, nvbx_mapper* m, const float* pts, int64_t n, const float* depth, int32_t rows, int32_t cols,
                                 const nvbx_camera* cam, const nvbx_align_options* options, nvbx_align_result* res, AlignArgs& a) {
  return align_check(who, m, pts, n, depth, rows, cols, cam, nullptr, true, options, res, MODE_ALIGN, nullptr, nullptr, nullptr, nullptr, a);
}

extern "C" void nvbx_default_align_options(nvbx_align_options* o) {
  if (!o) return;
  o->max_iterations = 10; o->subsampling = 4; o->min_weight = 1e-4f; o->huber_delta_m = 0.0f;
  o->damping = 0.0; o->min_pivot_ratio = 1e-9; o->stop_translation_m = 1e-5; o->stop_rotation_rad = 1e-5;
  o->min_valid = 50; o->max_depth_m = 0.0f;
}

extern "C" int nvbx_align_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const float T_L_S_guess[16], const nvbx_align_options* options,
                                 nvbx_align_result* result_dev) {
  return align_run("nvbx_align_points", m, points_xyz_dev, n, nullptr, 0, 0, nullptr, T_L_S_guess, options, result_dev, MODE_ALIGN, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int nvbx_align_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const float T_L_C_guess[16], const nvbx_camera* camera,
                                const nvbx_align_options* options, nvbx_align_result* result_dev) {
  if (depth_entry_refused("nvbx_align_depth", m, depth_dev, camera)) return NVBX_E_INVALID;
  return align_run("nvbx_align_depth", m, nullptr, 0, depth_dev, rows, cols, camera, T_L_C_guess, options, result_dev, MODE_ALIGN, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int nvbx_linearize_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const float T_L_S[16], const nvbx_align_options* options,
                                     nvbx_align_result* result_dev, float* points_L_dev, float* residual_dev, float* gradient_dev, uint8_t* valid_dev) {
  return align_run("nvbx_linearize_points", m, points_xyz_dev, n, nullptr, 0, 0, nullptr, T_L_S, options, result_dev, MODE_LINEARIZE, points_L_dev, residual_dev,
                   gradient_dev, valid_dev);
}

// ---- the calls with a colour term: the plain calls' checks and launches over an AlignArgs with `color` set
extern "C" void nvbx_default_align_color_options(nvbx_align_color_options* o) {
  if (!o) return;
  o->color_weight = 1.0f; o->min_color_weight = 1e-4f; o->color_huber_levels = 0.0f; o->pad = 0;
}

extern "C" int nvbx_align_points_color(nvbx_mapper* m, const float* points_xyz_dev, const uint8_t* colors_rgb_dev, int64_t n, const float T_L_S_guess[16],
                                       const nvbx_align_options* options, const nvbx_align_color_options* color_options, nvbx_align_result* result_dev,
                                       nvbx_align_color_result* color_result_dev) {
  const AlignColorIn c{colors_rgb_dev, color_options, color_result_dev, nullptr, nullptr, nullptr};
  return align_run("nvbx_align_points_color", m, points_xyz_dev, n, nullptr, 0, 0, nullptr, T_L_S_guess, options, result_dev, MODE_ALIGN, nullptr, nullptr, nullptr,
                   nullptr, &c);
}

extern "C" int nvbx_align_depth_color(nvbx_mapper* m, const float* depth_dev, const uint8_t* color_rgb_dev, int32_t rows, int32_t cols, const float T_L_C_guess[16],
                                      const nvbx_camera* camera, const nvbx_align_options* options, const nvbx_align_color_options* color_options,
                                      nvbx_align_result* result_dev, nvbx_align_color_result* color_result_dev) {
  if (depth_entry_refused("nvbx_align_depth_color", m, depth_dev, camera)) return NVBX_E_INVALID;
  const AlignColorIn c{color_rgb_dev, color_options, color_result_dev, nullptr, nullptr, nullptr};
  return align_run("nvbx_align_depth_color", m, nullptr, 0, depth_dev, rows, cols, camera, T_L_C_guess, options, result_dev, MODE_ALIGN, nullptr, nullptr, nullptr,
                   nullptr, &c);
}

extern "C" int nvbx_linearize_points_color(nvbx_mapper* m, const float* points_xyz_dev, const uint8_t* colors_rgb_dev, int64_t n, const float T_L_S[16],
                                           const nvbx_align_options* options, const nvbx_align_color_options* color_options, nvbx_align_result* result_dev,
                                           nvbx_align_color_result* color_result_dev, float* points_L_dev, float* residual_dev, float* gradient_dev,
                                           uint8_t* valid_dev, float* luminance_dev, float* color_gradient_dev, uint8_t* color_valid_dev) {
  const AlignColorIn c{colors_rgb_dev, color_options, color_result_dev, luminance_dev, color_gradient_dev, color_valid_dev};
  return align_run("nvbx_linearize_points_color", m, points_xyz_dev, n, nullptr, 0, 0, nullptr, T_L_S, options, result_dev, MODE_LINEARIZE, points_L_dev,
                   residual_dev, gradient_dev, valid_dev, &c);
}
