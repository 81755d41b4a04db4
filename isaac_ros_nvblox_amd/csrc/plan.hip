// plan.hip -- which goal can be reached and how far the drive is (SEMANTICS.md "Cost field and paths"): nvbx_cost_field turns a
// distance image (the ESDF slice) and a set of source pixels into the integer cost-to-go field, nvbx_trace_paths walks down such a field.  Both read
// the image only; the classes and step costs are nvbx_plan_math.h's, shared with the host.
//
// The field is the fixed point of a relaxation over 32 x 32 pixel tiles; no workgroup ever waits for another, every loop is bounded.
// k_plan_classify: a workgroup per tile writes the class word of its pixels (NVBX_PLAN_BLOCKED or the penalty), fills its part of the field with
//   UNREACHED, then goes through the source list, sets the accepted sources that lie in its tile to 0 and writes both of its active flags.
// k_plan_relax: one round.  A workgroup whose tile is not active ends after one byte load.  An active one loads the tile's costs and class words
//   with a one-pixel halo into LDS (9.2 KB), pulls min(G(q) + c(p, q)) over the eight neighbours, in place, until a sweep changes nothing or the
//   sweep limit is hit, and stores the pixels that fell.  A changed pixel on the rim marks the up to three neighbouring tiles that hold it in their
//   halo active for the next round (plain byte stores into the other of two flag sets); a tile cut off by the limit marks itself.  A workgroup
//   that changed anything adds one to the counter the host reads once per batch of rounds.
//   Every stored value is the cost of a real move sequence and values only fall, so a halo read before or after a neighbour's store of the same
//   round is a valid bound either way, and that store re-activates the reader (DESIGN.md 2.21 has the argument in full).
// k_plan_trace: a lane per start, the path rule of the header.
#include <algorithm>
#include <cmath>
#include "nvbx_mapper.h"
#include "nvbx_plan_math.h"

using namespace nvbx;

constexpr int PL_T = 32;                  // tile side in pixels
constexpr int PL_H = PL_T + 2;            // ... with the halo
constexpr int PL_TPB = 256;               // four pixels per thread
constexpr int PL_PPT = PL_T * PL_T / PL_TPB;
constexpr size_t PL_HEAD = 64;            // bytes in front of the scratch: [0] workgroups that changed something in this batch, [1] accepted sources

struct PlanArgs {
  const float* img; int32_t rows, cols, ntx, nty;
  nvbx_cost_options o;
  int32_t* cls;                           // [rows][cols] class words
  int32_t* cost;                          // [rows][cols] the field
  uint8_t* active;                        // [2][ntx * nty]
  uint32_t* head;
  const int32_t* src; int32_t n_src;
  int32_t sweeps;
};

__global__ __launch_bounds__(PL_TPB) void k_plan_classify(PlanArgs a) {
  const int t = threadIdx.x;
  const int32_t ntiles = a.ntx * a.nty;
  for (int32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int32_t ty = tile / a.ntx, tx = tile - ty * a.ntx;
#pragma unroll
    for (int k = 0; k < PL_PPT; k++) {
      const int i = t + PL_TPB * k;
      const int32_t r = ty * PL_T + (i >> 5), c = tx * PL_T + (i & 31);
      if (r < a.rows && c < a.cols) {
        const int64_t g = (int64_t)r * a.cols + c;
        a.cls[g] = nvbx_plan_class(a.img[g], &a.o);
        a.cost[g] = NVBX_COST_UNREACHED;
      }
    }
    __syncthreads();                      // (the fill is behind us: a source's 0 lands on top of it)
    int found = 0;
    for (int32_t s = t; s < a.n_src; s += PL_TPB) {
      const int32_t r = a.src[2 * (int64_t)s], c = a.src[2 * (int64_t)s + 1];
      if (r < 0 || c < 0 || r >= a.rows || c >= a.cols || r / PL_T != ty || c / PL_T != tx) continue;
      const int64_t g = (int64_t)r * a.cols + c;
      if (nvbx_plan_class(a.img[g], &a.o) < 0) continue;
      a.cost[g] = 0; found = 1;
      atomicAdd(&a.head[1], 1u);
    }
    const int any = __syncthreads_or(found);
    if (t == 0) { a.active[tile] = (uint8_t)(any != 0); a.active[ntiles + tile] = 0; }
  }
}

__global__ __launch_bounds__(PL_TPB) void k_plan_relax(PlanArgs a, int32_t parity) {
  __shared__ int32_t s_g[PL_H * PL_H], s_k[PL_H * PL_H];
  const int t = threadIdx.x;
  const int32_t ntiles = a.ntx * a.nty;
  uint8_t* cur = a.active + (size_t)parity * ntiles;
  uint8_t* nxt = a.active + (size_t)(parity ^ 1) * ntiles;
  for (int32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int on = cur[tile];
    __syncthreads();                      // (every thread has read the flag; the previous tile's LDS readers are done)
    if (!on) continue;                    // uniform
    if (t == 0) cur[tile] = 0;            // this set is the next round's target: its owner empties it
    const int32_t ty = tile / a.ntx, tx = tile - ty * a.ntx;
    for (int i = t; i < PL_H * PL_H; i += PL_TPB) {
      const int32_t r = ty * PL_T + i / PL_H - 1, c = tx * PL_T + i % PL_H - 1;
      int32_t k = NVBX_PLAN_BLOCKED, g = NVBX_COST_UNREACHED;
      if (r >= 0 && c >= 0 && r < a.rows && c < a.cols) { k = a.cls[(int64_t)r * a.cols + c]; g = a.cost[(int64_t)r * a.cols + c]; }
      s_k[i] = k; s_g[i] = g;
    }
    __syncthreads();
    int32_t orig[PL_PPT];
#pragma unroll
    for (int k = 0; k < PL_PPT; k++) { const int i = t + PL_TPB * k; orig[k] = s_g[((i >> 5) + 1) * PL_H + (i & 31) + 1]; }
    int sweep = 0, more = 0;
    do {
      int ch = 0;
#pragma unroll
      for (int k = 0; k < PL_PPT; k++) {
        const int i = t + PL_TPB * k;
        const int li = ((i >> 5) + 1) * PL_H + (i & 31) + 1;
        const int32_t kp = s_k[li];
        if (kp < 0) continue;
        const int32_t g = s_g[li];
        int32_t best = g;
        // along the axes: (0,1) (1,0) (0,-1) (-1,0)
        const int32_t kr = s_k[li + 1], kd = s_k[li + PL_H], kl = s_k[li - 1], ku = s_k[li - PL_H];
        const int32_t gr = s_g[li + 1], gd = s_g[li + PL_H], gl = s_g[li - 1], gu = s_g[li - PL_H];
        if (kr >= 0 && gr != NVBX_COST_UNREACHED) best = min(best, gr + nvbx_plan_step(0, kp, kr));
        if (kd >= 0 && gd != NVBX_COST_UNREACHED) best = min(best, gd + nvbx_plan_step(0, kp, kd));
        if (kl >= 0 && gl != NVBX_COST_UNREACHED) best = min(best, gl + nvbx_plan_step(0, kp, kl));
        if (ku >= 0 && gu != NVBX_COST_UNREACHED) best = min(best, gu + nvbx_plan_step(0, kp, ku));
        // diagonally, only between two traversable edge neighbours: no corner is cut
        if (kd >= 0 && kr >= 0) { const int32_t kq = s_k[li + PL_H + 1], gq = s_g[li + PL_H + 1]; if (kq >= 0 && gq != NVBX_COST_UNREACHED) best = min(best, gq + nvbx_plan_step(1, kp, kq)); }
        if (kd >= 0 && kl >= 0) { const int32_t kq = s_k[li + PL_H - 1], gq = s_g[li + PL_H - 1]; if (kq >= 0 && gq != NVBX_COST_UNREACHED) best = min(best, gq + nvbx_plan_step(1, kp, kq)); }
        if (ku >= 0 && kl >= 0) { const int32_t kq = s_k[li - PL_H - 1], gq = s_g[li - PL_H - 1]; if (kq >= 0 && gq != NVBX_COST_UNREACHED) best = min(best, gq + nvbx_plan_step(1, kp, kq)); }
        if (ku >= 0 && kr >= 0) { const int32_t kq = s_k[li - PL_H + 1], gq = s_g[li - PL_H + 1]; if (kq >= 0 && gq != NVBX_COST_UNREACHED) best = min(best, gq + nvbx_plan_step(1, kp, kq)); }
        if (best < g) { s_g[li] = best; ch = 1; }      // (a neighbour may read the old or the new value in this sweep: both are bounds)
      }
      sweep++;
      more = __syncthreads_or(ch);
    } while (more && sweep < a.sweeps);
    int any = 0;
#pragma unroll
    for (int k = 0; k < PL_PPT; k++) {
      const int i = t + PL_TPB * k;
      const int ly = i >> 5, lx = i & 31;
      const int32_t g = s_g[(ly + 1) * PL_H + lx + 1];
      if (!(g < orig[k])) continue;       // (a pixel outside the image holds UNREACHED and never falls)
      a.cost[(int64_t)(ty * PL_T + ly) * a.cols + tx * PL_T + lx] = g;
      any = 1;
      const int dy = ly == 0 ? -1 : ly == PL_T - 1 ? 1 : 0, dx = lx == 0 ? -1 : lx == PL_T - 1 ? 1 : 0;
      const bool oky = dy != 0 && ty + dy >= 0 && ty + dy < a.nty, okx = dx != 0 && tx + dx >= 0 && tx + dx < a.ntx;
      if (oky) nxt[(ty + dy) * a.ntx + tx] = 1;
      if (okx) nxt[ty * a.ntx + tx + dx] = 1;
      if (oky && okx) nxt[(ty + dy) * a.ntx + tx + dx] = 1;
    }
    any = __syncthreads_or(any);
    if (t == 0 && (any || more)) {
      if (more) nxt[tile] = 1;            // cut off by the sweep limit: goes on in the next round
      atomicAdd(&a.head[0], 1u);
    }
  }
}

struct TraceArgs {
  const float* img; int32_t rows, cols;
  nvbx_cost_options o;
  const int32_t* cost; const int32_t* starts; int32_t n;
  int32_t* path; int32_t capacity; int32_t* length;
};

__device__ inline int32_t pl_class_at(const TraceArgs& a, int32_t r, int32_t c) {
  if (r < 0 || c < 0 || r >= a.rows || c >= a.cols) return NVBX_PLAN_BLOCKED;
  return nvbx_plan_class(a.img[(int64_t)r * a.cols + c], &a.o);
}

__global__ __launch_bounds__(64) void k_plan_trace(TraceArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * 64 + threadIdx.x);
  if (i >= a.n) return;
  constexpr int MV[8][2] = NVBX_PLAN_MOVES;
  int32_t r = a.starts[2 * (int64_t)i], c = a.starts[2 * (int64_t)i + 1];
  int32_t len = 0;
  if (r >= 0 && c >= 0 && r < a.rows && c < a.cols && a.cost[(int64_t)r * a.cols + c] != NVBX_COST_UNREACHED) {
    int32_t* out = a.path + (int64_t)i * a.capacity * 2;
    const int64_t limit = (int64_t)a.rows * a.cols;      // G falls by at least 10 per step: no path of a field is longer
    len = -1;
    for (int64_t step = 0; step < limit; step++) {
      const int32_t g = a.cost[(int64_t)r * a.cols + c];
      if (step < a.capacity) { out[2 * step] = r; out[2 * step + 1] = c; }
      if (g == 0) { len = (int32_t)(step + 1); break; }
      const int32_t kp = pl_class_at(a, r, c);
      if (g < 0 || kp < 0) break;
      int d = 0;
      for (; d < 8; d++) {
        const int32_t qr = r + MV[d][0], qc = c + MV[d][1];
        const int32_t kq = pl_class_at(a, qr, qc);
        if (kq < 0) continue;
        if (d >= 4 && (pl_class_at(a, qr, c) < 0 || pl_class_at(a, r, qc) < 0)) continue;
        const int32_t gq = a.cost[(int64_t)qr * a.cols + qc];
        if (gq == NVBX_COST_UNREACHED || gq < 0 || gq >= g) continue;      // (the next pixel lies strictly lower: the walk cannot circle)
        if ((int64_t)gq + nvbx_plan_step(d >= 4, kp, kq) == (int64_t)g) { r = qr; c = qc; break; }
      }
      if (d == 8) break;
    }
  }
  a.length[i] = len;
}

// ------------------------------------------------------------------------------------------------ C-ABI
namespace {

int plan_check(const char* who, const nvbx_mapper* m, const void* image, int32_t rows, int32_t cols, const nvbx_cost_options* o, const void* cost) {
  if (!m) return refuse(who, ": the mapper is NULL");
  if (!image || !o || !cost) return refuse(who, ": image_dev, options and cost_dev are required");
  if (rows <= 0 || cols <= 0 || (int64_t)rows * cols > NVBX_PLAN_MAX_PIXELS) return refuse(who, ": rows and cols must be > 0 and rows x cols <= 2^22");
  if (const char* why = nvbx_plan_options_problem(o)) return refuse(who, why);
  return NVBX_OK;
}

}  // namespace

extern "C" void nvbx_default_cost_options(nvbx_cost_options* o) {
  if (!o) return;
  o->robot_radius_m = 0.25f; o->inflation_radius_m = 0.75f; o->penalty_per_m = 100.0f; o->unknown_value = 1000.0f;
  o->max_penalty = 200; o->unknown_penalty = 50; o->allow_unknown = 0; o->pad = 0;
}

extern "C" int nvbx_cost_field(nvbx_mapper* m, const float* image_dev, int32_t rows, int32_t cols, const nvbx_cost_options* options,
                               const int32_t* sources_rc_dev, int32_t n_sources, int32_t* cost_dev, int32_t* accepted_dev) {
  const char* who = "nvbx_cost_field";
  const int rc = plan_check(who, m, image_dev, rows, cols, options, cost_dev);
  if (rc) return rc;
  if (n_sources < 0) return refuse(who, ": n_sources is negative");
  if (n_sources > 0 && !sources_rc_dev) return refuse(who, ": sources_rc_dev is required with n_sources > 0");
  NVBX_HIP(hipSetDevice(m->device));
  if (m->join_side_keeping_held()) return NVBX_E_DEVICE;      // the image only: everything held back stays held back
  const int64_t n = (int64_t)rows * cols;
  PlanArgs a{};
  a.img = image_dev; a.rows = rows; a.cols = cols; a.ntx = (cols + PL_T - 1) / PL_T; a.nty = (rows + PL_T - 1) / PL_T;
  a.o = *options; a.cost = cost_dev; a.src = sources_rc_dev; a.n_src = n_sources; a.sweeps = m->plan_knobs.tile_sweeps;
  const int64_t ntiles = (int64_t)a.ntx * a.nty;
  if (m->plan_scratch.ensure(m->stream, PL_HEAD + (size_t)n * 4 + (size_t)ntiles * 2)) return NVBX_E_DEVICE;
  a.head = m->plan_scratch.as<uint32_t>();
  a.cls = reinterpret_cast<int32_t*>(m->plan_scratch.as<uint8_t>() + PL_HEAD);
  a.active = m->plan_scratch.as<uint8_t>() + PL_HEAD + (size_t)n * 4;
  const dim3 grid((unsigned)ntiles);      // at most 2^22 / 32 tiles
  NVBX_HIP(hipMemsetAsync(a.head, 0, PL_HEAD, m->stream));
  NVBX_LAUNCH(m, k_plan_classify, grid, dim3(PL_TPB), a);
  NVBX_HIP(hipGetLastError());
  // Rounds in batches, one read of the changed counter per batch; a batch in which nothing changed ends the call.  After k rounds every pixel
  // whose best path has at most k moves is final, so n rounds reach the fixed point and one more batch sees it: more can only mean a bug.
  const int batch = m->plan_knobs.rounds_per_wait;
  const int64_t max_rounds = n + batch;
  int32_t parity = 0;
  for (int64_t rounds = 0; n_sources > 0;) {
    NVBX_HIP(hipMemsetAsync(a.head, 0, sizeof(uint32_t), m->stream));
    for (int k = 0; k < batch; k++, parity ^= 1) NVBX_LAUNCH(m, k_plan_relax, grid, dim3(PL_TPB), a, parity);
    NVBX_HIP(hipGetLastError());
    rounds += batch;
    uint32_t changed = 0;
    NVBX_HIP(hipMemcpyAsync(&changed, a.head, sizeof(changed), hipMemcpyDeviceToHost, m->stream));
    NVBX_HIP(hipStreamSynchronize(m->stream));
    if (!changed) break;
    if (rounds >= max_rounds) { set_error("nvbx_cost_field: the relaxation did not reach its fixed point within rows x cols rounds"); return NVBX_E_DEVICE; }
  }
  if (accepted_dev) NVBX_HIP(hipMemcpyAsync(accepted_dev, a.head + 1, sizeof(int32_t), hipMemcpyDeviceToDevice, m->stream));
  return m->wait_stream();
}

extern "C" int nvbx_trace_paths(nvbx_mapper* m, const float* image_dev, int32_t rows, int32_t cols, const nvbx_cost_options* options,
                                const int32_t* cost_dev, const int32_t* starts_rc_dev, int32_t n_starts, int32_t* path_rc_dev, int32_t capacity,
                                int32_t* length_dev) {
  const char* who = "nvbx_trace_paths";
  const int rc = plan_check(who, m, image_dev, rows, cols, options, cost_dev);
  if (rc) return rc;
  if (n_starts < 0 || capacity < 0) return refuse(who, ": n_starts and capacity must be >= 0");
  if (n_starts > 0 && (!starts_rc_dev || !path_rc_dev || !length_dev)) return refuse(who, ": starts_rc_dev, path_rc_dev and length_dev are required with n_starts > 0");
  if (n_starts == 0) return NVBX_OK;
  NVBX_HIP(hipSetDevice(m->device));
  if (m->join_side_keeping_held()) return NVBX_E_DEVICE;
  TraceArgs a{};
  a.img = image_dev; a.rows = rows; a.cols = cols; a.o = *options; a.cost = cost_dev; a.starts = starts_rc_dev; a.n = n_starts;
  a.path = path_rc_dev; a.capacity = capacity; a.length = length_dev;
  NVBX_LAUNCH(m, k_plan_trace, dim3((unsigned)((n_starts + 63) / 64)), dim3(64), a);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}
