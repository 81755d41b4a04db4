// plan.hip -- which goal can be reached and how far the drive is (SEMANTICS.md "Cost field and paths"): nvbx_cost_field turns a
// distance image (the ESDF slice) and a set of source pixels into the integer cost-to-go field, nvbx_trace_paths walks down such a field.  Both read
// the image only; the classes and step costs are nvbx_plan_math.h's, shared with the host.
//
// The field is the fixed point of a relaxation over 32 x 32 pixel tiles; no workgroup ever waits for another, every loop is bounded.
// k_plan_classify: a workgroup per tile writes the class word of its pixels (NVBX_PLAN_BLOCKED or the penalty), fills its part of the field with
//   UNREACHED, then goes through the source list, sets the accepted sources that lie in its tile to 0 and writes both of its active flags (active:
//   an accepted source in the tile or in its halo; nvbx_plan_grid.h's plan_grid_seed, shared with plan3d.hip).
// k_plan_relax: one round.  A workgroup whose tile is not active ends after one byte load.  An active one loads the tile's costs and class words
//   with a one-pixel halo into LDS (9.2 KB), pulls min(G(q) + c(p, q)) over the eight neighbours, in place, until a sweep changes nothing or the
//   sweep limit is hit, and stores the pixels that fell.  A changed pixel on the rim marks the up to three neighbouring tiles that hold it in their
//   halo active for the next round (plain byte stores into the other of two flag sets); a tile cut off by the limit marks itself.  A workgroup
//   that changed anything adds one to the counter the host reads once per batch of rounds.
//   Every stored value is the cost of a real move sequence and values only fall, so a halo read before or after a neighbour's store of the same
//   round is a valid bound either way, and that store re-activates the reader (DESIGN.md 2.21 has the argument in full).
// k_plan_trace: a lane per start, the path rule of the header: nvbx_plan_grid.h's walk over PlGrid's eight moves.
// The scratch layout, the host's loop over batches of rounds and the argument checks are nvbx_plan_grid.h's too.
#include <algorithm>
#include <cmath>
#include "nvbx_plan_grid.h"

using namespace nvbx;

constexpr int PL_T = 32;                  // tile side in pixels
constexpr int PL_H = PL_T + 2;            // ... with the halo
constexpr int PL_TPB = 256;               // four pixels per thread
constexpr int PL_PPT = PL_T * PL_T / PL_TPB;
constexpr PlanWords PL_WORDS{"image", "rows and cols", "rows x cols", "rc"};

struct PlanArgs {
  const float* img; int32_t rows, cols, ntx, nty;
  PlanGridArgs g;                         // cls and cost are [rows][cols], active [2][ntx * nty]
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
        a.g.cls[g] = nvbx_plan_class(a.img[g], &a.g.o);
        a.g.cost[g] = NVBX_COST_UNREACHED;
      }
    }
    __syncthreads();                      // (the fill is behind us: a source's 0 lands on top of it)
    const int32_t dim[2] = {a.rows, a.cols}, org[2] = {ty * PL_T, tx * PL_T};
    plan_grid_seed<PL_TPB, PL_T, PL_T>(a.g, a.img, dim, org, tile, ntiles);
  }
}

__global__ __launch_bounds__(PL_TPB) void k_plan_relax(PlanArgs a, int32_t parity) {
  __shared__ int32_t s_g[PL_H * PL_H], s_k[PL_H * PL_H];
  const int t = threadIdx.x;
  const int32_t ntiles = a.ntx * a.nty;
  uint8_t* cur = a.g.active + (size_t)parity * ntiles;
  uint8_t* nxt = a.g.active + (size_t)(parity ^ 1) * ntiles;
  for (int32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int on = cur[tile];
    __syncthreads();                      // (every thread has read the flag; the previous tile's LDS readers are done)
    if (!on) continue;                    // uniform
    if (t == 0) cur[tile] = 0;            // this set is the next round's target: its owner empties it
    const int32_t ty = tile / a.ntx, tx = tile - ty * a.ntx;
    for (int i = t; i < PL_H * PL_H; i += PL_TPB) {
      const int32_t r = ty * PL_T + i / PL_H - 1, c = tx * PL_T + i % PL_H - 1;
      int32_t k = NVBX_PLAN_BLOCKED, g = NVBX_COST_UNREACHED;
      if (r >= 0 && c >= 0 && r < a.rows && c < a.cols) { k = a.g.cls[(int64_t)r * a.cols + c]; g = a.g.cost[(int64_t)r * a.cols + c]; }
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
    } while (more && sweep < a.g.sweeps);
    int any = 0;
#pragma unroll
    for (int k = 0; k < PL_PPT; k++) {
      const int i = t + PL_TPB * k;
      const int ly = i >> 5, lx = i & 31;
      const int32_t g = s_g[(ly + 1) * PL_H + lx + 1];
      if (!(g < orig[k])) continue;       // (a pixel outside the image holds UNREACHED and never falls)
      a.g.cost[(int64_t)(ty * PL_T + ly) * a.cols + tx * PL_T + lx] = g;
      any = 1;
      const int dy = ly == 0 ? -1 : ly == PL_T - 1 ? 1 : 0, dx = lx == 0 ? -1 : lx == PL_T - 1 ? 1 : 0;
      const bool oky = dy != 0 && ty + dy >= 0 && ty + dy < a.nty, okx = dx != 0 && tx + dx >= 0 && tx + dx < a.ntx;
      if (oky) nxt[(ty + dy) * a.ntx + tx] = 1;
      if (okx) nxt[ty * a.ntx + tx + dx] = 1;
      if (oky && okx) nxt[(ty + dy) * a.ntx + tx + dx] = 1;
    }
    plan_grid_round_end(a.g, nxt, tile, any, more);
  }
}

struct PlGrid {                           // the eight moves of nvbx_plan_math.h, for the walk
  static constexpr int D = 2, MOVES = 8;
  __device__ static int move(int d, int c) { constexpr int MV[8][2] = NVBX_PLAN_MOVES; return MV[d][c]; }
  __device__ static int k(int d) { return d < 4 ? 1 : 2; }
  __device__ static int32_t step(int k, int32_t kp, int32_t kq) { return nvbx_plan_step(k > 1, kp, kq); }
};

__global__ __launch_bounds__(64) void k_plan_trace(PlanTraceArgs<2> a) { plan_grid_trace<PlGrid>(a); }

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" void nvbx_default_cost_options(nvbx_cost_options* o) {
  if (!o) return;
  o->robot_radius_m = 0.25f; o->inflation_radius_m = 0.75f; o->penalty_per_m = 100.0f; o->unknown_value = 1000.0f;
  o->max_penalty = 200; o->unknown_penalty = 50; o->allow_unknown = 0; o->pad = 0;
}

extern "C" int nvbx_cost_field(nvbx_mapper* m, const float* image_dev, int32_t rows, int32_t cols, const nvbx_cost_options* options,
                               const int32_t* sources_rc_dev, int32_t n_sources, int32_t* cost_dev, int32_t* accepted_dev) {
  const char* who = "nvbx_cost_field";
  const int32_t dim[2] = {rows, cols};
  if (const int rc = plan_grid_check_field<2>(who, PL_WORDS, m, image_dev, dim, options, sources_rc_dev, n_sources, cost_dev)) return rc;
  PlanArgs a{};
  a.img = image_dev; a.rows = rows; a.cols = cols; a.ntx = (cols + PL_T - 1) / PL_T; a.nty = (rows + PL_T - 1) / PL_T;
  const int64_t n = (int64_t)rows * cols, ntiles = (int64_t)a.ntx * a.nty;      // at most 2^22 / 32 tiles
  if (const int rc = plan_grid_setup(m, &a.g, n, ntiles, options, sources_rc_dev, n_sources, cost_dev)) return rc;
  const dim3 grid((unsigned)ntiles);
  NVBX_LAUNCH(m, k_plan_classify, grid, dim3(PL_TPB), a);
  return plan_grid_relax(m, who, PL_WORDS.product, a.g, n, [&](int32_t parity) { NVBX_LAUNCH(m, k_plan_relax, grid, dim3(PL_TPB), a, parity); }, accepted_dev);
}

extern "C" int nvbx_trace_paths(nvbx_mapper* m, const float* image_dev, int32_t rows, int32_t cols, const nvbx_cost_options* options,
                                const int32_t* cost_dev, const int32_t* starts_rc_dev, int32_t n_starts, int32_t* path_rc_dev, int32_t capacity,
                                int32_t* length_dev) {
  const int32_t dim[2] = {rows, cols};
  return plan_grid_trace_call<2>("nvbx_trace_paths", PL_WORDS, m, image_dev, dim, options, cost_dev, starts_rc_dev, n_starts, path_rc_dev, capacity, length_dev,
                                 [&](const PlanTraceArgs<2>& a, dim3 grid, dim3 block) { NVBX_LAUNCH(m, k_plan_trace, grid, block, a); });
}
