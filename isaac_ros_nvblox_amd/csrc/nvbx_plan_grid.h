// nvbx_plan_grid.h -- what the cost field (plan.hip) and the cost volume (plan3d.hip, 2.23) do the same way, written down once:
// the scratch layout and the common kernel arguments, the host's loop over batches of relaxation rounds, the seeding of the sources, the end of
// a round, the path walk and the argument checks.  A grid has D axes, the last one fastest.  What differs -- the tile, the relaxation kernel, the
// moves and their costs -- stays in the two files; a grid trait (PlGrid, PvGrid) hands the moves to the walk.
#ifndef NVBX_PLAN_GRID_H_
#define NVBX_PLAN_GRID_H_
#include <string>
#include "nvbx_mapper.h"
#include "nvbx_plan3d_math.h"

namespace nvbx {

// m->plan_scratch: [head][n class words][2][ntiles] active-tile flags.  The head's words: [0] workgroups that changed something in this batch of
// rounds, [1] accepted sources.
constexpr size_t PLAN_HEAD = 64;
static_assert(NVBX_PLAN3D_MAX_VOXELS == NVBX_PLAN_MAX_PIXELS, "plan_grid_check has one limit, 2^22 cells");

struct PlanGridArgs {                     // the part of the kernel arguments that both planners have
  nvbx_cost_options o;
  int32_t* cls;                           // [n] class words
  int32_t* cost;                          // [n] the field
  uint8_t* active;                        // [2][ntiles]
  uint32_t* head;
  const int32_t* src; int32_t n_src;      // [n_src][D]
  int32_t sweeps;
};

template <int D> struct PlanTraceArgs {
  const float* grid; int32_t dim[D];
  nvbx_cost_options o;
  const int32_t* cost; const int32_t* starts; int32_t n;
  int32_t* path; int32_t capacity; int32_t* length;
};

struct PlanWords { const char* grid; const char* dims; const char* product; const char* axes; };      // what a caller's messages call its inputs

template <int D> __host__ __device__ inline bool plan_inside(const int32_t* dim, const int32_t* p) {
  bool in = true;
  for (int c = 0; c < D; c++) in = in & (p[c] >= 0) & (p[c] < dim[c]);      // (& on purpose: one test, no branch per axis)
  return in;
}
template <int D> __host__ __device__ inline int64_t plan_index(const int32_t* dim, const int32_t* p) {      // of a cell inside the grid: nothing is negative, so the products are unsigned
  uint64_t g = (uint64_t)(uint32_t)p[0] * (uint32_t)dim[1] + (uint32_t)p[1];
  for (int c = 2; c < D; c++) g = g * (uint32_t)dim[c] + (uint32_t)p[c];
  return (int64_t)g;
}

// ------------------------------------------------------------------------------------------------ device
// The end of a classify workgroup of TPB threads: its tile (origin org, extent T...), behind the barrier that follows the fill.  An accepted
// source -- inside the grid, on a traversable cell -- in the tile or in its one-cell halo makes the tile active: the 0 is a value no relaxation
// stores, so nobody else would wake the neighbour of a tile whose only reached cell is a source on its rim.  Only the tile that owns the cell
// writes the 0 and counts it.
template <int TPB, int... T> __device__ inline void plan_grid_seed(const PlanGridArgs& g, const float* grid, const int32_t* dim, const int32_t* org, int32_t tile, int32_t ntiles) {
  constexpr int D = sizeof...(T), ext[D] = {T...};
  int found = 0;
  for (int32_t s = threadIdx.x; s < g.n_src; s += TPB) {
    int32_t p[D];
    for (int c = 0; c < D; c++) p[c] = g.src[D * (int64_t)s + c];
    if (!plan_inside<D>(dim, p)) continue;
    bool near = true, own = true;
    for (int c = 0; c < D; c++) { const int32_t off = p[c] - org[c]; near = near && off >= -1 && off <= ext[c]; own = own && off >= 0 && off < ext[c]; }
    if (!near) continue;
    const int64_t at = plan_index<D>(dim, p);
    if (nvbx_plan_class(grid[at], &g.o) < 0) continue;
    found = 1;
    if (!own) continue;                   // the neighbour that owns it seeds and counts it
    g.cost[at] = 0;
    atomicAdd(&g.head[1], 1u);
  }
  const int any = __syncthreads_or(found);
  if (threadIdx.x == 0) { g.active[tile] = (uint8_t)(any != 0); g.active[ntiles + tile] = 0; }
}

// The end of a relaxation workgroup's tile.  any: this thread stored a cell that fell; more: the sweep limit cut the tile off (uniform).
__device__ inline void plan_grid_round_end(const PlanGridArgs& g, uint8_t* nxt, int32_t tile, int any, int more) {
  any = __syncthreads_or(any);
  if (threadIdx.x == 0 && (any || more)) {
    if (more) nxt[tile] = 1;              // cut off by the sweep limit: goes on in the next round
    atomicAdd(&g.head[0], 1u);
  }
}

template <int D> __device__ inline int32_t plan_class_at(const PlanTraceArgs<D>& a, const int32_t* p) {
  return plan_inside<D>(a.dim, p) ? nvbx_plan_class(a.grid[plan_index<D>(a.dim, p)], &a.o) : NVBX_PLAN_BLOCKED;
}

// The path walk, a lane per start (blocks of 64).  G: D axes, MOVES moves in the order they are tried, move(d, c) = component c of move d,
// k(d) = the number of its nonzero components, step(k, kp, kq) = its cost between two traversable cells with class words kp and kq.
template <class G> __device__ inline void plan_grid_trace(const PlanTraceArgs<G::D>& a) {
  constexpr int D = G::D;
  const int32_t i = (int32_t)(blockIdx.x * 64 + threadIdx.x);
  if (i >= a.n) return;
  int32_t p[D];
  for (int c = 0; c < D; c++) p[c] = a.starts[D * (int64_t)i + c];
  int32_t len = 0;
  if (plan_inside<D>(a.dim, p) && a.cost[plan_index<D>(a.dim, p)] != NVBX_COST_UNREACHED) {
    int32_t* out = a.path + (int64_t)i * a.capacity * D;
    int64_t limit = 1;                    // G falls by at least 10 per step: no path of a field is longer than the grid has cells
    for (int c = 0; c < D; c++) limit *= a.dim[c];
    len = -1;
    for (int64_t step = 0; step < limit; step++) {
      const int32_t g = a.cost[plan_index<D>(a.dim, p)];
      if (step < a.capacity) for (int c = 0; c < D; c++) out[D * step + c] = p[c];
      if (g == 0) { len = (int32_t)(step + 1); break; }
      const int32_t kp = plan_class_at<D>(a, p);
      if (g < 0 || kp < 0) break;
      int d = 0;
      for (; d < G::MOVES; d++) {
        int32_t q[D];
        for (int c = 0; c < D; c++) q[c] = p[c] + G::move(d, c);
        const int32_t kq = plan_class_at<D>(a, q);
        if (kq < 0) continue;
        const int k = G::k(d);
        bool clear = true;                // no corner is cut: every cell p + e, e_c in {0, d_c}, between p and q is traversable
#pragma unroll
        for (int e = 1; e < (1 << D) - 1 && clear && k > 1; e++) {
          int32_t b[D]; bool twice = false, is_q = true;      // e with a bit on an axis along which d does not move names a cell a smaller e has named
          for (int c = 0; c < D; c++) { const bool on = e >> c & 1, flat = G::move(d, c) == 0; b[c] = on ? q[c] : p[c]; twice = twice || (on && flat); is_q = is_q && (on || flat); }
          if (!twice && !is_q) clear = plan_class_at<D>(a, b) >= 0;
        }
        if (!clear) continue;
        const int32_t gq = a.cost[plan_index<D>(a.dim, q)];
        if (gq == NVBX_COST_UNREACHED || gq < 0 || gq >= g) continue;      // (the next cell lies strictly lower: the walk cannot circle)
        if ((int64_t)gq + G::step(k, kp, kq) == (int64_t)g) { for (int c = 0; c < D; c++) p[c] = q[c]; break; }
      }
      if (d == G::MOVES) break;
    }
  }
  a.length[i] = len;
}

// ------------------------------------------------------------------------------------------------ host
// the refusals that the cost-to-go and the trace entry points share, in their order
template <int D> inline int plan_grid_check(const char* who, const PlanWords& w, const nvbx_mapper* m, const void* grid, const int32_t* dim, const nvbx_cost_options* o, const void* cost) {
  if (!m) return refuse(who, ": the mapper is NULL");
  if (!grid || !o || !cost) return refuse(who, (std::string(": ") + w.grid + "_dev, options and cost_dev are required").c_str());
  int64_t n = 1;
  for (int c = 0; c < D; c++)
    if (dim[c] <= 0 || (n *= dim[c]) > NVBX_PLAN_MAX_PIXELS) return refuse(who, (std::string(": ") + w.dims + " must be > 0 and " + w.product + " <= 2^22").c_str());
  if (const char* why = nvbx_plan_options_problem(o)) return refuse(who, why);
  return NVBX_OK;
}

template <int D> inline int plan_grid_check_field(const char* who, const PlanWords& w, const nvbx_mapper* m, const void* grid, const int32_t* dim, const nvbx_cost_options* o,
                                                  const void* src, int32_t n_src, const void* cost) {
  if (const int rc = plan_grid_check<D>(who, w, m, grid, dim, o, cost)) return rc;
  if (n_src < 0) return refuse(who, ": n_sources is negative");
  if (n_src > 0 && !src) return refuse(who, (std::string(": sources_") + w.axes + "_dev is required with n_sources > 0").c_str());
  return NVBX_OK;
}

// Behind the checks of a cost-to-go call: begins the call (it reads its input only: everything held back stays held back), sizes the
// scratch for n cells and ntiles tiles, points g into it and clears the head.
inline int plan_grid_setup(nvbx_mapper* m, PlanGridArgs* g, int64_t n, int64_t ntiles, const nvbx_cost_options* o, const int32_t* src, int32_t n_src, int32_t* cost) {
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  if (m->plan_scratch.ensure(m->stream, PLAN_HEAD + (size_t)n * 4 + (size_t)ntiles * 2)) return NVBX_E_DEVICE;
  uint8_t* base = m->plan_scratch.as<uint8_t>();
  g->head = reinterpret_cast<uint32_t*>(base); g->cls = reinterpret_cast<int32_t*>(base + PLAN_HEAD); g->active = base + PLAN_HEAD + (size_t)n * 4;
  g->o = *o; g->cost = cost; g->src = src; g->n_src = n_src; g->sweeps = m->plan_knobs.tile_sweeps;
  NVBX_HIP(hipMemsetAsync(g->head, 0, PLAN_HEAD, m->stream));
  return NVBX_OK;
}

// Behind the classify launch: rounds in batches (round(parity) enqueues one), one read of the changed counter per batch; a batch in which nothing
// changed ends the call.  After k rounds every cell whose best path has at most k moves is final, so n rounds reach the fixed point and one more
// batch sees it: more can only mean a bug.  cells: the caller's word for n in that message.
template <class Round> inline int plan_grid_relax(nvbx_mapper* m, const char* who, const char* cells, const PlanGridArgs& g, int64_t n, Round&& round, int32_t* accepted_dev) {
  NVBX_HIP(hipGetLastError());
  const int batch = m->plan_knobs.rounds_per_wait;
  int32_t parity = 0;
  for (int64_t rounds = 0; g.n_src > 0;) {
    NVBX_HIP(hipMemsetAsync(g.head, 0, sizeof(uint32_t), m->stream));
    for (int k = 0; k < batch; k++, parity ^= 1) round(parity);
    NVBX_HIP(hipGetLastError());
    rounds += batch;
    uint32_t changed = 0;
    NVBX_HIP(hipMemcpyAsync(&changed, g.head, sizeof(changed), hipMemcpyDeviceToHost, m->stream));
    NVBX_HIP(hipStreamSynchronize(m->stream));
    if (!changed) break;
    if (rounds >= n + batch) { set_error((std::string(who) + ": the relaxation did not reach its fixed point within " + cells + " rounds").c_str()); return NVBX_E_DEVICE; }
  }
  if (accepted_dev) NVBX_HIP(hipMemcpyAsync(accepted_dev, g.head + 1, sizeof(int32_t), hipMemcpyDeviceToDevice, m->stream));
  return m->wait_stream();
}

// A whole trace entry point: the checks, then launch(args) for the caller's kernel on ceil(n_starts / 64) blocks of 64.
template <int D, class Launch> inline int plan_grid_trace_call(const char* who, const PlanWords& w, nvbx_mapper* m, const float* grid, const int32_t* dim, const nvbx_cost_options* o,
                                                               const int32_t* cost, const int32_t* starts, int32_t n_starts, int32_t* path, int32_t capacity, int32_t* length, Launch&& launch) {
  if (const int rc = plan_grid_check<D>(who, w, m, grid, dim, o, cost)) return rc;
  if (n_starts < 0 || capacity < 0) return refuse(who, ": n_starts and capacity must be >= 0");
  if (n_starts > 0 && (!starts || !path || !length))
    return refuse(who, (std::string(": starts_") + w.axes + "_dev, path_" + w.axes + "_dev and length_dev are required with n_starts > 0").c_str());
  if (n_starts == 0) return NVBX_OK;
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  PlanTraceArgs<D> a{};
  a.grid = grid; a.o = *o; a.cost = cost; a.starts = starts; a.n = n_starts; a.path = path; a.capacity = capacity; a.length = length;
  for (int c = 0; c < D; c++) a.dim[c] = dim[c];
  launch(a, dim3((unsigned)((n_starts + 63) / 64)), dim3(64));
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

}  // namespace nvbx
#endif
