// plan3d.hip -- which goal can be reached through free space and what the flight costs (SEMANTICS.md "Cost volume and 3-D paths"):
// nvbx_cost_volume turns a distance volume (the box nvbx_esdf_dense_grid writes, z fastest) and a set of source voxels into the integer cost-to-go
// field over 26-connected moves, nvbx_trace_paths_3d walks down such a field.  Both read the volume only; the classes are nvbx_plan_math.h's, the
// moves and step costs nvbx_plan3d_math.h's, shared with the host.
//
// The field is the fixed point of a relaxation over 8 x 8 x 8 voxel tiles; no workgroup ever waits for another, every loop is bounded.
// k_plan3d_classify: a workgroup per tile writes the class word of its voxels (NVBX_PLAN_BLOCKED or the penalty), fills its part of the field with
//   UNREACHED, then goes through the source list, sets the accepted sources that lie in its tile to 0 and writes both of its active flags (active:
//   an accepted source in the tile or in its halo; nvbx_plan_grid.h's plan_grid_seed, shared with plan.hip).
// k_plan3d_relax: one round.  A workgroup whose tile is not active ends after one byte load.  An active one stages ONE word per voxel of the tile
//   and its one-voxel halo in LDS: -1 for a voxel that is not traversable (or outside the volume), UNREACHED for an unreached one, else
//   H = G + pen -- so that a pull over a move with k nonzero components is H(q) + B_k + pen(p), one LDS read.  Each thread owns two voxels and
//   reads the 26 neighbour classes of each ONCE per tile visit into a traversability mask, from which the allowed moves follow (a move is
//   allowed iff every voxel p + e, e_i in {0, d_i}, e != 0, is traversable: one AND and one compare per move against a constant); the sweeps
//   then read costs only.  It sweeps in place until a sweep changes nothing or the sweep limit is hit and stores the voxels that fell.  A fallen
//   voxel on the rim marks the up to seven neighbouring tiles that hold it in their halo active for the next round (plain byte stores into the
//   other of two flag sets); a tile cut off by the limit marks itself.  A workgroup that changed anything adds one to the counter the host reads
//   once per batch of rounds.
//   Every stored value is the cost of a real move sequence and values only fall, so a halo read before or after a neighbour's store of the same
//   round is a valid bound either way, and that store re-activates the reader (DESIGN.md 2.23 has the argument in full).
// k_plan3d_trace: a lane per start, the path rule of the header: nvbx_plan_grid.h's walk over PvGrid's 26 moves; classes are recomputed from the volume.
// The scratch layout, the host's loop over batches of rounds and the argument checks are nvbx_plan_grid.h's too.
#include <algorithm>
#include <cmath>
#include "nvbx_plan_grid.h"

using namespace nvbx;

constexpr int PV_TX = 8, PV_TY = 8, PV_TZ = 8;                         // the tile in voxels (DESIGN.md 2.23 has the choice; z is the fastest axis of the volume)
constexpr int PV_HY = PV_TY + 2, PV_HZ = PV_TZ + 2;                    // ... with the halo
constexpr int PV_HX = PV_TX + 2;
constexpr int PV_ROW = PV_HZ;                                          // LDS words between y and y + 1
constexpr int PV_PLANE = 104;                                          // LDS words between x and x + 1: >= HY x HZ = 100 and = 8 (mod 32), see pv_local
constexpr int PV_CELLS = PV_HX * PV_HY * PV_HZ;                        // 1 000 staged words
constexpr int PV_TPB = 256;                                            // two voxels per thread
constexpr int PV_VOX = PV_TX * PV_TY * PV_TZ;
constexpr int PV_PPT = PV_VOX / PV_TPB;
static_assert(PV_PLANE >= PV_HY * PV_HZ && PV_PLANE % 32 == 8 && PV_TZ == 8 && PV_TX % 4 == 0 && PV_VOX % PV_TPB == 0, "the LDS layout of pv_local");

constexpr PlanWords PV_WORDS{"volume", "nx, ny and nz", "nx x ny x nz", "xyz"};

struct Plan3Args {
  const float* vol; int32_t nx, ny, nz, ntx, nty, ntz;
  PlanGridArgs g;                         // cls and cost are [nx][ny][nz], active [2][ntx * nty * ntz]
};

// Voxel i of a tile, 0 .. 511: z runs fastest, then x, then y.  The 32 lanes that one ds_read_b32 cycle serves hold 8 z of four neighbouring x:
// LDS words z + PV_PLANE x with PV_PLANE = 8 (mod 32) fall on 32 different banks, for the voxel itself and for each of its 26 neighbours.
__device__ inline void pv_local(int i, int* lx, int* ly, int* lz) { *lz = i & (PV_TZ - 1); *lx = (i / PV_TZ) % PV_TX; *ly = i / (PV_TZ * PV_TX); }
__device__ inline void pv_tile(const Plan3Args& a, int32_t tile, int32_t* tx, int32_t* ty, int32_t* tz) {
  *tz = tile % a.ntz; const int32_t r = tile / a.ntz; *ty = r % a.nty; *tx = r / a.nty;
}
__device__ inline int64_t pv_at(const Plan3Args& a, int32_t x, int32_t y, int32_t z) { return ((int64_t)x * a.ny + y) * a.nz + z; }

__global__ __launch_bounds__(PV_TPB) void k_plan3d_classify(Plan3Args a) {
  const int t = threadIdx.x;
  const int32_t ntiles = a.ntx * a.nty * a.ntz;
  for (int32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int32_t tx, ty, tz; pv_tile(a, tile, &tx, &ty, &tz);
#pragma unroll
    for (int k = 0; k < PV_PPT; k++) {
      const int i = t + PV_TPB * k;
      const int lz = i & (PV_TZ - 1), ly = (i / PV_TZ) % PV_TY, lx = i / (PV_TZ * PV_TY);      // (rows of z, then y: the stores of a wave are 32-byte runs, eight of them next to each other where nz = 8)
      const int32_t x = tx * PV_TX + lx, y = ty * PV_TY + ly, z = tz * PV_TZ + lz;
      if (x < a.nx && y < a.ny && z < a.nz) {
        const int64_t g = pv_at(a, x, y, z);
        a.g.cls[g] = nvbx_plan_class(a.vol[g], &a.g.o);
        a.g.cost[g] = NVBX_COST_UNREACHED;
      }
    }
    __syncthreads();                      // (the fill is behind us: a source's 0 lands on top of it)
    const int32_t dim[3] = {a.nx, a.ny, a.nz}, org[3] = {tx * PV_TX, ty * PV_TY, tz * PV_TZ};
    plan_grid_seed<PV_TPB, PV_TX, PV_TY, PV_TZ>(a.g, a.vol, dim, org, tile, ntiles);
  }
}

// What the relaxation knows of the 26 moves at compile time: the LDS offset of the neighbour, the base cost, and the set of neighbours (bits in
// the order of NVBX_PLAN_MOVES_3D) that must be traversable for the move to be allowed -- the target and, for a diagonal, the 2 or 6 voxels between.
struct PvMoves { int off[26]; int base[26]; uint32_t need[26]; };
constexpr PvMoves pv_moves() {
  constexpr int MV[26][3] = NVBX_PLAN_MOVES_3D;
  PvMoves m{};
  for (int d = 0; d < 26; d++) {
    const int k = (MV[d][0] != 0) + (MV[d][1] != 0) + (MV[d][2] != 0);
    m.off[d] = MV[d][0] * PV_PLANE + MV[d][1] * PV_ROW + MV[d][2];
    m.base[d] = k == 1 ? 10 : k == 2 ? 14 : 17;
    m.need[d] = 0;
    for (int e = 0; e < 26; e++) {        // e is one of p + e iff each of its components is 0 or d's
      bool sub = true;
      for (int c = 0; c < 3; c++) sub = sub && (MV[e][c] == 0 || MV[e][c] == MV[d][c]);
      if (sub) m.need[d] |= 1u << e;
    }
  }
  return m;
}

__global__ __launch_bounds__(PV_TPB) void k_plan3d_relax(Plan3Args a, int32_t parity) {
  __shared__ int32_t s_h[PV_HX * PV_PLANE];
  constexpr PvMoves M = pv_moves();
  const int t = threadIdx.x;
  const int32_t ntiles = a.ntx * a.nty * a.ntz;
  uint8_t* cur = a.g.active + (size_t)parity * ntiles;
  uint8_t* nxt = a.g.active + (size_t)(parity ^ 1) * ntiles;
  for (int32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int on = cur[tile];
    __syncthreads();                      // (every thread has read the flag; the previous tile's LDS readers are done)
    if (!on) continue;                    // uniform
    if (t == 0) cur[tile] = 0;            // this set is the next round's target: its owner empties it
    int32_t tx, ty, tz; pv_tile(a, tile, &tx, &ty, &tz);
    for (int i = t; i < PV_CELLS; i += PV_TPB) {
      const int hz = i % PV_HZ, hy = (i / PV_HZ) % PV_HY, hx = i / (PV_HZ * PV_HY);
      const int32_t x = tx * PV_TX + hx - 1, y = ty * PV_TY + hy - 1, z = tz * PV_TZ + hz - 1;
      int32_t h = -1;                     // not traversable, or outside the volume
      if (x >= 0 && y >= 0 && z >= 0 && x < a.nx && y < a.ny && z < a.nz) {
        const int64_t g = pv_at(a, x, y, z);
        const int32_t k = a.g.cls[g], c = a.g.cost[g];
        if (k >= 0) h = c == NVBX_COST_UNREACHED ? c : c + k;
      }
      s_h[hx * PV_PLANE + hy * PV_ROW + hz] = h;
    }
    __syncthreads();
    int li[PV_PPT]; int32_t kp[PV_PPT], g0[PV_PPT], g[PV_PPT]; uint32_t ok[PV_PPT];
#pragma unroll
    for (int k = 0; k < PV_PPT; k++) {
      int lx, ly, lz; pv_local(t + PV_TPB * k, &lx, &ly, &lz);
      li[k] = (lx + 1) * PV_PLANE + (ly + 1) * PV_ROW + lz + 1;
      const int32_t h = s_h[li[k]];
      ok[k] = 0; kp[k] = 0; g[k] = NVBX_COST_UNREACHED;
      if (h >= 0) {                       // traversable, hence inside the volume
        kp[k] = a.g.cls[pv_at(a, tx * PV_TX + lx, ty * PV_TY + ly, tz * PV_TZ + lz)];
        g[k] = h == NVBX_COST_UNREACHED ? h : h - kp[k];
        uint32_t trav = 0;
#pragma unroll
        for (int d = 0; d < 26; d++) trav |= (uint32_t)(s_h[li[k] + M.off[d]] >= 0) << d;
#pragma unroll
        for (int d = 0; d < 26; d++) ok[k] |= (uint32_t)((trav & M.need[d]) == M.need[d]) << d;
      }
      g0[k] = g[k];
    }
    int sweep = 0, more = 0;
    do {
      int ch = 0;
#pragma unroll
      for (int k = 0; k < PV_PPT; k++) {
        if (!ok[k]) continue;             // not traversable, or no move leads here
        uint32_t best = (uint32_t)g[k], okk = ok[k];
        asm volatile("" : "+v"(okk));     // (opaque per sweep: otherwise the 26 bit tests are hoisted out of the loop as 52 lane masks, more SGPRs than there are)
#pragma unroll
        for (int d = 0; d < 26; d++) {
          // unsigned, so that one min does it: a blocked neighbour holds 0xffffffff, an unreached one 0x7fffffff (+ c: above every cost, no
          // wrap), and a move that is not allowed is raised to 0xffffffff by the sign-extended complement of its bit
          const uint32_t h = (uint32_t)s_h[li[k] + M.off[d]];          // (a neighbour may hold its old or its new value in this sweep: both are bounds)
          const uint32_t shut = ~(uint32_t)((int32_t)(okk << (31 - d)) >> 31);
          best = min(best, (h + (uint32_t)(M.base[d] + kp[k])) | shut);
        }
        if (best < (uint32_t)g[k]) { g[k] = (int32_t)best; s_h[li[k]] = (int32_t)best + kp[k]; ch = 1; }
      }
      sweep++;
      more = __syncthreads_or(ch);
    } while (more && sweep < a.g.sweeps);
    int any = 0;
#pragma unroll
    for (int k = 0; k < PV_PPT; k++) {
      if (!(g[k] < g0[k])) continue;      // (a voxel outside the volume is not traversable and never falls)
      int i = t + PV_TPB * k;
      asm volatile("" : "+v"(i));         // (opaque: the rim tests below are worked out here, not kept as lane masks across the sweeps)
      int lx, ly, lz; pv_local(i, &lx, &ly, &lz);
      a.g.cost[pv_at(a, tx * PV_TX + lx, ty * PV_TY + ly, tz * PV_TZ + lz)] = g[k];
      any = 1;
      const int dx = lx == 0 ? -1 : lx == PV_TX - 1 ? 1 : 0, dy = ly == 0 ? -1 : ly == PV_TY - 1 ? 1 : 0, dz = lz == 0 ? -1 : lz == PV_TZ - 1 ? 1 : 0;
      const bool okx = dx != 0 && tx + dx >= 0 && tx + dx < a.ntx, oky = dy != 0 && ty + dy >= 0 && ty + dy < a.nty, okz = dz != 0 && tz + dz >= 0 && tz + dz < a.ntz;
#pragma unroll
      for (int e = 1; e < 8; e++) {       // the face, edge and corner neighbours that hold this voxel in their halo
        if (((e & 1) && !okx) || ((e & 2) && !oky) || ((e & 4) && !okz)) continue;
        const int32_t qx = tx + ((e & 1) ? dx : 0), qy = ty + ((e & 2) ? dy : 0), qz = tz + ((e & 4) ? dz : 0);
        nxt[(qx * a.nty + qy) * a.ntz + qz] = 1;
      }
    }
    plan_grid_round_end(a.g, nxt, tile, any, more);
  }
}

struct PvGrid {                           // the 26 moves of nvbx_plan3d_math.h, for the walk
  static constexpr int D = 3, MOVES = 26;
  __device__ static int move(int d, int c) { constexpr int MV[26][3] = NVBX_PLAN_MOVES_3D; return MV[d][c]; }
  __device__ static int k(int d) { return d < NVBX_PLAN_MOVES_3D_AXIS ? 1 : d < NVBX_PLAN_MOVES_3D_FACE ? 2 : 3; }
  __device__ static int32_t step(int k, int32_t kp, int32_t kq) { return nvbx_plan3d_step(k, kp, kq); }
};

__global__ __launch_bounds__(64) void k_plan3d_trace(PlanTraceArgs<3> a) { plan_grid_trace<PvGrid>(a); }

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" int nvbx_cost_volume(nvbx_mapper* m, const float* volume_dev, int32_t nx, int32_t ny, int32_t nz, const nvbx_cost_options* options,
                                const int32_t* sources_xyz_dev, int32_t n_sources, int32_t* cost_dev, int32_t* accepted_dev) {
  const char* who = "nvbx_cost_volume";
  const int32_t dim[3] = {nx, ny, nz};
  if (const int rc = plan_grid_check_field<3>(who, PV_WORDS, m, volume_dev, dim, options, sources_xyz_dev, n_sources, cost_dev)) return rc;
  Plan3Args a{};
  a.vol = volume_dev; a.nx = nx; a.ny = ny; a.nz = nz;
  a.ntx = (nx + PV_TX - 1) / PV_TX; a.nty = (ny + PV_TY - 1) / PV_TY; a.ntz = (nz + PV_TZ - 1) / PV_TZ;
  const int64_t n = (int64_t)nx * ny * nz, ntiles = (int64_t)a.ntx * a.nty * a.ntz;      // at most 2^22 / 8 tiles: a line of voxels
  if (const int rc = plan_grid_setup(m, &a.g, n, ntiles, options, sources_xyz_dev, n_sources, cost_dev)) return rc;
  const dim3 grid((unsigned)ntiles);
  NVBX_LAUNCH(m, k_plan3d_classify, grid, dim3(PV_TPB), a);
  return plan_grid_relax(m, who, PV_WORDS.product, a.g, n, [&](int32_t parity) { NVBX_LAUNCH(m, k_plan3d_relax, grid, dim3(PV_TPB), a, parity); }, accepted_dev);
}

extern "C" int nvbx_trace_paths_3d(nvbx_mapper* m, const float* volume_dev, int32_t nx, int32_t ny, int32_t nz, const nvbx_cost_options* options,
                                   const int32_t* cost_dev, const int32_t* starts_xyz_dev, int32_t n_starts, int32_t* path_xyz_dev, int32_t capacity,
                                   int32_t* length_dev) {
  const int32_t dim[3] = {nx, ny, nz};
  return plan_grid_trace_call<3>("nvbx_trace_paths_3d", PV_WORDS, m, volume_dev, dim, options, cost_dev, starts_xyz_dev, n_starts, path_xyz_dev, capacity, length_dev,
                                 [&](const PlanTraceArgs<3>& a, dim3 grid, dim3 block) { NVBX_LAUNCH(m, k_plan3d_trace, grid, block, a); });
}
