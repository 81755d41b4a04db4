// nvbx_view.h -- the view calculation shared by every depth path ([U] ViewCalculator::getBlocksInImageViewRaycast restated): the sensor
// models (pinhole camera, spinning LiDAR), the block walk and the view-marking launch k_mark_view.  Included by tsdf.hip (camera frames and
// the depth-frame state machine), lidar.hip (the LiDAR-only launches) and measure.hip (the multi-GPU measurement exchange).
//
//   k_mark_view      one wavefront per 8x8 tile of the sub-sampled ray grid.  Phase 1: each lane walks its ray through
//                    the block grid (Amanatides-Woo) and drops the block keys into a 4-8 KiB LDS set (rays of one tile
//                    share almost all their blocks) -- no HBM access inside the walk.  Phase 2 (flush): the set is
//                    compacted (ballot + popcount) and ONE key per lane goes to HBM: CAS insert-if-absent into the hash
//                    (device-side allocation from the slot stack), per-entry frame stamp, and a wave-aggregated append
//                    of {slot, Index3D} to the frame's view list (exactly once per block and frame).  A camera tile
//                    (< 100 blocks) flushes once; long LiDAR rays flush whenever the set is half full.
// The sensor models, FrameSet and the kernels live in the global namespace: the kernel names they spell are what profiles/ and tools/ match.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include "nvbx_mapper.h"
#include "nvbx_lidar_math.h"
#include "nvbx_esdf_edt.h"
#include "nvbx_sphere_trace.h"
#include "nvbx_esdf_mark.h"
#include "nvbx_color_worker.h"

using namespace nvbx;

// Per-workgroup time stamps (-DNVBX_WG_TIMES variant, tools/wg_timeline*.py; nothing in the product build): s_memrealtime, a constant 100 MHz clock
// shared by all CUs, into the buffer of nvbx_debug_wg_times (tsdf.hip) -- a translation unit that records defines NVBX_WGT_HERE (nvbx_internal.h).
#ifdef NVBX_WG_TIMES
#define NVBX_T(k, i) NVBX_TV(k, i, wall_clock64())
#else
#define NVBX_T(k, i) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------ sensor models
// Camera(fu, fv, cu, cv, w, h): conversions/image_conversions.cpp:27-32.  Everything it needs is in Frame.
struct CameraSensor {
  static constexpr bool kLongRays = false;
#ifndef NVBX_CAM_TR
#define NVBX_CAM_TR 8
#define NVBX_CAM_TC 8
#define NVBX_CAM_SEG 1
#endif
#ifndef NVBX_CAM_GR
#define NVBX_CAM_GR 2
#define NVBX_CAM_GC 2
#endif
  static constexpr int kTileRows = NVBX_CAM_TR, kTileCols = NVBX_CAM_TC;     // rays per wavefront: one tile of the ray grid (tools/lidar_tile_sweep.sh cam)
  static constexpr int kSetSize = 512, kFlushRounds = 2; // a tile crosses < 100 blocks: 4 KiB set, 128 keys per flush pass
  static constexpr int kSegments = NVBX_CAM_SEG;         // lanes per ray
  static constexpr int kProbeDepth = 2;                  // hash probe positions fetched up front per key in a flush
  static constexpr bool kRiders = true;                  // workers of other passes may ride in the view-marking launch (256 threads each: a riding worker uses four wavefronts as it likes)
  static constexpr int kThreads = 64 * NVBX_CAM_GR * NVBX_CAM_GC;      // one wavefront per tile: the tiles of a group share the workgroup's key set
  // Tiles per workgroup: kGroupRows x kGroupCols NEIGHBOURING tiles share ONE LDS key set.  Every ray starts in the camera's block and
  // the rays of neighbouring tiles run through the same blocks for their first metres, so with one tile per workgroup the block at the
  // origin had its stamp claimed by ALL 336 tiles of a 640x480 frame at the same moment -- returning atomics on one address serialise
  // at ~12 ns each in the memory-side atomic unit (tools/micro/atomic_scope_bench.hip: 336 of them = 4.0 us for the last; whatever the
  // scope, there are no XCD-local atomics) -- and the tiles' flush took 4.2 of their 10.7 us (tools/wg_timeline.py).  Four tiles per set:
  // a quarter of the contenders on every hot stamp, and the workgroup's other three wavefronts, idle before, do the work.
  static constexpr int kGroupRows = NVBX_CAM_GR, kGroupCols = NVBX_CAM_GC;
  // end point (camera frame) of the ray through the centre of pixel (prow, pcol) at depth `de` along the optical axis
  __device__ void ray_end(const Frame& f, int prow, int pcol, float de, float* pc) const {
    const float rx = (((float)pcol + 0.5f) - f.cu) / f.fu;
    const float ry = (((float)prow + 0.5f) - f.cv) / f.fv;
    pc[0] = de * rx; pc[1] = de * ry; pc[2] = de;
  }
  // measured depth at the voxel centre `pc` and the voxel's own depth; 1 = update, 0 = voxel not touched,
  // -1 = the voxel projects onto invalid depth (weight decays if invalid_depth_decay_factor >= 0)
  template <typename Img>
  __device__ int sample(const Frame& f, const Img& depth, const float* pc, float* ds, float* vd) const {
    float u, v;
    if (!cam_project(f, pc, &u, &v)) return 0;
    *vd = pc[2];
    if (f.max_dist > 0.0f && *vd > f.max_dist) return 0;
    return interp_depth(depth, f.rows, f.cols, u, v, f.interp_nearest, ds);
  }
};

// Lidar: nvbx_lidar_math.h.  el_tab[k] = {sin, cos} of beam row k's elevation, az_tab[j] = {sin, cos} of column j's azimuth.
struct LidarSensor {
  static constexpr bool kLongRays = true;
  // long rays: the walk is a serial chain per ray and the flushes are chains of dependent HBM round trips, so the lever is the number
  // of wavefronts in flight: FEW rays per wavefront, MANY lanes per ray.  A 200 m ray is ~250 dependent block steps; its lanes share
  // it: lane s replays the (cheap, insert-free) traversal up to its segment -- the same float operations in the same order, so the
  // state is bit-identical -- and then walks only its segment with set inserts.  Measured (tools/lidar_tile_sweep.sh, 1024x64 beams,
  // ray subsampling 2, us per scan): 4x4 rays x 4 segments 155 | 2x4x8 113 | 2x2x16 82 | 1x4x16 74 | 1x2x32 75 | 1x1x64 111.
#ifndef NVBX_LIDAR_TR
#define NVBX_LIDAR_TR 1
#define NVBX_LIDAR_TC 2
#define NVBX_LIDAR_SEG 32
#endif
  static constexpr int kTileRows = NVBX_LIDAR_TR, kTileCols = NVBX_LIDAR_TC;      // (tuning knobs: tools/lidar_tile_sweep.sh)
#ifndef NVBX_LIDAR_FR
#define NVBX_LIDAR_FR 6
#define NVBX_LIDAR_PD 4
#endif
#ifndef NVBX_LIDAR_SET
#define NVBX_LIDAR_SET 1024
#define NVBX_LIDAR_FLUSH 256
#endif
  static constexpr int kSetSize = NVBX_LIDAR_SET, kFlushRounds = NVBX_LIDAR_FR; // early flush at 256 keys: 6 x 64 >= 256 + one step's additions
  static constexpr int kSegments = NVBX_LIDAR_SEG;
  static constexpr int kProbeDepth = NVBX_LIDAR_PD;
  static constexpr bool kRiders = false;
  static constexpr int kThreads = 64;
  static constexpr int kGroupRows = 1, kGroupCols = 1;   // one tile (bundle of rays) per workgroup
  nvbx_lidar_model l;
  const float2* el_tab; const float2* az_tab;
  float max_diff_m, max_ray_dist_m;
  __device__ void beam_dir(int row, int col, float* d) const {
    const float2 e = el_tab[row], a = az_tab[col];
    d[0] = e.y * a.y; d[1] = e.y * a.x; d[2] = e.x;
  }
  __device__ void ray_end(const Frame&, int prow, int pcol, float de, float* pc) const {
    float d[3]; beam_dir(prow, pcol, d);
    pc[0] = de * d[0]; pc[1] = de * d[1]; pc[2] = de * d[2];
  }
  // [U] interpolateLidarImage restated: bilinear if the four beams are valid and agree within max_diff_m, else the
  // nearest beam if the voxel centre lies within max_ray_dist_m of that beam's ray.  Depth = range along the beam.
  template <typename Img>
  __device__ int sample(const Frame& f, const Img& img, const float* pc, float* ds, float* vd) const { int px; return sample_px(f, img, pc, ds, vd, &px); }
  // the same, also reporting which rule measured: *nearest_px = pixel index (row * cols + col) of the beam the nearest-beam rule used, -1 otherwise
  template <typename Img>
  __device__ int sample_px(const Frame& f, const Img& img, const float* pc, float* ds, float* vd, int* nearest_px) const {
    *nearest_px = -1;
    const float r = nvbx_lidar_range(pc);
    *vd = r;
    if (f.max_dist > 0.0f && r > f.max_dist) return 0;      // (before the projection: it costs two atan2)
    float u, v;
    if (!nvbx_lidar_project(&l, pc, r, &u, &v)) return 0;
    const float uc = u - 0.5f, vc = v - 0.5f;
    const float fx = floorf(uc), fy = floorf(vc);
    const int x0 = (int)fx, y0 = (int)fy;
    if (!(x0 < 0 || y0 < 0 || x0 + 1 > f.cols - 1 || y0 + 1 > f.rows - 1)) {
      const int32_t i00 = pix(y0, x0, f.cols);
      const float f00 = img(i00), f10 = img(i00 + 1), f01 = img(i00 + f.cols), f11 = img(i00 + f.cols + 1);
      __builtin_amdgcn_sched_barrier(0);      // both rows' loads in flight before the first tap is looked at (else: two serial round trips)
      if (depth_valid4(f00, f10, f01, f11)) {
        const float mx = fmaxf(fmaxf(f00, f10), fmaxf(f01, f11)), mn = fminf(fminf(f00, f10), fminf(f01, f11));
        if (mx - mn <= max_diff_m) {
          const float ax = uc - fx, ay = vc - fy;
          const float top = __builtin_fmaf(ax, f10, (1.0f - ax) * f00);
          const float bot = __builtin_fmaf(ax, f11, (1.0f - ax) * f01);
          *ds = __builtin_fmaf(ay, bot, (1.0f - ay) * top);
          return 1;
        }
      }
    }
    const int c = (int)floorf(u), rr = (int)floorf(v);
    if (c < 0 || rr < 0 || c >= f.cols || rr >= f.rows) return 0;
    const float d = img(pix(rr, c, f.cols));
    if (!depth_valid(d)) return 0;
    float dir[3]; beam_dir(rr, c, dir);
    const float dot = __builtin_fmaf(pc[2], dir[2], __builtin_fmaf(pc[1], dir[1], pc[0] * dir[0]));
    const float ex = __builtin_fmaf(-dot, dir[0], pc[0]), ey = __builtin_fmaf(-dot, dir[1], pc[1]), ez = __builtin_fmaf(-dot, dir[2], pc[2]);
    // (squared distances compared: one IEEE square root less per voxel on the VALU-bound LiDAR path; the oracle does the same)
    if (__builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)) > max_ray_dist_m * max_ray_dist_m) return 0;
    *ds = d;
    *nearest_px = pix(rr, c, f.cols);
    return 1;
  }
};

constexpr int LSET_FLUSH = NVBX_LIDAR_FLUSH;     // early-flush threshold (long rays): keeps the 1024-entry set <= ~30 % full, probes short


// Claim an entry's stamp word for (frame, camera bit); `cur` = the word as last seen.  True iff THIS call moved the entry to the
// frame (the caller then appends the block to the view list exactly once); otherwise it only makes sure the camera's bit is set.
__device__ inline bool stamp_claim(uint32_t* p, uint32_t cur, uint32_t frame_id, uint32_t cam_bit) {
  const uint32_t want = (frame_id << 8) | cam_bit;
  for (;;) {
    if (stamp_frame(cur) == frame_id) { if (!(cur & cam_bit)) atomicOr(p, cam_bit); return false; }
    const uint32_t old = atomicCAS(p, cur, want);
    if (old == cur) return true;
    cur = old;                          // another tile got there first (or `cur` was a guess): look again
  }
}
// One block key -> HBM: insert-if-absent, stamp the entry with this frame (and this camera's bit), and report whether THIS call was
// the first of the frame to do so (the caller then appends {slot, x, y, z} to the view list exactly once).  The common case -- the
// block exists and a neighbouring tile has stamped it already -- is ONE 16-B load: key, slot and stamp arrive together.
// `entry_out` (optional): the block's hash entry whenever it exists after the call (-1: table full) -- also when this call was not the
// first, so that a caller that needs the slot of a block ANOTHER thread of the same launch has just inserted never has to look the key
// up again with plain loads (hash_find may read a stale EMPTY from L1 / a non-coherent L2 and report "absent").
__device__ inline bool mark_block(const DMap& m, u64 key, uint32_t frame_id, uint32_t cam_bit, int4* rec_out, int32_t* entry_out = nullptr) {
  int32_t x, y, z; unpack_key(key, &x, &y, &z);
  uint32_t h = table_pos(m, x, y, z);
  uint32_t slot = SLOT_INVALID, cur = STAMP_NEVER;
  bool found = false;
  if (entry_out) *entry_out = -1;
  for (uint32_t probe = 0; probe <= m.mask; ++probe) {
    const uint4 e = *reinterpret_cast<const uint4*>(&m.table[h]);
    const u64 k = ((u64)e.y << 32) | (u64)e.x;
    if (k == key) { if (entry_out) *entry_out = (int32_t)h; if (stamp_frame(e.w) == frame_id && (e.w & cam_bit)) return false; slot = e.z; cur = e.w; found = true; break; }
    if (k == KEY_EMPTY) break;           // (may be a stale EMPTY: hash_insert's CAS is the truth)
    h = (h + 1) & m.mask;
  }
  if (!found) {
    bool is_new;
    const int32_t hi = hash_insert(m, x, y, z, F_TSDF, &is_new);
    if (hi < 0) return false;
    h = (uint32_t)hi;
    if (entry_out) *entry_out = hi;
  }
  if (!stamp_claim(&m.table[h].stamp, cur, frame_id, cam_bit)) return false;
  while (slot == SLOT_INVALID) slot = ld_slot_acquire(&m.table[h]);     // the inserting lane publishes right after its CAS
  *rec_out = make_int4((int32_t)slot, x, y, z);
  return true;
}

// wave-aggregated append of this lane's record (if `first`) to the frame's view list: one returning atomic per wave
__device__ inline void view_append(int32_t* cnt, int4* view_list, int32_t list_cap, bool first, int4 rec, int lane) {
  const u64 mask = __ballot(first);
  if (!mask) return;
  int32_t base = 0;
  const int leader = __ffsll((long long)mask) - 1;
  if (lane == leader) base = atomicAdd(cnt, (int32_t)__popcll(mask));
  base = __shfl(base, leader);
  if (first) {
    const int32_t pos = base + (int32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (pos < list_cap) view_list[pos] = rec;
  }
}

// [U] workspace bounds of the view calculator (workspace_bounds_type, mapper_initialization.cpp:337-358): a block is kept
// iff its cube overlaps the bounds (height bounds: z only)
__device__ inline bool block_in_workspace(const Frame& f, int32_t bx, int32_t by, int32_t bz) {
  if (f.ws_type == 0) return true;
  const int32_t cur[3] = {bx, by, bz};
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (f.ws_type == 1 && a < 2) continue;
    const float lo = (float)cur[a] * f.block_size, hi = (float)(cur[a] + 1) * f.block_size;
    if (!(hi > f.ws_min[a]) || !(lo < f.ws_max[a])) ok = false;
  }
  return ok;
}
// insert `key` into the tile's LDS set; false = probe window exhausted (caller sends the key to HBM itself)
template <int LSET>
__device__ inline bool lset_insert(u64* lset, int32_t bx, int32_t by, int32_t bz, u64 key, bool* added) {
  static_assert((LSET & (LSET - 1)) == 0, "power of two");
  const uint32_t lh = ((index_hash(bx, by, bz) * 2654435761u) >> 16) & (LSET - 1);
  *added = false;
#pragma unroll 1
  for (int p = 0; p < 16; p++) {
    const u64 old = atomicCAS(&lset[(lh + p) & (LSET - 1)], KEY_EMPTY, key);
    if (old == KEY_EMPTY) { *added = true; return true; }
    if (old == key) return true;
  }
  return false;
}
// Amanatides-Woo: advance to the next block along the ray (select without dynamic register indexing)
// Amanatides-Woo through the block grid with the crossing parameters in CLOSED FORM: crossing number k of axis a lies at
//   T_a(k) = fmaf(k, tdelta_a, tmax0_a)            (one rounding; the checker evaluates the same fmaf: oracle/nvblox_oracle.c raycast_blocks)
// instead of tmax_a accumulated by k additions.  Same traversal up to the last bit of a near-tie -- and a state that depends on the crossing
// COUNTS (n_x, n_y, n_z) alone, so a lane can enter the traversal at any step in O(1) (dda_jump) instead of replaying every step before it:
// a LiDAR lane used to replay up to 234 steps of a 200 m ray before its own 16 (35 of the slowest bundle's 78 us, tools/wg_timeline_lidar.py).
// A step: the axis with the smallest next crossing (ties: x before y before z), select-only.
struct Dda { int32_t cur[3], step[3], n[3]; float t0[3], dt[3], tm[3]; };
__device__ inline float dda_T(const Dda& d, int a, int32_t k) { return __builtin_fmaf((float)k, d.dt[a], d.t0[a]); }
__device__ inline void dda_step(Dda& d) {
  const bool s1 = d.tm[1] < d.tm[0];
  const float m01 = s1 ? d.tm[1] : d.tm[0];
  const bool s2 = d.tm[2] < m01;
  const bool a0 = !s1 && !s2, a1 = s1 && !s2;
  d.n[0] += a0 ? 1 : 0; d.n[1] += a1 ? 1 : 0; d.n[2] += s2 ? 1 : 0;
  d.cur[0] += a0 ? d.step[0] : 0; d.cur[1] += a1 ? d.step[1] : 0; d.cur[2] += s2 ? d.step[2] : 0;
  d.tm[0] = dda_T(d, 0, d.n[0]); d.tm[1] = dda_T(d, 1, d.n[1]); d.tm[2] = dda_T(d, 2, d.n[2]);
}
// undo the last step taken: of the crossings taken, the one with the LARGEST parameter (ties: z before y before x -- the reverse of dda_step's order)
__device__ inline void dda_unstep(Dda& d) {
  const float l0 = d.n[0] > 0 ? dda_T(d, 0, d.n[0] - 1) : -1.0f, l1 = d.n[1] > 0 ? dda_T(d, 1, d.n[1] - 1) : -1.0f, l2 = d.n[2] > 0 ? dda_T(d, 2, d.n[2] - 1) : -1.0f;
  const bool s2 = d.n[2] > 0 && l2 >= l1 && l2 >= l0;
  const bool a1 = !s2 && d.n[1] > 0 && l1 >= l0;
  const bool a0 = !s2 && !a1 && d.n[0] > 0;
  d.n[0] -= a0 ? 1 : 0; d.n[1] -= a1 ? 1 : 0; d.n[2] -= s2 ? 1 : 0;
  d.cur[0] -= a0 ? d.step[0] : 0; d.cur[1] -= a1 ? d.step[1] : 0; d.cur[2] -= s2 ? d.step[2] : 0;
  d.tm[0] = dda_T(d, 0, d.n[0]); d.tm[1] = dda_T(d, 1, d.n[1]); d.tm[2] = dda_T(d, 2, d.n[2]);
}
// Enter the traversal after exactly K steps (from the initial state).  (1) a parameter tau at which about K crossings have happened (the crossing
// density is linear in the parameter); (2) the EXACT state "every crossing with T < tau taken" -- counted per axis with the same fmaf the
// traversal compares, so it is a state the step-by-step traversal passes through whatever the estimate was; (3) a few steps forwards or
// backwards until the count is K.  `inv[a]` = 1 / tdelta_a (0 for an axis the ray does not move along).
__device__ inline void dda_jump(Dda& d, int32_t K, const float* inv) {
  const float s1 = (inv[0] + inv[1]) + inv[2];
  float s0 = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; a++) s0 = s0 + (inv[a] > 0.0f ? 1.0f - d.t0[a] * inv[a] : 0.0f);
  const float tau = s1 > 0.0f ? ((float)K - s0) / s1 : 0.0f;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    int32_t k = 0;
    if (inv[a] > 0.0f) {
      const float e = ceilf((tau - d.t0[a]) * inv[a]);
      k = e > 0.0f ? (e < 1.0e6f ? (int32_t)e : 1000000) : 0;
      while (k > 0 && dda_T(d, a, k - 1) >= tau) k--;
      while (k < 1000000 && dda_T(d, a, k) < tau) k++;
    }
    d.n[a] = k; d.cur[a] += k * d.step[a]; d.tm[a] = dda_T(d, a, k);
  }
  int32_t have = (d.n[0] + d.n[1]) + d.n[2];
  while (have < K) { dda_step(d); have++; }
  while (have > K) { dda_unstep(d); have--; }
}
// The ray of depth pixel (prow, pcol) with measured depth `d` through the block grid: traversal state at the sensor's block, number of block
// steps to the block of the end point min(d + truncation, max integration distance) (-1: no ray -- inactive lane or invalid depth), 1 / tdelta.
template <typename Sensor>
__device__ inline int32_t view_ray_setup(const Frame& f, const Sensor& sensor, bool& active, float d, int prow, int pcol, Dda& dd, float* inv_dt) {
  int32_t nsteps = -1;
  if (active) {
    if (!(d > 0.0f)) active = false;
    else {
      float de = d + f.trunc;
      if (f.max_dist > 0.0f && de > f.max_dist) de = f.max_dist;
      float pc[3], pl[3];
      sensor.ray_end(f, prow, pcol, de, pc);
      apply_rt(f.R_LC, f.t_LC, pc[0], pc[1], pc[2], pl);
      nsteps = 0;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const float s = f.t_LC[a] / f.block_size, t = pl[a] / f.block_size;
        dd.cur[a] = (int32_t)floorf(s);
        const int32_t end = (int32_t)floorf(t);
        const int32_t db = end - dd.cur[a]; nsteps += db < 0 ? -db : db;
        const float ray = t - s;
        dd.step[a] = ray > 0.0f ? 1 : (ray < 0.0f ? -1 : 0);
        const float corrected = dd.step[a] > 0 ? 1.0f : 0.0f;
        const float dist_to_boundary = corrected - (s - (float)dd.cur[a]);
        if (fabsf(ray) < 1e-9f) { dd.t0[a] = 2.0f; dd.dt[a] = 2.0f; }
        else { dd.t0[a] = dist_to_boundary / ray; dd.dt[a] = (float)dd.step[a] / ray; inv_dt[a] = fabsf(ray); }
        dd.tm[a] = dd.t0[a];
      }
    }
  }
  return nsteps;
}
// Flush: compact the set (ballot + popcount), then every key goes to HBM with the dependent round trips taken
// PHASE-WISE over up to R keys per lane at once: (A) the first PD probe positions of every key are loaded together
// (2 cover ~98 % of lookups at a room-sized map's load factor, 4 are used for the larger LiDAR maps), (B) resolved -- a key further down its probe chain, a new block, or a
// slot not published yet takes the general mark_block path, (C) the frame-stamp exchanges of all keys not yet stamped
// are issued together, (D) ONE wave-aggregated returning atomicAdd reserves view-list space for all first-stampers,
// (E) records are stored.  A camera tile flushes ~60 keys in one such pass; a long LiDAR bundle 256+ keys per pass
// instead of 64 per dependent round.  Whole wave must call.
// NW = wavefronts of the workgroup that share the set (camera: 4 tiles per workgroup; LiDAR: 1): wave w compacts the w-th part of the
// set, the parts' counts meet in LDS (s_part), and key number i of the compacted list goes to thread i of the workgroup.
template <int LSET, int R, int PD, int NW = 1>
__device__ inline void flush_set(const DMap& m, const Frame& f, u64* lset, u64* lkeys, int32_t* cnt, int4* view_list, int32_t list_cap,
                                 int lane, bool clear, int32_t* s_part = nullptr) {
  __syncthreads();
  const int wave = NW > 1 ? (int)(threadIdx.x >> 6) : 0;
  constexpr int PART = LSET / NW;
  static_assert(PART % 64 == 0, "whole wavefronts per part");
  int32_t nk = 0;
  if (NW > 1) {              // counts first: where this wave's keys go depends on the parts before it
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < PART / 64; i++) c += (int32_t)__popcll(__ballot(lset[wave * PART + i * 64 + lane] != KEY_EMPTY));
    if (lane == 0) s_part[wave] = c;
    __syncthreads();
    int32_t before = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) { const int32_t cw = s_part[w]; if (w < wave) before += cw; nk += cw; }
    int32_t pos = before;
#pragma unroll
    for (int i = 0; i < PART / 64; i++) {
      const u64 kk = lset[wave * PART + i * 64 + lane];
      const u64 mask = __ballot(kk != KEY_EMPTY);
      if (kk != KEY_EMPTY) lkeys[pos + (int32_t)__popcll(mask & ((1ull << lane) - 1ull))] = kk;
      pos += (int32_t)__popcll(mask);
      if (clear) lset[wave * PART + i * 64 + lane] = KEY_EMPTY;
    }
  } else {
#pragma unroll
    for (int i = 0; i < LSET / 64; i++) {
      const u64 kk = lset[i * 64 + lane];
      const u64 mask = __ballot(kk != KEY_EMPTY);
      if (kk != KEY_EMPTY) lkeys[nk + (int32_t)__popcll(mask & ((1ull << lane) - 1ull))] = kk;
      nk += (int32_t)__popcll(mask);
      if (clear) lset[i * 64 + lane] = KEY_EMPTY;
    }
  }
  __syncthreads();
  NVBX_T(0, 3);
#ifndef NVBX_WGT_WALK_START
  if (NW > 1) NVBX_TV(0, 6, nk);
#endif
  // key number kb + r * (NW * 64) + (this thread's number in the workgroup): wave w takes the w-th 64 keys of every round
  const int tlane = NW > 1 ? (int)threadIdx.x : lane;
  for (int32_t kb = 0; kb < nk; kb += R * NW * 64) {         // one pass per R x NW x 64 keys (workgroup-uniform)
    const int rounds = min(R, (nk - kb + NW * 64 - 1) / (NW * 64));
    u64 key[R]; uint32_t h[R]; uint4 e[R][PD]; bool have[R];
    // (A) the first PD probe positions of every key, all in flight
#pragma unroll
    for (int r = 0; r < R; r++) {
      have[r] = r < rounds && (kb + r * NW * 64 + tlane) < nk;
      key[r] = have[r] ? lkeys[kb + r * NW * 64 + tlane] : KEY_EMPTY;
      int32_t x, y, z; unpack_key(key[r], &x, &y, &z);
      h[r] = have[r] ? table_pos(m, x, y, z) : 0u;
    }
#pragma unroll
    for (int r = 0; r < R; r++) if (r < rounds) {
#pragma unroll
      for (int q = 0; q < PD; q++) e[r][q] = *reinterpret_cast<const uint4*>(&m.table[(h[r] + q) & m.mask]);
    }
    // (B) resolve + (C) stamp exchanges in flight
    bool fast[R], first[R], claim[R], ins[R]; uint32_t old[R], seen[R], slot[R], hpos[R]; int4 rec[R];
    const uint32_t want = (f.frame_id << 8) | f.cam_bit;
    bool any_ins = false;
#pragma unroll
    for (int r = 0; r < R; r++) {
      fast[r] = false; first[r] = false; claim[r] = false; ins[r] = false; old[r] = 0u; seen[r] = 0u; hpos[r] = 0u; slot[r] = SLOT_INVALID; rec[r] = make_int4(0, 0, 0, 0);
      if (r < rounds && have[r]) {
        uint32_t hh = h[r], st = 0; bool open = true, hit = false;        // open: no EMPTY entry seen yet on the probe chain
        int qe = -1;                                                      // first EMPTY position of the chain, if the key is not in front of it
#pragma unroll
        for (int q = 0; q < PD; q++) {
          const u64 kq = ((u64)e[r][q].y << 32) | (u64)e[r][q].x;
          if (open && !fast[r] && kq == key[r]) { slot[r] = e[r][q].z; st = e[r][q].w; hh = (h[r] + q) & m.mask; fast[r] = true; hit = true; }
          if (open && kq == KEY_EMPTY) { open = false; if (!hit) qe = q; }
        }
        if (slot[r] == SLOT_INVALID) fast[r] = false;              // being inserted right now: general path waits for the slot
        if (fast[r]) {
          hpos[r] = hh; seen[r] = st;
          if (stamp_frame(st) != f.frame_id) { claim[r] = true; old[r] = atomicCAS(&m.table[hh].stamp, st, want); }   // the returning atomics of a pass: in flight together
          else if (!(st & f.cam_bit)) atomicOr(&m.table[hh].stamp, f.cam_bit);     // stamped by another camera of this batch: add our bit (not waited for)
        } else if (qe >= 0) { ins[r] = true; any_ins = true; hpos[r] = (h[r] + qe) & m.mask;        // a NEW block (as far as this pass can see)
        }
      }
    }
    // (B') new blocks, batch-wise: the pass's key inserts in flight together, then ONE pop of the free stack for all the wavefront's winners
    // (hash_insert pops one slot per block: two returning atomics on ONE address each -- free-stack top and high-water mark --, ~12 ns apiece
    // chip-wide, i.e. 2.7 ms of a first LiDAR scan's 112 k new blocks before anything else; and a chain of ~8 dependent round trips per key, R
    // keys one after the other).  A lane that loses its insert (another wavefront's key landed in the entry first) takes the general path.
    bool won[R];
#pragma unroll
    for (int r = 0; r < R; r++) won[r] = false;
    if (__ballot(any_ins)) {
      u64 oldk[R];
#pragma unroll
      for (int r = 0; r < R; r++) if (ins[r]) oldk[r] = atomicCAS(&m.table[hpos[r]].key, KEY_EMPTY, key[r]);
      int32_t wtotal = 0, wpre[R];
#pragma unroll
      for (int r = 0; r < R; r++) {
        won[r] = ins[r] && oldk[r] == KEY_EMPTY;
        const u64 mask = __ballot(won[r]);
        wpre[r] = wtotal + (int32_t)__popcll(mask & ((1ull << lane) - 1ull));
        wtotal += (int32_t)__popcll(mask);
      }
      if (wtotal) {
        int32_t top = 0;
        if (lane == 0) {
          top = atomicSub(&m.counters[C_FREE_TOP], wtotal);
          if (top < wtotal) { atomicAdd(&m.counters[C_FREE_TOP], wtotal - (top > 0 ? top : 0)); atomicExch(&m.counters[C_OVERFLOW], 1); }     // pool exhausted: give back what was not there
        }
        top = __shfl(top, 0);
        uint32_t ost[R];
#pragma unroll
        for (int r = 0; r < R; r++) if (won[r]) {
          const int32_t idx = top - 1 - wpre[r];
          slot[r] = idx >= 0 ? m.free_stack[idx] : SLOT_NONE;
          ost[r] = atomicCAS(&m.table[hpos[r]].stamp, STAMP_NEVER, want);          // (a fresh entry's stamp; somebody may have met the key and claimed it already)
        }
        int32_t hwm = 0;
#pragma unroll
        for (int r = 0; r < R; r++) if (won[r]) {
          int32_t x, y, z; unpack_key(key[r], &x, &y, &z);
          if (slot_ok(slot[r])) {
            m.slot_index[3 * slot[r]] = x; m.slot_index[3 * slot[r] + 1] = y; m.slot_index[3 * slot[r] + 2] = z;
            m.slot_entry[slot[r]] = hpos[r];
            atomicOr(&m.slot_flags[slot[r]], F_TSDF);
            hwm = max(hwm, (int32_t)slot[r] + 1);
          }
          __hip_atomic_store(&m.table[hpos[r]].slot, slot[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // published: every winner of the pass BEFORE this wavefront waits for anybody else's
          first[r] = ost[r] == STAMP_NEVER || stamp_claim(&m.table[hpos[r]].stamp, ost[r], f.frame_id, f.cam_bit);
          rec[r] = make_int4((int32_t)slot[r], x, y, z);
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) hwm = max(hwm, __shfl_xor(hwm, o));
        if (lane == 0 && hwm) atomicMax(&m.counters[C_HIGH_WATER], hwm);
      }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (r < rounds && have[r]) {
        if (fast[r]) {
          first[r] = claim[r] && (old[r] == seen[r] || stamp_claim(&m.table[hpos[r]].stamp, old[r], f.frame_id, f.cam_bit));   // (a lost CAS: another tile claimed it, add our bit)
          if (first[r]) { int32_t x, y, z; unpack_key(key[r], &x, &y, &z); rec[r] = make_int4((int32_t)slot[r], x, y, z); }
        } else if (!won[r]) {
          first[r] = mark_block(m, key[r], f.frame_id, f.cam_bit, &rec[r]);     // longer probe chain, a lost insert, or slot not published yet
        }
      }
    }
    NVBX_T(0, 4);
    // (D) one reservation for the whole pass
    int32_t total = 0; int32_t pre[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const u64 mask = (r < rounds) ? __ballot(first[r]) : 0ull;
      pre[r] = total + (int32_t)__popcll(mask & ((1ull << lane) - 1ull));
      total += (int32_t)__popcll(mask);
    }
    if (total) {
      int32_t base = 0;
      if (lane == 0) base = atomicAdd(cnt, total);
      base = __shfl(base, 0);
      // (E)
#pragma unroll
      for (int r = 0; r < R; r++) if (r < rounds && first[r]) { const int32_t pos = base + pre[r]; if (pos < list_cap) view_list[pos] = rec[r]; }
      NVBX_T(0, 5);
    }
  }
  __syncthreads();
}

// Workgroups [0, n_edt_wg) (camera launches only, when an EDT was held back by updateEsdf) are EDT workers with all four
// wavefronts -- dispatched first: the EDT is the longer chain; the workgroups after them mark the view (first wavefront only).
// The frames of one launch set: ONE depth frame, or a batch of up to MAX_BATCH camera frames of the same image size that
// nvbx_integrate_depth_batch integrates with one view-marking launch and one TSDF-update launch (the reference feeds up to four
// cameras through one mapper, one integrateDepth call each: nvblox_node.hpp:298-332).  Kernel argument (SGPRs / scalar loads).
template <typename Img, int NB> struct FrameSet { Frame f[NB]; Img img[NB]; int32_t n; };

// workgroups of one frame's view marking: its tile groups, padded to a multiple of the XCD count (XCD-banded numbering in the kernel)
template <typename Sensor> static int mark_view_tile_wgs(const Frame& f) {
  const int tiles_x = (f.n_ray_cols + Sensor::kTileCols - 1) / Sensor::kTileCols, tiles_y = (f.n_ray_rows + Sensor::kTileRows - 1) / Sensor::kTileRows;
  const int n_groups = ((tiles_x + Sensor::kGroupCols - 1) / Sensor::kGroupCols) * ((tiles_y + Sensor::kGroupRows - 1) / Sensor::kGroupRows);
  return NSH * ((n_groups + NSH - 1) / NSH);
}
template <typename Sensor> static size_t mark_view_smem(bool edt_rides) {
  const size_t mark = 2 * (size_t)Sensor::kSetSize * sizeof(u64);
  return (Sensor::kRiders && edt_rides && sizeof(EdtShared) > mark) ? sizeof(EdtShared) : mark;
}
// Occupancy of the two fused launches, by batch size (the attribute's arguments depend on the template parameter).  One camera frame launches ~960
// workgroups -- fewer than are resident at the compiler's own register choice (87 VGPRs = 5 waves per SIMD = 1 280 workgroups of four wavefronts), and
// squeezing it costs time (8 waves per SIMD asked for: 11.2 -> 13.1 us).  A batch of eight launches 2 256: the tiles, dispatched behind the riders,
// started when the first 1 280 workgroups were done (11-15 us into a 31 us launch, tools/wg_timeline_batch.py) -- there 8 waves per SIMD (64 VGPRs,
// 26 spilled to scratch) are worth it: 31.6 -> 26.9 us; the fused TSDF / colour launch likewise (three 8-wavefront workgroups per CU -> four): 30.5 -> 28.6 us.
#ifndef NVBX_MARK_VIEW_ATTR
#define NVBX_MARK_VIEW_ATTR __attribute__((amdgpu_waves_per_eu(NB > 1 ? 8 : 1, NB > 1 ? 8 : 8)))
#endif
#ifndef NVBX_FUSED_ATTR
#define NVBX_FUSED_ATTR __attribute__((amdgpu_waves_per_eu(NB > 1 ? 8 : 1, NB > 1 ? 8 : 8)))
#endif
// The launch's body as a function of the workgroup's NUMBER (`wg_index`, not blockIdx.x): k_mark_view passes blockIdx.x; k_mark_view_pair (round 6) runs the
// bodies of TWO mappers' view-marking launches in one grid -- the second mapper's workgroups are numbered from its own 0 (every part's count is a multiple
// of 8, so blockIdx.x & 7 -- the shard of the sharded counters, my_shard() -- is also wg_index & 7).
template <typename Img, typename Sensor, int NB>
__device__ __forceinline__ void mark_view_body(const DMap& m, const FrameSet<Img, NB>& fs, const Sensor& sensor, int4* view_list, int32_t list_cap,
                                               int32_t reset_esdf_dirty, int32_t n_edt_wg, const EsdfArgs& ea, const TraceRiderT<NB>& tr, const int32_t wg_index, unsigned char* smem) {
  constexpr int LSET = Sensor::kSetSize, FR = Sensor::kFlushRounds;
  int32_t tile_wg = wg_index;      // this workgroup's number among the tiles
  NVBX_T(0, 0);
  // this launch has STARTED, so every launch enqueued before it on the stream has finished -- among them the tr.fence_report colour-reading launches
  // whose images' frames wait for exactly this news (frames.hip)
  if (wg_index == 0 && threadIdx.x == 0) __hip_atomic_store(&m.host_mirror[4], tr.fence_report, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (Sensor::kRiders) {
    // riders: [EDT workers][sphere-tracing workers of a held-back colour frame (colour deferral)] -- before the tiles, or
    // (tr.n_tile_wg > 0) after them.  All counts are multiples of 8, so a workgroup's XCD (blockIdx.x & 7) is also its number's & 7.
    const int32_t rider = tr.n_tile_wg > 0 ? wg_index - tr.n_tile_wg : wg_index;
    const bool is_rider = tr.n_tile_wg > 0 ? rider >= 0 : rider < n_edt_wg + tr.n_wg + tr.n_scan_wg + tr.n_mark_wg;
    if (is_rider) {
      if (Sensor::kThreads > 256 && threadIdx.x >= 256) return;      // (a rider is a 256-thread worker: the wavefronts a wider tile group needs go home at once -- they are not waited for by the others' barriers)
      if (rider < n_edt_wg) esdf_edt_worker(m, ea, (int)rider, n_edt_wg, reinterpret_cast<EdtShared*>(smem));
      // (sphere tracing: all four wavefronts; independent of the view marking -- it reads the TSDF and the insert-only hash, and new entries point at all-zero blocks)
      else if (rider < n_edt_wg + tr.n_wg) {
        const int tw = (int)(rider - n_edt_wg);
        if (NB > 1 && tr.lanes == 2) sphere_trace_worker<NB, 2>(m, tr.ps, tr.synth, tr.srows, tr.scols, tr.max_steps, tr.max_len, tr.eps_m, tw);
        else if (tr.lanes == 4) sphere_trace_worker<NB, 4>(m, tr.ps, tr.synth, tr.srows, tr.scols, tr.max_steps, tr.max_len, tr.eps_m, tw);
        else sphere_trace_worker<NB, 8>(m, tr.ps, tr.synth, tr.srows, tr.scols, tr.max_steps, tr.max_len, tr.eps_m, tw);
      }
      // (candidate discovery of the held-back colour frame(s), for the fused colour + TSDF launch that follows: four wavefronts of 64 slots each)
      else if (rider < n_edt_wg + tr.n_wg + tr.n_scan_wg)
        color_scan_worker<NB>(m, tr.ps, tr.cand, tr.cand_cnt_idx, tr.cand_reset_idx, (int)(rider - n_edt_wg - tr.n_wg) * 4 + (int)(threadIdx.x >> 6), tr.n_scan_wg * 4);
      // (ESDF site marking of the held-back update, first wavefront only: it reads the TSDF as the last update left it -- nothing in this launch
      //  writes voxels -- and allocates ESDF blocks beside the view marking's TSDF blocks; `ea` is its argument then: no EDT rides, n_edt_wg = 0)
      // (all four wavefronts are workers -- a frame dirties ~300 blocks, 4 x 256 workers take at most one entry each: an entry is a chain of
      //  dependent round trips, and a worker with two of them was the launch's tail; the workgroup then counts itself in as one arrival)
      else {
        const int w = (int)(rider - n_edt_wg - tr.n_wg - tr.n_scan_wg);
        esdf_mark_worker(m, ea, w * 4 + (int)(threadIdx.x >> 6), tr.n_mark_wg * 4);
        if (ea.self_reset) { __syncthreads(); if (threadIdx.x < 64) esdf_mark_pass_done(m, ea, tr.n_mark_wg, w); }
      }
      if (rider >= n_edt_wg) NVBX_INV_TSDF_READER(m);       // (sphere tracing, candidates, marking: still no TSDF writer beside them when they end)
      NVBX_T(0, 7);
      return;
    }
    if (tr.n_tile_wg == 0) tile_wg -= n_edt_wg + tr.n_wg + tr.n_scan_wg + tr.n_mark_wg;
  }
  __shared__ int32_t s_part[8];
  u64* lset = reinterpret_cast<u64*>(smem);
  u64* lkeys = lset + LSET;
  const int lane = threadIdx.x & 63;
  constexpr int TR = Sensor::kTileRows, TC = Sensor::kTileCols, NSEG = Sensor::kSegments;
  constexpr int GR = Sensor::kGroupRows, GC = Sensor::kGroupCols, NW = GR * GC;       // tiles (wavefronts) per workgroup
  static_assert(TR * TC * NSEG <= 64, "one wavefront per tile");
  static_assert(NW * 64 == Sensor::kThreads && NW <= 8, "one wavefront per tile of the group");
  const int wave = NW > 1 ? (int)(threadIdx.x >> 6) : 0;
  const Frame& f0 = fs.f[0];                    // (image size, subsampling and view frame id are the same for every frame of a batch)
  const int tiles_x = (f0.n_ray_cols + TC - 1) / TC, tiles_y = (f0.n_ray_rows + TR - 1) / TR;
  const int groups_x = (tiles_x + GC - 1) / GC, groups_y = (tiles_y + GR - 1) / GR;
  // XCD-aware numbering: workgroups go round-robin over the 8 XCDs (each with its own L2), so the tile groups of one XCD (wg & 7) are a
  // contiguous band of group rows -- neighbouring tiles share most of their blocks, i.e. their hash lines (n_edt_wg is a multiple of 8)
  const int wg_all = (int)tile_wg;
  const int n_groups = groups_x * groups_y, per_xcd = (n_groups + NSH - 1) / NSH;
  const int cam = NB > 1 ? wg_all / (NSH * per_xcd) : 0;        // batch: NSH * per_xcd workgroups per camera, camera after camera
  const int wg = wg_all - cam * (NSH * per_xcd);
  const Frame& f = fs.f[cam < fs.n ? cam : 0];
  const Img& depth = fs.img[cam < fs.n ? cam : 0];
  const int group = (wg & (NSH - 1)) * per_xcd + (wg >> 3);
  const int gy = group / groups_x, gx = group - gy * groups_x;
  const int ty = gy * GR + wave / GC, tx = gx * GC + wave % GC;
  const bool tile_ok = (wg >> 3) < per_xcd && group < n_groups && cam < fs.n && ty < tiles_y && tx < tiles_x;
  const int ray = lane / NSEG, seg = lane % NSEG;
  const int ri = ty * TR + ray / TC, ci = tx * TC + ray % TC;
  bool active = tile_ok && ray < TR * TC && ri < f.n_ray_rows && ci < f.n_ray_cols;
  // the ray's depth pixel is requested first: its HBM round trip overlaps the LDS set initialisation
  int prow = ri * f.subsample; if (prow >= f.rows) prow = f.rows - 1;
  int pcol = ci * f.subsample; if (pcol >= f.cols) pcol = f.cols - 1;
  const float d = active ? depth(pix(prow, pcol, f.cols)) : 0.0f;
  for (int i = (int)threadIdx.x; i < LSET; i += NW * 64) lset[i] = KEY_EMPTY;
  if (wg_all == 0 && threadIdx.x == 0) m.counters[C_VIEW_COUNT + ((f.frame_id + 1) & 3)] = 0;   // next frame's counter
  if (Sensor::kLongRays && wg_all == 0 && threadIdx.x < NSH) { *shc_at(m, S_LIDAR_SPARSE, threadIdx.x, 0) = 0; *shc_at(m, S_LIDAR_SPARSE, threadIdx.x, 1) = 0; }     // (field 1: the dense launch's work list, filled by the beam-centric one)
  // an ESDF dirty list already consumed by a marking pass (fused into integrateColor) is emptied before k_integrate_tsdf appends
  if (reset_esdf_dirty && wg_all == 0 && threadIdx.x < NSH) *shc_at(m, S_LIST_ESDF_DIRTY, threadIdx.x, 0) = 0;
  __syncthreads();
  NVBX_T(0, 1);

  Dda dd{};                                     // traversal state of this lane's ray (cur = block, n = crossings taken per axis)
  float inv_dt[3] = {0.0f, 0.0f, 0.0f};          // 1 / tdelta per axis (= |ray| in blocks), for dda_jump
  const int32_t nsteps = view_ray_setup(f, sensor, active, d, prow, pcol, dd, inv_dt);
  // this lane's share of the ray: steps [k0, k1]; the traversal is ENTERED at step k0 (dda_jump: no replay of the steps before it)
  int32_t k0 = 0, k1 = nsteps;
  if (NSEG > 1 && nsteps >= 0) {
    const int32_t q = (nsteps + NSEG) / NSEG;                  // ceil((nsteps + 1) / NSEG)
    k0 = seg * q; k1 = min(nsteps, k0 + q - 1);
    if (k0 > nsteps) k1 = -1;                                   // short ray: nothing left for this segment
    else if (k0 > 0) dda_jump(dd, k0, inv_dt);
  }
  int32_t* cnt = &m.counters[C_VIEW_COUNT + (f.frame_id & 3)];
#ifdef NVBX_WGT_WALK_START
  NVBX_TV(0, 6, wall_clock64() + (unsigned long long)(nsteps & 0));        // (experiment: when the ray set-up is done -- the depth pixel has arrived)
#endif
  if (!Sensor::kLongRays) {
    // camera: a tile's rays cross < 100 blocks in ~20 steps -- walk every ray to its end, then flush once
    for (int32_t k = k0; k <= k1; k++) {                   // (this lane's segment of the ray; the whole ray if it is not shared)
      const u64 key = pack_key(dd.cur[0], dd.cur[1], dd.cur[2]);
      const bool inside = block_in_workspace(f, dd.cur[0], dd.cur[1], dd.cur[2]);
      const uint32_t lh = ((index_hash(dd.cur[0], dd.cur[1], dd.cur[2]) * 2654435761u) >> 16) & (LSET - 1);
      // first probe issued, the traversal step runs in the shadow of the LDS round trip, then the result is looked at
      u64 old = KEY_EMPTY;
      if (inside) old = atomicCAS(&lset[lh], KEY_EMPTY, key);
      dda_step(dd);
      bool spill = false;
      if (inside && old != KEY_EMPTY && old != key) {          // occupied by another block: continue along the probe window
        spill = true;
#pragma unroll 1
        for (int p = 1; p < 16; p++) {
          const u64 o2 = atomicCAS(&lset[(lh + p) & (LSET - 1)], KEY_EMPTY, key);
          if (o2 == KEY_EMPTY || o2 == key) { spill = false; break; }
        }
      }
      if (__ballot(spill)) {                     // probe window exhausted (rare): this key goes to HBM directly
        int4 rec = make_int4(0, 0, 0, 0);
        const bool first = spill && mark_block(m, key, f.frame_id, f.cam_bit, &rec);
        view_append(cnt, view_list, list_cap, first, rec, lane);
      }
    }
    NVBX_T(0, 2);
    flush_set<LSET, FR, Sensor::kProbeDepth, NW>(m, f, lset, lkeys, cnt, view_list, list_cap, lane, false, s_part);
    NVBX_T(0, 7);
    return;
  }
  // LiDAR: hundreds of steps per ray and little sharing at long range -- wave-uniform loop, flush whenever the set is
  // half full
  int32_t nset = 0;                                   // keys in the LDS set (wave-uniform)
#ifdef NVBX_WG_TIMES
  unsigned long long t_flush = 0, n_flush = 0, n_keys = 0;     // (tools/wg_timeline_lidar.py: time inside the flushes, their number, keys sent to HBM)
#endif
  for (int32_t j = 0; __ballot(k0 + j <= k1) != 0ull; j++) {
    bool spill = false, added = false;
    u64 key = KEY_EMPTY;
    if (k0 + j <= k1) {
      key = pack_key(dd.cur[0], dd.cur[1], dd.cur[2]);
      spill = block_in_workspace(f, dd.cur[0], dd.cur[1], dd.cur[2]) && !lset_insert<LSET>(lset, dd.cur[0], dd.cur[1], dd.cur[2], key, &added);
      dda_step(dd);
    }
    nset += (int32_t)__popcll(__ballot(added));
    if (__ballot(spill)) {
      int4 rec = make_int4(0, 0, 0, 0);
      const bool first = spill && mark_block(m, key, f.frame_id, f.cam_bit, &rec);
      view_append(cnt, view_list, list_cap, first, rec, lane);
    }
    const bool last = __ballot(k0 + j + 1 <= k1) == 0ull;
#ifdef NVBX_WG_TIMES
    const unsigned long long tf0 = (last || nset > LSET_FLUSH) ? wall_clock64() : 0ull;
    if (last || nset > LSET_FLUSH) NVBX_TV(0, 1, tf0);          // (slot 1: start of the LAST flush; slots 3, 4, 5: its phases, flush_set)
#endif
    if (last || nset > LSET_FLUSH) {
      flush_set<LSET, FR, Sensor::kProbeDepth>(m, f, lset, lkeys, cnt, view_list, list_cap, lane, !last);
#ifdef NVBX_WG_TIMES
      t_flush += wall_clock64() - tf0; n_flush++; n_keys += (unsigned long long)nset;
#endif
      nset = 0;
    }
  }
#ifdef NVBX_WG_TIMES
  NVBX_TV(0, 2, t_flush); NVBX_TV(0, 6, (n_flush << 32) | n_keys); NVBX_T(0, 7);
#endif
}

template <typename Img, typename Sensor, int NB>
__global__ __launch_bounds__(Sensor::kThreads) NVBX_MARK_VIEW_ATTR void k_mark_view(DMap m, FrameSet<Img, NB> fs, Sensor sensor, int4* view_list, int32_t list_cap,
                                                                int32_t reset_esdf_dirty, int32_t n_edt_wg, EsdfArgs ea, TraceRiderT<NB> tr) {
  // LDS: the tile's key set (2 * LSET u64), or -- when a distance transform rides (camera, classic order) -- at least an EdtShared; sized by
  // the launch (mark_view_smem below): EVERY workgroup of the launch holds it, the riders too, and it decides how many are resident
  // (a batch of 8 cameras: 2 688 tile workgroups beside 1 200 sphere-tracing ones)
  extern __shared__ __align__(16) unsigned char smem[];
  mark_view_body<Img, Sensor, NB>(m, fs, sensor, view_list, list_cap, reset_esdf_dirty, n_edt_wg, ea, tr, (int32_t)blockIdx.x, smem);
}
static_assert(sizeof(DMap) + sizeof(FrameSet<DepthF32, MAX_BATCH>) + sizeof(TraceRiderT<MAX_BATCH>) + sizeof(EsdfArgs) + 64 <= 4096, "k_mark_view<.., MAX_BATCH>: kernel arguments");

// (host) the sub-sampled ray grid of every frame of a launch set (ray indices i with i * s < rows + s - 1) and the frame's camera bit
template <typename Img, int NB> static void size_ray_grid(FrameSet<Img, NB>& fs) {
  const int s = fs.f[0].subsample;
  for (int c = 0; c < fs.n; c++) {
    fs.f[c].n_ray_rows = (fs.f[c].rows + s - 1 + s - 1) / s;
    fs.f[c].n_ray_cols = (fs.f[c].cols + s - 1 + s - 1) / s;
    fs.f[c].cam_bit = 1u << c;
  }
}

// (host) what the depth paths call across files -- library-internal, not exported
#pragma GCC visibility push(hidden)
int next_frame_id(nvbx_mapper* m);                                                                   // tsdf.hip
int integrate_lidar_frame(nvbx_mapper* m, FrameSet<DepthF32, 1> fs, const LidarSensor& sensor);     // tsdf.hip
void launch_mark_view_camera(nvbx_mapper* m, const FrameSet<DepthF32, 1>& fs);                       // tsdf.hip
int launch_view_grid(nvbx_mapper* m, const FrameSet<DepthF32, 1>& fs, const LidarSensor& sensor, int tiles, int32_t fence_report, bool* used);     // lidar.hip
int launch_lidar_sparse(nvbx_mapper* m, const FrameSet<DepthF32, 1>& fs, const LidarSensor& sensor, bool plain, uint8_t** view_class, int32_t** dense_list);
int wgt_bind_lidar(unsigned long long* buf);     // lidar.hip, -DNVBX_WG_TIMES: that translation unit's time-stamp buffer
#pragma GCC visibility pop
