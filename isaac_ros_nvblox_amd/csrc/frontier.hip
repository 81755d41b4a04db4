// frontier.hip -- where known free space ends and the unseen begins, and how much unseen space a pose would look into (SEMANTICS.md
// "Frontiers and view gain"): nvbx_find_frontiers scans the TSDF layer for free voxels with unknown face neighbours and
// returns them as a labelled sparse voxel volume of the shape nvbx_match_features returns, nvbx_frontier_clusters chains that scan with
// nvbx_label_components, nvbx_view_gain walks the rays of nvbx_render_view through the voxel classes.  All three read TSDF voxels only.
//
// k_find_frontiers: a 512-thread workgroup per TSDF slot, thread = voxel z + 8y + 64x, so wavefront w holds the slab x = w and a __ballot
// of a class is that slab as one 64-bit word (bit 8y + z).  The block's classes are 16 words in LDS (free, unknown); a workgroup with no
// free voxel, or none inside the box, ends there.  Otherwise six lanes resolve the face neighbours (find_slot), wavefront f < 6 classifies
// the facing 8 x 8 face of neighbour f into one more word (a missing neighbour: all unknown), and every thread counts its six neighbours
// from LDS with shifts.  A block with a frontier voxel claims its entry with one atomic add on the output count.
// k_view_gain: a lane per ray, workgroups grouped by view; the lane keeps the last resolved {block, slot} and probes the hash only when a
// sample leaves that block; four wave-level sums, four atomics per wavefront into the view's record.
#include <algorithm>
#include <cmath>
#include "nvbx_mapper.h"
#include "nvbx_projective.h"

using namespace nvbx;

constexpr int FR_TPB = 512;

struct FrontierArgs {
  float min_weight, free_dist;
  int32_t min_unknown;
  int32_t box[6];                                  // inclusive, global voxel coordinates: min x y z, max x y z
  int32_t* block_idx; int32_t* label; float* score;
  int64_t capacity; unsigned long long* count;
};

// the voxel classes of SEMANTICS.md: observed = weight >= min_weight (in a block that carries the TSDF layer), free = observed and
// distance > free_dist (a NaN distance is not free), unknown = not observed
__device__ inline bool fr_observed(float2 v, float min_weight) { return v.y >= min_weight; }
__device__ inline bool fr_free(float2 v, float min_weight, float free_dist) { return fr_observed(v, min_weight) && v.x > free_dist; }
__device__ inline int fr_bit(u64 w, int b) { return (int)((w >> b) & 1ull); }


__global__ __launch_bounds__(FR_TPB) void k_find_frontiers(DMap m, FrontierArgs a) {
  __shared__ u64 s_free[8], s_unk[8], s_face[6];      // own slabs (bit 8y + z); faces -x +x (bit 8y + z), -y +y (8x + z), -z +z (8x + y)
  __shared__ uint32_t s_nb[6];
  __shared__ long long s_e;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int vx = w, vy = (t >> 3) & 7, vz = t & 7;
  const int32_t hw = min(m.counters[C_HIGH_WATER], (int32_t)m.capacity);
  for (int32_t slot = blockIdx.x; slot < hw; slot += gridDim.x) {
    if (!(m.slot_flags[slot] & F_TSDF)) continue;      // uniform
    const int32_t bx = m.slot_index[3 * slot], by = m.slot_index[3 * slot + 1], bz = m.slot_index[3 * slot + 2];
    const int32_t gx = (int32_t)(8u * (uint32_t)bx) + vx, gy = (int32_t)(8u * (uint32_t)by) + vy, gz = (int32_t)(8u * (uint32_t)bz) + vz;
    const bool inbox = gx >= a.box[0] && gx <= a.box[3] && gy >= a.box[1] && gy <= a.box[4] && gz >= a.box[2] && gz <= a.box[5];
    __syncthreads();                                   // (the previous block's readers are done)
    const float2 v = m.tsdf[(size_t)slot * 512 + t];
    const bool is_free = fr_free(v, a.min_weight, a.free_dist);
    const u64 fw = __ballot(is_free), uw = __ballot(!fr_observed(v, a.min_weight));
    if (lane == 0) { s_free[w] = fw; s_unk[w] = uw; }
    if (!__syncthreads_or(is_free && inbox)) continue;      // no free voxel (inside the box): no neighbour is touched
    if (t < 6) {      // face neighbour t: axis t >> 1, direction -1 / +1
      const int d = (t & 1) ? 1 : -1;
      const int32_t nx = bx + ((t >> 1) == 0 ? d : 0), ny = by + ((t >> 1) == 1 ? d : 0), nz = bz + ((t >> 1) == 2 ? d : 0);
      s_nb[t] = nvbx_index_in_range(nx, ny, nz) ? find_slot(m, nx, ny, nz, F_TSDF) : SLOT_NONE;
    }
    __syncthreads();
    if (w < 6) {
      // the neighbour's face that touches this block: its coordinate on the axis is 7 on the low side, 0 on the high side; lane = 8 p + q
      const uint32_t ns = s_nb[w];
      const int axis = w >> 1, c0 = (w & 1) ? 0 : 7, p = lane >> 3, q = lane & 7;
      bool unk = true;
      if (slot_ok(ns)) {
        const int nt = axis == 0 ? 64 * c0 + lane : axis == 1 ? 64 * p + 8 * c0 + q : 64 * p + 8 * q + c0;
        unk = !fr_observed(m.tsdf[(size_t)ns * 512 + nt], a.min_weight);
      }
      const u64 fb = __ballot(unk);
      if (lane == 0) s_face[w] = fb;
    }
    __syncthreads();
    int nu = 0;
    if (is_free) {
      const int b = 8 * vy + vz;
      nu += vx > 0 ? fr_bit(s_unk[vx - 1], b) : fr_bit(s_face[0], b);
      nu += vx < 7 ? fr_bit(s_unk[vx + 1], b) : fr_bit(s_face[1], b);
      nu += vy > 0 ? fr_bit(s_unk[vx], b - 8) : fr_bit(s_face[2], 8 * vx + vz);
      nu += vy < 7 ? fr_bit(s_unk[vx], b + 8) : fr_bit(s_face[3], 8 * vx + vz);
      nu += vz > 0 ? fr_bit(s_unk[vx], b - 1) : fr_bit(s_face[4], 8 * vx + vy);
      nu += vz < 7 ? fr_bit(s_unk[vx], b + 1) : fr_bit(s_face[5], 8 * vx + vy);
    }
    const bool frontier = is_free && inbox && nu >= a.min_unknown;
    if (!__syncthreads_or(frontier)) continue;
    if (t == 0) s_e = (long long)atomicAdd(a.count, 1ull);
    __syncthreads();
    const long long e = s_e;
    if (e >= a.capacity) continue;                     // uniform: counted, not written anywhere
    if (t < 3) a.block_idx[3 * e + t] = m.slot_index[3 * slot + t];
    a.label[(size_t)e * 512 + t] = frontier ? 0 : -1;
    if (a.score) a.score[(size_t)e * 512 + t] = frontier ? (float)nu : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------ view gain
struct GainArgs {
  const float* poses; int32_t n_views;
  float fu, fv, cu, cv; int32_t subsample, srows, scols;
  float voxel_size, max_range, pose_lim, min_weight, free_dist;
  int32_t* gains;                                      // [n_views][4]: rays, unknown_samples, free_samples, rays_hit
};
constexpr int GAIN_TPB = 256;

__device__ inline int32_t wave_sum(int32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(GAIN_TPB) void k_view_gain(DMap m, GainArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int n_rays = a.srows * a.scols;
  const float2* pool = m.tsdf;
  for (int32_t view = blockIdx.y; view < a.n_views; view += gridDim.y) {
    float T[12];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const float x = a.poses[16 * (size_t)view + i];
      ok = ok && fabsf(x) < INFINITY;
      if (i < 12) T[i] = x;
    }
    // nvbx_pose_in_range on the device: finite, and the range stays inside the addressable blocks
    ok = ok && fabsf(T[3]) < a.pose_lim && fabsf(T[7]) < a.pose_lim && fabsf(T[11]) < a.pose_lim;
    int32_t* rec = a.gains + 4 * (size_t)view;
    if (!ok) {                                         // uniform: the record stays zero, rays = -1
      if (blockIdx.x == 0 && tid == 0) rec[0] = -1;
      continue;
    }
    const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    const float o[3] = {T[3], T[7], T[11]};
    const int ray = (int)blockIdx.x * GAIN_TPB + tid;
    const bool valid = ray < n_rays;
    const int r = valid ? ray / a.scols : 0, c = valid ? ray - r * a.scols : 0;
    float dl[3];      // the ray of nvbx_render_view (k_render, render.hip): the same function
    (void)pinhole_ray(a.fu, a.fv, a.cu, a.cv, a.subsample, R, r, c, dl);
    int32_t n_unknown = 0, n_free = 0, n_hit = 0;
    if (valid) {
      int32_t lbx = 0, lby = 0, lbz = 0; uint32_t lslot = SLOT_NONE; bool have = false;
      for (int32_t k = 0; k < (1 << 23); k++) {        // (k + 0.5 is exact in f32; a range the pose check accepts ends far below)
        const float t = ((float)k + 0.5f) * a.voxel_size;
        if (!(t < a.max_range)) break;
        const float px = o[0] + t * dl[0], py = o[1] + t * dl[1], pz = o[2] + t * dl[2];
        const int32_t gx = voxel_of(px, a.voxel_size), gy = voxel_of(py, a.voxel_size), gz = voxel_of(pz, a.voxel_size);
        const int32_t bx = gx >> 3, by = gy >> 3, bz = gz >> 3;
        if (!have || bx != lbx || by != lby || bz != lbz) {
          lslot = nvbx_index_in_range(bx, by, bz) ? find_slot(m, bx, by, bz, F_TSDF) : SLOT_NONE;
          lbx = bx; lby = by; lbz = bz; have = true;
        }
        float2 v = make_float2(0.0f, 0.0f);
        if (slot_ok(lslot)) v = pool[(size_t)lslot * 512 + (gz & 7) + 8 * (gy & 7) + 64 * (gx & 7)];
        if (!slot_ok(lslot) || !fr_observed(v, a.min_weight)) n_unknown++;
        else if (v.x > a.free_dist) n_free++;
        else { n_hit = 1; break; }
      }
    }
    const int32_t s_rays = wave_sum(valid ? 1 : 0), s_unk = wave_sum(n_unknown), s_fr = wave_sum(n_free), s_hit = wave_sum(n_hit);
    if (lane == 0 && s_rays) {
      atomicAdd(&rec[0], s_rays); atomicAdd(&rec[1], s_unk); atomicAdd(&rec[2], s_fr); atomicAdd(&rec[3], s_hit);
    }
  }
}

// ------------------------------------------------------------------------------------------------ C-ABI
namespace {

int frontier_check(const nvbx_mapper* m, const char* who, float min_weight, float free_distance_m, int32_t min_unknown, const int32_t* box,
                   const void* block_idx, const void* label, int64_t capacity, const void* count) {
  if (tsdf_reader_refused(m, who)) return NVBX_E_INVALID;
  if (min_unknown < 1 || min_unknown > 6) return refuse(who, ": min_unknown_neighbours must be 1 .. 6");
  if (std::isnan(min_weight) || std::isnan(free_distance_m)) return refuse(who, ": min_weight / free_distance_m is not a number");
  return sparse_volume_refused(who, box, block_idx, label, capacity, count);
}

// the launches of nvbx_find_frontiers; the arguments have been checked
int frontier_launch(nvbx_mapper* m, float min_weight, float free_distance_m, int32_t min_unknown, const int32_t* box, nvbx_index3d* block_idx_dev,
                    int32_t* label_dev, float* score_dev, int64_t capacity, int64_t* count_dev) {
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;      // TSDF voxels and flags only: held-back colour and ESDF work stays held back (query.hip)
  FrontierArgs a{};
  a.min_weight = min_weight; a.free_dist = free_distance_m; a.min_unknown = min_unknown;
  for (int k = 0; k < 3; k++) { a.box[k] = box ? box[k] : INT32_MIN; a.box[3 + k] = box ? box[3 + k] : INT32_MAX; }
  a.block_idx = reinterpret_cast<int32_t*>(block_idx_dev); a.label = label_dev; a.score = score_dev;
  a.capacity = capacity; a.count = reinterpret_cast<unsigned long long*>(count_dev);
  const dim3 grid((unsigned)std::min<int64_t>(m->capacity, 8192));
  NVBX_HIP(hipMemsetAsync(count_dev, 0, sizeof(int64_t), m->stream));
  NVBX_LAUNCH(m, k_find_frontiers, grid, dim3(FR_TPB), m->d, a);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

}  // namespace

extern "C" int nvbx_find_frontiers(nvbx_mapper* m, float min_weight, float free_distance_m, int32_t min_unknown_neighbours, const int32_t box_min_max_vox[6],
                                   nvbx_index3d* block_idx_dev, int32_t* label_dev, float* score_dev, int64_t capacity_blocks, int64_t* count_dev) {
  if (!m) return NVBX_E_INVALID;
  const int rc = frontier_check(m, "nvbx_find_frontiers", min_weight, free_distance_m, min_unknown_neighbours, box_min_max_vox, block_idx_dev, label_dev,
                                capacity_blocks, count_dev);
  if (rc) return rc;
  return frontier_launch(m, min_weight, free_distance_m, min_unknown_neighbours, box_min_max_vox, block_idx_dev, label_dev, score_dev, capacity_blocks, count_dev);
}

extern "C" int nvbx_frontier_clusters(nvbx_mapper* m, float min_weight, float free_distance_m, int32_t min_unknown_neighbours, const int32_t box_min_max_vox[6],
                                      int32_t connectivity, int32_t min_voxels, nvbx_index3d* block_idx_dev, int32_t* label_dev, float* score_dev,
                                      int32_t* component_id_dev, int64_t capacity_blocks, int64_t* block_count_dev, nvbx_component* components_dev,
                                      int64_t capacity_components, int64_t* component_count_dev) {
  if (!m) return NVBX_E_INVALID;
  const char* who = "nvbx_frontier_clusters";
  int rc = frontier_check(m, who, min_weight, free_distance_m, min_unknown_neighbours, box_min_max_vox, block_idx_dev, label_dev, capacity_blocks, block_count_dev);
  if (rc) return rc;
  // nvbx_label_components' refusals, looked at before the scan is launched: a refused call launches nothing
  rc = seg_check(who, connectivity, min_voxels, capacity_blocks > 0 && !component_id_dev ? ": component_id_dev is required with capacity_blocks > 0" : nullptr,
                 components_dev, capacity_components, component_count_dev);
  if (rc) return rc;
  rc = frontier_launch(m, min_weight, free_distance_m, min_unknown_neighbours, box_min_max_vox, block_idx_dev, label_dev, score_dev, capacity_blocks, block_count_dev);
  if (rc) return rc;
  return nvbx_label_components(m, block_idx_dev, label_dev, score_dev, capacity_blocks, block_count_dev, connectivity, min_voxels, component_id_dev,
                               components_dev, capacity_components, component_count_dev);
}

extern "C" int nvbx_view_gain(nvbx_mapper* m, const float* T_L_C_dev, int32_t n_views, const nvbx_camera* camera, int32_t subsampling, float max_range_m,
                              float min_weight, float free_distance_m, nvbx_gain* gains_dev) {
  if (!m) return NVBX_E_INVALID;
  const char* who = "nvbx_view_gain";
  if (tsdf_reader_refused(m, who)) return NVBX_E_INVALID;
  if (!camera || subsampling < 0 || n_views < 0) return refuse(who, ": invalid argument");
  if (n_views > 0 && (!T_L_C_dev || !gains_dev)) return refuse(who, ": T_L_C_dev and gains_dev are required with n_views > 0");
  if (!nvbx_camera_valid(camera)) return refuse(who, ": invalid camera");
  const SubsampledSize ss = subsampled_size(m, subsampling, camera->height, camera->width);
  if (!ss.ok()) return refuse(who, ": image too small for the subsampling");
  const float reach = max_range_m > 0.0f ? max_range_m : m->p.sphere_tracing_max_ray_length_m;
  if (!std::isfinite(reach)) return refuse(who, ": max_range_m is not finite");
  if (std::isnan(min_weight) || std::isnan(free_distance_m)) return refuse(who, ": min_weight / free_distance_m is not a number");
  if (n_views == 0) return NVBX_OK;
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  GainArgs a{};
  a.poses = T_L_C_dev; a.n_views = n_views;
  a.fu = camera->fu; a.fv = camera->fv; a.cu = camera->cu; a.cv = camera->cv; a.subsample = ss.s; a.srows = ss.rows; a.scols = ss.cols;
  a.voxel_size = m->p.voxel_size; a.max_range = reach;
  a.pose_lim = nvbx_pose_limit(m->p.voxel_size * 8.0f, reach);      // (nvbx_pose_in_range's bound)
  a.min_weight = min_weight; a.free_dist = free_distance_m;
  a.gains = reinterpret_cast<int32_t*>(gains_dev);
  NVBX_HIP(hipMemsetAsync(gains_dev, 0, sizeof(nvbx_gain) * (size_t)n_views, m->stream));
  const dim3 grid((unsigned)(((int64_t)ss.rows * ss.cols + GAIN_TPB - 1) / GAIN_TPB), (unsigned)std::min<int32_t>(n_views, 65535));
  NVBX_LAUNCH(m, k_view_gain, grid, dim3(GAIN_TPB), m->d, a);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}
