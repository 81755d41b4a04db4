// change.hip -- what differs between two maps (nvbx_find_changes / nvbx_change_clusters; SEMANTICS.md "Change detection").
// [U] change detection between mapping sessions: nothing of the kind is readable in the reference tree.
//
// Mapper m ("now") is scanned against a reference mapper ref ("before") under p_M = T_M_R p_R; both are read-only throughout, everything
// runs on m's stream.
//   k_find_changes   one 512-thread workgroup per TSDF slot of m (grid-stride), lane = voxel z + 8y + 64x.  The lane loads and classifies
//                    its own voxel; a block without an observed voxel inside the box ends there, with 4 KiB read and ref never touched.
//                    Otherwise the lanes' sample positions reach at most 3 x 3 x 3 blocks of ref: the workgroup finds the lowest block index
//                    per axis (wave shuffle minimum, one LDS atomic per wavefront), 27 lanes probe ref's table once and leave the slots in
//                    LDS -- none found: the block ends -- and every lane takes its eight corners through that table (change_corners, a copy
//                    of k_merge_fuse's; nearest sampling: one load), classifies the sample and labels its voxel.  A block with a label
//                    claims its entry with one atomic add on the output count, as k_find_frontiers does, and writes 2 KiB of labels
//                    (and 2 KiB of scores).  Three integer wave sums, one atomic each per workgroup.
//   k_change_result  one wavefront: the caller's result record from the counters the scan left.  Only where no voxel was compared does it
//                    look through ref's slot flags for a TSDF block, to tell an empty reference from no overlap.
#include <algorithm>
#include <cmath>
#include "nvbx_mapper.h"
#include "nvbx_query_point.h"
#include "nvbx_merge_math.h"

using namespace nvbx;

constexpr int CH_TPB = 512;

// nvbx_mapper::change_buf, zeroed per call
struct ChangeScratch { unsigned long long scanned, compared, appeared, removed; };
static_assert(sizeof(ChangeScratch) <= 64, "nvbx_mapper::change_buf");
static_assert(sizeof(nvbx_change_result) == 64 && sizeof(nvbx_change_options) == 24, "C-ABI layout");

struct ChangeArgs {
  float R_RM[9], t_RM[3];                          // p_R = R_RM p_M + t_RM: the samples
  float vs, min_weight, ref_min_weight, free_dist, occ_dist;
  int32_t nearest;
  int32_t box[6];                                  // inclusive, global voxel coordinates of m: min x y z, max x y z
  int32_t* block_idx; int32_t* label; float* score;
  int64_t capacity; unsigned long long* count;
  ChangeScratch* sc;
};

// The eight corners of one lane's sample through the workgroup's table of block slots: k_merge_fuse's corner fetch (merge.hip), kept here as a
// copy -- lifted into a shared header it cost k_merge_fuse registers.  s_slot[x + 3y + 9z] (LDS) holds the slots of the
// 3 x 3 x 3 blocks from (B0, B1, B2), SLOT_NONE where ref has no TSDF block.  b: the lane's base voxel (nvbx_interp_axis), ok: whether it has one
// and took part in the minimum.  cd[i + 2j + 4k] = distance of corner b + (i, j, k); a z pair inside a block is one 16-B load, as in q_point.
// -> every corner exists with weight >= min_weight.
__device__ inline bool change_corners(const uint2* pool, const uint32_t* s_slot, const int32_t b[3], int32_t B0, int32_t B1, int32_t B2, bool ok,
                                      float min_weight, float cd[8]) {
  // block offsets 0 .. 2 per axis (ok lanes: never less, they took part in the minimum; never more, the block's centres span 7 voxels)
  const int lx = b[0] & 7, ly = b[1] & 7, lz = b[2] & 7;
  const int ox0 = ok ? (b[0] >> 3) - B0 : 0, oy0 = ok ? (b[1] >> 3) - B1 : 0, oz0 = ok ? (b[2] >> 3) - B2 : 0;
  const int ox1 = ok ? ((b[0] + 1) >> 3) - B0 : 0, oy1 = ok ? ((b[1] + 1) >> 3) - B1 : 0, oz1 = ok ? ((b[2] + 1) >> 3) - B2 : 0;
  bool all = ok && ox0 >= 0 && oy0 >= 0 && oz0 >= 0 && ox1 <= 2 && oy1 <= 2 && oz1 <= 2;
#pragma unroll
  for (int q = 0; q < 4; q++) {                                   // q = i + 2j: corners (i, j, 0) and (i, j, 1)
    const int i_ = q & 1, j_ = q >> 1;
    const int ox = i_ ? ox1 : ox0, oy = j_ ? oy1 : oy0;
    const int xx = (lx + i_) & 7, yy = (ly + j_) & 7;
    uint2 e0 = make_uint2(0, 0), e1 = make_uint2(0, 0);
    if (all) {
      const uint32_t s0 = s_slot[ox + 3 * oy + 9 * oz0];
      if (lz != 7) {
        if (slot_ok(s0)) { const uint4 w = ld_pair(pool + (size_t)s0 * 512 + lz + 8 * yy + 64 * xx); e0 = make_uint2(w.x, w.y); e1 = make_uint2(w.z, w.w); }
        else all = false;
      } else {
        const uint32_t s1 = s_slot[ox + 3 * oy + 9 * oz1];
        if (slot_ok(s0) && slot_ok(s1)) { e0 = pool[(size_t)s0 * 512 + 7 + 8 * yy + 64 * xx]; e1 = pool[(size_t)s1 * 512 + 8 * yy + 64 * xx]; }
        else all = false;
      }
    }
    cd[q] = __uint_as_float(e0.x); cd[q + 4] = __uint_as_float(e1.x);
    all = all && __uint_as_float(e0.y) >= min_weight && __uint_as_float(e1.y) >= min_weight;
  }
  return all;
}

// (8 waves per SIMD, four workgroups a CU: the compiler's own choice is 66 VGPRs, two over that occupancy's 64; asked for, it needs 54 and no scratch)
__global__ __launch_bounds__(CH_TPB) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_find_changes(DMap m, DMap ref, ChangeArgs a) {
  __shared__ uint32_t s_slot[27];
  __shared__ int32_t s_min[3];
  __shared__ uint32_t s_cnt[3];
  __shared__ long long s_e;
  const int tid = threadIdx.x;
  const int vx = tid >> 6, vy = (tid >> 3) & 7, vz = tid & 7;
  if (tid < 3) s_cnt[tid] = 0u;
  const uint2* rpool = reinterpret_cast<const uint2*>(ref.tsdf);
  uint32_t n_cmp = 0u, n_app = 0u, n_rem = 0u, n_scan = 0u;
  const int32_t hw = min(m.counters[C_HIGH_WATER], (int32_t)m.capacity);
  for (int32_t slot = blockIdx.x; slot < hw; slot += gridDim.x) {
    if (!(m.slot_flags[slot] & F_TSDF)) continue;      // uniform
    n_scan++;
    // 1. the own voxel and its class
    const int32_t bx = m.slot_index[3 * slot], by = m.slot_index[3 * slot + 1], bz = m.slot_index[3 * slot + 2];
    const int32_t gx = 8 * bx + vx, gy = 8 * by + vy, gz = 8 * bz + vz;
    const bool inbox = gx >= a.box[0] && gx <= a.box[3] && gy >= a.box[1] && gy <= a.box[4] && gz >= a.box[2] && gz <= a.box[5];
    const float2 v = m.tsdf[(size_t)slot * 512 + tid];
    const bool obs = v.y >= a.min_weight;
    const bool m_free = obs && v.x > a.free_dist, m_occ = obs && v.x <= a.occ_dist;
    const bool need = obs && inbox;                    // (voxels_compared counts NEAR voxels too: every observed voxel in the box is sampled)
    __syncthreads();                                   // the previous block's readers of s_slot, s_min and s_e are done
    if (tid < 3) s_min[tid] = INT32_MAX;
    // 2. nothing to compare: no block of ref is touched
    if (!__syncthreads_or(need)) continue;
    // 3. the sample position, its base (nearest: its own) voxel, and the lowest block of ref the workgroup reaches
    const float pm0 = ((float)gx + 0.5f) * a.vs, pm1 = ((float)gy + 0.5f) * a.vs, pm2 = ((float)gz + 0.5f) * a.vs;
    float pr[3];
    apply_rt(a.R_RM, a.t_RM, pm0, pm1, pm2, pr);
    int32_t b[3] = {0, 0, 0}; float t[3] = {0.0f, 0.0f, 0.0f};
    bool ok;
    if (!a.nearest) {
      const bool ok0 = nvbx_interp_axis(pr[0], a.vs, &b[0], &t[0]), ok1 = nvbx_interp_axis(pr[1], a.vs, &b[1], &t[1]), ok2 = nvbx_interp_axis(pr[2], a.vs, &b[2], &t[2]);
      ok = ok0 && ok1 && ok2;
    } else {
      const float n0 = floorf(pr[0] / a.vs), n1 = floorf(pr[1] / a.vs), n2 = floorf(pr[2] / a.vs);
      ok = n0 >= -8388608.0f && n0 <= 8388607.0f && n1 >= -8388608.0f && n1 <= 8388607.0f && n2 >= -8388608.0f && n2 <= 8388607.0f;      // (a NaN fails)
      if (ok) { b[0] = (int32_t)n0; b[1] = (int32_t)n1; b[2] = (int32_t)n2; }
    }
    ok = ok && need;
    {
      int32_t m0 = ok ? (b[0] >> 3) : INT32_MAX, m1 = ok ? (b[1] >> 3) : INT32_MAX, m2 = ok ? (b[2] >> 3) : INT32_MAX;
#pragma unroll
      for (int o = 32; o; o >>= 1) { m0 = min(m0, __shfl_xor(m0, o)); m1 = min(m1, __shfl_xor(m1, o)); m2 = min(m2, __shfl_xor(m2, o)); }
      if ((tid & 63) == 0 && m0 != INT32_MAX) { atomicMin(&s_min[0], m0); atomicMin(&s_min[1], m1); atomicMin(&s_min[2], m2); }
    }
    __syncthreads();
    const int32_t B0 = s_min[0], B1 = s_min[1], B2 = s_min[2];
    if (B0 == INT32_MAX) continue;                     // uniform: no lane has an addressable sample
    // 4. the blocks of ref the samples can reach, resolved once
    uint32_t rs = SLOT_NONE;
    if (tid < 27) {
      const int32_t x = B0 + tid % 3, y = B1 + (tid / 3) % 3, z = B2 + tid / 9;
      if (nvbx_index_in_range(x, y, z)) rs = q_probe(ref, x, y, z, F_TSDF);
      s_slot[tid] = rs;
    }
    if (!__syncthreads_or(slot_ok(rs))) continue;      // ref has none of them: every sample is UNKNOWN
    // 5. the sample
    bool valid = false; float d_ref = 0.0f;
    if (!a.nearest) {
      float cd[8];
      valid = change_corners(rpool, s_slot, b, B0, B1, B2, ok, a.ref_min_weight, cd);
      if (valid) { float g[3]; d_ref = nvbx_interp_trilinear(cd, t[0], t[1], t[2], a.vs, g); }
    } else if (ok) {
      const int o0 = (b[0] >> 3) - B0, o1 = (b[1] >> 3) - B1, o2 = (b[2] >> 3) - B2;
      if (o0 >= 0 && o0 <= 2 && o1 >= 0 && o1 <= 2 && o2 >= 0 && o2 <= 2) {
        const uint32_t s = s_slot[o0 + 3 * o1 + 9 * o2];
        if (slot_ok(s)) {
          const uint2 e = rpool[(size_t)s * 512 + (b[2] & 7) + 8 * (b[1] & 7) + 64 * (b[0] & 7)];
          valid = __uint_as_float(e.y) >= a.ref_min_weight; d_ref = __uint_as_float(e.x);
        }
      }
    }
    // 6. classes and label (valid implies observed and in the box)
    const bool r_free = valid && d_ref > a.free_dist, r_occ = valid && d_ref <= a.occ_dist;
    const bool appeared = m_occ && r_free, removed = m_free && r_occ;
    n_cmp += valid ? 1u : 0u; n_app += appeared ? 1u : 0u; n_rem += removed ? 1u : 0u;
    const bool labelled = appeared || removed;
    // 8. a block with a label claims its entry
    if (!__syncthreads_or(labelled)) continue;
    if (tid == 0) s_e = (long long)atomicAdd(a.count, 1ull);
    __syncthreads();
    const long long e = s_e;
    if (e >= a.capacity) continue;                     // uniform: counted, not written anywhere
    // 9. 2 KiB of labels, 2 KiB of scores
    if (tid < 3) a.block_idx[3 * e + tid] = m.slot_index[3 * slot + tid];
    a.label[(size_t)e * 512 + tid] = appeared ? 0 : removed ? 1 : -1;
    if (a.score) a.score[(size_t)e * 512 + tid] = labelled ? fabsf(v.x - d_ref) : 0.0f;
  }
  // 7. the workgroup's counts: wavefront sums, LDS, one atomic each
#pragma unroll
  for (int o = 32; o; o >>= 1) { n_cmp += __shfl_xor(n_cmp, o); n_app += __shfl_xor(n_app, o); n_rem += __shfl_xor(n_rem, o); }
  __syncthreads();
  if ((tid & 63) == 0) { atomicAdd(&s_cnt[0], n_cmp); atomicAdd(&s_cnt[1], n_app); atomicAdd(&s_cnt[2], n_rem); }
  __syncthreads();
  if (tid == 0) {
    if (n_scan) atomicAdd(&a.sc->scanned, (unsigned long long)n_scan);
    if (s_cnt[0]) atomicAdd(&a.sc->compared, (unsigned long long)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&a.sc->appeared, (unsigned long long)s_cnt[1]);
    if (s_cnt[2]) atomicAdd(&a.sc->removed, (unsigned long long)s_cnt[2]);
  }
}

__global__ __launch_bounds__(64) void k_change_result(DMap ref, const ChangeScratch* sc, const unsigned long long* count, nvbx_change_result* out) {
  if (blockIdx.x != 0) return;
  const ChangeScratch s = *sc;
  // an empty reference shows as "nothing compared": only then are ref's slots looked through (uniform)
  bool ref_has_tsdf = s.compared != 0ull;
  if (s.scanned != 0ull && s.compared == 0ull) {
    const int32_t hw = min(ref.counters[C_HIGH_WATER], (int32_t)ref.capacity);
    bool mine = false;
    for (int32_t i = threadIdx.x; i < hw; i += 64) mine = mine || (ref.slot_flags[i] & F_TSDF);
    ref_has_tsdf = __any(mine ? 1 : 0) != 0;
  }
  if (threadIdx.x != 0) return;
  nvbx_change_result r;
  r.blocks_scanned = (int64_t)s.scanned; r.voxels_compared = (int64_t)s.compared;
  r.voxels_appeared = (int64_t)s.appeared; r.voxels_removed = (int64_t)s.removed;
  r.blocks_changed = (int64_t)*count;
  r.status = s.scanned == 0ull ? NVBX_CHANGE_EMPTY_MAP : !ref_has_tsdf ? NVBX_CHANGE_EMPTY_REFERENCE : s.compared == 0ull ? NVBX_CHANGE_NO_OVERLAP : NVBX_CHANGE_OK;
  for (int k = 0; k < 5; k++) r.pad[k] = 0;
  *out = r;
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" void nvbx_default_change_options(nvbx_change_options* o) {
  if (!o) return;
  o->min_weight = 1e-4f; o->ref_min_weight = 1e-4f; o->free_distance_m = 0.0f; o->occupied_distance_m = 0.0f; o->sampling = NVBX_CHANGE_TRILINEAR; o->pad = 0;
}

namespace {

// the refusals of nvbx_find_changes in their order; *o = the options with the defaults filled in and free_distance_m resolved
int change_check(const char* who, const nvbx_mapper* m, const nvbx_mapper* ref, const float* T, const nvbx_change_options* options, const int32_t* box,
                 const void* block_idx, const void* label, int64_t capacity, const void* count, const void* result_dev, nvbx_change_options* o) {
  if (!m || !ref) return refuse(who, ": both mappers are required");
  if (options) *o = *options; else nvbx_default_change_options(o);
  if (!T) return refuse(who, ": the pose is required");
  if (ref == m) return refuse(who, ": ref and m are the same mapper");
  if (ref->device != m->device) return refuse(who, ": the mappers are on different devices");
  if (ref->p.voxel_size != m->p.voxel_size) return refuse(who, ": the mappers' voxel sizes differ");
  if (tsdf_reader_refused(m, who) || tsdf_reader_refused(ref, who)) return NVBX_E_INVALID;
  if (!nvbx_pose_in_range(T, m->p.voxel_size * 8.0f, 0.0f)) return refuse(who, ": the pose is not finite or out of range");
  if (!nvbx_merge_rotation_ok(T, nullptr, nullptr)) return refuse(who, ": the upper-left 3 x 3 of T_M_R is not a rotation (|R^T R - I| > 1e-5 or det <= 0)");
  if (std::isnan(o->min_weight) || std::isnan(o->ref_min_weight) || std::isnan(o->free_distance_m) || std::isnan(o->occupied_distance_m))
    return refuse(who, ": a weight or distance option is not a number");
  if (o->free_distance_m == 0.0f) o->free_distance_m = m->p.voxel_size;
  if (o->occupied_distance_m > o->free_distance_m) return refuse(who, ": occupied_distance_m > free_distance_m");
  if (o->sampling != NVBX_CHANGE_TRILINEAR && o->sampling != NVBX_CHANGE_NEAREST) return refuse(who, ": sampling must be 0 (trilinear) or 1 (nearest)");
  if (sparse_volume_refused(who, box, block_idx, label, capacity, count)) return NVBX_E_INVALID;
  if ((uintptr_t)result_dev & 7) return refuse(who, ": result_dev must be 8-byte aligned");
  return NVBX_OK;
}

// the launches of nvbx_find_changes; the arguments have been checked
int change_launch(nvbx_mapper* m, nvbx_mapper* ref, const float* T, const nvbx_change_options& o, const int32_t* box, nvbx_index3d* block_idx_dev,
                  int32_t* label_dev, float* score_dev, int64_t capacity, int64_t* count_dev, nvbx_change_result* result_dev) {
  NVBX_HIP(hipSetDevice(m->device));
  // TSDF voxels and flags only: held-back colour and ESDF work of both mappers stays held back (frontier.hip)
  if (ref->begin_call_keeping_held() || m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  { const int rc = nvbx_mapper_wait_for(m, ref); if (rc) return rc; }
  ChangeArgs a{};
  float R_MR[9], t_MR[3];
  nvbx_merge_transforms(T, R_MR, t_MR, a.R_RM, a.t_RM);
  a.vs = m->p.voxel_size; a.min_weight = o.min_weight; a.ref_min_weight = o.ref_min_weight;
  a.free_dist = o.free_distance_m; a.occ_dist = o.occupied_distance_m; a.nearest = o.sampling == NVBX_CHANGE_NEAREST;
  for (int k = 0; k < 3; k++) { a.box[k] = box ? box[k] : INT32_MIN; a.box[3 + k] = box ? box[3 + k] : INT32_MAX; }
  a.block_idx = reinterpret_cast<int32_t*>(block_idx_dev); a.label = label_dev; a.score = score_dev;
  a.capacity = capacity; a.count = reinterpret_cast<unsigned long long*>(count_dev);
  a.sc = m->change_buf.as<ChangeScratch>();
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(m->capacity, m->change_knobs.grid)));      // (NVBX_CHANGE_GRID)
  NVBX_HIP(hipMemsetAsync(a.sc, 0, sizeof(ChangeScratch), m->stream));
  NVBX_HIP(hipMemsetAsync(count_dev, 0, sizeof(int64_t), m->stream));
  NVBX_LAUNCH(m, k_find_changes, grid, dim3(CH_TPB), m->d, ref->d, a);
  if (result_dev) NVBX_LAUNCH(m, k_change_result, dim3(1), dim3(64), ref->d, (const ChangeScratch*)a.sc, (const unsigned long long*)a.count, result_dev);
  NVBX_HIP(hipGetLastError());
  return nvbx_mapper_wait_for(ref, m);                // later work on ref runs behind the scan's reads
}

}  // namespace

extern "C" int nvbx_find_changes(nvbx_mapper* m, nvbx_mapper* ref, const float T_M_R[16], const nvbx_change_options* options, const int32_t box_min_max_vox[6],
                                 nvbx_index3d* block_idx_dev, int32_t* label_dev, float* score_dev, int64_t capacity_blocks, int64_t* count_dev,
                                 nvbx_change_result* result_dev) {
  nvbx_change_options o;
  const int rc = change_check("nvbx_find_changes", m, ref, T_M_R, options, box_min_max_vox, block_idx_dev, label_dev, capacity_blocks, count_dev, result_dev, &o);
  if (rc) return rc;
  return change_launch(m, ref, T_M_R, o, box_min_max_vox, block_idx_dev, label_dev, score_dev, capacity_blocks, count_dev, result_dev);
}

extern "C" int nvbx_change_clusters(nvbx_mapper* m, nvbx_mapper* ref, const float T_M_R[16], const nvbx_change_options* options, const int32_t box_min_max_vox[6],
                                    int32_t connectivity, int32_t min_voxels, nvbx_index3d* block_idx_dev, int32_t* label_dev, float* score_dev,
                                    int32_t* component_id_dev, int64_t capacity_blocks, int64_t* block_count_dev, nvbx_component* components_dev,
                                    int64_t capacity_components, int64_t* component_count_dev, nvbx_change_result* result_dev) {
  const char* who = "nvbx_change_clusters";
  nvbx_change_options o;
  int rc = change_check(who, m, ref, T_M_R, options, box_min_max_vox, block_idx_dev, label_dev, capacity_blocks, block_count_dev, result_dev, &o);
  if (rc) return rc;
  // nvbx_label_components' refusals, looked at before the scan is launched: a refused call launches nothing
  rc = seg_check(who, connectivity, min_voxels, capacity_blocks > 0 && !component_id_dev ? ": component_id_dev is required with capacity_blocks > 0" : nullptr,
                 components_dev, capacity_components, component_count_dev);
  if (rc) return rc;
  rc = change_launch(m, ref, T_M_R, o, box_min_max_vox, block_idx_dev, label_dev, score_dev, capacity_blocks, block_count_dev, result_dev);
  if (rc) return rc;
  return nvbx_label_components(m, block_idx_dev, label_dev, score_dev, capacity_blocks, block_count_dev, connectivity, min_voxels, component_id_dev,
                               components_dev, capacity_components, component_count_dev);
}
