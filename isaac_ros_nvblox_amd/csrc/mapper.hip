// mapper.hip -- a mapper's lifetime, memory, parameters and counters (host code + small utility kernels).  Its held-back work: held.hip; layer
// access: layers.hip; map files: map_io.hip; per-kernel timing: profile.hip.
#include <cstdlib>
#include <cstring>
#include "nvbx_mapper.h"
using namespace nvbx;

namespace nvbx {
static thread_local std::string g_err;
void set_error(const char* what, hipError_t e) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
}
void set_error(const char* what) { g_err = what; }
}  // namespace nvbx

extern "C" const char* nvbx_last_error(void) { return nvbx::g_err.c_str(); }
// ------------------------------------------------------------------------------------------------ utility kernels
__global__ void k_init_map(DMap m) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m.capacity) { m.free_stack[i] = m.capacity - 1 - i; m.slot_flags[i] = 0; m.slot_stamp[i] = STAMP_NEVER; m.slot_consumed[i] = STAMP_NEVER; m.slot_cam[i] = STAMP_NEVER; }
  if (i < (uint32_t)(S_NUM * NSH * SH_STRIDE)) {       // sharded counters: zero, ESDF window records min = +inf / max = -inf
    const int id = (int)i / (NSH * SH_STRIDE), field = (int)i % SH_STRIDE;
    int32_t v = 0;
    if (id == S_ESDF_REC || id == S_ESDF_REC + 1) { if (field < 2) v = INT32_MAX; else if (field < 4) v = INT32_MIN; }
    m.shc[i] = v;
  }
  if (i < C_NUM) {
    int32_t v = 0;
    if (i == C_FREE_TOP) v = (int32_t)m.capacity;
    const int a = (int)i - C_ESDF_AABB;
    if (a >= 0 && a < 4) v = a < 2 ? INT32_MAX : INT32_MIN;
    const int w3 = (int)i - C_ESDF3_WIN;
    if (w3 >= 0 && w3 < 6) v = w3 < 3 ? INT32_MAX : INT32_MIN;
#ifdef NVBX_CHECK_INVARIANTS
    if (i >= C_INV_I1 && i <= C_INV_I3) v = m.counters[i];      // (violations survive clear(): a mapper answers for all its launches when it is closed)
#endif
    m.counters[i] = v;
  }
}

__global__ __launch_bounds__(512) void k_recompute_band(DMap m, float trunc) {
  const int32_t hw = m.counters[C_HIGH_WATER];
  for (int32_t slot = blockIdx.x; slot < hw; slot += gridDim.x) {
    if (!(m.slot_flags[slot] & F_TSDF)) continue;             // uniform
    const float2 v = m.tsdf[(size_t)slot * 512 + threadIdx.x];
    publish_band(m.slot_flags, (uint32_t)slot, (int)threadIdx.x, in_band(v.x, v.y, trunc));
  }
}

// ------------------------------------------------------------------------------------------------ host helpers
std::vector<PoolArr> nvbx_mapper::pool_arrays(int64_t cap) {
  const size_t n = (size_t)cap, mv = (size_t)mesh_verts(cap);
  auto per_block = [n](auto** p, size_t bpb, int fill) { return PoolArr{reinterpret_cast<void**>(p), bpb, fill, bpb * n}; };
  auto other = [](auto** p, size_t bytes) { return PoolArr{reinterpret_cast<void**>(p), 0, -1, bytes}; };
  return {
      // (grow_map copies the per-block arrays in this order)
      per_block(&d.free_stack, 4, -1), per_block(&d.slot_flags, 4, 0), per_block(&d.slot_index, 12, 0), per_block(&d.slot_entry, 4, 0), per_block(&d.slot_stamp, 4, 0xFF),
      per_block(&d.slot_consumed, 4, 0xFF), per_block(&d.slot_cam, 4, 0xFF), per_block(&d.tsdf, 4096, 0), per_block(&d.color, 4096, 0), per_block(&d.esdf, 4096, 0),
      per_block(&view_list, 16, -1),       // int4 {slot, x, y, z} per block in view
      per_block(&export_idx, 12, -1), per_block(&cleared_idx, 12, -1), per_block(&d.site_bits, 8, 0), per_block(&d.obs_bits, 8, 0), per_block(&d.inside_bits, 8, 0),
      per_block(&mesh_rec, sizeof(MeshRecord), -1),
      PoolArr{reinterpret_cast<void**>(&d.freespace), 512 * 16, 0, 0},       // on first use: ensure_freespace_pool (dynamics.hip)
      // the feature layer, on nvbx_enable_features (features.hip); no fill: a block's payload is written whole before its slot is flagged
      PoolArr{&feat_val, 1024 * (size_t)feat_channels, -1, 0}, PoolArr{reinterpret_cast<void**>(&feat_w), feat_channels ? (size_t)2048 : 0, -1, 0},
      // grow_map has code of its own for these: the hash table is rebuilt, the work lists and mesh arenas move segment by segment
      other(&d.table, hash_slots(cap) * sizeof(Entry)), other(&d.lists, (size_t)N_LISTS * NSH * n * 4),
      other(&mesh_vert, mv * 12), other(&mesh_nrm, mv * 12), other(&mesh_col, mv * 4), other(&mesh_tri, mv * 2 * 12),
      // one size at every capacity
      other(&d.counters, C_NUM * 4), other(&d.shc, S_NUM * NSH * SH_STRIDE * 4), other(&export_count, 64),
      // decay's spare hash tables, on first use: prepare_tables (maintenance.hip)
      other(&table_spare, 0), other(&table_dirty, 0)};
}

static int alloc_all(nvbx_mapper* m) {
  const int64_t cap = m->capacity;
  const uint64_t tsz = nvbx_mapper::hash_slots(cap);
  DMap& d = m->d;
  d.capacity = (uint32_t)cap; d.mask = (uint32_t)(tsz - 1);
  { uint32_t lg = 0; while ((1ull << lg) < tsz) lg++; d.shift = 32u - lg; }
  for (const PoolArr& a : m->pool_arrays(cap)) if (a.bytes) NVBX_HIP(hipMalloc(a.p, a.bytes));
  m->mesh_vert_cap = nvbx_mapper::mesh_verts(cap); m->mesh_tri_cap = m->mesh_vert_cap * 2;
  // (k_init_map of the -DNVBX_CHECK_INVARIANTS variant keeps some of them across clear().  ON THE MAPPER'S STREAM: a memset on the null stream is
  //  not ordered with a non-blocking stream and landed after k_init_map once in a while -- a map with no free slot, tests/cpp rccl_fusion)
  NVBX_HIP(hipMemsetAsync(d.counters, 0, C_NUM * 4, m->stream));
  if (m->staging.ensure(m->stream, 8 << 20)) return NVBX_E_DEVICE;
  if (m->change_buf.ensure(m->stream, 64)) return NVBX_E_DEVICE;      // (change.hip's counters: there from the start, the call itself allocates nothing)
  NVBX_HIP(hipHostMalloc(&m->h_counters, C_NUM * 4));
  NVBX_HIP(hipHostMalloc(&m->h_shc, S_NUM * NSH * SH_STRIDE * 4));
  NVBX_HIP(hipHostMalloc(&m->h_mirror, 64, hipHostMallocMapped));
  { void* dp = nullptr; NVBX_HIP(hipHostGetDevicePointer(&dp, m->h_mirror, 0)); d.host_mirror = (int32_t*)dp; }
  m->h_mirror[0] = (int32_t)cap; m->h_mirror[1] = 0; m->h_mirror[2] = 0; m->h_mirror[3] = 0; m->h_mirror[4] = 0; m->h_mirror[8] = 0;      // ([4]: fence progress of held-back colour frames, frames.hip -- never reset)
  return NVBX_OK;
}

static int reset_map(nvbx_mapper* m) {
  DMap& d = m->d;
  const int64_t cap = m->capacity;
  NVBX_HIP(hipMemsetAsync(d.table, 0xFF, ((size_t)d.mask + 1) * sizeof(Entry), m->stream));
  NVBX_HIP(hipMemsetAsync(d.tsdf, 0, cap * 4096, m->stream));
  NVBX_HIP(hipMemsetAsync(d.color, 0, cap * 4096, m->stream));
  NVBX_HIP(hipMemsetAsync(d.esdf, 0, cap * 4096, m->stream));
  NVBX_HIP(hipMemsetAsync(d.site_bits, 0, cap * 8, m->stream));
  NVBX_HIP(hipMemsetAsync(d.obs_bits, 0, cap * 8, m->stream));
  NVBX_HIP(hipMemsetAsync(d.inside_bits, 0, cap * 8, m->stream));
  NVBX_HIP(hipMemsetAsync(m->export_count, 0, 64, m->stream));
  if (d.freespace) NVBX_HIP(hipMemsetAsync(d.freespace, 0, cap * 512 * 16, m->stream));
  const int64_t n = std::max<int64_t>(cap, std::max<int64_t>(C_NUM, S_NUM * NSH * SH_STRIDE));
  NVBX_LAUNCH(m, k_init_map, dim3((unsigned)((n + 255) / 256)), dim3(256), d);
  NVBX_HIP(hipGetLastError());
  m->reset_marking(); m->held.drop(*m); m->lidar_integrated = false;
  if (m->h_mirror) { m->h_mirror[0] = (int32_t)m->capacity; m->h_mirror[1] = 0; m->h_mirror[2] = 0; m->h_mirror[3] = 0; }
  m->frame_id = 0; m->esdf_epoch = 0; m->mesh_epoch = 0; m->last_view_frame = 0; m->last_camera_view_frame = 0; m->synth_rows = m->synth_cols = 0;
  return NVBX_OK;
}

// (a polled stream write -- hipStreamWriteValue32 of a sequence number into pinned memory, the host spinning on it -- was measured in round 5 and not
//  kept: the write is itself ~15 us late, a frame waited for took 0.066 instead of 0.052 ms; EXPERIMENTS.md)
int nvbx_mapper::wait_stream() {
  NVBX_HIP(hipStreamSynchronize(stream));
  return NVBX_OK;
}
int nvbx_mapper::fetch_counters() {
  if (begin_call()) return NVBX_E_DEVICE;
  NVBX_HIP(hipMemcpyAsync(h_counters, d.counters, C_NUM * 4, hipMemcpyDeviceToHost, stream));
  NVBX_HIP(hipMemcpyAsync(h_shc, d.shc, S_NUM * NSH * SH_STRIDE * 4, hipMemcpyDeviceToHost, stream));
  return wait_stream();
}

// log-odds of a probability, evaluated on the host in float (the oracle does the same with the same libm)
float nvbx::log_odds(float p) { return logf(p / (1.0f - p)); }

// T_L_C row-major 4x4 -> forward and inverse rigid transforms, fixed evaluation order (matches oracle rt_from_T)
Frame nvbx_mapper::make_frame(const float T[16], const nvbx_camera* cam, int32_t rows, int32_t cols, int32_t subsample) const {
  Frame f{};
  nvbx_pose_unpack(T, f.R_LC, f.t_LC);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) f.R_CL[3 * i + j] = f.R_LC[3 * j + i];
  for (int i = 0; i < 3; i++) {
    float s = f.R_CL[3 * i + 0] * f.t_LC[0];
    s = s + f.R_CL[3 * i + 1] * f.t_LC[1];
    s = s + f.R_CL[3 * i + 2] * f.t_LC[2];
    f.t_CL[i] = -s;
  }
  f.fu = cam->fu; f.fv = cam->fv; f.cu = cam->cu; f.cv = cam->cv; f.w = cam->width; f.h = cam->height;
  f.rows = rows; f.cols = cols;
  f.voxel_size = p.voxel_size; f.block_size = p.voxel_size * 8.0f;
  f.trunc = p.truncation_distance_vox * p.voxel_size;
  f.max_dist = p.max_integration_distance_m; f.max_weight = p.max_weight;
  f.weighting_mode = p.weighting_mode; f.interp_nearest = p.depth_interp_nearest;
  f.invalid_decay = p.invalid_depth_decay_factor;
  f.weighting_variant = p.tsdf_weighting_variant; f.skip_at_neg_trunc = p.tsdf_skip_at_negative_truncation; f.clamp_before_blend = p.tsdf_weight_clamp_before_blend;
  f.occlusion_thresh = p.color_occlusion_threshold_vox < 0.0f ? f.trunc : p.color_occlusion_threshold_vox * p.voxel_size;
  f.occupancy = p.projective_layer_type == 1 ? 1 : 0;
  f.lo_free = log_odds(p.free_region_occupancy_probability); f.lo_occupied = log_odds(p.occupied_region_occupancy_probability);
  f.lo_unobserved = log_odds(p.unobserved_region_occupancy_probability); f.occ_half_width = p.occupied_region_half_width_m;
  f.ws_type = p.workspace_bounds_type;
  for (int i = 0; i < 3; i++) { f.ws_min[i] = p.workspace_bounds_min_corner_m[i]; f.ws_max[i] = p.workspace_bounds_max_corner_m[i]; }
  f.subsample = subsample < 1 ? 1 : subsample;
  f.n_ray_rows = 0; f.n_ray_cols = 0;
  f.frame_id = frame_id;
  return f;
}

EsdfArgs nvbx_mapper::make_esdf_args() const {
  EsdfArgs c{};
  const float vs = p.voxel_size;
  c.kz_min = (int32_t)floorf(p.esdf_slice_min_height / vs);
  c.kz_max = (int32_t)floorf(p.esdf_slice_max_height / vs);
  c.kz_out = (int32_t)floorf(p.esdf_slice_height / vs);
  c.bz_lo = c.kz_min >> 3; c.bz_hi = c.kz_max >> 3; c.bz_out = c.kz_out >> 3; c.vz_out = c.kz_out & 7;
  const float r = p.esdf_max_distance_m / vs;
  c.max_sq = r * r;
  c.ri = (int32_t)floorf(r); if (c.ri > 63) c.ri = 63; if (c.ri < 1) c.ri = 1;
  c.rb = (c.ri + 7) / 8;
  c.site_dist_m = p.esdf_max_site_distance_vox * vs;
  c.min_weight = p.esdf_min_weight; c.voxel_size = vs; c.site_rule = p.projective_layer_type == 1 ? 2 : p.esdf_site_rule;
  c.epoch = esdf_epoch; c.mark_pass = mark_pass;
  c.rec = C_ESDF_UPD + 8 * (int)(esdf_epoch & 1); c.rec_next = C_ESDF_UPD + 8 * (int)((esdf_epoch + 1) & 1);
  c.self_reset = c.keep_list = pipelined_order ? 1 : 0;       // (see EsdfArgs)
  // ground-plane-relative band: only with a usable plane (pointing up) and a positive thickness; else the fixed heights
  c.plane_on = (p.esdf_use_ground_plane && p.esdf_ground_plane[2] > 1e-3f && p.slice_height_thickness_m > 0.0f) ? 1 : 0;
  for (int i = 0; i < 4; i++) c.pl[i] = p.esdf_ground_plane[i];
  c.above = p.slice_height_above_plane_m; c.thick = p.slice_height_thickness_m;
  return c;
}

// Parameter values the kernels' loop bounds and address arithmetic rely on (the reference CHECKs the same kind of thing in its
// setters and aborts; here the call fails with NVBX_E_INVALID).  Returns nullptr if fine, else what is wrong.
static const char* params_problem(const nvbx_mapper_params* p) {
  auto pos = [](float v) { return std::isfinite(v) && v > 0.0f; };
  if (!pos(p->voxel_size)) return "voxel_size must be > 0";
  if (!pos(p->max_integration_distance_m)) return "max_integration_distance_m must be > 0 (it bounds the view rays)";
  if (!pos(p->lidar_max_integration_distance_m)) return "lidar_max_integration_distance_m must be > 0 (it bounds the view rays)";
  if (p->max_integration_distance_m / (p->voxel_size * 8.0f) > 65536.0f || p->lidar_max_integration_distance_m / (p->voxel_size * 8.0f) > 65536.0f)
    return "integration distance exceeds 65536 blocks";
  if (!pos(p->truncation_distance_vox)) return "truncation_distance_vox must be > 0";
  if (!pos(p->max_weight)) return "max_weight must be > 0";
  if (p->projective_layer_type < 0 || p->projective_layer_type > 2) return "projective_layer_type must be 0 (TSDF), 1 (occupancy) or 2 (TSDF + freespace)";
  if (p->esdf_mode < 0 || p->esdf_mode > 1) return "esdf_mode must be 0 (2-D) or 1 (3-D)";
  if (p->tsdf_weighting_variant < 0 || p->tsdf_weighting_variant > 1 || p->esdf_propagation < 0 || p->esdf_propagation > 1 ||
      p->mesh_ambiguity_rule < 0 || p->mesh_ambiguity_rule > 2 || p->mesh_normal_rule < 0 || p->mesh_normal_rule > 1) return "open-choice switch out of range";
  if (p->esdf_propagation == 1 && p->esdf_mode == 1) return "esdf_propagation 1 (iterative) is defined for the 2-D slice only";
  if (p->sphere_tracing_max_steps < 0 || p->sphere_tracing_max_steps > (1 << 20)) return "sphere_tracing_max_steps out of range";
  if (p->projective_layer_type == 1) {
    auto prob = [](float v) { return v > 0.0f && v < 1.0f; };
    if (!prob(p->free_region_occupancy_probability) || !prob(p->occupied_region_occupancy_probability) || !prob(p->unobserved_region_occupancy_probability) ||
        !prob(p->free_region_decay_probability) || !prob(p->occupied_region_decay_probability)) return "occupancy probabilities must lie strictly between 0 and 1";
  }
  return nullptr;
}

// ------------------------------------------------------------------------------------------------ C-ABI: lifetime
// THE read of the mapper's NVBX_* environment variables, all through nvbx_knobs.h (the frame pool's own is process-wide: frames.hip)
static void read_knobs(nvbx_mapper* m) { const auto env = [](const char* name) -> const char* { return getenv(name); }; nvbx_knobs_read(&m->knobs, env); nvbx_plan_knobs_read(&m->plan_knobs, env); nvbx_change_knobs_read(&m->change_knobs, env); nvbx_resample_knobs_read(&m->resample_knobs, env); }
extern "C" int nvbx_mapper_reload_knobs(nvbx_mapper* m) {
  if (!m) return NVBX_E_INVALID;
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call()) return NVBX_E_DEVICE;          // (anything held back under the old settings is carried out)
  read_knobs(m);
  return NVBX_OK;
}
extern "C" int nvbx_mapper_create(int device, void* hip_stream, const nvbx_mapper_params* params, int64_t block_capacity, nvbx_mapper** out) {
  if (!params || !out || (block_capacity != 0 && (block_capacity < 64 || block_capacity > (1ll << 24)))) {
    set_error("nvbx_mapper_create: invalid argument (null pointer, or block_capacity outside 64 .. 2^24 and not 0 = automatic)"); return NVBX_E_INVALID;
  }
  if (const char* why = params_problem(params)) { set_error(why); return NVBX_E_INVALID; }
  NVBX_HIP(hipSetDevice(device));
  if (block_capacity == 0) {      // automatic: ~4 % of the free HBM (12.4 KiB per block), 2^16 .. 2^20 blocks (1 M blocks = 12 GiB of a 288 GB MI355X); grows on demand
    size_t free_b = 0, total_b = 0; NVBX_HIP(hipMemGetInfo(&free_b, &total_b));
    int64_t want = (int64_t)((double)free_b * 0.04 / 12700.0), cap = 1ll << 16;
    while (cap * 2 <= want && cap < (1ll << 20)) cap *= 2;
    block_capacity = cap;
  }
  nvbx_mapper* m = new nvbx_mapper();
  m->device = device; m->p = *params; m->capacity = block_capacity;
  read_knobs(m);
  // the pools double on demand up to this many blocks (nvbx_mapper_set_max_capacity; NVBX_MAX_BLOCKS in the environment)
  m->max_capacity = std::max<int64_t>(block_capacity, 1ll << 22);
  if (m->knobs.max_blocks > 0) m->max_capacity = std::max<int64_t>(block_capacity, std::min<int64_t>(m->knobs.max_blocks, 1ll << 24));
  if (hip_stream) { m->stream = (hipStream_t)hip_stream; m->own_stream = false; }
  else { hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking); if (e != hipSuccess) { set_error("hipStreamCreate", e); delete m; return NVBX_E_DEVICE; } m->own_stream = true; }
  nvbx::frames_register_stream(device, m->stream); m->stream_registered = true;      // (frames let go of without a fence wait for this stream too, frames.hip)
  m->defer_edt = m->knobs.defer_edt != 0;
  // colour deferral of a new mapper (nvbx_mapper_set_color_deferral overrides): NVBX_COLOR_DEFERRAL = 0 / 1 / 2 in the environment
  { const int cd = m->knobs.color_deferral; if (cd >= 0) { m->color_deferral = cd != 0; m->color_staging = cd == 2; } }
  int rc = alloc_all(m); if (rc) { nvbx_mapper_destroy(m); return rc; }
  rc = reset_map(m); if (rc) { nvbx_mapper_destroy(m); return rc; }
  hipError_t e = hipStreamSynchronize(m->stream);
  if (e != hipSuccess) { set_error("create sync", e); nvbx_mapper_destroy(m); return NVBX_E_DEVICE; }
  *out = m;
  return NVBX_OK;
}

extern "C" int nvbx_mapper_destroy(nvbx_mapper* m) {
  if (!m) return NVBX_OK;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  if (m->ev_order) (void)hipEventDestroy(m->ev_order);
  for (const PoolArr& a : m->pool_arrays(m->capacity)) if (*a.p) (void)hipFree(*a.p);      // (a half-built mapper: what was not allocated is null)
  // (the stream is idle: whatever read a held-back colour frame has finished)
  (void)m->take_pending(); m->release_consumed_frames();
  if (m->stream_registered) nvbx::frames_forget_owner(m, m->device, m->stream);
  for (auto& s : m->spans) { if (s.a) (void)hipEventDestroy(s.a); if (s.b) (void)hipEventDestroy(s.b); }
  for (hipEvent_t e : m->event_pool) if (e) (void)hipEventDestroy(e);
  if (m->h_counters) (void)hipHostFree(m->h_counters);
  if (m->h_shc) (void)hipHostFree(m->h_shc);
  if (m->h_mirror) (void)hipHostFree(m->h_mirror);
  if (m->slice_pinned) (void)hipHostFree(m->slice_pinned);
  if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
  delete m;      // (the scratch buffers: ~DevBuf)
  return NVBX_OK;
}

extern "C" int nvbx_mapper_set_params(nvbx_mapper* m, const nvbx_mapper_params* params) {
  if (!m || !params) return NVBX_E_INVALID;
  if (const char* why = params_problem(params)) { set_error(why); return NVBX_E_INVALID; }
  if (params->voxel_size != m->p.voxel_size) { set_error("voxel_size cannot change after creation"); return NVBX_E_INVALID; }
  if (params->projective_layer_type != m->p.projective_layer_type || params->esdf_mode != m->p.esdf_mode) {
    // what the voxels of the existing map MEAN would change under it (the reference fixes both at construction too)
    if (nvbx_num_blocks(m, F_TSDF | 0u) != 0 || nvbx_num_blocks(m, NVBX_LAYER_OCCUPANCY) != 0 || nvbx_num_blocks(m, F_ESDF) != 0) {
      set_error("projective_layer_type / esdf_mode can only change while the map is empty"); return NVBX_E_INVALID;
    }
  }
  if (m->begin_call()) return NVBX_E_DEVICE;        // work enqueued under the old parameters (a held-back EDT) is launched first
  const bool trunc_changed = params->truncation_distance_vox != m->p.truncation_distance_vox;
  m->p = *params;
  if (trunc_changed && m->p.projective_layer_type != 1) {       // F_BAND is defined by the truncation distance: recompute it for every TSDF block
    NVBX_LAUNCH(m, k_recompute_band, dim3((unsigned)std::min<int64_t>(m->capacity, 2048)), dim3(512), m->d, m->p.truncation_distance_vox * m->p.voxel_size);
    NVBX_HIP(hipGetLastError());
  }
  return NVBX_OK;
}
#ifdef NVBX_CHECK_INVARIANTS
// Variant-only (tools/build_variant.sh inv "-DNVBX_CHECK_INVARIANTS"; not part of include/nvblox_hip.h): the violation counters of DESIGN.md 2.8's
// invariants as the kernels counted them -- out[0] = I1 (a TSDF-reading rider of launch 1 beside a running TSDF writer), out[1] = I3 (a colour worker
// handed a record whose slot does not name the block), out[2] = I4 (the marking pass took an entry of a slot without a layer), out[3] = writers
// still counted as running (must be 0 between launches), out[4] = I8 (host side: a colour-reading launch enqueued on a frame nobody holds).
// selftest != 0: first makes one reader meet a (pretended) writer, so a caller can see that the counters count.
__global__ void k_inv_selftest(DMap m) {
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&m.counters[C_INV_WRITERS], 1);
  __syncthreads();
  NVBX_INV_TSDF_READER(m);
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicSub(&m.counters[C_INV_WRITERS], 1);
}
extern "C" int nvbx_debug_invariants(nvbx_mapper* m, int64_t out[5], int32_t selftest) {
  if (!m || !out) return NVBX_E_INVALID;
  if (selftest) { NVBX_LAUNCH(m, k_inv_selftest, dim3(1), dim3(64), m->d); NVBX_HIP(hipGetLastError()); }
  if (m->fetch_counters()) return NVBX_E_DEVICE;
  out[0] = m->h_counters[C_INV_I1]; out[1] = m->h_counters[C_INV_I3]; out[2] = m->h_counters[C_INV_I4]; out[3] = m->h_counters[C_INV_WRITERS]; out[4] = m->inv_i8;
  return NVBX_OK;
}
#endif
extern "C" int nvbx_mapper_get_params(const nvbx_mapper* m, nvbx_mapper_params* out) {
  if (!m || !out) return NVBX_E_INVALID;
  *out = m->p; return NVBX_OK;
}
extern "C" int nvbx_synchronize(nvbx_mapper* m) {
  if (!m) return NVBX_E_INVALID;
  if (m->begin_call()) return NVBX_E_DEVICE;
  return m->wait_stream();
}
extern "C" void nvbx_default_params(nvbx_mapper_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->voxel_size = 0.05f; p->max_integration_distance_m = 8.0f; p->truncation_distance_vox = 4.0f; p->max_weight = 5.0f;
  p->weighting_mode = 0; p->raycast_subsampling_factor = 4;
  p->esdf_min_weight = 0.1f; p->esdf_max_site_distance_vox = 2.0f; p->esdf_max_distance_m = 2.0f;
  p->esdf_slice_height = 0.09f; p->esdf_slice_min_height = 0.09f; p->esdf_slice_max_height = 0.65f;
  p->mesh_min_weight = 0.1f; p->mesh_weld_vertices = 1;
  p->sphere_tracing_subsampling = 4; p->sphere_tracing_max_steps = 100;
  p->sphere_tracing_max_ray_length_m = 15.0f; p->sphere_tracing_surface_eps_vox = 0.1f;
  p->tsdf_decay_factor = 0.95f; p->tsdf_decayed_weight_threshold = 0.001f;
  p->esdf_site_rule = 0; p->depth_interp_nearest = 0;
  p->lidar_max_integration_distance_m = 10.0f;
  p->lidar_linear_interpolation_max_allowable_difference_vox = 2.0f;
  p->lidar_nearest_interpolation_max_allowable_dist_to_ray_vox = 0.5f;
  p->invalid_depth_decay_factor = -1.0f;
  p->projective_layer_type = 0;
  p->free_region_occupancy_probability = 0.45f; p->occupied_region_occupancy_probability = 0.55f;
  p->unobserved_region_occupancy_probability = 0.5f; p->occupied_region_half_width_m = 0.1f;
  p->free_region_decay_probability = 0.55f; p->occupied_region_decay_probability = 0.30f;
  p->esdf_mode = 0;
  p->max_tsdf_distance_for_occupancy_m = 0.15f; p->max_unobserved_to_keep_consecutive_occupancy_ms = 200;
  p->min_duration_since_occupied_for_freespace_ms = 1000; p->min_consecutive_occupancy_duration_for_reset_ms = 2000;
  p->check_neighborhood = 1; p->initialize_to_high_confidence_freespace = 0;
  p->tsdf_weighting_variant = 0; p->tsdf_skip_at_negative_truncation = 0; p->tsdf_weight_clamp_before_blend = 0;
  p->color_occlusion_threshold_vox = -1.0f; p->esdf_propagation = 0; p->mesh_ambiguity_rule = 0; p->mesh_normal_rule = 0;
  p->decay_deallocate_decayed_blocks = 1; p->tsdf_set_free_distance_on_decayed = 0; p->tsdf_decayed_free_distance_vox = 4.0f; p->occupancy_decay_to_free = 0;
}
__global__ void k_selftest_arith(const float* a, const float* b, float* q, float* r, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    q[i] = NVBX_DIV(a[i], b[i]);
    r[i] = NVBX_SQRT(fabsf(a[i]));
  }
}
extern "C" int nvbx_selftest_arith(const float* a_dev, const float* b_dev, float* quot_dev, float* root_dev, int64_t n) {
  if (!a_dev || !b_dev || !quot_dev || !root_dev || n < 0) { set_error("nvbx_selftest_arith: invalid argument"); return NVBX_E_INVALID; }
  if (n > 0) k_selftest_arith<<<dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256)>>>(a_dev, b_dev, quot_dev, root_dev, n);
  NVBX_HIP(hipGetLastError());
  NVBX_HIP(hipDeviceSynchronize());
  return NVBX_OK;
}
extern "C" int nvbx_get_stream(nvbx_mapper* m, void** hip_stream_out) {
  if (!m || !hip_stream_out) return NVBX_E_INVALID;
  *hip_stream_out = (void*)m->stream;
  return NVBX_OK;
}
// Two mappers on two streams (a MultiMapper whose foreground mapper runs beside the background mapper): `waiter`'s stream takes up work enqueued
// after this call only when everything enqueued on `producer`'s stream so far has finished.
extern "C" int nvbx_mapper_wait_for(nvbx_mapper* waiter, nvbx_mapper* producer) {
  if (!waiter || !producer) return NVBX_E_INVALID;
  if (waiter == producer || waiter->stream == producer->stream) return NVBX_OK;
  if (waiter->device != producer->device) { set_error("nvbx_mapper_wait_for: mappers on different devices"); return NVBX_E_INVALID; }
  NVBX_HIP(hipSetDevice(producer->device));
  if (!producer->ev_order) NVBX_HIP(hipEventCreateWithFlags(&producer->ev_order, hipEventDisableTiming));
  NVBX_HIP(hipEventRecord(producer->ev_order, producer->stream));
  NVBX_HIP(hipStreamWaitEvent(waiter->stream, producer->ev_order, 0));
  return NVBX_OK;
}
extern "C" int nvbx_mapper_clear(nvbx_mapper* m) {
  if (!m) return NVBX_E_INVALID;
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call()) return NVBX_E_DEVICE;
  return reset_map(m);
}

extern "C" int nvbx_get_counters(nvbx_mapper* m, nvbx_counters* out) {
  if (!m || !out) return NVBX_E_INVALID;
  if (m->fetch_counters()) return NVBX_E_DEVICE;
  const int32_t* c = m->h_counters;
  memset(out, 0, sizeof(*out));
  out->blocks_allocated = (int64_t)m->capacity - (int64_t)c[C_FREE_TOP];       // every slot is free or live
  out->tsdf_blocks_in_view = m->last_view_frame ? c[C_VIEW_COUNT + (m->last_view_frame & 3)] : 0;
  out->color_blocks_updated = m->shc_sum(S_LIST_COLOR, 0);
  const int epar = (int)((m->esdf_epoch + 1) & 1);                    // record of the last finished update (epoch - 1)
  out->esdf_columns_marked = m->esdf_epoch ? m->shc_sum(S_ESDF_REC + epar, 4) : 0;
  out->esdf_blocks_swept = m->esdf_epoch ? m->shc_sum(S_ESDF_REC + epar, 5) : 0;
  out->esdf_window_voxels = m->esdf_epoch ? c[C_ESDF_UPD + 8 * epar + 6] : 0;
  if (m->p.esdf_mode == 1) { out->esdf_columns_marked = m->esdf3_blocks_marked; out->esdf_blocks_swept = m->esdf3_window_voxels / 512; out->esdf_window_voxels = m->esdf3_window_voxels; }
  const int mpar = (int)((m->mesh_epoch + 1) & 1);                    // record of the last finished mesh update
  out->mesh_blocks_updated = m->mesh_epoch ? m->shc_sum(S_MESH_REC + mpar, 0) : 0;
  out->mesh_vertices = m->mesh_epoch ? m->shc_sum(S_MESH_REC + mpar, 2) : 0;
  out->mesh_triangles = m->mesh_epoch ? m->shc_sum(S_MESH_REC + mpar, 3) : 0;
  out->capacity_overflow = c[C_OVERFLOW];
  out->lidar_blocks_beam_centric = m->shc_sum(S_LIDAR_SPARSE, 0);
  return NVBX_OK;
}
