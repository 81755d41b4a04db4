// layers.hip -- layer access of the C-ABI: which blocks a layer (or the last view) holds; whole blocks out of / into the map as the reference's voxel structs.
#include <cstring>
#include "nvbx_mapper.h"
using namespace nvbx;

// collect Index3D of every live slot carrying `layer` (order arbitrary; host sorts)
__global__ void k_collect_indices(DMap m, uint32_t layer, int32_t* out, int32_t cap) {
  const int32_t hw = m.counters[C_HIGH_WATER];
  for (int32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < hw; s += gridDim.x * blockDim.x) {
    if (m.slot_flags[s] & layer) {
      const int32_t p = atomicAdd(&m.counters[C_TMP], 1);
      if (p < cap) { out[3 * p] = m.slot_index[3 * s]; out[3 * p + 1] = m.slot_index[3 * s + 1]; out[3 * p + 2] = m.slot_index[3 * s + 2]; }
    }
  }
}
__global__ void k_zero_tmp(DMap m) { m.counters[C_TMP] = 0; }

// view list ({slot, x, y, z} records of one frame) -> Index3D.  cam_mask != 0 (the frame was a batch): only the blocks the
// cameras of the mask had in view -- "the last depth view" of a batch is its last camera's, as separate calls would leave it.
__global__ void k_viewlist_to_indices(DMap m, const int4* list, int32_t count_idx, uint32_t cam_mask, int32_t* out, int32_t cap) {
  int32_t n = m.counters[count_idx]; if (n > cap) n = cap;
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int4 r = list[i];
    bool ok = slot_ok((uint32_t)r.x) && m.slot_flags[(uint32_t)r.x];
    if (ok && cam_mask && !(m.table[m.slot_entry[(uint32_t)r.x]].stamp & cam_mask)) ok = false;
    out[3 * i] = ok ? r.y : INT32_MIN; out[3 * i + 1] = ok ? r.z : INT32_MIN; out[3 * i + 2] = ok ? r.w : INT32_MIN;
  }
}

// sharded work list (slot ids) -> Index3D, written to out[0..n) in list order; *n_out = entries
__global__ void k_shardlist_to_indices(DMap m, int list, int32_t* out, int32_t cap, int32_t* n_out) {
  ListView v; int32_t n = list_open(m, list, &v); if (n > cap) n = cap;
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = n;
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t s = (uint32_t)list_at(m, list, v, i);
    if (slot_ok(s) && m.slot_flags[s]) { out[3 * i] = m.slot_index[3 * s]; out[3 * i + 1] = m.slot_index[3 * s + 1]; out[3 * i + 2] = m.slot_index[3 * s + 2]; }
    else { out[3 * i] = INT32_MIN; out[3 * i + 1] = INT32_MIN; out[3 * i + 2] = INT32_MIN; }
  }
}

// gather n blocks of `layer` into a dense buffer in the REFERENCE voxel struct layout (z + 8y + 64x order).
// found[i] = 1 if the block exists.  One 512-thread workgroup per block.
// `layer` is the INTERNAL flag; occupancy = 1: the projective pool holds log-odds and leaves as nvbx_occupancy_voxel {f32}
__global__ __launch_bounds__(512) void k_gather_blocks(DMap m, uint32_t layer, int32_t occupancy, const int32_t* idx, int32_t n, uint8_t* out, int32_t* found) {
  const int i = blockIdx.x; if (i >= n) return;
  const uint32_t s = find_slot(m, idx[3 * i], idx[3 * i + 1], idx[3 * i + 2], layer);
  const int t = threadIdx.x;
  if (t == 0) found[i] = slot_ok(s) ? 1 : 0;
  if (!slot_ok(s)) {            // absent block: zeros, never stale staging bytes
    const size_t vb = layer == F_ESDF ? sizeof(nvbx_esdf_voxel) : (layer == F_FREESPACE ? sizeof(nvbx_freespace_voxel) : ((layer == F_TSDF && occupancy) ? 4 : 8));
    for (size_t q = t; q < 512 * vb / 4; q += 512) reinterpret_cast<uint32_t*>(out + (size_t)i * 512 * vb)[q] = 0u;
    return;
  }
  if (layer == F_TSDF && occupancy) { reinterpret_cast<float*>(out)[(size_t)i * 512 + t] = m.tsdf[(size_t)s * 512 + t].x; }
  else if (layer == F_TSDF) { reinterpret_cast<float2*>(out)[(size_t)i * 512 + t] = m.tsdf[(size_t)s * 512 + t]; }
  else if (layer == F_COLOR) { reinterpret_cast<uint2*>(out)[(size_t)i * 512 + t] = m.color[(size_t)s * 512 + t]; }
  else if (layer == F_FREESPACE) {
    const int4 v = m.freespace[(size_t)s * 512 + t];
    nvbx_freespace_voxel o;
    o.last_occupied_timestamp_ms = (int64_t)(((u64)(uint32_t)v.y << 32) | (u64)(uint32_t)v.x);
    o.consecutive_occupancy_duration_ms = (int64_t)v.z;
    o.is_high_confidence_freespace = (uint8_t)(v.w & 1); o.initialized = (uint8_t)((v.w >> 1) & 1);
    for (int q = 0; q < 6; q++) o.pad[q] = 0;
    reinterpret_cast<nvbx_freespace_voxel*>(out)[(size_t)i * 512 + t] = o;
  }
  else if (layer == F_ESDF) {
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7;             // reference order
    const uint2 v = m.esdf[(size_t)s * 512 + x + 8 * y + 64 * z];  // device order
    nvbx_esdf_voxel o;
    o.squared_distance_vox = __uint_as_float(v.x);
    o.parent_direction[0] = (int8_t)(v.y & 0xFF); o.parent_direction[1] = (int8_t)((v.y >> 8) & 0xFF); o.parent_direction[2] = (int8_t)((v.y >> 16) & 0xFF);
    o.observed = (v.y & ESDF_OBSERVED) ? 1 : 0; o.is_inside = (v.y & ESDF_INSIDE) ? 1 : 0; o.is_site = (v.y & ESDF_SITE) ? 1 : 0; o.pad = 0;
    reinterpret_cast<nvbx_esdf_voxel*>(out)[(size_t)i * 512 + t] = o;
  }
}

// allocateBlockAtIndex + whole-block write from reference structs: workgroup i writes block idx[i] from in[i][512]
__global__ __launch_bounds__(512) void k_scatter_blocks(DMap m, uint32_t layer, int32_t occupancy, const int32_t* idx, const uint8_t* in_all, size_t block_bytes,
                                                        int32_t mesh_list, int32_t bz_out, int32_t vz_out, float trunc) {
  __shared__ uint32_t s_slot;
  __shared__ u64 s_sites, s_obs, s_ins;
  const int t = threadIdx.x;
  const int32_t x = idx[3 * blockIdx.x], y = idx[3 * blockIdx.x + 1], z = idx[3 * blockIdx.x + 2];
  const uint8_t* in = in_all + (size_t)blockIdx.x * block_bytes;
  if (t == 0) {
    bool is_new; const int32_t h = hash_insert(m, x, y, z, layer, &is_new);
    uint32_t s = SLOT_NONE;
    // (a duplicate index in one batch: the workgroup that lost the insert waits for the winner to publish the slot, as mark_block does)
    if (h >= 0) { do { s = ld_slot_acquire(&m.table[h]); } while (s == SLOT_INVALID); }
    if (slot_ok(s)) {
      uint32_t add = layer;
      if (layer == F_TSDF) add |= F_DIRTY_ESDF | F_DIRTY_MESH;
      const uint32_t old = atomicOr(&m.slot_flags[s], add);
      if (layer == F_TSDF) {
        if (!(old & F_DIRTY_ESDF)) list_append(m, S_LIST_ESDF_DIRTY, (int32_t)s);
        if (!(old & F_DIRTY_MESH)) list_append(m, mesh_list, (int32_t)s);
      }
      if (layer == F_ESDF && z == bz_out) {     // (3-D ESDF: only the slice plane's blocks span the slicer's image)
        atomicMin(&m.counters[C_ESDF_AABB + 0], x); atomicMin(&m.counters[C_ESDF_AABB + 1], y);
        atomicMax(&m.counters[C_ESDF_AABB + 2], x); atomicMax(&m.counters[C_ESDF_AABB + 3], y);
      }
    }
    s_slot = s; s_sites = 0ull; s_obs = 0ull; s_ins = 0ull;
  }
  __syncthreads();
  const uint32_t s = s_slot;
  if (!slot_ok(s)) return;
  if (layer == F_TSDF && occupancy) m.tsdf[(size_t)s * 512 + t] = make_float2(reinterpret_cast<const float*>(in)[t], 0.0f);
  else if (layer == F_TSDF) {
    const float2 v = reinterpret_cast<const float2*>(in)[t];
    m.tsdf[(size_t)s * 512 + t] = v;
    publish_band(m.slot_flags, s, t, in_band(v.x, v.y, trunc));        // (uniform branch: every wavefront is here)
  }
  else if (layer == F_COLOR) m.color[(size_t)s * 512 + t] = reinterpret_cast<const uint2*>(in)[t];
  else if (layer == F_ESDF) {
    const int vx = t >> 6, vy = (t >> 3) & 7, vz = t & 7;
    const nvbx_esdf_voxel v = reinterpret_cast<const nvbx_esdf_voxel*>(in)[t];
    m.esdf[(size_t)s * 512 + vx + 8 * vy + 64 * vz] =
        make_uint2(__float_as_uint(v.squared_distance_vox),
                   esdf_meta(v.parent_direction[0], v.parent_direction[1], v.parent_direction[2], v.observed, v.is_inside, v.is_site));
    // keep the slice plane's site mask (what k_esdf_edt reads) consistent with the written voxels
    if (z == bz_out && vz == vz_out) {
      if (v.is_site) atomicOr(&s_sites, 1ull << (vx + 8 * vy));
      if (v.observed) atomicOr(&s_obs, 1ull << (vx + 8 * vy));
      if (v.is_inside) atomicOr(&s_ins, 1ull << (vx + 8 * vy));
    }
    __syncthreads();
    if (t == 0) { m.site_bits[s] = (z == bz_out) ? s_sites : 0ull; m.obs_bits[s] = (z == bz_out) ? s_obs : 0ull; m.inside_bits[s] = (z == bz_out) ? s_ins : 0ull; }
  }
}
// ------------------------------------------------------------------------------------------------ C-ABI: layer access
// API layer id -> internal slot flag; 0 = this mapper cannot hold that layer (it reads as empty).  The projective layer of a
// mapper (TSDF or occupancy, Mapper's ProjectiveLayerType) lives in the same pool under the same internal flag.
uint32_t nvbx::internal_layer(const nvbx_mapper* m, uint32_t layer) {
  const bool occ = m->p.projective_layer_type == 1;
  if (layer == NVBX_LAYER_OCCUPANCY) return occ ? F_TSDF : 0u;
  if (layer == F_TSDF) return occ ? 0u : F_TSDF;
  if (layer == F_FREESPACE) return m->d.freespace ? F_FREESPACE : 0u;
  return layer;
}

static void sort_indices(nvbx_index3d* v, int64_t n) {
  std::sort(v, v + n, [](const nvbx_index3d& a, const nvbx_index3d& b) {
    if (a.x != b.x) return a.x < b.x; if (a.y != b.y) return a.y < b.y; return a.z < b.z; });
}
// The n indices a kernel has left in export_idx -> the caller, sorted: out[0 .. min(count, capacity)); returns the count.  filter: entries written as
// INT32_MIN (deallocated since / not in the mask) are dropped first -- the count is theirs, so even a count-only call downloads.
static int64_t download_indices(nvbx_mapper* m, int64_t n, bool filter, nvbx_index3d* out, int64_t capacity) {
  if (!filter && !(out && std::min(n, capacity) > 0)) return n;
  std::vector<nvbx_index3d> tmp((size_t)n);
  if (n > 0) NVBX_HIP(hipMemcpy(tmp.data(), m->export_idx, (size_t)n * 12, hipMemcpyDeviceToHost));
  if (filter) { tmp.erase(std::remove_if(tmp.begin(), tmp.end(), [](const nvbx_index3d& i) { return i.x == INT32_MIN; }), tmp.end()); n = (int64_t)tmp.size(); }
  const int64_t k = std::min(n, capacity);
  if (out && k > 0) { sort_indices(tmp.data(), n); memcpy(out, tmp.data(), (size_t)k * 12); }
  return n;
}

extern "C" int64_t nvbx_block_indices(nvbx_mapper* m, uint32_t layer, nvbx_index3d* out, int64_t capacity) {
  if (!m || !layer_listable(layer)) return NVBX_E_INVALID;
  layer = internal_layer(m, layer);
  if (!layer) return 0;
  if (m->begin_call()) return NVBX_E_DEVICE;
  NVBX_LAUNCH(m, k_zero_tmp, dim3(1), dim3(1), m->d);
  NVBX_LAUNCH(m, k_collect_indices, dim3(256), dim3(256), m->d, layer, m->export_idx, (int32_t)m->capacity);
  if (m->fetch_counters()) return NVBX_E_DEVICE;
  int64_t n = m->h_counters[C_TMP];
  if (n > m->capacity) n = m->capacity;
  return download_indices(m, n, false, out, capacity);
}
extern "C" int64_t nvbx_num_blocks(nvbx_mapper* m, uint32_t layer) { return nvbx_block_indices(m, layer, nullptr, 0); }

extern "C" int64_t nvbx_last_depth_view(nvbx_mapper* m, nvbx_index3d* out, int64_t capacity) {
  if (!m) return NVBX_E_INVALID;
  if (m->last_view_frame == 0) return 0;
  if (m->begin_call()) return NVBX_E_DEVICE;
  const uint32_t cam_mask = m->last_view_batch > 1 ? (1u << (m->last_view_batch - 1)) : 0u;
  NVBX_LAUNCH(m, k_viewlist_to_indices, dim3(64), dim3(256), m->d, (const int4*)m->view_list, C_VIEW_COUNT + (int)(m->last_view_frame & 3), cam_mask, m->export_idx, (int32_t)m->capacity);
  if (m->fetch_counters()) return NVBX_E_DEVICE;
  int64_t n = m->h_counters[C_VIEW_COUNT + (m->last_view_frame & 3)]; if (n > m->capacity) n = m->capacity;
  return download_indices(m, n, true, out, capacity);
}
extern "C" int64_t nvbx_last_color_view(nvbx_mapper* m, nvbx_index3d* out, int64_t capacity) {
  if (!m) return NVBX_E_INVALID;
  if (m->begin_call()) return NVBX_E_DEVICE;
  NVBX_LAUNCH(m, k_shardlist_to_indices, dim3(64), dim3(256), m->d, (int)S_LIST_COLOR, m->export_idx, (int32_t)m->capacity, m->export_count);
  int32_t n32 = 0;
  NVBX_HIP(hipMemcpyAsync(&n32, m->export_count, 4, hipMemcpyDeviceToHost, m->stream));
  NVBX_HIP(hipStreamSynchronize(m->stream));
  return download_indices(m, n32, false, out, capacity);
}

size_t nvbx::ref_voxel_bytes(uint32_t layer) { return layer == F_ESDF ? sizeof(nvbx_esdf_voxel) : (layer == NVBX_LAYER_OCCUPANCY ? sizeof(nvbx_occupancy_voxel) : (layer == F_FREESPACE ? sizeof(nvbx_freespace_voxel) : 8)); }

extern "C" int nvbx_get_blocks(nvbx_mapper* m, uint32_t layer, const nvbx_index3d* idx, int64_t n, void* voxels_out, int32_t* found_out) {
  if (!m || !idx || !voxels_out || n < 0 || !layer_readable(layer)) return NVBX_E_INVALID;
  if (m->begin_call()) return NVBX_E_DEVICE;
  const size_t bb = 512 * ref_voxel_bytes(layer);
  const uint32_t ilayer = internal_layer(m, layer);
  if (!ilayer) { if (found_out) memset(found_out, 0, (size_t)n * 4); return NVBX_OK; }
  const int64_t chunk = std::max<int64_t>(1, (int64_t)((m->staging.bytes - 65536) / (bb + 16)));
  for (int64_t o = 0; o < n; o += chunk) {
    const int64_t c = std::min(chunk, n - o);
    int32_t* d_idx = m->staging.as<int32_t>(); int32_t* d_found = d_idx + 3 * c;
    uint8_t* d_out = m->staging.as<uint8_t>() + (((size_t)c * 16 + 255) & ~(size_t)255);
    NVBX_HIP(hipMemcpyAsync(d_idx, idx + o, (size_t)c * 12, hipMemcpyHostToDevice, m->stream));
    NVBX_LAUNCH(m, k_gather_blocks, dim3((unsigned)c), dim3(512), m->d, ilayer, (int32_t)(layer == NVBX_LAYER_OCCUPANCY), d_idx, (int32_t)c, d_out, d_found);
    NVBX_HIP(hipMemcpyAsync((uint8_t*)voxels_out + (size_t)o * bb, d_out, (size_t)c * bb, hipMemcpyDeviceToHost, m->stream));
    if (found_out) NVBX_HIP(hipMemcpyAsync(found_out + o, d_found, (size_t)c * 4, hipMemcpyDeviceToHost, m->stream));
    NVBX_HIP(hipStreamSynchronize(m->stream));
  }
  return NVBX_OK;
}
extern "C" int nvbx_get_block(nvbx_mapper* m, uint32_t layer, nvbx_index3d idx, void* voxels_out) {
  int32_t found = 0;
  const int rc = nvbx_get_blocks(m, layer, &idx, 1, voxels_out, &found);
  if (rc) return rc;
  return found ? NVBX_OK : NVBX_E_NOTFOUND;
}
extern "C" int nvbx_set_blocks(nvbx_mapper* m, uint32_t layer, const nvbx_index3d* idx, int64_t n, const void* voxels_in) {
  if (!m || (n > 0 && (!voxels_in || !idx)) || n < 0 || !layer_writable(layer)) return NVBX_E_INVALID;
  const uint32_t ilayer = internal_layer(m, layer);
  if (!ilayer) { set_error("nvbx_set_blocks: this mapper's projective layer type does not hold that layer"); return NVBX_E_INVALID; }
  for (int64_t i = 0; i < n; i++) if (!nvbx_index_in_range(idx[i].x, idx[i].y, idx[i].z)) { set_error("nvbx_set_blocks: block index outside +-2^20"); return NVBX_E_INVALID; }
  if (m->begin_call()) return NVBX_E_DEVICE;
  if (m->capacity < m->max_capacity) {          // explicit allocation (allocateBlockAtIndex, loadMap): room for all of it, plus the usual head-room
    if (m->fetch_counters()) return NVBX_E_DEVICE;
    m->h_mirror[0] = m->h_counters[C_FREE_TOP];
    const int rcg = m->maybe_grow(n); if (rcg) return rcg;
  }
  if (m->begin_dirtying()) return NVBX_E_DEVICE;
  const size_t bb = 512 * ref_voxel_bytes(layer);
  const EsdfArgs ea = m->make_esdf_args();
  const int64_t chunk = std::max<int64_t>(1, (int64_t)((m->staging.bytes - 65536) / (bb + 16)));
  for (int64_t o = 0; o < n; o += chunk) {
    const int64_t c = std::min(chunk, n - o);
    int32_t* d_idx = m->staging.as<int32_t>();
    uint8_t* d_in = m->staging.as<uint8_t>() + (((size_t)c * 16 + 255) & ~(size_t)255);
    NVBX_HIP(hipMemcpyAsync(d_idx, idx + o, (size_t)c * 12, hipMemcpyHostToDevice, m->stream));
    NVBX_HIP(hipMemcpyAsync(d_in, (const uint8_t*)voxels_in + (size_t)o * bb, (size_t)c * bb, hipMemcpyHostToDevice, m->stream));
    NVBX_LAUNCH(m, k_scatter_blocks, dim3((unsigned)c), dim3(512), m->d, ilayer, (int32_t)(layer == NVBX_LAYER_OCCUPANCY), (const int32_t*)d_idx, (const uint8_t*)d_in, bb,
                (int32_t)m->mesh_list_live(), ea.bz_out, ea.vz_out, m->p.truncation_distance_vox * m->p.voxel_size);
    NVBX_HIP(hipStreamSynchronize(m->stream));
  }
  return NVBX_OK;
}
extern "C" int nvbx_set_block(nvbx_mapper* m, uint32_t layer, nvbx_index3d idx, const void* voxels_in) {
  return nvbx_set_blocks(m, layer, &idx, 1, voxels_in);
}
