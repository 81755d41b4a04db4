// nvbx_map_transfer.h -- what nvbx_merge_map (merge.hip) and nvbx_resample_map (resample.hip) share: one mapper's TSDF and colour brought into
// another under a rigid transform.  The calls differ in the candidate box of a source block (a Box functor), in their
// fuse kernel and in a few refusals; everything else is here, once:
//   k_transfer_count<Box>  one thread per (source slot, candidate 0 .. 26): the candidate box of the slot's block and, for every candidate dst
//                          lacks, an insert into a scratch key set -- the distinct ones are counted.  Nothing of dst is written: the host
//                          waits for the counts, grows dst's pools if it must, or refuses (NVBX_E_CAPACITY) with dst untouched.
//   k_transfer_index<Box>  the same enumeration again, now with mark_block on dst: missing blocks are allocated, every candidate is stamped
//                          with the call's frame id and appended to dst's view list exactly once -- the work list of the call's fuse launch
//                          (k_apply_index is the pattern).
//   k_transfer_result      one thread: the caller's result record from the counters the launches left.
//   transfer_call          the host sequence around them (its launch spans are named by the template's text: k_transfer_count<Box> for both calls).
// The fuse kernels stay with their calls: lifting code out of k_merge_fuse costs it registers.
#pragma once
#include "nvbx_view.h"
#include "nvbx_merge_math.h"      // (nvbx_merge_rotation_ok)

// head of nvbx_mapper::merge_buf (zeroed per call); the key set follows at TRANSFER_KEYS_OFFSET
struct TransferScratch { int32_t src_blocks, need_slots, need_tsdf, dst_free; unsigned long long voxels, colors; };
constexpr size_t TRANSFER_KEYS_OFFSET = 64;
static_assert(sizeof(TransferScratch) <= TRANSFER_KEYS_OFFSET, "scratch head");
static_assert(sizeof(nvbx_merge_result) == 64, "C-ABI layout");

// candidate c (0 .. 26) of source slot s: false if the slot holds no TSDF block or the box has no such block.  Box: trivially copyable, a kernel
// argument; box(si, lo, hi) is the call's candidate box of source block si (nvbx_merge_candidate_box, nvbx_resample_candidate_box)
template <class Box>
__device__ inline bool transfer_candidate(const DMap& src, const Box& box, int32_t s, int c, int32_t* x, int32_t* y, int32_t* z) {
  if (!(src.slot_flags[s] & F_TSDF)) return false;
  const int32_t si[3] = {src.slot_index[3 * s], src.slot_index[3 * s + 1], src.slot_index[3 * s + 2]};
  int32_t lo[3], hi[3];
  if (!box(si, lo, hi)) return false;
  *x = lo[0] + c % 3; *y = lo[1] + (c / 3) % 3; *z = lo[2] + c / 9;
  return *x <= hi[0] && *y <= hi[1] && *z <= hi[2];
}

template <class Box>
__global__ void k_transfer_count(DMap dst, DMap src, Box box, TransferScratch* sc, u64* keys, uint32_t kmask) {
  const int64_t n = (int64_t)src.counters[C_HIGH_WATER] * 27;
  if (blockIdx.x == 0 && threadIdx.x == 0) sc->dst_free = dst.counters[C_FREE_TOP];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t s = (int32_t)(i / 27); const int c = (int)(i - (int64_t)s * 27);
    if (c == 0 && (src.slot_flags[s] & F_TSDF)) atomicAdd(&sc->src_blocks, 1);
    int32_t x, y, z;
    if (!transfer_candidate(src, box, s, c, &x, &y, &z)) continue;
    // what dst has: an entry with a slot (a block of any layer shares it), and whether that slot carries a TSDF block
    const u64 key = pack_key(x, y, z);
    bool has_slot = false, has_tsdf = false;
    uint32_t h = table_pos(dst, x, y, z);
    for (uint32_t probe = 0; probe <= dst.mask; ++probe) {
      const uint4 e = ld_entry(dst, h);
      const u64 k = ((u64)e.y << 32) | (u64)e.x;
      if (k == key) { has_slot = true; has_tsdf = slot_ok(e.z) && (dst.slot_flags[e.z] & F_TSDF); break; }
      if (k == KEY_EMPTY) break;
      h = (h + 1) & dst.mask;
    }
    if (has_tsdf) continue;
    uint32_t kh = (index_hash(x, y, z) * 2654435761u) & kmask;
    for (uint32_t probe = 0; probe <= kmask; ++probe) {
      const u64 old = atomicCAS(&keys[kh], KEY_EMPTY, key);
      if (old == KEY_EMPTY) { atomicAdd(&sc->need_tsdf, 1); if (!has_slot) atomicAdd(&sc->need_slots, 1); break; }
      if (old == key) break;
      kh = (kh + 1) & kmask;
    }
  }
}

template <class Box>
__global__ void k_transfer_index(DMap dst, DMap src, Box box, uint32_t frame_id, int4* view_list, int32_t list_cap) {
  int32_t* cnt = &dst.counters[C_VIEW_COUNT + (frame_id & 3)];
  if (blockIdx.x == 0 && threadIdx.x == 0) dst.counters[C_VIEW_COUNT + ((frame_id + 1) & 3)] = 0;
  const int64_t n = (int64_t)src.counters[C_HIGH_WATER] * 27;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t s = (int32_t)(i / 27); const int c = (int)(i - (int64_t)s * 27);
    int32_t x, y, z;
    if (!transfer_candidate(src, box, s, c, &x, &y, &z)) continue;
    int4 rec;
    if (!mark_block(dst, pack_key(x, y, z), frame_id, 1u, &rec)) continue;      // (stamped already: another source block's candidate too)
    const int32_t p = atomicAdd(cnt, 1);
    if (p < list_cap) view_list[p] = rec;
  }
}

// empty != 0: nothing was enumerated (src has no TSDF block).  (static: defined in both calls' translation units)
static __global__ void k_transfer_result(DMap dst, uint32_t frame_id, const TransferScratch* sc, int64_t src_blocks, int64_t allocated, int32_t empty, nvbx_merge_result* out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  nvbx_merge_result r;
  r.source_blocks = src_blocks;
  r.candidate_blocks = empty ? 0 : (int64_t)dst.counters[C_VIEW_COUNT + (frame_id & 3)];
  r.blocks_allocated = allocated;
  r.voxels_fused = empty ? 0 : (int64_t)sc->voxels;
  r.color_voxels_fused = empty ? 0 : (int64_t)sc->colors;
  r.status = empty ? NVBX_MERGE_EMPTY_SOURCE : (r.voxels_fused == 0 ? NVBX_MERGE_NO_OVERLAP : NVBX_MERGE_OK);
  for (int k = 0; k < 5; k++) r.pad[k] = 0;
  *out = r;
}

// THE refusals both calls make, in their order, in two parts around each call's own voxel-size refusals -> 0, or NVBX_E_INVALID with the error
// set.  missing: what the call found missing among its pointers (its own condition and text), null = nothing
static inline int transfer_pointers_refused(const char* who, const nvbx_mapper* dst, const nvbx_mapper* src, const char* missing, const void* result_dev) {
  if (!dst || !src) return refuse(who, ": both mappers are required");
  if (missing) return refuse(who, missing);
  if ((uintptr_t)result_dev & 7) return refuse(who, ": result_dev must be 8-byte aligned");
  if (src == dst) return refuse(who, ": src and dst are the same mapper");
  if (src->device != dst->device) return refuse(who, ": the mappers are on different devices");
  return 0;
}
// pose_block_size: the block size the pose's range is measured in (dst's in the merge, src's in resampling)
static inline int transfer_values_refused(const char* who, const nvbx_mapper* dst, const nvbx_mapper* src, const float T_D_S[16], float pose_block_size, float min_weight, float weight_scale) {
  if (src->p.projective_layer_type != 0 || dst->p.projective_layer_type != 0) return refuse(who, ": both mappers must be TSDF mappers without a freespace layer (projective_layer_type 0)");
  if (!nvbx_pose_in_range(T_D_S, pose_block_size, 0.0f)) return refuse(who, ": the pose is not finite or out of range");
  if (!nvbx_merge_rotation_ok(T_D_S, nullptr, nullptr)) return refuse(who, ": the upper-left 3 x 3 of T_D_S is not a rotation (|R^T R - I| > 1e-5 or det <= 0)");
  if (min_weight != min_weight) return refuse(who, ": min_weight is not a number");
  if (!std::isfinite(weight_scale) || !(weight_scale > 0.0f)) return refuse(who, ": weight_scale must be finite and > 0");
  return 0;
}

// The call after its refusals.  verb: "merged" / "resampled", what the capacity refusals say was not done; fuse_cap: the most workgroups of the
// fuse launch; fuse(grid, frame_id, mesh_list, sc) enqueues that launch on dst's stream.  Everything runs on dst's stream, src is read only.
template <class Box, class Fuse>
inline int transfer_call(const char* who, const char* verb, nvbx_mapper* dst, nvbx_mapper* src, const Box& box, int64_t fuse_cap, nvbx_merge_result* result_dev, Fuse&& fuse) {
  NVBX_HIP(hipSetDevice(dst->device));
  // src: held-back work is carried out; its block count sizes the key set (waits for src's stream)
  if (src->fetch_counters()) return NVBX_E_DEVICE;
  const int64_t src_hw = src->h_counters[C_HIGH_WATER];
  const int64_t src_live = std::max<int64_t>(1, (int64_t)src->capacity - (int64_t)src->h_counters[C_FREE_TOP]);
  if (dst->begin_call()) return NVBX_E_DEVICE;
  { const int rc = nvbx_mapper_wait_for(dst, src); if (rc) return rc; }
  // the key set: distinct candidates are at most 27 per source block; load <= 1/2
  uint64_t entries = 64; while (entries < (uint64_t)src_live * 54) entries <<= 1;
  if (entries > (1ull << 31)) return refuse(who, ": the source map is too large to enumerate");
  if (dst->merge_buf.ensure(dst->stream, TRANSFER_KEYS_OFFSET + (size_t)entries * 8)) return NVBX_E_DEVICE;
  TransferScratch* sc = dst->merge_buf.as<TransferScratch>();
  u64* keys = reinterpret_cast<u64*>(dst->merge_buf.as<unsigned char>() + TRANSFER_KEYS_OFFSET);
  NVBX_HIP(hipMemsetAsync(sc, 0, TRANSFER_KEYS_OFFSET, dst->stream));
  TransferScratch h{};
  const unsigned enum_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((src_hw * 27 + 255) / 256, 2048));
  if (src_hw > 0) {
    NVBX_HIP(hipMemsetAsync(keys, 0xFF, (size_t)entries * 8, dst->stream));
    NVBX_LAUNCH(dst, k_transfer_count<Box>, dim3(enum_grid), dim3(256), dst->d, src->d, box, sc, keys, (uint32_t)(entries - 1));
    NVBX_HIP(hipGetLastError());
    NVBX_HIP(hipMemcpyAsync(&h, sc, sizeof(h), hipMemcpyDeviceToHost, dst->stream));
    NVBX_HIP(hipStreamSynchronize(dst->stream));                    // the one wait between enumerating and allocating
  }
  if (h.src_blocks == 0) {
    NVBX_LAUNCH(dst, k_transfer_result, dim3(1), dim3(64), dst->d, 0u, (const TransferScratch*)sc, (int64_t)0, (int64_t)0, 1, result_dev);
    NVBX_HIP(hipGetLastError());
    return nvbx_mapper_wait_for(src, dst);
  }
  // room for every candidate dst lacks, or nothing is touched
  {
    const auto no_room = [&](const char* why) { set_error((std::string(who) + why + ", nothing was " + verb).c_str()); return (int)NVBX_E_CAPACITY; };
    const int64_t need = h.need_slots, free_now = h.dst_free;
    if (need > free_now + (dst->max_capacity - dst->capacity)) return no_room(": dst's max_capacity cannot hold the candidate blocks");
    const int64_t cap_before = dst->capacity;
    if (dst->capacity < dst->max_capacity) {
      dst->h_mirror[0] = (int32_t)free_now;
      const int rc = dst->maybe_grow(need); if (rc) return rc;
    }
    if (need > free_now + (dst->capacity - cap_before)) return no_room(": dst's block pools could not grow to hold the candidate blocks");
  }
  if (dst->begin_dirtying()) return NVBX_E_DEVICE;
  { const int rc = next_frame_id(dst); if (rc) return rc; }
  NVBX_LAUNCH(dst, k_transfer_index<Box>, dim3(enum_grid), dim3(256), dst->d, src->d, box, dst->frame_id, (int4*)dst->view_list, (int32_t)dst->capacity);
  const unsigned fuse_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(dst->capacity, (int64_t)h.src_blocks * 27), fuse_cap));
  fuse(fuse_grid, dst->frame_id, dst->mesh_list_live(), sc);
  NVBX_LAUNCH(dst, k_transfer_result, dim3(1), dim3(64), dst->d, dst->frame_id, (const TransferScratch*)sc, (int64_t)h.src_blocks, (int64_t)h.need_tsdf, 0, result_dev);
  NVBX_HIP(hipGetLastError());
  dst->last_view_frame = dst->frame_id; dst->last_view_batch = 1;      // (the view list now holds the candidates; the last CAMERA view stays what it was)
  { const int rc = nvbx_mapper_wait_for(src, dst); if (rc) return rc; }      // later work on src runs behind the call's reads
  return NVBX_OK;
}
