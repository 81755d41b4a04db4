// feature_merge.hip -- one mapper's feature layer brought into another under a rigid transform (nvbx_merge_features; SEMANTICS.md "Feature
// merging").  A call of its own, meant to follow nvbx_merge_map with the same pose: it allocates nothing, a candidate block
// counts only where dst already has it with the TSDF layer -- so nothing waits on the host between enumerating and fusing.
//
// Launches, all on dst's stream, src read-only throughout.  The candidate of a slot (transfer_candidate), the refusal helpers and the
// transforms are the merge's (nvbx_map_transfer.h, nvbx_merge_math.h); the candidate box is nvbx_feature_merge_math.h's.
//   k_feature_merge_index   one thread per (source slot, candidate 0 .. 26): slots with F_FEATURE only; a read-only probe of dst's table (the
//                           block with its TSDF layer, or nothing), a CAS into the scratch key set, and the first arriver appends {slot, block
//                           index} to the work list in scratch.  dst's view list is not touched.
//   k_feature_merge_fuse    one 512-thread workgroup per work-list entry, lane = voxel z + 8y + 64x.  Every lane transforms its centre and takes
//                           the source voxel that contains it; the workgroup finds the lowest source block index per axis (the voxels of one
//                           block span at most 14 indices per axis: 3 x 3 x 3 blocks), 27 lanes probe src's table once and leave the slots that
//                           carry F_FEATURE in LDS; every lane reads its source weight, a workgroup-wide OR decides whether the block is
//                           touched at all; then a loop over the C / 8 chunks: one 16-B gather from src, one 16-B load of the lane's own
//                           voxel (none in a block flagged by this call), eight blends in f32, one 16-B store.  No lane probes a hash in the
//                           loop, no two lanes write one voxel, registers do not scale with C.
//   k_feature_merge_result  one thread: the caller's result record from the counters the launches left.
#include "nvbx_map_transfer.h"
#include "nvbx_query_point.h"       // q_probe
#include "nvbx_feature.h"           // half8, feature_voxel_of
#include "nvbx_feature_merge_math.h"

using namespace nvbx;

// head of the call's scratch (nvbx_mapper::merge_buf, zeroed per call); the key set follows at TRANSFER_KEYS_OFFSET, the work list behind it
struct FeatMergeScratch { int32_t src_blocks, n_work, flagged, pad; unsigned long long voxels; };
static_assert(sizeof(FeatMergeScratch) <= TRANSFER_KEYS_OFFSET, "scratch head");
static_assert(sizeof(nvbx_feature_merge_options) == 32, "C-ABI layout");
static_assert(sizeof(nvbx_feature_merge_result) == 64, "C-ABI layout");

struct FeatMergeArgs {
  float R_SD[9], t_SD[3];       // p_S = R_SD p_D + t_SD
  float vs, min_weight, weight_scale, max_weight;
  int32_t nch;                  // C / 8
  const half8* src_val; const float* src_w;
  half8* dst_val; float* dst_w;
};
// the candidate box of source block si (nvbx_map_transfer.h)
struct FeatMergeBox {
  float R_DS[9], t_DS[3];       // p_D = R_DS p_S + t_DS
  float vs;
  __device__ bool operator()(const int32_t si[3], int32_t lo[3], int32_t hi[3]) const { return nvbx_feature_merge_candidate_box(R_DS, t_DS, si, vs, lo, hi); }
};

__global__ __launch_bounds__(256) void k_feature_merge_index(DMap dst, DMap src, FeatMergeBox box, FeatMergeScratch* sc, u64* keys, uint32_t kmask, int4* work, int32_t work_cap) {
  const int64_t n = (int64_t)src.counters[C_HIGH_WATER] * 27;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t s = (int32_t)(i / 27); const int c = (int)(i - (int64_t)s * 27);
    if (!(src.slot_flags[s] & F_FEATURE)) continue;
    if (c == 0) atomicAdd(&sc->src_blocks, 1);
    int32_t x, y, z;
    if (!transfer_candidate(src, box, s, c, &x, &y, &z)) continue;
    const uint32_t slot = q_probe(dst, x, y, z, F_TSDF);             // read only: a block dst lacks is no candidate
    if (!slot_ok(slot)) continue;
    const u64 key = pack_key(x, y, z);
    uint32_t kh = (index_hash(x, y, z) * 2654435761u) & kmask;
    for (uint32_t probe = 0; probe <= kmask; ++probe) {
      const u64 old = atomicCAS(&keys[kh], KEY_EMPTY, key);
      if (old == KEY_EMPTY) {                                       // the first arriver
        const int32_t p = atomicAdd(&sc->n_work, 1);
        if (p < work_cap) work[p] = make_int4((int32_t)slot, x, y, z);
        break;
      }
      if (old == key) break;
      kh = (kh + 1) & kmask;
    }
  }
}

__global__ __launch_bounds__(512) void k_feature_merge_fuse(DMap dst, DMap src, FeatMergeArgs a, const int4* work, int32_t work_cap, FeatMergeScratch* sc) {
  __shared__ uint32_t s_slot[27];
  __shared__ int32_t s_min[3];
  __shared__ uint32_t s_cnt;
  int32_t n = sc->n_work;
  if (n > work_cap) n = work_cap;
  const int tid = threadIdx.x;
  if (tid == 0) s_cnt = 0u;
  const int vx = tid >> 6, vy = (tid >> 3) & 7, vz = tid & 7;
  const int nch = a.nch;
  uint32_t n_fused = 0u, n_flagged = 0u;
  for (int32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int4 rec = work[i];
    const uint32_t slot = (uint32_t)rec.x;
    const bool fresh = !(dst.slot_flags[slot] & F_FEATURE);        // uniform; read ahead of the barriers below, set behind them
    if (tid < 3) s_min[tid] = INT32_MAX;
    // the voxel centre in src and the source voxel that contains it
    const float pd0 = ((float)(8 * rec.y + vx) + 0.5f) * a.vs, pd1 = ((float)(8 * rec.z + vy) + 0.5f) * a.vs, pd2 = ((float)(8 * rec.w + vz) + 0.5f) * a.vs;
    float ps[3];
    apply_rt(a.R_SD, a.t_SD, pd0, pd1, pd2, ps);
    int32_t g[3] = {0, 0, 0};
    const bool ok = feature_voxel_of(ps[0], ps[1], ps[2], a.vs, g);
    __syncthreads();                                                // s_min is reset, the last block's table has been read by everyone
    {
      int32_t m0 = ok ? (g[0] >> 3) : INT32_MAX, m1 = ok ? (g[1] >> 3) : INT32_MAX, m2 = ok ? (g[2] >> 3) : INT32_MAX;
#pragma unroll
      for (int o = 32; o; o >>= 1) { m0 = min(m0, __shfl_xor(m0, o)); m1 = min(m1, __shfl_xor(m1, o)); m2 = min(m2, __shfl_xor(m2, o)); }
      if ((tid & 63) == 0) { atomicMin(&s_min[0], m0); atomicMin(&s_min[1], m1); atomicMin(&s_min[2], m2); }
    }
    __syncthreads();
    const int32_t B0 = s_min[0], B1 = s_min[1], B2 = s_min[2];
    if (tid < 27) {                                                 // the source blocks the voxels can lie in, resolved once
      uint32_t s = SLOT_NONE;
      const int32_t x = B0 + tid % 3, y = B1 + (tid / 3) % 3, z = B2 + tid / 9;
      if (B0 != INT32_MAX && nvbx_index_in_range(x, y, z)) s = q_probe(src, x, y, z, F_FEATURE);
      s_slot[tid] = s;
    }
    __syncthreads();
    // the lane's source voxel and its weight
    uint32_t ss = SLOT_NONE;
    if (ok) {
      const int o0 = (g[0] >> 3) - B0, o1 = (g[1] >> 3) - B1, o2 = (g[2] >> 3) - B2;
      if (o0 <= 2 && o1 <= 2 && o2 <= 2) ss = s_slot[o0 + 3 * o1 + 9 * o2];      // (>= 0: B is the minimum; never more than 2)
    }
    const int st = (g[2] & 7) + 8 * (g[1] & 7) + 64 * (g[0] & 7);
    const float ws = slot_ok(ss) ? a.src_w[(size_t)ss * 512 + st] : 0.0f;
    const bool pass = ws > 0.0f && ws >= a.min_weight;
    if (!__syncthreads_or(pass ? 1 : 0)) continue;                  // no voxel of the block contributes: nothing is written, the slot is not flagged
    if (fresh && tid == 0) { atomicOr(&dst.slot_flags[slot], F_FEATURE); n_flagged++; }
    n_fused += pass ? 1u : 0u;
    if (!pass && !fresh) continue;                                  // (its voxel stays as it is; no barrier below this line)
    float* wp = a.dst_w + (size_t)slot * 512 + tid;
    const float w0 = (fresh || !pass) ? 0.0f : *wp;
    const float w1 = ws * a.weight_scale;
    const float tw = w0 + w1;
    const float ca = NVBX_DIV(w0, tw), cb = NVBX_DIV(w1, tw);       // the feature integrator's blend, w1 in place of 1
    *wp = pass ? fminf(tw, a.max_weight) : 0.0f;
    const half8* sp = a.src_val + (size_t)(slot_ok(ss) ? ss : 0u) * nch * 512 + st;
    half8* vp = a.dst_val + (size_t)slot * nch * 512 + tid;
#pragma unroll 2
    for (int k = 0; k < nch; k++) {
      half8 o;
      if (pass) {
        const half8 f = sp[(size_t)k * 512];
        half8 old;
        if (fresh) { for (int q = 0; q < 8; q++) old[q] = (_Float16)0.0f; } else old = vp[(size_t)k * 512];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const float nv = (float)old[q] * ca + (float)f[q] * cb;
          o[q] = (_Float16)nv;                          // round to nearest even
        }
      } else {
#pragma unroll
        for (int q = 0; q < 8; q++) o[q] = (_Float16)0.0f;
      }
      vp[(size_t)k * 512] = o;
    }
  }
  // the workgroup's counts: wavefront sums, LDS, one atomic each
#pragma unroll
  for (int o = 32; o; o >>= 1) n_fused += __shfl_xor(n_fused, o);
  __syncthreads();
  if ((tid & 63) == 0 && n_fused) atomicAdd(&s_cnt, n_fused);
  __syncthreads();
  if (tid == 0) { if (s_cnt) atomicAdd(&sc->voxels, (unsigned long long)s_cnt); if (n_flagged) atomicAdd(&sc->flagged, (int32_t)n_flagged); }
}

__global__ void k_feature_merge_result(const FeatMergeScratch* sc, int32_t work_cap, nvbx_feature_merge_result* out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  nvbx_feature_merge_result r;
  r.source_blocks = sc->src_blocks;
  r.candidate_blocks = sc->n_work < work_cap ? sc->n_work : work_cap;
  r.blocks_flagged = sc->flagged;
  r.voxels_fused = (int64_t)sc->voxels;
  r.status = r.source_blocks == 0 ? NVBX_MERGE_EMPTY_SOURCE : (r.voxels_fused == 0 ? NVBX_MERGE_NO_OVERLAP : NVBX_MERGE_OK);
  for (int k = 0; k < 7; k++) r.pad[k] = 0;
  *out = r;
}

static const char* const FEATURE_MERGE_WHO = "nvbx_merge_features";

extern "C" void nvbx_default_feature_merge_options(nvbx_feature_merge_options* o) {
  if (!o) return;
  o->min_weight = 0.0f; o->weight_scale = 1.0f;
  for (int k = 0; k < 6; k++) o->reserved[k] = 0;
}

extern "C" int nvbx_merge_features(nvbx_mapper* dst, nvbx_mapper* src, const float T_D_S[16], const nvbx_feature_merge_options* options,
                                   nvbx_feature_merge_result* result_dev) {
  const char* who = FEATURE_MERGE_WHO;
  if (const int rc = transfer_pointers_refused(who, dst, src, (!T_D_S || !result_dev) ? ": the pose and result_dev are required" : nullptr, result_dev)) return rc;
  nvbx_feature_merge_options o;
  if (options) o = *options; else nvbx_default_feature_merge_options(&o);
  if (src->p.voxel_size != dst->p.voxel_size) return refuse(who, ": the mappers' voxel sizes differ");
  if (const int rc = transfer_values_refused(who, dst, src, T_D_S, dst->p.voxel_size * 8.0f, o.min_weight, o.weight_scale)) return rc;
  if (o.min_weight < 0.0f) return refuse(who, ": min_weight is negative");
  if (!dst->feat_channels || !src->feat_channels) return refuse(who, ": both mappers need the feature layer (nvbx_enable_features)");
  if (dst->feat_channels != src->feat_channels) return refuse(who, ": the mappers' feature channel counts differ");
  FeatMergeArgs a{};
  FeatMergeBox box{};
  nvbx_merge_transforms(T_D_S, box.R_DS, box.t_DS, a.R_SD, a.t_SD);
  box.vs = a.vs = dst->p.voxel_size; a.min_weight = o.min_weight; a.weight_scale = o.weight_scale; a.max_weight = dst->p.max_weight;
  a.nch = dst->feat_channels / 8;
  NVBX_HIP(hipSetDevice(dst->device));
  // src: held-back work is carried out; its block count sizes the scratch (waits for src's stream -- the call's only host wait)
  if (src->fetch_counters()) return NVBX_E_DEVICE;
  const int64_t src_hw = src->h_counters[C_HIGH_WATER];
  const int64_t src_live = std::max<int64_t>(1, (int64_t)src->capacity - (int64_t)src->h_counters[C_FREE_TOP]);
  if (dst->begin_call()) return NVBX_E_DEVICE;
  { const int rc = nvbx_mapper_wait_for(dst, src); if (rc) return rc; }
  // the key set: distinct candidates are at most 27 per source block, load <= 1/2; the work list: one record per distinct candidate
  uint64_t entries = 64; while (entries < (uint64_t)src_live * 54) entries <<= 1;
  if (entries > (1ull << 31)) return refuse(who, ": the source map is too large to enumerate");
  const int64_t work_cap = std::min<int64_t>(src_live * 27, (int64_t)dst->capacity);
  const size_t work_offset = TRANSFER_KEYS_OFFSET + (size_t)entries * 8;
  if (dst->merge_buf.ensure(dst->stream, work_offset + (size_t)work_cap * 16)) return NVBX_E_DEVICE;
  FeatMergeScratch* sc = dst->merge_buf.as<FeatMergeScratch>();
  u64* keys = reinterpret_cast<u64*>(dst->merge_buf.as<unsigned char>() + TRANSFER_KEYS_OFFSET);
  int4* work = reinterpret_cast<int4*>(dst->merge_buf.as<unsigned char>() + work_offset);
  a.src_val = static_cast<const half8*>(src->feat_val); a.src_w = src->feat_w;
  a.dst_val = static_cast<half8*>(dst->feat_val); a.dst_w = dst->feat_w;
  NVBX_HIP(hipMemsetAsync(sc, 0, TRANSFER_KEYS_OFFSET, dst->stream));
  if (src_hw > 0) {
    NVBX_HIP(hipMemsetAsync(keys, 0xFF, (size_t)entries * 8, dst->stream));
    const unsigned enum_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((src_hw * 27 + 255) / 256, 2048));
    NVBX_LAUNCH(dst, k_feature_merge_index, dim3(enum_grid), dim3(256), dst->d, src->d, box, sc, keys, (uint32_t)(entries - 1), work, (int32_t)work_cap);
    const unsigned fuse_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(work_cap, 2048));
    NVBX_LAUNCH(dst, k_feature_merge_fuse, dim3(fuse_grid), dim3(512), dst->d, src->d, a, (const int4*)work, (int32_t)work_cap, sc);
  }
  NVBX_LAUNCH(dst, k_feature_merge_result, dim3(1), dim3(64), (const FeatMergeScratch*)sc, (int32_t)work_cap, result_dev);
  NVBX_HIP(hipGetLastError());
  return nvbx_mapper_wait_for(src, dst);                            // later work on src runs behind the call's reads
}
