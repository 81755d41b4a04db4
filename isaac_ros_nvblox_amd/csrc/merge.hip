// merge.hip -- one mapper's TSDF and colour brought into another under a rigid transform (nvbx_merge_map; SEMANTICS.md "Map merging",
// DESIGN.md 2.17).  [U] submap fusion after loop closure / multi-session / multi-robot mapping: nothing of the kind is readable in the reference tree.
//
// Launches, all on dst's stream, src read-only throughout.  The candidate enumeration (k_transfer_count<MergeBox>, k_transfer_index<MergeBox>), the
// result record (k_transfer_result) and the host sequence around them are nvbx_map_transfer.h's, shared with resample.hip; this file has the
// candidate box (MergeBox: nvbx_merge_math.h), the call's own refusals and
//   k_merge_fuse    one 512-thread workgroup per candidate block, lane = voxel z + 8y + 64x.  The lanes' sample positions reach at most
//                   3 x 3 x 3 source blocks: the workgroup finds the lowest block index per axis, 27 lanes probe src's table once and leave the
//                   slots (and whether they carry colour) in LDS; every lane then takes its eight corners -- a z pair is one 16-B load inside a
//                   block, as in q_point -- through that table, interpolates distance and weight, fuses, blends the nearest colour voxel and
//                   writes its own voxel: no two lanes write one voxel, the result does not depend on scheduling.  Band bits per wavefront
//                   (publish_band), dirty flags and lists per block as in k_apply_fuse.
#include "nvbx_map_transfer.h"
#include "nvbx_query_point.h"
#include "nvbx_merge_math.h"

struct MergeArgs {
  float R_SD[9], t_SD[3];       // p_S = R_SD p_D + t_SD: the samples
  float vs, min_weight, weight_scale, trunc, max_weight;
  int32_t merge_color, mesh_list;
  uint32_t frame_id;
};
// the candidate box of source block si (nvbx_map_transfer.h)
struct MergeBox {
  float R_DS[9], t_DS[3];       // p_D = R_DS p_S + t_DS
  float vs;
  __device__ bool operator()(const int32_t si[3], int32_t lo[3], int32_t hi[3]) const { return nvbx_merge_candidate_box(R_DS, t_DS, si, vs, lo, hi); }
};
static_assert(sizeof(nvbx_merge_options) == 16, "C-ABI layout");

__global__ __launch_bounds__(512) void k_merge_fuse(DMap dst, DMap src, MergeArgs a, const int4* view_list, int32_t list_cap, TransferScratch* sc) {
  __shared__ uint32_t s_slot[27], s_color[27];
  __shared__ int32_t s_min[3];
  __shared__ uint32_t s_cnt[2];
  int32_t n = dst.counters[C_VIEW_COUNT + (a.frame_id & 3)];
  if (n > list_cap) n = list_cap;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 64) __hip_atomic_store(&dst.host_mirror[0], dst.counters[C_FREE_TOP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (tid < 2) s_cnt[tid] = 0u;
  const int vx = tid >> 6, vy = (tid >> 3) & 7, vz = tid & 7;
  const uint2* spool = reinterpret_cast<const uint2*>(src.tsdf);
  uint32_t n_fused = 0u, n_color = 0u;
  for (int32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int4 rec = view_list[i];
    const uint32_t slot = (uint32_t)rec.x;
    if (!slot_ok(slot)) continue;                                   // (uniform)
    if (tid < 3) s_min[tid] = INT32_MAX;
    float2* vp = &dst.tsdf[(size_t)slot * 512 + tid];
    float2 cur = *vp;
    // the sample position and its base voxel
    const float pd0 = ((float)(8 * rec.y + vx) + 0.5f) * a.vs, pd1 = ((float)(8 * rec.z + vy) + 0.5f) * a.vs, pd2 = ((float)(8 * rec.w + vz) + 0.5f) * a.vs;
    float ps[3];
    apply_rt(a.R_SD, a.t_SD, pd0, pd1, pd2, ps);
    int32_t b[3] = {0, 0, 0}; float t[3] = {0.0f, 0.0f, 0.0f};
    const bool ok0 = nvbx_interp_axis(ps[0], a.vs, &b[0], &t[0]), ok1 = nvbx_interp_axis(ps[1], a.vs, &b[1], &t[1]), ok2 = nvbx_interp_axis(ps[2], a.vs, &b[2], &t[2]);
    const bool ok = ok0 && ok1 && ok2;
    __syncthreads();                                                // s_min is reset, the last block's table has been read by everyone
    {
      int32_t m0 = ok ? (b[0] >> 3) : INT32_MAX, m1 = ok ? (b[1] >> 3) : INT32_MAX, m2 = ok ? (b[2] >> 3) : INT32_MAX;
#pragma unroll
      for (int o = 32; o; o >>= 1) { m0 = min(m0, __shfl_xor(m0, o)); m1 = min(m1, __shfl_xor(m1, o)); m2 = min(m2, __shfl_xor(m2, o)); }
      if ((tid & 63) == 0) { atomicMin(&s_min[0], m0); atomicMin(&s_min[1], m1); atomicMin(&s_min[2], m2); }
    }
    __syncthreads();
    const int32_t B0 = s_min[0], B1 = s_min[1], B2 = s_min[2];
    if (tid < 27) {                                                 // the source blocks the samples can reach, resolved once
      uint32_t s = SLOT_NONE, cf = 0u;
      const int32_t x = B0 + tid % 3, y = B1 + (tid / 3) % 3, z = B2 + tid / 9;
      constexpr int32_t L = 1 << 20;                                 // (block indices the hash key can hold)
      if (B0 != INT32_MAX && x >= -L && x < L && y >= -L && y < L && z >= -L && z < L) {
        s = q_probe(src, x, y, z, F_TSDF);
        if (slot_ok(s)) cf = src.slot_flags[s] & F_COLOR;
      }
      s_slot[tid] = s; s_color[tid] = cf;
    }
    __syncthreads();
    // corners: block offsets 0 .. 2 from (B0, B1, B2) per axis (ok lanes: never more, the block's centres span 7 voxels)
    const int lx = b[0] & 7, ly = b[1] & 7, lz = b[2] & 7;
    const int ox0 = ok ? (b[0] >> 3) - B0 : 0, oy0 = ok ? (b[1] >> 3) - B1 : 0, oz0 = ok ? (b[2] >> 3) - B2 : 0;
    const int ox1 = ok ? ((b[0] + 1) >> 3) - B0 : 0, oy1 = ok ? ((b[1] + 1) >> 3) - B1 : 0, oz1 = ok ? ((b[2] + 1) >> 3) - B2 : 0;
    bool all = ok && ox1 <= 2 && oy1 <= 2 && oz1 <= 2;
    float cd[8], cw[8];
#pragma unroll
    for (int q = 0; q < 4; q++) {                                   // q = i + 2j: corners (i, j, 0) and (i, j, 1)
      const int i_ = q & 1, j_ = q >> 1;
      const int ox = i_ ? ox1 : ox0, oy = j_ ? oy1 : oy0;
      const int xx = (lx + i_) & 7, yy = (ly + j_) & 7;
      uint2 e0 = make_uint2(0, 0), e1 = make_uint2(0, 0);
      if (all) {
        const int q0 = ox + 3 * oy + 9 * oz0, q1 = ox + 3 * oy + 9 * oz1;
        const uint32_t s0 = s_slot[q0];
        if (lz != 7) {
          if (slot_ok(s0)) { const uint4 w = ld_pair(spool + (size_t)s0 * 512 + lz + 8 * yy + 64 * xx); e0 = make_uint2(w.x, w.y); e1 = make_uint2(w.z, w.w); }
          else all = false;
        } else {
          const uint32_t s1 = s_slot[q1];
          if (slot_ok(s0) && slot_ok(s1)) { e0 = spool[(size_t)s0 * 512 + 7 + 8 * yy + 64 * xx]; e1 = spool[(size_t)s1 * 512 + 8 * yy + 64 * xx]; }
          else all = false;
        }
      }
      cd[q] = __uint_as_float(e0.x); cw[q] = __uint_as_float(e0.y); cd[q + 4] = __uint_as_float(e1.x); cw[q + 4] = __uint_as_float(e1.y);
      all = all && cw[q] >= a.min_weight && cw[q + 4] >= a.min_weight;
    }
    bool fused = false, colored = false;
    if (all) {
      float g[3];
      const float ds = nvbx_interp_trilinear(cd, t[0], t[1], t[2], a.vs, g);
      const float ws = nvbx_interp_trilinear(cw, t[0], t[1], t[2], a.vs, g) * a.weight_scale;
      const float w = cur.y + ws;
      if (w > 0.0f) {
        float d = NVBX_DIV(ds * ws + cur.x * cur.y, w);
        d = __builtin_amdgcn_fmed3f(d, -a.trunc, a.trunc);
        cur = make_float2(d, fminf(w, a.max_weight));
        *vp = cur;
        fused = true;
      }
    }
    if (a.merge_color && fused) {                                   // the nearest source colour voxel: floor(p / vs) per axis, one of b, b + 1
      const int32_t n0 = (int32_t)floorf(ps[0] / a.vs), n1 = (int32_t)floorf(ps[1] / a.vs), n2 = (int32_t)floorf(ps[2] / a.vs);
      const int o0 = (n0 >> 3) - B0, o1 = (n1 >> 3) - B1, o2 = (n2 >> 3) - B2;
      if (o0 >= 0 && o0 <= 2 && o1 >= 0 && o1 <= 2 && o2 >= 0 && o2 <= 2) {
        const int oi = o0 + 3 * o1 + 9 * o2;
        const uint32_t cs = s_slot[oi];
        if (slot_ok(cs) && s_color[oi]) {
          const uint2 sv = src.color[(size_t)cs * 512 + (n2 & 7) + 8 * (n1 & 7) + 64 * (n0 & 7)];
          const float sw = __uint_as_float(sv.y);
          if (sw > 0.0f) {
            uint2* cp = &dst.color[(size_t)slot * 512 + tid];
            const uint2 dv = *cp;
            const float w0 = __uint_as_float(dv.y);
            const uint32_t r8 = blend_u8((float)(dv.x & 0xFF), w0, (float)(sv.x & 0xFF), sw);
            const uint32_t g8 = blend_u8((float)((dv.x >> 8) & 0xFF), w0, (float)((sv.x >> 8) & 0xFF), sw);
            const uint32_t b8 = blend_u8((float)((dv.x >> 16) & 0xFF), w0, (float)((sv.x >> 16) & 0xFF), sw);
            *cp = make_uint2(r8 | (g8 << 8) | (b8 << 16), __float_as_uint(fminf(w0 + sw, a.max_weight)));
            colored = true;
          }
        }
      }
    }
    n_fused += fused ? 1u : 0u; n_color += colored ? 1u : 0u;
    uint32_t old = 0u;
    if (tid == 0) old = atomicOr(&dst.slot_flags[slot], F_TSDF | F_DIRTY_ESDF | F_DIRTY_MESH);
    publish_band(dst.slot_flags, slot, tid, in_band(cur.x, cur.y, a.trunc));      // (every wavefront is here)
    const int any_color = __syncthreads_or(colored ? 1 : 0);
    if (tid == 0) {
      if (any_color) atomicOr(&dst.slot_flags[slot], F_COLOR);
      if (!(old & F_DIRTY_ESDF)) list_append(dst, S_LIST_ESDF_DIRTY, (int32_t)slot);
      if (!(old & F_DIRTY_MESH)) list_append(dst, a.mesh_list, (int32_t)slot);
    }
  }
  // the workgroup's counts: wavefront sums, LDS, one atomic each
#pragma unroll
  for (int o = 32; o; o >>= 1) { n_fused += __shfl_xor(n_fused, o); n_color += __shfl_xor(n_color, o); }
  __syncthreads();
  if ((tid & 63) == 0) { atomicAdd(&s_cnt[0], n_fused); atomicAdd(&s_cnt[1], n_color); }
  __syncthreads();
  if (tid == 0) { if (s_cnt[0]) atomicAdd(&sc->voxels, (unsigned long long)s_cnt[0]); if (s_cnt[1]) atomicAdd(&sc->colors, (unsigned long long)s_cnt[1]); }
}

static const char* const MERGE_WHO = "nvbx_merge_map";

extern "C" void nvbx_default_merge_options(nvbx_merge_options* o) {
  if (!o) return;
  o->min_weight = 1e-4f; o->weight_scale = 1.0f; o->merge_color = 1; o->pad = 0;
}

extern "C" int nvbx_merge_map(nvbx_mapper* dst, nvbx_mapper* src, const float T_D_S[16], const nvbx_merge_options* options, nvbx_merge_result* result_dev) {
  if (const int rc = transfer_pointers_refused(MERGE_WHO, dst, src, (!T_D_S || !result_dev) ? ": the pose and result_dev are required" : nullptr, result_dev)) return rc;
  nvbx_merge_options o;
  if (options) o = *options; else nvbx_default_merge_options(&o);
  if (src->p.voxel_size != dst->p.voxel_size) return refuse(MERGE_WHO, ": the mappers' voxel sizes differ");
  if (const int rc = transfer_values_refused(MERGE_WHO, dst, src, T_D_S, dst->p.voxel_size * 8.0f, o.min_weight, o.weight_scale)) return rc;
  MergeArgs a{};
  MergeBox box{};
  nvbx_merge_transforms(T_D_S, box.R_DS, box.t_DS, a.R_SD, a.t_SD);
  box.vs = a.vs = dst->p.voxel_size; a.min_weight = o.min_weight; a.weight_scale = o.weight_scale;
  a.trunc = dst->p.truncation_distance_vox * dst->p.voxel_size; a.max_weight = dst->p.max_weight;
  a.merge_color = o.merge_color ? 1 : 0;
  return transfer_call(MERGE_WHO, "merged", dst, src, box, 2048, result_dev, [&](unsigned grid, uint32_t frame_id, int32_t mesh_list, TransferScratch* sc) {
    a.frame_id = frame_id; a.mesh_list = mesh_list;
    NVBX_LAUNCH(dst, k_merge_fuse, dim3(grid), dim3(512), dst->d, src->d, a, (const int4*)dst->view_list, (int32_t)dst->capacity, sc);
  });
}
