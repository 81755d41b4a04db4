// resample.hip -- one mapper's TSDF and colour brought into a mapper of a coarser (or the same) voxel size under a rigid transform
// (nvbx_resample_map; SEMANTICS.md "Resampling").  [U] nothing of the kind is readable in the reference tree.  The merge's
// rule (merge.hip) with two voxel sizes and n^3 sub-samples per destination voxel.
//
// Launches, all on dst's stream, src read-only throughout.  The candidate enumeration (k_transfer_count<ResampleBox>,
// k_transfer_index<ResampleBox>), the result record (k_transfer_result) and the host sequence around them are nvbx_map_transfer.h's, shared
// with merge.hip; this file has the candidate box (ResampleBox: nvbx_resample_math.h), the call's own refusals and
//   k_resample_fuse    one 512-thread workgroup per candidate block, lane = voxel z + 8y + 64x.  The taps of the block reach at most
//                      N x N x N source blocks (N = nvbx_resample_reach <= 8, from the host): the eight corner lanes give the lowest block
//                      index per axis (the sample position is monotone in every destination coordinate), N^3 lanes probe src's table once
//                      and leave slot and colour flag in LDS; every lane then runs its n^3 taps -- eight corners each through that table, a
//                      z pair inside one block is one 16-B load -- sums distance and weight over the valid ones, fuses when at least half
//                      are valid, blends the colour voxel nearest to its centre and writes its own voxel.  No lane probes the hash in
//                      the loop, no two lanes write one voxel, the result does not depend on scheduling.
#include "nvbx_map_transfer.h"
#include "nvbx_query_point.h"
#include "nvbx_resample_math.h"

struct ResampleArgs {
  float R_SD[9], t_SD[3];       // p_S = R_SD p_D + t_SD: the samples
  float vs_s, vs_d, min_weight, weight_scale, trunc, max_weight;
  float off0, off1, off2, off3; // tap offsets (nvbx_resample_tap_offset), in destination voxels
  int32_t taps, reach;          // n, N
  int32_t merge_color, mesh_list;
  uint32_t frame_id;
};
// the candidate box of source block si (nvbx_map_transfer.h)
struct ResampleBox {
  float R_DS[9], t_DS[3];       // p_D = R_DS p_S + t_DS
  float vs_s, vs_d;
  int32_t taps;
  __device__ bool operator()(const int32_t si[3], int32_t lo[3], int32_t hi[3]) const { return nvbx_resample_candidate_box(R_DS, t_DS, si, vs_s, vs_d, taps, lo, hi); }
};
static_assert(sizeof(nvbx_resample_options) == 16, "C-ABI layout");


__device__ inline float resample_tap_off(const ResampleArgs& a, int i) { return i == 0 ? a.off0 : i == 1 ? a.off1 : i == 2 ? a.off2 : a.off3; }

// One tap at p_S: k_merge_fuse's sample (merge.hip) through a table of N^3 block slots, s_slot[x + N y + N^2 z] (LDS) from block (B0, B1, B2)
// on.  A corner outside the table counts as missing (it cannot be: N bounds the reach -- the check keeps every LDS index inside the table).
// true: all eight corners exist with weight >= min_weight; *d_out, *w_out = the trilinear interpolants of distance and weight.
__device__ inline bool resample_tap(const uint2* spool, const uint32_t* s_slot, int32_t B0, int32_t B1, int32_t B2, int N, const float ps[3], float vs,
                                    float min_weight, float* d_out, float* w_out) {
  int32_t b[3] = {0, 0, 0}; float t[3] = {0.0f, 0.0f, 0.0f};
  const bool ok0 = nvbx_interp_axis(ps[0], vs, &b[0], &t[0]), ok1 = nvbx_interp_axis(ps[1], vs, &b[1], &t[1]), ok2 = nvbx_interp_axis(ps[2], vs, &b[2], &t[2]);
  const bool ok = ok0 && ok1 && ok2;
  const int lx = b[0] & 7, ly = b[1] & 7, lz = b[2] & 7;
  const uint32_t un = (uint32_t)N;
  // block offsets from the table's origin, unsigned: one comparison covers both ends
  const uint32_t ox0 = (uint32_t)(b[0] >> 3) - (uint32_t)B0, oy0 = (uint32_t)(b[1] >> 3) - (uint32_t)B1, oz0 = (uint32_t)(b[2] >> 3) - (uint32_t)B2;
  const uint32_t ox1 = (uint32_t)((b[0] + 1) >> 3) - (uint32_t)B0, oy1 = (uint32_t)((b[1] + 1) >> 3) - (uint32_t)B1, oz1 = (uint32_t)((b[2] + 1) >> 3) - (uint32_t)B2;
  bool all = ok && ox0 < un && oy0 < un && oz0 < un && ox1 < un && oy1 < un && oz1 < un;
  float cd[8], cw[8];
#pragma unroll
  for (int q = 0; q < 4; q++) {                                     // q = i + 2j: corners (i, j, 0) and (i, j, 1)
    const int i_ = q & 1, j_ = q >> 1;
    const uint32_t ox = i_ ? ox1 : ox0, oy = j_ ? oy1 : oy0;
    const int xx = (lx + i_) & 7, yy = (ly + j_) & 7;
    uint2 e0 = make_uint2(0, 0), e1 = make_uint2(0, 0);
    if (all) {
      const uint32_t q0 = ox + un * (oy + un * oz0), q1 = ox + un * (oy + un * oz1);
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
    all = all && cw[q] >= min_weight && cw[q + 4] >= min_weight;
  }
  float g[3];
  *d_out = nvbx_interp_trilinear(cd, t[0], t[1], t[2], vs, g);
  *w_out = nvbx_interp_trilinear(cw, t[0], t[1], t[2], vs, g);
  return all;
}

__global__ __launch_bounds__(512) void k_resample_fuse(DMap dst, DMap src, ResampleArgs a, const int4* view_list, int32_t list_cap, TransferScratch* sc) {
  __shared__ uint32_t s_slot[512];
  __shared__ unsigned char s_color[512];
  __shared__ int32_t s_min[3];
  __shared__ uint32_t s_cnt[2];
  int32_t n = dst.counters[C_VIEW_COUNT + (a.frame_id & 3)];
  if (n > list_cap) n = list_cap;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 64) __hip_atomic_store(&dst.host_mirror[0], dst.counters[C_FREE_TOP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (tid < 2) s_cnt[tid] = 0u;
  const int vx = tid >> 6, vy = (tid >> 3) & 7, vz = tid & 7;
  const int taps = a.taps, N = a.reach, N3 = N * N * N;
  const int taps3 = taps * taps * taps;
  const bool corner = (vx == 0 || vx == 7) && (vy == 0 || vy == 7) && (vz == 0 || vz == 7);
  const float off_lo = a.off0, off_hi = resample_tap_off(a, taps - 1);
  const uint2* spool = reinterpret_cast<const uint2*>(src.tsdf);
  uint32_t n_fused = 0u, n_color = 0u;
  for (int32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int4 rec = view_list[i];
    const uint32_t slot = (uint32_t)rec.x;
    if (!slot_ok(slot)) continue;                                   // (uniform)
    if (tid < 3) s_min[tid] = INT32_MAX;
    float2* vp = &dst.tsdf[(size_t)slot * 512 + tid];
    float2 cur = *vp;
    const float g0 = (float)(8 * rec.y + vx) + 0.5f, g1 = (float)(8 * rec.z + vy) + 0.5f, g2 = (float)(8 * rec.w + vz) + 0.5f;
    __syncthreads();                                                // s_min is reset, the last block's table has been read by everyone
    if (corner) {                                                   // the block's extreme taps: the lowest source block index per axis is at one of them
      float pc[3];
      apply_rt(a.R_SD, a.t_SD, (g0 + (vx ? off_hi : off_lo)) * a.vs_d, (g1 + (vy ? off_hi : off_lo)) * a.vs_d, (g2 + (vz ? off_hi : off_lo)) * a.vs_d, pc);
      int32_t b[3] = {0, 0, 0}; float t[3];
      const bool ok0 = nvbx_interp_axis(pc[0], a.vs_s, &b[0], &t[0]), ok1 = nvbx_interp_axis(pc[1], a.vs_s, &b[1], &t[1]), ok2 = nvbx_interp_axis(pc[2], a.vs_s, &b[2], &t[2]);
      if (ok0 && ok1 && ok2) { atomicMin(&s_min[0], b[0] >> 3); atomicMin(&s_min[1], b[1] >> 3); atomicMin(&s_min[2], b[2] >> 3); }
    }
    __syncthreads();
    const int32_t B0 = s_min[0], B1 = s_min[1], B2 = s_min[2];
    if (tid < N3) {                                                 // the source blocks the taps can reach, resolved once
      uint32_t s = SLOT_NONE, cf = 0u;
      const int32_t x = B0 + tid % N, y = B1 + (tid / N) % N, z = B2 + tid / (N * N);
      constexpr int32_t L = 1 << 20;                                 // (block indices the hash key can hold)
      if (B0 != INT32_MAX && x >= -L && x < L && y >= -L && y < L && z >= -L && z < L) {
        s = q_probe(src, x, y, z, F_TSDF);
        if (slot_ok(s)) cf = src.slot_flags[s] & F_COLOR;
      }
      s_slot[tid] = s; s_color[tid] = cf ? 1 : 0;
    }
    __syncthreads();
    // the taps, x outer, y, z inner: sums start at -0 so that one tap's sum is the tap's value, bit for bit
    float D = -0.0f, W = -0.0f;
    int valid = 0;
    for (int ix = 0; ix < taps; ix++) {
      const float pd0 = (g0 + resample_tap_off(a, ix)) * a.vs_d;
      for (int iy = 0; iy < taps; iy++) {
        const float pd1 = (g1 + resample_tap_off(a, iy)) * a.vs_d;
        for (int iz = 0; iz < taps; iz++) {
          const float pd2 = (g2 + resample_tap_off(a, iz)) * a.vs_d;
          float ps[3], d, w;
          apply_rt(a.R_SD, a.t_SD, pd0, pd1, pd2, ps);
          if (resample_tap(spool, s_slot, B0, B1, B2, N, ps, a.vs_s, a.min_weight, &d, &w)) { D = D + d; W = W + w; valid++; }
        }
      }
    }
    bool fused = false, colored = false;
    if (2 * valid >= taps3) {
      const float ds = NVBX_DIV(D, (float)valid);
      const float ws = NVBX_DIV(W, (float)taps3) * a.weight_scale;
      const float w = cur.y + ws;
      if (w > 0.0f) {
        float d = NVBX_DIV(ds * ws + cur.x * cur.y, w);
        d = __builtin_amdgcn_fmed3f(d, -a.trunc, a.trunc);
        cur = make_float2(d, fminf(w, a.max_weight));
        *vp = cur;
        fused = true;
      }
    }
    if (a.merge_color && fused) {                                   // the source colour voxel nearest to the voxel's centre: floor(p / vs_s) per axis
      float ps[3];
      apply_rt(a.R_SD, a.t_SD, g0 * a.vs_d, g1 * a.vs_d, g2 * a.vs_d, ps);
      const int32_t n0 = (int32_t)floorf(ps[0] / a.vs_s), n1 = (int32_t)floorf(ps[1] / a.vs_s), n2 = (int32_t)floorf(ps[2] / a.vs_s);
      const uint32_t o0 = (uint32_t)(n0 >> 3) - (uint32_t)B0, o1 = (uint32_t)(n1 >> 3) - (uint32_t)B1, o2 = (uint32_t)(n2 >> 3) - (uint32_t)B2;
      const uint32_t un = (uint32_t)N;
      if (o0 < un && o1 < un && o2 < un) {
        const uint32_t oi = o0 + un * (o1 + un * o2);
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

static const char* const RESAMPLE_WHO = "nvbx_resample_map";
static const float RESAMPLE_IDENTITY[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

extern "C" void nvbx_default_resample_options(nvbx_resample_options* o) {
  if (!o) return;
  o->min_weight = 1e-4f; o->weight_scale = 1.0f; o->merge_color = 1; o->taps = 0;
}

extern "C" int nvbx_resample_map(nvbx_mapper* dst, nvbx_mapper* src, const float T_D_S[16], const nvbx_resample_options* options, nvbx_merge_result* result_dev) {
  if (const int rc = transfer_pointers_refused(RESAMPLE_WHO, dst, src, !result_dev ? ": result_dev is required" : nullptr, result_dev)) return rc;
  nvbx_resample_options o;
  if (options) o = *options; else nvbx_default_resample_options(&o);
  if (!T_D_S) T_D_S = RESAMPLE_IDENTITY;
  double r = 0.0;
  if (!nvbx_resample_ratio(dst->p.voxel_size, src->p.voxel_size, &r)) return refuse(RESAMPLE_WHO, ": dst's voxel size must be 1 to 4 times src's (upsampling and ratios above 4 are not supported)");
  const int taps = nvbx_resample_taps(r, o.taps);
  if (!taps) return refuse(RESAMPLE_WHO, ": taps must be 0 (by the ratio) or 1 .. 4");
  if (const int rc = transfer_values_refused(RESAMPLE_WHO, dst, src, T_D_S, src->p.voxel_size * 8.0f, o.min_weight, o.weight_scale)) return rc;
  ResampleArgs a{};
  ResampleBox box{};
  nvbx_merge_transforms(T_D_S, box.R_DS, box.t_DS, a.R_SD, a.t_SD);
  box.vs_s = a.vs_s = src->p.voxel_size; box.vs_d = a.vs_d = dst->p.voxel_size; a.min_weight = o.min_weight; a.weight_scale = o.weight_scale;
  a.trunc = dst->p.truncation_distance_vox * dst->p.voxel_size; a.max_weight = dst->p.max_weight;
  a.merge_color = o.merge_color ? 1 : 0;
  box.taps = a.taps = taps; a.reach = nvbx_resample_reach(r, taps);
  a.off0 = nvbx_resample_tap_offset(0, taps); a.off1 = nvbx_resample_tap_offset(taps > 1 ? 1 : 0, taps);
  a.off2 = nvbx_resample_tap_offset(taps > 2 ? 2 : 0, taps); a.off3 = nvbx_resample_tap_offset(taps > 3 ? 3 : 0, taps);
  if (a.reach < 1 || a.reach > 8) return refuse(RESAMPLE_WHO, ": the reach of a destination block exceeds 8 source blocks per axis");      // (cannot be: r <= 4)
  return transfer_call(RESAMPLE_WHO, "resampled", dst, src, box, dst->resample_knobs.grid, result_dev, [&](unsigned grid, uint32_t frame_id, int32_t mesh_list, TransferScratch* sc) {      // (NVBX_RESAMPLE_GRID)
    a.frame_id = frame_id; a.mesh_list = mesh_list;
    NVBX_LAUNCH(dst, k_resample_fuse, dim3(grid), dim3(512), dst->d, src->d, a, (const int4*)dst->view_list, (int32_t)dst->capacity, sc);
  });
}
