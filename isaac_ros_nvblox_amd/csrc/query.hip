// query.hip -- interpolated TSDF / ESDF point queries with gradients (nvbx_query_points; SEMANTICS.md "Point queries").
// [U] Upstream serves the same request with Interpolator::interpolateOnGPU (nvblox/interpolation/interpolation_3d.h) and the batched
// TSDF / ESDF queries of its Python binding; neither is readable in the reference tree.
//
// One lane = one query point; grid-stride, no atomics, every output written once.  Per lane: the corner voxels b .. b + 1 lie in
// 1, 2, 4 or 8 blocks (an axis with b & 7 == 7 crosses a block face).  The arithmetic (corner coordinates, the interpolant, its
// gradient, the ESDF corner value) is the inline code of include/nvblox_hip_device.h, shared with the caller-side helpers
// nvbx_dev_interpolate_*: the two agree bit for bit by construction.
#include <algorithm>
#include <cstdlib>
#include "nvbx_mapper.h"
#include "../../include/nvblox_hip_device.h"

using namespace nvbx;

namespace {

enum { Q_TSDF = 0, Q_ESDF3 = 1, Q_ESDF2 = 2 };

// slot of block (x, y, z) if it carries `flag`, else SLOT_NONE -- one 16-B entry load per probe (the table is not written while a
// query runs: every writer is stream-ordered before it)
__device__ inline uint32_t q_probe(const DMap& m, int32_t x, int32_t y, int32_t z, uint32_t flag) {
  const u64 key = pack_key(x, y, z);
  uint32_t h = table_pos(m, x, y, z);
  for (uint32_t probe = 0; probe <= m.mask; ++probe) {
    const uint4 e = ld_entry(m, h);
    const u64 k = ((u64)e.y << 32) | (u64)e.x;
    if (k == key) return (slot_ok(e.z) && (m.slot_flags[e.z] & flag)) ? e.z : SLOT_NONE;
    if (k == KEY_EMPTY) return SLOT_NONE;
    h = (h + 1) & m.mask;
  }
  return SLOT_NONE;
}

// Wave-level de-duplication of the probes (NVBX_QUERY_DEDUP=1; not the default: DESIGN.md 2.11): the lanes that still need a block take the key of the first of them
// (readlane: the key is wave-uniform, so the probe chain runs on the scalar unit), one chain serves every lane with that key.
// At most DEDUP_ROUNDS distinct keys per wave and corner offset; the lanes left over probe on their own.
constexpr int DEDUP_ROUNDS = 4;
template <bool DEDUP>
__device__ inline uint32_t q_lookup(const DMap& m, bool need, int32_t x, int32_t y, int32_t z, uint32_t flag) {
  uint32_t s = SLOT_NONE;
  if (DEDUP) {
    bool pend = need;
    for (int r = 0; r < DEDUP_ROUNDS; r++) {
      const unsigned long long bal = __ballot(pend);
      if (!bal) break;
      const int leader = __ffsll((long long)bal) - 1;
      const int32_t lx = __builtin_amdgcn_readlane(x, leader), ly = __builtin_amdgcn_readlane(y, leader), lz = __builtin_amdgcn_readlane(z, leader);
      const uint32_t ls = q_probe(m, lx, ly, lz, flag);
      if (pend && x == lx && y == ly && z == lz) { s = ls; pend = false; }
    }
    if (pend) s = q_probe(m, x, y, z, flag);
  } else if (need) {
    s = q_probe(m, x, y, z, flag);
  }
  return s;
}

// corner (i, j, k) of the lane: block offset o = (i & cx) | (j & cy) << 1 | (k & cz) << 2 from the base block
template <int KIND, bool DEDUP>
__global__ __launch_bounds__(256) void k_query_points(DMap m, const float* __restrict__ pts, int64_t n, float vs, float min_weight, float unknown,
                                                      int32_t plane_vz, float* __restrict__ dist, float* __restrict__ grad, uint8_t* __restrict__ valid) {
  constexpr uint32_t FLAG = KIND == Q_TSDF ? F_TSDF : F_ESDF;
  constexpr int NC = KIND == Q_ESDF2 ? 4 : 8;
  const uint2* pool = KIND == Q_TSDF ? reinterpret_cast<const uint2*>(m.tsdf) : m.esdf;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    int32_t b[3] = {0, 0, plane_vz}; float t[3] = {0.0f, 0.0f, 0.0f};
    bool ok = nvbx_interp_axis(p[0], vs, &b[0], &t[0]) && nvbx_interp_axis(p[1], vs, &b[1], &t[1]);
    if (KIND != Q_ESDF2) ok = ok && nvbx_interp_axis(p[2], vs, &b[2], &t[2]);
    const int32_t bx = b[0] >> 3, by = b[1] >> 3, bz = b[2] >> 3;
    const int vx = b[0] & 7, vy = b[1] & 7, vz = b[2] & 7;
    const int cx = vx == 7, cy = vy == 7, cz = KIND != Q_ESDF2 && vz == 7;
    const int cross = cx | (cy << 1) | (cz << 2);
    // slots of the blocks the corners lie in (o: constant index -> registers)
    uint32_t sl[8];
#pragma unroll
    for (int o = 0; o < 8; o++) {
      sl[o] = SLOT_NONE;
      if (KIND == Q_ESDF2 && (o & 4)) continue;
      const bool need = ok && (o & ~cross) == 0;
      sl[o] = q_lookup<DEDUP>(m, need, bx + (o & 1), by + ((o >> 1) & 1), bz + (o >> 2), FLAG);
    }
    // corner values; the pair along the layout's fastest axis (TSDF z, ESDF x) is one 16-B load when it stays inside a block
    float c[8];
    bool all = ok;
#pragma unroll
    for (int q = 0; q < NC / 2; q++) {
      uint2 e0, e1; uint32_t s0, s1;
      if (KIND == Q_TSDF) {          // q = i + 2j: corners (i, j, 0) and (i, j, 1)
        const int i_ = q & 1, j_ = q >> 1;
        const int o = (i_ & cx) | ((j_ & cy) << 1);
        s0 = o == 0 ? sl[0] : o == 1 ? sl[1] : o == 2 ? sl[2] : sl[3];
        s1 = cz ? (o == 0 ? sl[4] : o == 1 ? sl[5] : o == 2 ? sl[6] : sl[7]) : s0;
        const int xx = (vx + i_) & 7, yy = (vy + j_) & 7;
        const size_t v0 = (size_t)s0 * 512 + vz + 8 * yy + 64 * xx;
        if (!cz) {
          if (slot_ok(s0)) { const uint4 w = ld_pair(pool + v0); e0 = make_uint2(w.x, w.y); e1 = make_uint2(w.z, w.w); } else { e0 = e1 = make_uint2(0, 0); }
        } else {
          e0 = slot_ok(s0) ? pool[v0] : make_uint2(0, 0);
          e1 = slot_ok(s1) ? pool[(size_t)s1 * 512 + 8 * yy + 64 * xx] : make_uint2(0, 0);
        }
        const float2 f0 = make_float2(__uint_as_float(e0.x), __uint_as_float(e0.y)), f1 = make_float2(__uint_as_float(e1.x), __uint_as_float(e1.y));
        all = all && slot_ok(s0) && slot_ok(s1) && f0.y >= min_weight && f1.y >= min_weight;
        c[i_ + 2 * j_] = f0.x; c[i_ + 2 * j_ + 4] = f1.x;
      } else {                       // q = j + 2k: corners (0, j, k) and (1, j, k)
        const int j_ = q & 1, k_ = q >> 1;
        const int o = ((j_ & cy) << 1) | ((k_ & cz) << 2);
        s0 = o == 0 ? sl[0] : o == 2 ? sl[2] : o == 4 ? sl[4] : sl[6];
        s1 = cx ? (o == 0 ? sl[1] : o == 2 ? sl[3] : o == 4 ? sl[5] : sl[7]) : s0;
        const int yy = (vy + j_) & 7, zz = (vz + k_) & 7;
        const size_t v0 = (size_t)s0 * 512 + vx + 8 * yy + 64 * zz;
        if (!cx) {
          if (slot_ok(s0)) { const uint4 w = ld_pair(pool + v0); e0 = make_uint2(w.x, w.y); e1 = make_uint2(w.z, w.w); } else { e0 = e1 = make_uint2(0, 0); }
        } else {
          e0 = slot_ok(s0) ? pool[v0] : make_uint2(0, 0);
          e1 = slot_ok(s1) ? pool[(size_t)s1 * 512 + 8 * yy + 64 * zz] : make_uint2(0, 0);
        }
        float d0 = 0.0f, d1 = 0.0f;
        const bool o0 = nvbx_interp_esdf_value(e0, vs, &d0), o1 = nvbx_interp_esdf_value(e1, vs, &d1);
        all = all && slot_ok(s0) && slot_ok(s1) && o0 && o1;
        c[2 * j_ + 4 * k_] = d0; c[2 * j_ + 4 * k_ + 1] = d1;
      }
    }
    float g[3] = {0.0f, 0.0f, 0.0f}, d = unknown;
    if (all) d = KIND == Q_ESDF2 ? nvbx_interp_bilinear(c, t[0], t[1], vs, g) : nvbx_interp_trilinear(c, t[0], t[1], t[2], vs, g);
    else g[0] = g[1] = g[2] = 0.0f;
    dist[i] = d;
    if (grad) { grad[3 * i] = g[0]; grad[3 * i + 1] = g[1]; grad[3 * i + 2] = g[2]; }
    if (valid) valid[i] = all ? 1 : 0;
  }
}

template <int KIND>
int launch_query(nvbx_mapper* m, const float* pts, int64_t n, float min_weight, float unknown, int32_t plane_vz, float* dist, float* grad, uint8_t* valid) {
  // (A/B, tools/query_bench.py: 1 = the wave-level de-duplication; measured slower on coherent and uniform batches alike)
  static const int dedup = getenv("NVBX_QUERY_DEDUP") ? atoi(getenv("NVBX_QUERY_DEDUP")) : 0;
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), block(256);
  if (dedup) NVBX_LAUNCH(m, (k_query_points<KIND, true>), grid, block, m->d, pts, n, m->p.voxel_size, min_weight, unknown, plane_vz, dist, grad, valid);
  else NVBX_LAUNCH(m, (k_query_points<KIND, false>), grid, block, m->d, pts, n, m->p.voxel_size, min_weight, unknown, plane_vz, dist, grad, valid);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

}  // namespace

extern "C" int nvbx_query_points(nvbx_mapper* m, uint32_t layer, const float* points_xyz_dev, int64_t n, float min_weight, float unknown_value,
                                 float* distance_dev, float* gradient_xyz_dev, uint8_t* valid_dev) {
  if (!m || (layer != NVBX_LAYER_TSDF && layer != NVBX_LAYER_ESDF) || n < 0 || (n > 0 && (!points_xyz_dev || !distance_dev))) {
    set_error("nvbx_query_points: invalid argument"); return NVBX_E_INVALID;
  }
  if (layer == NVBX_LAYER_TSDF && m->p.projective_layer_type == 1) { set_error("nvbx_query_points: an occupancy mapper has no TSDF layer"); return NVBX_E_INVALID; }
  if (n == 0) return NVBX_OK;
  if (layer == NVBX_LAYER_ESDF) {
    if (m->join_side()) return NVBX_E_DEVICE;                 // a held-back updateEsdf (colour deferral, held-back EDT) is carried out first
    const EsdfArgs a = m->make_esdf_args();
    return m->p.esdf_mode == 1 ? launch_query<Q_ESDF3>(m, points_xyz_dev, n, min_weight, unknown_value, -1, distance_dev, gradient_xyz_dev, valid_dev)
                               : launch_query<Q_ESDF2>(m, points_xyz_dev, n, min_weight, unknown_value, a.kz_out, distance_dev, gradient_xyz_dev, valid_dev);
  }
  // The TSDF query reads TSDF voxels and the TSDF flags only.  What colour deferral holds back -- a colour frame (writes the colour layer),
  // an updateEsdf (ESDF layer, site masks, ESDF-dirty list), the distance transform of the last update and the union step of the multi-GPU
  // exchange -- writes none of them, and every TSDF writer enqueued before this call is already on the stream.  So the held-back work stays
  // held back (as for nvbx_detect_dynamics): the query sees what classic order would show at this point, and the next integrateDepth
  // still carries the held-back frame in its two-launch pipelined order.
  if (m->join_side_keeping_held()) return NVBX_E_DEVICE;
  return launch_query<Q_TSDF>(m, points_xyz_dev, n, min_weight, unknown_value, 0, distance_dev, gradient_xyz_dev, valid_dev);
}
