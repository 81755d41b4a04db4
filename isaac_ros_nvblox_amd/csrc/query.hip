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
#include "nvbx_query_point.h"      // q_probe, q_lookup, q_point: one lane's query (shared with align.hip)

using namespace nvbx;

namespace {

template <int KIND>
__global__ __launch_bounds__(256) void k_query_points(DMap m, const float* __restrict__ pts, int64_t n, float vs, float min_weight, float unknown,
                                                      int32_t plane_vz, float* __restrict__ dist, float* __restrict__ grad, uint8_t* __restrict__ valid) {
  const uint2* pool = KIND == Q_TSDF ? reinterpret_cast<const uint2*>(m.tsdf) : m.esdf;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    float g[3], d;
    const bool all = q_point<KIND>(m, pool, p, vs, min_weight, unknown, plane_vz, &d, g);
    dist[i] = d;
    if (grad) { grad[3 * i] = g[0]; grad[3 * i + 1] = g[1]; grad[3 * i + 2] = g[2]; }
    if (valid) valid[i] = all ? 1 : 0;
  }
}

template <int KIND>
int launch_query(nvbx_mapper* m, const float* pts, int64_t n, float min_weight, float unknown, int32_t plane_vz, float* dist, float* grad, uint8_t* valid) {
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), block(256);
  NVBX_LAUNCH(m, k_query_points<KIND>, grid, block, m->d, pts, n, m->p.voxel_size, min_weight, unknown, plane_vz, dist, grad, valid);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

}  // namespace

extern "C" int nvbx_query_points(nvbx_mapper* m, uint32_t layer, const float* points_xyz_dev, int64_t n, float min_weight, float unknown_value,
                                 float* distance_dev, float* gradient_xyz_dev, uint8_t* valid_dev) {
  if (!m || (layer != NVBX_LAYER_TSDF && layer != NVBX_LAYER_ESDF) || n < 0 || (n > 0 && (!points_xyz_dev || !distance_dev))) {
    set_error("nvbx_query_points: invalid argument"); return NVBX_E_INVALID;
  }
  if (layer == NVBX_LAYER_TSDF && tsdf_reader_refused(m, "nvbx_query_points")) return NVBX_E_INVALID;
  if (n == 0) return NVBX_OK;
  if (layer == NVBX_LAYER_ESDF) {
    if (m->begin_call()) return NVBX_E_DEVICE;                 // a held-back updateEsdf (colour deferral, held-back EDT) is carried out first
    const EsdfArgs a = m->make_esdf_args();
    return m->p.esdf_mode == 1 ? launch_query<Q_ESDF3>(m, points_xyz_dev, n, min_weight, unknown_value, -1, distance_dev, gradient_xyz_dev, valid_dev)
                               : launch_query<Q_ESDF2>(m, points_xyz_dev, n, min_weight, unknown_value, a.kz_out, distance_dev, gradient_xyz_dev, valid_dev);
  }
  // The TSDF query reads TSDF voxels and the TSDF flags only.  What colour deferral holds back -- a colour frame (writes the colour layer),
  // an updateEsdf (ESDF layer, site masks, ESDF-dirty list), the distance transform of the last update and the union step of the multi-GPU
  // exchange -- writes none of them, and every TSDF writer enqueued before this call is already on the stream.  So the held-back work stays
  // held back (as for nvbx_detect_dynamics): the query sees what classic order would show at this point, and the next integrateDepth
  // still carries the held-back frame in its two-launch pipelined order.
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  return launch_query<Q_TSDF>(m, points_xyz_dev, n, min_weight, unknown_value, 0, distance_dev, gradient_xyz_dev, valid_dev);
}
