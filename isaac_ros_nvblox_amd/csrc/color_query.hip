// color_query.hip -- interpolated colour point queries with the luminance gradient (nvbx_query_colors; SEMANTICS.md "Colour alignment and colour
// queries").  [U] The colour sibling of nvbx_query_points: nothing of the kind is readable in the reference tree.
//
// One lane = one query point; grid-stride, no atomics, every output written once.  The lane's arithmetic is q_color (nvbx_query_point.h), the
// inline code k_align_accumulate's colour term runs, so the two agree bit for bit by construction.
#include <algorithm>
#include "nvbx_mapper.h"
#include "nvbx_query_point.h"

using namespace nvbx;

namespace {

template <bool RGB>
__global__ __launch_bounds__(256) void k_query_colors(DMap m, const float* __restrict__ pts, int64_t n, float vs, float min_color_weight,
                                                      float* __restrict__ rgb, float* __restrict__ lum, float* __restrict__ grad,
                                                      uint8_t* __restrict__ valid) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    float y, g[3], c[3];
    const bool all = q_color<RGB>(m, p, vs, min_color_weight, nullptr, &y, g, c);
    if (RGB) { rgb[3 * i] = c[0]; rgb[3 * i + 1] = c[1]; rgb[3 * i + 2] = c[2]; }
    if (lum) lum[i] = y;
    if (grad) { grad[3 * i] = g[0]; grad[3 * i + 1] = g[1]; grad[3 * i + 2] = g[2]; }
    valid[i] = all ? 1 : 0;
  }
}

}  // namespace

extern "C" int nvbx_query_colors(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, float min_color_weight, float* rgb_dev, float* luminance_dev,
                                 float* gradient_xyz_dev, uint8_t* valid_dev) {
  if (!m || n < 0 || (n > 0 && (!points_xyz_dev || !valid_dev))) {
    set_error("nvbx_query_colors: invalid argument"); return NVBX_E_INVALID;
  }
  if (tsdf_reader_refused(m, "nvbx_query_colors")) return NVBX_E_INVALID;
  if (min_color_weight != min_color_weight) return refuse("nvbx_query_colors", ": min_color_weight is not a number");
  if (n == 0) return NVBX_OK;
  NVBX_HIP(hipSetDevice(m->device));
  // reads the colour layer, which a held-back integrateColor writes: that work is carried out first (as nvbx_render_view does with a colour output)
  if (m->begin_call()) return NVBX_E_DEVICE;
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), block(256);
  if (rgb_dev) NVBX_LAUNCH(m, k_query_colors<true>, grid, block, m->d, points_xyz_dev, n, m->p.voxel_size, min_color_weight, rgb_dev, luminance_dev, gradient_xyz_dev, valid_dev);
  else NVBX_LAUNCH(m, k_query_colors<false>, grid, block, m->d, points_xyz_dev, n, m->p.voxel_size, min_color_weight, rgb_dev, luminance_dev, gradient_xyz_dev, valid_dev);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}
