// nvblox/interpolation/interpolation_3d.h -- [U] Interpolator::interpolateOnGPU(points_L, layer, &distances, &success_flags), the
// batched TSDF / ESDF point query planners and collision checkers use (upstream's nvblox/interpolation/interpolation_3d.h, not readable
// in the reference tree).  One call of libnvblox_hip.so (nvbx_query_points) through the layer's c_handle(); semantics: SEMANTICS.md
// "Point queries" (trilinear over the 8 corner voxels, 2-D ESDF mappers bilinear in the slice plane).
//   - the std::vector overloads are synchronous, as upstream's are;
//   - the device-pointer overloads also return gradients and are asynchronous on the mapper's stream.
// A TSDF corner counts with weight >= min_weight (default: the mapper's mesh_min_weight); invalid points get unknown_value.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <vector>
#include "nvblox/core/types.h"
#include "nvblox/map/layer.h"
#include "nvblox_hip.h"

namespace nvblox {

class Interpolator {
 public:
  Interpolator() = default;
  Interpolator(const Interpolator&) = delete;
  Interpolator& operator=(const Interpolator&) = delete;
  ~Interpolator() { release(); }

  // < 0: the mapper's mesh_min_weight
  void min_weight(float w) { min_weight_ = w; }
  float min_weight() const { return min_weight_; }
  void unknown_value(float v) { unknown_value_ = v; }
  float unknown_value() const { return unknown_value_; }

  void interpolateOnGPU(const std::vector<Vector3f>& points_L, const TsdfLayer& layer, std::vector<float>* distances_ptr,
                        std::vector<bool>* success_flags_ptr) {
    interpolateHost(points_L, layer.c_handle(), NVBX_LAYER_TSDF, distances_ptr, success_flags_ptr);
  }
  void interpolateOnGPU(const std::vector<Vector3f>& points_L, const EsdfLayer& layer, std::vector<float>* distances_ptr,
                        std::vector<bool>* success_flags_ptr) {
    interpolateHost(points_L, layer.c_handle(), NVBX_LAYER_ESDF, distances_ptr, success_flags_ptr);
  }
  // device memory: points_L_dev[n][3] in, distances_dev[n], gradients_dev[n][3] (may be nullptr), success_flags_dev[n] (may be nullptr)
  // out; enqueued on the mapper's stream, no host synchronisation
  void interpolateOnGPU(const float* points_L_dev, int64_t n, const TsdfLayer& layer, float* distances_dev, float* gradients_dev,
                        uint8_t* success_flags_dev) {
    nvbx_mapper* m = layer.c_handle();
    checkNvbx(nvbx_query_points(m, NVBX_LAYER_TSDF, points_L_dev, n, tsdfMinWeight(m), unknown_value_, distances_dev, gradients_dev,
                                success_flags_dev), "nvbx_query_points");
  }
  void interpolateOnGPU(const float* points_L_dev, int64_t n, const EsdfLayer& layer, float* distances_dev, float* gradients_dev,
                        uint8_t* success_flags_dev) {
    checkNvbx(nvbx_query_points(layer.c_handle(), NVBX_LAYER_ESDF, points_L_dev, n, 0.0f, unknown_value_, distances_dev, gradients_dev,
                                success_flags_dev), "nvbx_query_points");
  }

 private:
  float tsdfMinWeight(nvbx_mapper* m) const {
    if (min_weight_ >= 0.0f) return min_weight_;
    nvbx_mapper_params p;
    checkNvbx(nvbx_mapper_get_params(m, &p), "nvbx_mapper_get_params");
    return p.mesh_min_weight;
  }
  void interpolateHost(const std::vector<Vector3f>& points_L, nvbx_mapper* m, uint32_t layer, std::vector<float>* distances_ptr,
                       std::vector<bool>* success_flags_ptr) {
    const size_t n = points_L.size();
    if (distances_ptr) distances_ptr->assign(n, unknown_value_);
    if (success_flags_ptr) success_flags_ptr->assign(n, false);
    if (n == 0) return;
    reserve(n);
    (void)hipMemcpy(points_dev_, points_L.data(), n * sizeof(Vector3f), hipMemcpyHostToDevice);      // (Vector3f: 12 packed bytes)
    const float mw = layer == NVBX_LAYER_TSDF ? tsdfMinWeight(m) : 0.0f;
    checkNvbx(nvbx_query_points(m, layer, points_dev_, (int64_t)n, mw, unknown_value_, dist_dev_, nullptr, valid_dev_), "nvbx_query_points");
    checkNvbx(nvbx_synchronize(m), "nvbx_synchronize");
    std::vector<float> d(n);
    std::vector<uint8_t> v(n);
    (void)hipMemcpy(d.data(), dist_dev_, n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipMemcpy(v.data(), valid_dev_, n, hipMemcpyDeviceToHost);
    if (distances_ptr) *distances_ptr = d;
    if (success_flags_ptr) for (size_t i = 0; i < n; i++) (*success_flags_ptr)[i] = v[i] != 0;
  }
  void reserve(size_t n) {
    if (n <= cap_) return;
    release();
    (void)hipMalloc((void**)&points_dev_, n * 3 * sizeof(float));
    (void)hipMalloc((void**)&dist_dev_, n * sizeof(float));
    (void)hipMalloc((void**)&valid_dev_, n);
    cap_ = n;
  }
  void release() {
    if (points_dev_) (void)hipFree(points_dev_);
    if (dist_dev_) (void)hipFree(dist_dev_);
    if (valid_dev_) (void)hipFree(valid_dev_);
    points_dev_ = dist_dev_ = nullptr; valid_dev_ = nullptr; cap_ = 0;
  }
  float min_weight_ = -1.0f;
  float unknown_value_ = 1000.0f;
  float* points_dev_ = nullptr;
  float* dist_dev_ = nullptr;
  uint8_t* valid_dev_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace nvblox
