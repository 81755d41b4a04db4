// nvblox/rays/sphere_tracer.h -- [U] SphereTracer: depth / depth + colour images of the map from any camera pose, and casts of a caller's
// own rays (upstream's nvblox/rays/sphere_tracer.h: renderImageOnGPU, renderRgbdImageOnGPU, castOnGPU; not readable in the reference tree).
// One call of libnvblox_hip.so each (nvbx_render_view_with / nvbx_cast_rays_with) through the layer's c_handle(); semantics: SEMANTICS.md
// "Rendering and ray casts".
//   - the tracer keeps its OWN maximum_steps / maximum_ray_length_m / surface_distance_epsilon_vox (upstream's defaults 100 / 15 m / 0.1) and
//     hands them over with every call: the mapper's parameters are neither read for them nor changed;
//   - truncation_distance_m is a property of the layer here (the mapper integrates with it): the argument is checked against the mapper's and
//     a call with another value renders nothing and returns false;
//   - images are the facade's Image<T> (library-owned frames); they are resized (and re-created in `memory_type` if they are of another);
//     a device image is ready in stream order on the mapper's stream, for any other memory type the call waits for the stream;
//   - the device-pointer castOnGPU is asynchronous on the mapper's stream, like Interpolator's device-pointer overloads.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include "nvblox/core/types.h"
#include "nvblox/map/layer.h"
#include "nvblox/sensors/camera.h"
#include "nvblox/sensors/image.h"
#include "nvblox_hip.h"

namespace nvblox {

class SphereTracer {
 public:
  SphereTracer() = default;

  int maximum_steps() const { return maximum_steps_; }
  float maximum_ray_length_m() const { return maximum_ray_length_m_; }
  float surface_distance_epsilon_vox() const { return surface_distance_epsilon_vox_; }
  // (at least one step, a threshold of at least 0: values below would read as "the mapper's" in nvbx_render_options)
  void maximum_steps(int maximum_steps) { maximum_steps_ = maximum_steps < 1 ? 1 : maximum_steps; }
  void maximum_ray_length_m(float maximum_ray_length_m) { maximum_ray_length_m_ = maximum_ray_length_m; }
  void surface_distance_epsilon_vox(float surface_distance_epsilon_vox) {
    surface_distance_epsilon_vox_ = surface_distance_epsilon_vox >= 0.0f ? surface_distance_epsilon_vox : 0.0f;      // (a NaN becomes 0 too)
  }

  // depth image of size (rows / f) x (cols / f): pixel (r, c) = the ray through the centre of camera pixel (r f, c f); 0 = no surface
  bool renderImageOnGPU(const Camera& camera, const Transform& T_L_C, const TsdfLayer& tsdf_layer, const float truncation_distance_m,
                        DepthImage* depth_image_ptr, const MemoryType memory_type = MemoryType::kDevice, const int ray_subsampling_factor = 1) {
    return render(camera, T_L_C, tsdf_layer.c_handle(), truncation_distance_m, depth_image_ptr, nullptr, memory_type, ray_subsampling_factor);
  }
  // ... and the colour of the voxel each ray hits (grey 127 where it has none, black where the ray hit nothing)
  bool renderRgbdImageOnGPU(const Camera& camera, const Transform& T_L_C, const TsdfLayer& tsdf_layer, const ColorLayer& color_layer,
                            const float truncation_distance_m, DepthImage* depth_image_ptr, ColorImage* color_image_ptr,
                            const MemoryType memory_type = MemoryType::kDevice, const int ray_subsampling_factor = 1) {
    if (color_layer.c_handle() != tsdf_layer.c_handle()) {
      std::fprintf(stderr, "[nvblox_hip] SphereTracer::renderRgbdImageOnGPU: the two layers belong to different mappers\n");
      return false;
    }
    return render(camera, T_L_C, tsdf_layer.c_handle(), truncation_distance_m, depth_image_ptr, color_image_ptr, memory_type, ray_subsampling_factor);
  }
  // device memory: origins_L_dev[n][3], unit directions_L_dev[n][3] in; t_dev[n] (metres along the ray, 0 = no hit), hit_dev[n] (may be nullptr),
  // colors_dev[n][3] (may be nullptr), normals_dev[n][3] (may be nullptr) out; enqueued on the mapper's stream, no host synchronisation
  bool castOnGPU(const float* origins_L_dev, const float* directions_L_dev, int64_t n, const TsdfLayer& tsdf_layer, const float truncation_distance_m,
                 float* t_dev, uint8_t* hit_dev = nullptr, uint8_t* colors_dev = nullptr, float* normals_dev = nullptr) {
    nvbx_mapper* m = tsdf_layer.c_handle();
    if (!truncationMatches(m, truncation_distance_m)) return false;
    const nvbx_render_options opt = options();
    checkNvbx(nvbx_cast_rays_with(m, &opt, origins_L_dev, directions_L_dev, n, maximum_ray_length_m_, t_dev, hit_dev, colors_dev, normals_dev),
              "nvbx_cast_rays");
    return true;
  }

 private:
  nvbx_render_options options() const { return nvbx_render_options{maximum_steps_, surface_distance_epsilon_vox_}; }
  static bool truncationMatches(nvbx_mapper* m, float truncation_distance_m) {
    nvbx_mapper_params p;
    checkNvbx(nvbx_mapper_get_params(m, &p), "nvbx_mapper_get_params");
    const float own = p.truncation_distance_vox * p.voxel_size;
    if (std::fabs(truncation_distance_m - own) <= 1e-5f * own) return true;
    std::fprintf(stderr, "[nvblox_hip] SphereTracer: truncation_distance_m %g differs from the layer's %g (the mapper's truncation_distance_vox * voxel_size)\n",
                 (double)truncation_distance_m, (double)own);
    return false;
  }
  template <typename T>
  static void fit(Image<T>* img, int rows, int cols, MemoryType memory_type) {
    if (img->memory_type() != memory_type) *img = Image<T>(rows, cols, memory_type);
    else img->resize(rows, cols);
  }
  bool render(const Camera& camera, const Transform& T_L_C, nvbx_mapper* m, float truncation_distance_m, DepthImage* depth, ColorImage* color,
              MemoryType memory_type, int f) {
    if (!depth || f < 1) { std::fprintf(stderr, "[nvblox_hip] SphereTracer: no depth image / subsampling < 1\n"); return false; }
    if (!truncationMatches(m, truncation_distance_m)) return false;
    const int rows = camera.rows() / f, cols = camera.cols() / f;
    fit(depth, rows, cols, memory_type);
    if (color) fit(color, rows, cols, memory_type);
    float T[16]; T_L_C.toRowMajor(T);
    const nvbx_render_options opt = options();
    int32_t r = 0, c = 0;
    checkNvbx(nvbx_render_view_with(m, &opt, T, &camera.c_abi(), f, maximum_ray_length_m_, depth->dataPtr(),
                                    color ? reinterpret_cast<uint8_t*>(color->dataPtr()) : nullptr, nullptr, (int64_t)rows * cols, &r, &c),
              "nvbx_render_view");
    if (memory_type != MemoryType::kDevice) checkNvbx(nvbx_synchronize(m), "nvbx_synchronize");
    return true;
  }
  int maximum_steps_ = 100;
  float maximum_ray_length_m_ = 15.0f;
  float surface_distance_epsilon_vox_ = 0.1f;
};

}  // namespace nvblox
