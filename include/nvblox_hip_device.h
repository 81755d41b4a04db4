/* nvblox_hip_device.h -- device-side read access to a libnvblox_hip map from the caller's OWN HIP kernels.
 *
 * Replaces, for this library, what nvblox_ros gets from nvblox/gpu_hash/internal/cuda/gpu_indexing.cuh and
 * GPULayerView<Block> (call sites: nvblox_ros/src/lib/conversions/esdf_slice_conversions.cu:18,
 * esdf_and_gradients_conversions.cu:19-23,88-125): a kernel that is not part of the library looks blocks up through
 * the hash and reads voxels in place -- no copy of the layer, no host round trip.
 *
 * Contract: fill an nvbx_device_view with nvbx_get_device_view() (include/nvblox_hip.h) and pass it BY VALUE to a kernel
 * launched on the mapper's stream (or ordered behind it with an event).  The view's pointers are valid until the next
 * call that can allocate blocks (the pools and the table grow on demand, nvbx_mapper_set_max_capacity in nvblox_hip.h) or
 * that decays the map (nvbx_decay_tsdf / nvbx_decay_occupancy build the table of the surviving blocks in a second buffer
 * and the two change places): fetch the view again after an integrate / upload / decay call, it costs nothing.  What a kernel reads through it is whatever the mapper calls enqueued before the kernel have
 * produced.  Read-only: writing through the view breaks the library's invariants.
 * Layouts: TSDF / colour voxel v = z + 8y + 64x in the block (the reference's order); ESDF voxel
 * v = x + 8y + 64z, packed {f32 squared_distance_vox, u32 meta}.
 * nvbx_dev_interpolate_tsdf / _esdf (bottom): the point query of nvbx_query_points as a device function, bit-identical to it. */
#ifndef NVBLOX_HIP_DEVICE_H_
#define NVBLOX_HIP_DEVICE_H_
#include <stdint.h>
#include "nvblox_hip.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#define NVBX_DEV_SLOT_NONE 0xFFFFFFFEu     /* values >= this are "no block" */

/* slot of block (x, y, z) if it carries `layer` (NVBX_LAYER_*), else NVBX_DEV_SLOT_NONE.  Probe start = the reference's
 * Index3DHash (nvblox_rviz_plugin/.../nvblox_hash_utils.h:43-48) scattered by a Fibonacci multiply; linear probing. */
__device__ inline uint32_t nvbx_dev_find_block(const nvbx_device_view& v, int32_t x, int32_t y, int32_t z, uint32_t layer) {
  const unsigned long long B = 1ull << 20;
  const unsigned long long key = (((unsigned long long)(long long)x + B) & 0x1FFFFFull) | ((((unsigned long long)(long long)y + B) & 0x1FFFFFull) << 21) |
                                 ((((unsigned long long)(long long)z + B) & 0x1FFFFFull) << 42);
  uint32_t h = (((uint32_t)x + (uint32_t)y * 17191u + (uint32_t)z * (17191u * 17191u)) * 2654435761u) >> v.table_shift;
  for (uint32_t probe = 0; probe <= v.table_mask; ++probe) {
    const uint4 e = reinterpret_cast<const uint4*>(v.table)[h];          /* {key lo, key hi, slot, view stamp} */
    const unsigned long long k = ((unsigned long long)e.y << 32) | (unsigned long long)e.x;
    if (k == key) return (e.z < NVBX_DEV_SLOT_NONE && (v.slot_flags[e.z] & layer)) ? e.z : NVBX_DEV_SLOT_NONE;
    if (k == ~0ull) return NVBX_DEV_SLOT_NONE;
    h = (h + 1) & v.table_mask;
  }
  return NVBX_DEV_SLOT_NONE;
}
__device__ inline bool nvbx_dev_slot_ok(uint32_t slot) { return slot < NVBX_DEV_SLOT_NONE; }

/* voxel (vx, vy, vz) in 0..7 of a block found above */
__device__ inline nvbx_tsdf_voxel nvbx_dev_tsdf_voxel(const nvbx_device_view& v, uint32_t slot, int vx, int vy, int vz) {
  return reinterpret_cast<const nvbx_tsdf_voxel*>(v.tsdf)[(size_t)slot * 512 + vz + 8 * vy + 64 * vx];
}
__device__ inline nvbx_color_voxel nvbx_dev_color_voxel(const nvbx_device_view& v, uint32_t slot, int vx, int vy, int vz) {
  return reinterpret_cast<const nvbx_color_voxel*>(v.color)[(size_t)slot * 512 + vz + 8 * vy + 64 * vx];
}
/* ESDF voxel unpacked to the reference's fields (esdf_and_gradients_conversions.cu:28-48 reads squared_distance_vox, observed, is_inside) */
__device__ inline nvbx_esdf_voxel nvbx_dev_esdf_voxel(const nvbx_device_view& v, uint32_t slot, int vx, int vy, int vz) {
  const uint2 p = reinterpret_cast<const uint2*>(v.esdf)[(size_t)slot * 512 + vx + 8 * vy + 64 * vz];
  nvbx_esdf_voxel o;
  o.squared_distance_vox = __uint_as_float(p.x);
  o.parent_direction[0] = (int8_t)(p.y & 0xFF); o.parent_direction[1] = (int8_t)((p.y >> 8) & 0xFF); o.parent_direction[2] = (int8_t)((p.y >> 16) & 0xFF);
  o.observed = (p.y >> 24) & 1u; o.is_inside = (p.y >> 25) & 1u; o.is_site = (p.y >> 26) & 1u; o.pad = 0;
  return o;
}
/* signed ESDF distance in metres at global voxel index (gx, gy, gz), or `unknown_value` (SignedDistanceFunctor,
 * esdf_and_gradients_conversions.cu:28-48) */
__device__ inline float nvbx_dev_esdf_distance_m(const nvbx_device_view& v, int32_t gx, int32_t gy, int32_t gz, float unknown_value) {
  const uint32_t s = nvbx_dev_find_block(v, gx >> 3, gy >> 3, gz >> 3, NVBX_LAYER_ESDF);
  if (!nvbx_dev_slot_ok(s)) return unknown_value;
  const nvbx_esdf_voxel e = nvbx_dev_esdf_voxel(v, s, gx & 7, gy & 7, gz & 7);
  if (!e.observed) return unknown_value;
  const float d = sqrtf(e.squared_distance_vox) * v.voxel_size;
  return e.is_inside ? -d : d;
}

/* ---- interpolated point queries (SEMANTICS.md "Point queries"; nvbx_query_points in nvblox_hip.h runs the same arithmetic).
 * The f32 evaluation order is stated ONCE, here: the library's kernel calls these functions too, so a caller's kernel and
 * nvbx_query_points give bit-identical answers whatever the caller's floating-point contraction flags.
 * Per axis: u = p / vs - 0.5 (IEEE division), b = floor(u), t = u - b; the corners are the voxels b + {0, 1}.  False when
 * a corner leaves the addressable range (block index in [-2^20, 2^20), i.e. voxel index in [-2^23, 2^23)) or p is not finite. */
__device__ inline bool nvbx_interp_axis(float p, float vs, int32_t* b, float* t) {
#pragma clang fp contract(off)
  const float u = p / vs - 0.5f;
  const float f = floorf(u);
  if (!(f >= -8388608.0f && f <= 8388606.0f)) return false;           /* (NaN fails too) */
  *b = (int32_t)f; *t = u - f;
  return true;
}
/* bilinear interpolant of c[i + 2j] (corner b + (i, j)) and its analytic gradient per metre (g[2] = 0) */
__device__ inline float nvbx_interp_bilinear(const float c[4], float tx, float ty, float vs, float g[3]) {
#pragma clang fp contract(off)
  const float dx0 = c[1] - c[0], dx1 = c[3] - c[2];
  const float a0 = c[0] + tx * dx0, a1 = c[2] + tx * dx1;
  g[0] = (dx0 + ty * (dx1 - dx0)) / vs;
  g[1] = (a1 - a0) / vs;
  g[2] = 0.0f;
  return a0 + ty * (a1 - a0);
}
/* trilinear interpolant of c[i + 2j + 4k] (corner b + (i, j, k)) and its analytic gradient per metre: the x component is the
 * (t_y, t_z)-weighted mean of the four x-differences over vs, likewise for y and z */
__device__ inline float nvbx_interp_trilinear(const float c[8], float tx, float ty, float tz, float vs, float g[3]) {
#pragma clang fp contract(off)
  const float dx00 = c[1] - c[0], dx10 = c[3] - c[2], dx01 = c[5] - c[4], dx11 = c[7] - c[6];
  const float a00 = c[0] + tx * dx00, a10 = c[2] + tx * dx10, a01 = c[4] + tx * dx01, a11 = c[6] + tx * dx11;   /* along x */
  const float dy0 = a10 - a00, dy1 = a11 - a01;
  const float b0 = a00 + ty * dy0, b1 = a01 + ty * dy1;                                                       /* along y */
  const float gx0 = dx00 + ty * (dx10 - dx00), gx1 = dx01 + ty * (dx11 - dx01);
  const float dz00 = c[4] - c[0], dz10 = c[5] - c[1], dz01 = c[6] - c[2], dz11 = c[7] - c[3];
  const float gz0 = dz00 + tx * (dz10 - dz00), gz1 = dz01 + tx * (dz11 - dz01);
  g[0] = (gx0 + tz * (gx1 - gx0)) / vs;
  g[1] = (dy0 + tz * (dy1 - dy0)) / vs;
  g[2] = (gz0 + ty * (gz1 - gz0)) / vs;
  return b0 + tz * (b1 - b0);
}
/* corner value of an ESDF voxel {f32 squared_distance_vox, u32 meta}: signed metres (k_esdf_dense's expression); false if unobserved */
__device__ inline bool nvbx_interp_esdf_value(uint2 e, float vs, float* d) {
#pragma clang fp contract(off)
  if (!((e.y >> 24) & 1u)) return false;
  float v = sqrtf(__uint_as_float(e.x)) * vs;
  if ((e.y >> 25) & 1u) v = v * -1.0f;
  *d = v;
  return true;
}

/* TSDF at p (metres, layer frame): trilinear over the 8 corner voxels, each of which must exist with weight >= min_weight.
 * Returns valid; otherwise *d = unknown_value and grad = 0.  grad may be NULL. */
__device__ inline bool nvbx_dev_interpolate_tsdf(const nvbx_device_view& v, const float p[3], float min_weight, float unknown_value,
                                                 float* d, float* grad) {
  int32_t b[3]; float t[3], c[8], g[3] = {0.0f, 0.0f, 0.0f};
  bool ok = nvbx_interp_axis(p[0], v.voxel_size, &b[0], &t[0]) && nvbx_interp_axis(p[1], v.voxel_size, &b[1], &t[1]) &&
            nvbx_interp_axis(p[2], v.voxel_size, &b[2], &t[2]);
  for (int k = 0; k < 8 && ok; k++) {
    const int32_t gx = b[0] + (k & 1), gy = b[1] + ((k >> 1) & 1), gz = b[2] + (k >> 2);
    const uint32_t s = nvbx_dev_find_block(v, gx >> 3, gy >> 3, gz >> 3, NVBX_LAYER_TSDF);
    if (!nvbx_dev_slot_ok(s)) { ok = false; break; }
    const nvbx_tsdf_voxel e = nvbx_dev_tsdf_voxel(v, s, gx & 7, gy & 7, gz & 7);
    if (!(e.weight >= min_weight)) { ok = false; break; }
    c[k] = e.distance;
  }
  float r = unknown_value;
  if (ok) r = nvbx_interp_trilinear(c, t[0], t[1], t[2], v.voxel_size, g);
  *d = r;
  if (grad) { grad[0] = g[0]; grad[1] = g[1]; grad[2] = g[2]; }
  return ok;
}
/* ESDF at p: plane_vz < 0 -- 3-D mode, trilinear; plane_vz >= 0 -- 2-D mode, bilinear over the (x, y) corners of the global voxel
 * plane z = plane_vz (floor(esdf_slice_height / voxel_size)), p[2] ignored, grad[2] = 0.  Corners must be observed. */
__device__ inline bool nvbx_dev_interpolate_esdf(const nvbx_device_view& v, const float p[3], int32_t plane_vz, float unknown_value,
                                                 float* d, float* grad) {
  const bool plane = plane_vz >= 0;
  int32_t b[3]; float t[3] = {0.0f, 0.0f, 0.0f}, c[8], g[3] = {0.0f, 0.0f, 0.0f};
  bool ok = nvbx_interp_axis(p[0], v.voxel_size, &b[0], &t[0]) && nvbx_interp_axis(p[1], v.voxel_size, &b[1], &t[1]);
  if (plane) b[2] = plane_vz; else ok = ok && nvbx_interp_axis(p[2], v.voxel_size, &b[2], &t[2]);
  const int nc = plane ? 4 : 8;
  for (int k = 0; k < nc && ok; k++) {
    const int32_t gx = b[0] + (k & 1), gy = b[1] + ((k >> 1) & 1), gz = b[2] + (k >> 2);
    const uint32_t s = nvbx_dev_find_block(v, gx >> 3, gy >> 3, gz >> 3, NVBX_LAYER_ESDF);
    if (!nvbx_dev_slot_ok(s)) { ok = false; break; }
    const uint2 e = reinterpret_cast<const uint2*>(v.esdf)[(size_t)s * 512 + (gx & 7) + 8 * (gy & 7) + 64 * (gz & 7)];
    ok = nvbx_interp_esdf_value(e, v.voxel_size, &c[k]);
  }
  float r = unknown_value;
  if (ok) r = plane ? nvbx_interp_bilinear(c, t[0], t[1], v.voxel_size, g) : nvbx_interp_trilinear(c, t[0], t[1], t[2], v.voxel_size, g);
  *d = r;
  if (grad) { grad[0] = g[0]; grad[1] = g[1]; grad[2] = g[2]; }
  return ok;
}
#endif  /* __HIPCC__ */
#endif  /* NVBLOX_HIP_DEVICE_H_ */
