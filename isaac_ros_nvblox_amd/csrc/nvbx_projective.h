// nvbx_projective.h -- THE definitions of the projective geometry that several launches must evaluate alike, float operation for float operation
// (numerical contract): the ray through a pixel of a subsampled pinhole image, the numbering of those rays over workgroups, a block's
// frustum test, the occlusion test against the synthetic depth image, the voxel that contains a point.  SEMANTICS.md's "bit for bit" between
// the colour frame, the feature frame, the renderer and the view gain holds because those callers share these functions.
#pragma once
#include "nvbx_mapper.h"

namespace nvbx {
// Host: the subsampled image of a height x width camera; s = the call's own subsampling if > 0, else the mapper's (at least 1).  !ok(): each caller refuses in its own words.
struct SubsampledSize { int32_t s, rows, cols; bool ok() const { return rows >= 2 && cols >= 2; } };
inline SubsampledSize subsampled_size(const nvbx_mapper* m, int32_t own, int32_t height, int32_t width) {
  const int32_t s = own > 0 ? own : std::max(1, m->p.sphere_tracing_subsampling);
  return SubsampledSize{s, height / s, width / s};
}
// Host: the candidate scan of a colour / feature frame (color_integrate_worker, k_integrate_features) -- its grid, one resident batch of
// 512-thread workgroups, and the slots a workgroup takes per iteration (1 .. 64), from the high-water mark the GPU last reported (a hint only).
// Up to 4 iterations of single slots: a room-sized map keeps the stride-grid pairing, which balances the in-band blocks better than runs of neighbours.
inline int candidate_scan_grid(const nvbx_mapper* m) { return (int)std::min<int64_t>(m->capacity, 1024); }
inline int32_t candidate_scan_chunk(const nvbx_mapper* m) {
  const int64_t hw_seen = std::max<int64_t>(1, __atomic_load_n(&m->h_mirror[1], __ATOMIC_RELAXED));
  int32_t ch = 1; while (ch < 64 && (int64_t)ch * candidate_scan_grid(m) * 4 < hw_seen) ch *= 2;
  return ch;
}
// Workgroups that trace ONE srows x scols image at rl lanes per ray: a 256-thread workgroup takes an 8 x (32 / rl) patch of rays, the count
// is rounded up to a multiple of NSH (trace_patch_pixel).  A batch launches this many per camera, camera after camera.
__host__ __device__ inline int trace_patch_workgroups(int rl, int32_t srows, int32_t scols) {
  const int ph = 256 / rl / 8;
  const int patches = ((scols + 7) / 8) * ((srows + ph - 1) / ph);
  return NSH * ((patches + NSH - 1) / NSH);
}

#ifdef __HIPCC__
// XCD-aware ray -> workgroup mapping.  Workgroups are dispatched round-robin over the 8 XCDs, each with its own L2: with rays dealt out in
// row-major order every XCD marches through EVERY part of the frustum and fetches its own copy of every TSDF block and hash line (PMC: 6.6 MB of
// HBM traffic for 1.0 MB of blocks).  Instead a workgroup takes an 8 x PH patch of rays, and the patches are numbered so that the workgroups of
// one XCD (number & 7) own a contiguous band of patch rows.  Thread tid of workgroup wg -> its ray's pixel (r, c); false: no ray.
template <int RL>
__device__ inline bool trace_patch_pixel(int wg, int tid, int32_t srows, int32_t scols, int* r, int* c) {
  constexpr int PW = 8, PH = (256 / RL) / PW;       // 256 / RL rays per 256-thread workgroup (8 x 4 at 8 lanes per ray)
  const int patches_x = (scols + PW - 1) / PW, patches_y = (srows + PH - 1) / PH;
  const int n_patch = patches_x * patches_y, per_xcd = (n_patch + NSH - 1) / NSH;
  const int patch = (wg & (NSH - 1)) * per_xcd + (wg >> 3);
  const int pr = tid / RL;                            // ray within the patch
  const int py = patch / patches_x, px = patch - py * patches_x;
  *r = py * PH + pr / PW; *c = px * PW + pr % PW;
  return patch < n_patch && (wg >> 3) < per_xcd && *r < srows && *c < scols;
}
// The ray of pixel (r, c) of the subsampled image: through the centre of full-resolution pixel (r s, c s).  dl = its unit direction in the map
// frame; returns the direction's camera-frame z, which turns the ray parameter t into depth (t * z).
__device__ inline float pinhole_ray(float fu, float fv, float cu, float cv, int32_t subsample, const float* R_LC, int r, int c, float* dl) {
  const float rx = (((float)(c * subsample) + 0.5f) - cu) / fu;
  const float ry = (((float)(r * subsample) + 0.5f) - cv) / fv;
  const float n = NVBX_SQRT((rx * rx + ry * ry) + 1.0f);          // (NVBX_SQRT / NVBX_DIV: the IEEE results, shorter sequences -- nvbx_arith.h)
  const float dcx = NVBX_DIV(rx, n), dcy = NVBX_DIV(ry, n), dcz = NVBX_DIV(1.0f, n);
  rotate(R_LC, dcx, dcy, dcz, dl);
  return dcz;
}
// The voxel that contains coordinate p, per axis: floor(p / vs), as a float (feature_voxel_of's range check) and as the index.
__device__ inline float voxel_floor(float p, float vs) { return floorf(NVBX_DIV(p, vs)); }
__device__ inline int32_t voxel_of(float p, float vs) { return (int32_t)voxel_floor(p, vs); }
// The six frustum planes on a camera-frame point pc: outside(q) for every plane q (left, right, top, bottom, behind, beyond max_dist) that pc
// lies outside of.  A block is out of view when all 8 corners are outside ONE plane.  (A callback, so that the caller's statements expand in
// place; color_scan_worker keeps a copy of corner and planes -- nvbx_color_worker.h says why.)
template <typename F>
__device__ inline void frustum_planes_outside(const FrameCore& f, const float* pc, F&& outside) {
  if (f.fu * pc[0] + f.cu * pc[2] < 0.0f) outside(0);
  if (f.fu * pc[0] + (f.cu - (float)f.w) * pc[2] > 0.0f) outside(1);
  if (f.fv * pc[1] + f.cv * pc[2] < 0.0f) outside(2);
  if (f.fv * pc[1] + (f.cv - (float)f.h) * pc[2] > 0.0f) outside(3);
  if (pc[2] < 0.0f) outside(4);
  if (f.max_dist > 0.0f && pc[2] > f.max_dist) outside(5);
}
// The frustum vote of one block by a workgroup: 8 lanes per camera, one per corner, count the corners outside each plane in LDS (s_out).  Every
// thread of the workgroup calls (three barriers); returns the mask of the cameras f[0 .. ncam) whose frustum the block touches (uniform).
template <int NB>
__device__ inline uint32_t frustum_vote(const FrameCore* fs, int ncam, int32_t bx, int32_t by, int32_t bz, int (*s_out)[6]) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid < 6 * NB) (&s_out[0][0])[tid] = 0;
  __syncthreads();
  if (tid < 8 * ncam) {
    const int c = NB == 1 ? 0 : (tid >> 3), q = tid & 7;      // (one camera: a constant index -- a per-lane index into the argument block is a vector load from memory)
    const FrameCore& f = fs[c];
    float pc[3];
    apply_rt(f.R_CL, f.t_CL, (float)(bx + (q & 1)) * f.block_size, (float)(by + ((q >> 1) & 1)) * f.block_size, (float)(bz + ((q >> 2) & 1)) * f.block_size, pc);
    frustum_planes_outside(f, pc, [&](int plane) { atomicAdd(&s_out[c][plane], 1); });
  }
  __syncthreads();
  uint32_t in_view = 0u;
  for (int c = 0; c < ncam; c++) {
    bool iv = true;
#pragma unroll
    for (int q = 0; q < 6; q++) if (s_out[c][q] == 8) iv = false;
    if (iv) in_view |= 1u << c;
  }
  return in_view;
}
// The bilinear footprint of full-resolution image point (u, v) in a rows x cols image of 1 / scale the resolution (the synthetic depth image:
// scale = the subsampling; a feature grid: its stride): *i00 = index of the upper-left tap (the others: + 1, + cols, + cols + 1), (*ax, *ay) =
// the blend weights; false: the footprint leaves the image.
__device__ inline bool scaled_taps(float u, float v, float scale, int32_t rows, int32_t cols, int32_t* i00, float* ax, float* ay) {
  const float uc = NVBX_DIV(u, scale) - 0.5f, vc = NVBX_DIV(v, scale) - 0.5f;
  const float fx = floorf(uc), fy = floorf(vc);
  const int x0 = (int)fx, y0 = (int)fy;
  *i00 = pix(y0, x0, cols); *ax = uc - fx; *ay = vc - fy;
  return !(x0 < 0 || y0 < 0 || x0 + 1 > cols - 1 || y0 + 1 > rows - 1);
}
// The occlusion test of a voxel at camera-frame depth vd, second step (the first: scaled_taps on the synthetic depth image; the caller issues
// the four loads, together with others of its own): all four taps hit a surface (> 0) and their blend lies within thresh of vd.
__device__ inline bool synth_depth_agrees(float s00, float s10, float s01, float s11, float sax, float say, float vd, float thresh) {   // [U] color_occlusion_threshold_vox
  if (!(s00 > 0.0f) || !(s10 > 0.0f) || !(s01 > 0.0f) || !(s11 > 0.0f)) return false;
  const float stop = (1.0f - sax) * s00 + sax * s10;
  const float sbot = (1.0f - sax) * s01 + sax * s11;
  const float sd = (1.0f - say) * stop + say * sbot;
  return !(fabsf(sd - vd) > thresh);
}
#endif  // __HIPCC__
}  // namespace nvbx
