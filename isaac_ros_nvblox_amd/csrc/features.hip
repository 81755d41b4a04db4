// features.hip -- the feature layer: per-pixel fp16 feature images (a vision backbone's coarse grid of C-channel vectors) averaged into the
// voxels a frame sees, and read back at 3-D points (SEMANTICS.md "Feature layer").
// [U] Upstream's FeatureLayer / projective feature integrator are not readable in the reference tree: the rules are the colour integrator's
// (nvbx_color_worker.h), restated here for a payload of C halfs per voxel.
//
// Storage (allocated by nvbx_enable_features, carried by pool growth; the pointers travel in the kernels' own argument structs, not in DMap):
//   feat_val : capacity x (C / 8) x 512 x 16 B -- block-major, then [chunk of 8 channels][voxel z + 8y + 64x][8 halfs]: the 64 lanes of a wavefront
//              (lane = voxel) touch 1 KiB contiguous per access, whatever C is
//   feat_w   : capacity x 512 x f32
// A block's payload counts only while its slot carries F_FEATURE.  Whoever takes the block's TSDF away clears the flag (one more constant in
// the atomicAnd that clears F_COLOR) and moves no byte of it; the first feature frame that reaches a voxel of an unflagged slot treats the
// whole block as empty, sets the flag and writes all 512 voxels.
//
// Two launches per frame, classic order (nothing rides anywhere):
//   k_feature_trace      the colour frame's sphere tracing (sphere_trace_camera, nvbx_sphere_trace.h) into a scratch image of this path's own;
//                        the colour path's synthetic depth, its work list and its counters are left alone
//   k_integrate_features one 512-thread workgroup per candidate block (lane = voxel), candidates found as color_integrate_worker finds them
//                        (chunked slot scan, ballot on the flags, frustum vote of 8 lanes).  Projection, synthetic-depth taps and the
//                        occlusion verdict once per voxel; then a loop over chunks of 8 channels: four 16-B tap loads, one 16-B voxel load,
//                        one 16-B voxel store per lane.  Registers do not scale with C.
// Whole blocks in the public layout are read by k_gather_feature_blocks and written by k_scatter_feature_blocks (nvbx_get_feature_blocks /
// nvbx_set_feature_blocks); another mapper's layer is merged in by feature_merge.hip.
#include <algorithm>
#include <cstring>
#include "nvbx_mapper.h"
#include "nvbx_sphere_trace.h"
#include "nvbx_feature.h"      // half8, feature_voxel_of

using namespace nvbx;

struct FeatTraceArgs { FrameCore f; float* synth; int32_t srows, scols, max_steps; float max_len, eps_m; };
struct FeatArgs {
  FrameCore f;                   // the full-resolution camera (rows, cols = its height, width), pose, parameters
  const half8* img;              // rows_f x cols_f x nch chunks, row-major HWC
  int32_t rows_f, cols_f, nch;   // nch = C / 8
  float stride;
  const float* synth; int32_t srows, scols;
  half8* val; float* w;          // the pools
  int32_t chunk;                 // slots per workgroup iteration of the candidate scan (1 .. 64)
};

// color.hip's sphere tracing launch for one camera, 8 lanes per ray, without the colour work list's reset: the same function
// (sphere_trace_camera), so the image is the colour frame's (and nvbx_render_view's)
constexpr int FEAT_TRACE_LANES = 8;
__global__ __launch_bounds__(256) void k_feature_trace(DMap m, FeatTraceArgs a) {
  (void)sphere_trace_camera<FEAT_TRACE_LANES>(m, a.f, a.synth, a.srows, a.scols, a.max_steps, a.max_len, a.eps_m, (int)blockIdx.x, true);
}

// one candidate block: every thread of the workgroup calls (barriers); `flags` = the slot's flags as this launch found them
__device__ inline void feature_integrate_block(const DMap& m, const FeatArgs& a, int32_t slot, int32_t bx, int32_t by, int32_t bz, uint32_t flags) {
  const int tid = threadIdx.x;
  const int vx = tid >> 6, vy = (tid >> 3) & 7, vz = tid & 7;
  const FrameCore& f = a.f;
  // ---- once per voxel: the colour integrator's tests (color_integrate_block; the occlusion test is the shared one), the feature grid in place of the colour image
  bool pass = false;
  float ax = 0.0f, ay = 0.0f; int32_t i00 = 0;
  {
    const float lx = voxel_center(bx, vx, f.block_size, f.voxel_size), ly = voxel_center(by, vy, f.block_size, f.voxel_size),
                lz = voxel_center(bz, vz, f.block_size, f.voxel_size);
    float pc[3];
    apply_rt(f.R_CL, f.t_CL, lx, ly, lz, pc);
    float u, v;
    bool ok = cam_project(f, pc, &u, &v);
    const float vd = pc[2];
    if (f.max_dist > 0.0f && vd > f.max_dist) ok = false;
    int32_t fi00, si00; float fax, fay, sax, say;
    const bool c_ok = scaled_taps(u, v, a.stride, a.rows_f, a.cols_f, &fi00, &fax, &fay);
    const bool s_ok = scaled_taps(u, v, (float)f.subsample, a.srows, a.scols, &si00, &sax, &say);
    if (ok && c_ok && s_ok) {
      const float* sp = a.synth + si00;
      const float s00 = sp[0], s10 = sp[1], s01 = sp[a.scols], s11 = sp[a.scols + 1];
      if (synth_depth_agrees(s00, s10, s01, s11, sax, say, vd, f.occlusion_thresh)) { pass = true; ax = fax; ay = fay; i00 = fi00; }
    }
  }
  if (!__syncthreads_or(pass ? 1 : 0)) return;         // no voxel of the block is reached: nothing is written, the slot is not flagged
  const bool fresh = !(flags & F_FEATURE);             // uniform: the block holds nothing yet -- every voxel is written
  if (fresh && tid == 0) atomicOr(&m.slot_flags[slot], F_FEATURE);
  float* wp = a.w + (size_t)slot * 512 + tid;
  const float w0 = (fresh || !pass) ? 0.0f : *wp;
  const float tw = w0 + 1.0f;
  const float ca = NVBX_DIV(w0, tw), cb = NVBX_DIV(1.0f, tw);      // blend_u8's weights (w1 = 1)
  if (pass) *wp = fminf(w0 + 1.0f, f.max_weight);
  else if (fresh) *wp = 0.0f;
  if (!pass && !fresh) return;                         // (no barrier below)
  const int nch = a.nch;
  const half8* t0 = a.img + (size_t)i00 * nch;         // tap (x0, y0); (x0 + 1, y0) is nch chunks on, the next row cols_f * nch
  const size_t row = (size_t)a.cols_f * nch;
  half8* vp = a.val + (size_t)slot * nch * 512 + tid;
  const float bx0 = 1.0f - ax, by0 = 1.0f - ay;
#pragma unroll 2
  for (int k = 0; k < nch; k++) {
    half8 o;
    if (pass) {
      const half8 t00 = t0[k], t10 = t0[nch + k], t01 = t0[row + k], t11 = t0[row + nch + k];
      half8 old;
      if (fresh) { for (int q = 0; q < 8; q++) old[q] = (_Float16)0.0f; } else old = vp[(size_t)k * 512];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const float top = bx0 * (float)t00[q] + ax * (float)t10[q];
        const float bot = bx0 * (float)t01[q] + ax * (float)t11[q];
        const float fv = by0 * top + ay * bot;
        const float nv = (float)old[q] * ca + fv * cb;
        o[q] = (_Float16)nv;                           // round to nearest even
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; q++) o[q] = (_Float16)0.0f;
    }
    vp[(size_t)k * 512] = o;
  }
}

// candidate discovery of color_integrate_worker (nvbx_color_worker.h) for one camera; a block a LiDAR scan left F_BAND_STALE is voted from its
// TSDF and NOT repaired (this launch writes nothing but the feature pools and F_FEATURE)
__global__ __launch_bounds__(512) void k_integrate_features(DMap m, FeatArgs a) {
  __shared__ int s_out[1][6];
  const int tid = threadIdx.x;
  const FrameCore& f = a.f;
  const int chunk = a.chunk;
  const int lane_c = tid & 63;
  const int32_t cap = (int32_t)m.capacity;
  const int32_t n_wg = (int32_t)gridDim.x;
  const int32_t wg = xcd_chunked((int32_t)blockIdx.x, n_wg);
  const int32_t hw = m.counters[C_HIGH_WATER];
  for (int32_t base = wg * chunk; base < hw; base += n_wg * chunk) {
    const int32_t ls = min(base + lane_c, cap - 1);
    const uint32_t lflags = lane_c < chunk ? m.slot_flags[ls] : 0u;
    int32_t lbx = 0, lby = 0, lbz = 0;
    if (lane_c < chunk) { lbx = m.slot_index[3 * ls]; lby = m.slot_index[3 * ls + 1]; lbz = m.slot_index[3 * ls + 2]; }
    u64 cand = __ballot(lane_c < chunk && base + lane_c < hw && (lflags & F_TSDF) && (lflags & (F_BAND | F_BAND_STALE)));      // (the same in all eight wavefronts: nobody writes these bits here)
    while (cand) {
      const int cj = __ffsll((long long)cand) - 1;
      cand &= cand - 1ull;
      const int32_t slot = base + cj;
      const uint32_t flags = __shfl(lflags, cj);
      const int32_t bx = __shfl(lbx, cj), by = __shfl(lby, cj), bz = __shfl(lbz, cj);
      if (flags & F_BAND_STALE) {      // uniform
        const float2 tv = m.tsdf[(size_t)slot * 512 + tid];
        if (!__syncthreads_or(in_band(tv.x, tv.y, f.trunc) ? 1 : 0)) continue;
      }
      if (!frustum_vote<1>(&f, 1, bx, by, bz, s_out)) continue;        // uniform
      feature_integrate_block(m, a, slot, bx, by, bz, flags);
    }
  }
}

// ---- readers
// one lane per (point, chunk): the nch lanes of a point write its C halfs as consecutive 16-B stores
__global__ __launch_bounds__(256) void k_query_features(DMap m, const half8* __restrict__ val, const float* __restrict__ w, int32_t nch, const float* __restrict__ pts,
                                                        int64_t n, float vs, half8* __restrict__ feat_out, float* __restrict__ w_out) {
  const int64_t total = n * nch;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / nch; const int k = (int)(i - p * nch);
    int32_t g[3] = {0, 0, 0};
    uint32_t slot = SLOT_NONE;
    if (feature_voxel_of(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], vs, g)) slot = find_slot(m, g[0] >> 3, g[1] >> 3, g[2] >> 3, F_FEATURE);
    half8 o; float wv = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; q++) o[q] = (_Float16)0.0f;
    if (slot_ok(slot)) {
      const int t = (g[2] & 7) + 8 * (g[1] & 7) + 64 * (g[0] & 7);
      o = val[((size_t)slot * nch + k) * 512 + t];
      if (k == 0) wv = w[(size_t)slot * 512 + t];
    }
    feat_out[i] = o;
    if (k == 0) w_out[p] = wv;
  }
}
// block i of the list -> the public layout: voxel t = vx 64 + vy 8 + vz, C contiguous halfs per voxel; an absent / unflagged block reads as zeros
__global__ __launch_bounds__(512) void k_gather_feature_blocks(DMap m, const half8* val, const float* w, int32_t nch, const int32_t* idx, int32_t n, half8* feat_out,
                                                               float* w_out, int32_t* found) {
  const int i = blockIdx.x; if (i >= n) return;
  const int t = threadIdx.x;
  const uint32_t s = find_slot(m, idx[3 * i], idx[3 * i + 1], idx[3 * i + 2], F_FEATURE);
  if (t == 0) found[i] = slot_ok(s) ? 1 : 0;
  w_out[(size_t)i * 512 + t] = slot_ok(s) ? w[(size_t)s * 512 + t] : 0.0f;
  half8 z;
#pragma unroll
  for (int q = 0; q < 8; q++) z[q] = (_Float16)0.0f;
  for (int k = 0; k < nch; k++) feat_out[((size_t)i * 512 + t) * nch + k] = slot_ok(s) ? val[((size_t)s * nch + k) * 512 + t] : z;
}
// the reverse: block i of the list, in the public layout, -> the pools.  Only a block whose slot carries the TSDF layer is written (features do not
// keep a block alive); all 512 voxels are replaced and the slot is flagged.  Nothing else of the map is touched.
__global__ __launch_bounds__(512) void k_scatter_feature_blocks(DMap m, half8* val, float* w, int32_t nch, const int32_t* idx, int32_t n, const half8* feat_in,
                                                                const float* w_in, int32_t* written) {
  const int i = blockIdx.x; if (i >= n) return;
  const int t = threadIdx.x;
  const int32_t x = idx[3 * i], y = idx[3 * i + 1], z = idx[3 * i + 2];
  const uint32_t s = nvbx_index_in_range(x, y, z) ? find_slot(m, x, y, z, F_TSDF) : SLOT_NONE;
  if (t == 0) written[i] = slot_ok(s) ? 1 : 0;
  if (!slot_ok(s)) return;
  w[(size_t)s * 512 + t] = w_in[(size_t)i * 512 + t];
  for (int k = 0; k < nch; k++) val[((size_t)s * nch + k) * 512 + t] = feat_in[((size_t)i * 512 + t) * nch + k];
  if (t == 0) atomicOr(&m.slot_flags[s], F_FEATURE);
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" int nvbx_enable_features(nvbx_mapper* m, int32_t channels) {
  if (!m) return NVBX_E_INVALID;
  if (channels < 8 || channels > 256 || (channels & 7)) { set_error("nvbx_enable_features: channels must be a multiple of 8, 8 .. 256"); return NVBX_E_INVALID; }
  if (m->p.projective_layer_type == 1) { set_error("nvbx_enable_features: an occupancy mapper carries no feature layer (the occlusion test sphere-traces a TSDF)"); return NVBX_E_INVALID; }
  if (m->feat_channels) {
    if (m->feat_channels == channels) return NVBX_OK;
    set_error("nvbx_enable_features: the layer is already on with another channel count"); return NVBX_E_INVALID;
  }
  if (m->begin_call()) return NVBX_E_DEVICE;
  const size_t vb = (size_t)m->capacity * 1024 * (size_t)channels, wb = (size_t)m->capacity * 2048;
  size_t free_b = 0, total_b = 0; NVBX_HIP(hipMemGetInfo(&free_b, &total_b));
  if (free_b < vb + wb + (64u << 20)) { set_error("nvbx_enable_features: the pools do not fit in free device memory"); return NVBX_E_DEVICE; }
  void* v = nullptr; void* w = nullptr;
  if (hipMalloc(&v, vb) != hipSuccess || hipMalloc(&w, wb) != hipSuccess) {
    (void)hipGetLastError(); if (v) (void)hipFree(v);
    set_error("nvbx_enable_features: device allocation failed"); return NVBX_E_DEVICE;
  }
  // (no fill: nothing reads a block's payload before the launch that flags its slot has written all of it)
  m->feat_val = v; m->feat_w = static_cast<float*>(w); m->feat_channels = channels;
  return NVBX_OK;
}

extern "C" int nvbx_integrate_features(nvbx_mapper* m, const void* feat_dev, int32_t rows_f, int32_t cols_f, int32_t stride, const float T_L_C[16],
                                       const nvbx_camera* camera) {
  if (!m || !feat_dev || !T_L_C || !camera || ((uintptr_t)feat_dev & 15)) { set_error("nvbx_integrate_features: invalid argument (the feature image is 16-byte aligned)"); return NVBX_E_INVALID; }
  if (!m->feat_channels) { set_error("nvbx_integrate_features: call nvbx_enable_features first"); return NVBX_E_INVALID; }
  if (!nvbx_camera_valid(camera)) { set_error("nvbx_integrate_features: camera sides 1 .. 32768, focal lengths > 0"); return NVBX_E_INVALID; }
  if (stride < 1 || rows_f < 1 || cols_f < 1 || (int64_t)cols_f * stride > camera->width || (int64_t)rows_f * stride > camera->height) {
    set_error("nvbx_integrate_features: stride >= 1, cols_f * stride <= camera width, rows_f * stride <= camera height"); return NVBX_E_INVALID; }
  if (!nvbx_pose_in_range(T_L_C, m->p.voxel_size * 8.0f, m->p.sphere_tracing_max_ray_length_m + m->p.max_integration_distance_m)) {
    set_error("nvbx_integrate_features: T_L_C is not finite or lies outside the addressable block range (+-2^20 blocks)"); return NVBX_E_INVALID; }
  const SubsampledSize ss = subsampled_size(m, 0, camera->height, camera->width);
  if (!ss.ok()) { set_error("nvbx_integrate_features: camera too small for the sphere-tracing subsampling"); return NVBX_E_INVALID; }
  if (m->begin_call()) return NVBX_E_DEVICE;            // held-back work is carried out first: classic order from here on
  if (m->feat_synth.ensure(m->stream, (size_t)ss.rows * ss.cols * 4)) return NVBX_E_DEVICE;
  const Frame fr = m->make_frame(T_L_C, camera, camera->height, camera->width, m->p.sphere_tracing_subsampling);
  FeatTraceArgs ta{}; ta.f = fr; ta.synth = m->feat_synth.as<float>(); ta.srows = ss.rows; ta.scols = ss.cols; ta.max_steps = m->p.sphere_tracing_max_steps;
  ta.max_len = m->p.sphere_tracing_max_ray_length_m; ta.eps_m = m->p.sphere_tracing_surface_eps_vox * m->p.voxel_size;
  NVBX_LAUNCH(m, k_feature_trace, dim3((unsigned)trace_patch_workgroups(FEAT_TRACE_LANES, ss.rows, ss.cols)), dim3(256), m->d, ta);
  FeatArgs a{}; a.f = fr; a.img = static_cast<const half8*>(feat_dev); a.rows_f = rows_f; a.cols_f = cols_f; a.nch = m->feat_channels / 8; a.stride = (float)stride;
  a.synth = ta.synth; a.srows = ss.rows; a.scols = ss.cols; a.val = static_cast<half8*>(m->feat_val); a.w = m->feat_w;
  a.chunk = candidate_scan_chunk(m);
  NVBX_LAUNCH(m, k_integrate_features, dim3((unsigned)candidate_scan_grid(m)), dim3(512), m->d, a);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

extern "C" int nvbx_query_features(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, void* feat_out_dev, float* weight_out_dev) {
  if (!m || n < 0 || (n > 0 && (!points_xyz_dev || !feat_out_dev || !weight_out_dev)) || ((uintptr_t)feat_out_dev & 15)) {
    set_error("nvbx_query_features: invalid argument (the feature output is 16-byte aligned)"); return NVBX_E_INVALID; }
  if (!m->feat_channels) { set_error("nvbx_query_features: call nvbx_enable_features first"); return NVBX_E_INVALID; }
  if (n == 0) return NVBX_OK;
  if (m->begin_call()) return NVBX_E_DEVICE;
  const int32_t nch = m->feat_channels / 8;
  NVBX_LAUNCH(m, k_query_features, dim3((unsigned)std::min<int64_t>((n * nch + 255) / 256, 8192)), dim3(256), m->d, static_cast<const half8*>(m->feat_val),
              (const float*)m->feat_w, nch, points_xyz_dev, n, m->p.voxel_size, static_cast<half8*>(feat_out_dev), weight_out_dev);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

extern "C" int nvbx_get_feature_blocks(nvbx_mapper* m, const nvbx_index3d* idx, int64_t n, void* feat_out, float* weight_out, int32_t* found_out) {
  if (!m || n < 0 || (n > 0 && (!idx || !feat_out || !weight_out))) { set_error("nvbx_get_feature_blocks: invalid argument"); return NVBX_E_INVALID; }
  if (!m->feat_channels) { set_error("nvbx_get_feature_blocks: call nvbx_enable_features first"); return NVBX_E_INVALID; }
  if (m->begin_call()) return NVBX_E_DEVICE;
  const int32_t nch = m->feat_channels / 8;
  const size_t fb = (size_t)512 * 16 * nch, wb = 2048;
  const int64_t chunk = std::max<int64_t>(1, (int64_t)((m->staging.bytes - 65536) / (fb + wb + 16)));
  for (int64_t o = 0; o < n; o += chunk) {
    const int64_t c = std::min(chunk, n - o);
    int32_t* d_idx = m->staging.as<int32_t>(); int32_t* d_found = d_idx + 3 * c;
    uint8_t* d_w = m->staging.as<uint8_t>() + (((size_t)c * 16 + 255) & ~(size_t)255);
    uint8_t* d_f = d_w + (size_t)c * wb;                         // (256-byte aligned: wb is)
    NVBX_HIP(hipMemcpyAsync(d_idx, idx + o, (size_t)c * 12, hipMemcpyHostToDevice, m->stream));
    NVBX_LAUNCH(m, k_gather_feature_blocks, dim3((unsigned)c), dim3(512), m->d, static_cast<const half8*>(m->feat_val), (const float*)m->feat_w, nch, (const int32_t*)d_idx,
                (int32_t)c, reinterpret_cast<half8*>(d_f), reinterpret_cast<float*>(d_w), d_found);
    NVBX_HIP(hipMemcpyAsync((uint8_t*)feat_out + (size_t)o * fb, d_f, (size_t)c * fb, hipMemcpyDeviceToHost, m->stream));
    NVBX_HIP(hipMemcpyAsync((uint8_t*)weight_out + (size_t)o * wb, d_w, (size_t)c * wb, hipMemcpyDeviceToHost, m->stream));
    if (found_out) NVBX_HIP(hipMemcpyAsync(found_out + o, d_found, (size_t)c * 4, hipMemcpyDeviceToHost, m->stream));
    NVBX_HIP(hipStreamSynchronize(m->stream));
  }
  return NVBX_OK;
}

extern "C" int nvbx_set_feature_blocks(nvbx_mapper* m, const nvbx_index3d* idx, int64_t n, const void* feat_in, const float* weight_in, int32_t* written_out) {
  if (!m || n < 0 || (n > 0 && (!idx || !feat_in || !weight_in))) { set_error("nvbx_set_feature_blocks: invalid argument"); return NVBX_E_INVALID; }
  if (!m->feat_channels) { set_error("nvbx_set_feature_blocks: call nvbx_enable_features first"); return NVBX_E_INVALID; }
  for (int64_t i = 0; i < n * 512; i++)
    if (!(weight_in[i] >= 0.0f)) { set_error("nvbx_set_feature_blocks: a weight is negative or not a number"); return NVBX_E_INVALID; }
  if (m->begin_call()) return NVBX_E_DEVICE;            // held-back work is carried out first
  const int32_t nch = m->feat_channels / 8;
  const size_t fb = (size_t)512 * 16 * nch, wb = 2048;
  const int64_t chunk = std::max<int64_t>(1, (int64_t)((m->staging.bytes - 65536) / (fb + wb + 16)));
  for (int64_t o = 0; o < n; o += chunk) {
    const int64_t c = std::min(chunk, n - o);
    int32_t* d_idx = m->staging.as<int32_t>(); int32_t* d_written = d_idx + 3 * c;
    uint8_t* d_w = m->staging.as<uint8_t>() + (((size_t)c * 16 + 255) & ~(size_t)255);
    uint8_t* d_f = d_w + (size_t)c * wb;                         // (256-byte aligned: wb is)
    NVBX_HIP(hipMemcpyAsync(d_idx, idx + o, (size_t)c * 12, hipMemcpyHostToDevice, m->stream));
    NVBX_HIP(hipMemcpyAsync(d_f, (const uint8_t*)feat_in + (size_t)o * fb, (size_t)c * fb, hipMemcpyHostToDevice, m->stream));
    NVBX_HIP(hipMemcpyAsync(d_w, (const uint8_t*)weight_in + (size_t)o * wb, (size_t)c * wb, hipMemcpyHostToDevice, m->stream));
    NVBX_LAUNCH(m, k_scatter_feature_blocks, dim3((unsigned)c), dim3(512), m->d, static_cast<half8*>(m->feat_val), m->feat_w, nch, (const int32_t*)d_idx, (int32_t)c,
                reinterpret_cast<const half8*>(d_f), reinterpret_cast<const float*>(d_w), d_written);
    if (written_out) NVBX_HIP(hipMemcpyAsync(written_out + o, d_written, (size_t)c * 4, hipMemcpyDeviceToHost, m->stream));
    NVBX_HIP(hipStreamSynchronize(m->stream));
  }
  return NVBX_OK;
}
