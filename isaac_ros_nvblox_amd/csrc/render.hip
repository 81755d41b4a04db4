// render.hip -- the map seen along rays: depth / colour / normal images from any pinhole pose (nvbx_render_view) and casts of a caller's own
// rays (nvbx_cast_rays); SEMANTICS.md "Rendering and ray casts", DESIGN.md 2.12.
// [U] Upstream serves the same requests with SphereTracer::renderImageOnGPU / renderRgbdImageOnGPU / castOnGPU (nvblox/rays/sphere_tracer.h),
// not readable in the reference tree.
//
// One launch per call, read-only on the map, no atomics, every output written once.  The march is sphere_trace_march (nvbx_sphere_trace.h), the
// function the colour frame's occlusion image runs: a group of RL lanes speculates along one ray, the sequence of t values is that of the serial
// march.  When a ray is done its group turns to the hit point P = o + t d:
//   normal  the 8 corner voxels of the trilinear interpolant at P lie in 1, 2, 4 or 8 blocks (an axis with b & 7 == 7 crosses a block face, the
//           rule of k_query_points): the group's lanes probe the distinct blocks in parallel (one 16-B entry load each), up to four lanes fetch one
//           z pair of corners each (one 16-B load inside a block), shuffles hand every lane the eight values, and the group's first lane runs
//           the interpolant's gradient -- the inline code of include/nvblox_hip_device.h, so the gradient is nvbx_query_points' bit for bit;
//   colour  the group's last lane probes the block of the voxel that contains P and reads its colour voxel.
// Colour and normal are template flags: an output that was not asked for costs no load.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "nvbx_mapper.h"
#include "nvbx_sphere_trace.h"
#include "../../include/nvblox_hip_device.h"

using namespace nvbx;

namespace {

enum { SRC_VIEW = 0, SRC_RAYS = 1 };
constexpr int RAYS_GRID_MAX = 8192;             // workgroups of a ray-list launch (the point query's cap); longer lists repeat the loop
constexpr float RENDER_MIN_WEIGHT = 1e-4f;     // the tracer's "observed" threshold: a corner of the normal's interpolant counts from here on

struct RenderArgs {
  // SRC_VIEW: pose, intrinsics, subsampling and the size of the rendered image
  float R_LC[9], t_LC[3]; float fu, fv, cu, cv; int32_t subsample, srows, scols;
  // SRC_RAYS: n rays in device memory; an origin further than origin_lim from the map's origin on some axis is "no hit" (block keys would alias)
  const float* origins; const float* dirs; int64_t n; float origin_lim;
  // the march
  float voxel_size, trunc, max_len, eps_m; int32_t max_steps;
  // outputs ([ray] or [ray][3]); hit, color, normal may be null
  float* depth; uint8_t* hit; uint8_t* color; float* normal;
};

// slot of block o (offset bits x | y << 1 | z << 2 from the base block) of the group: lane o % RL holds it in sl[o / RL]
template <int RL, int NW>
__device__ inline uint32_t group_slot(const uint32_t (&sl)[NW], int o, int gsh) {
  uint32_t r = SLOT_NONE;
#pragma unroll
  for (int w = 0; w < NW; w++) {
    const uint32_t cand = RL == 1 ? sl[w] : (uint32_t)__shfl((int)sl[w], gsh + (o & (RL - 1)));
    if (o / RL == w) r = cand;
  }
  return r;
}

// The group's ray is done: t, hit (group-uniform).  Every lane of the wavefront calls (shuffles, ballots); the group's first lane writes ray `idx`.
template <int RL, bool COLOR, bool NORMAL>
__device__ inline void render_epilogue(const DMap& m, const RenderArgs& a, const float* o, const float* dl, float t, bool hit, bool valid, int sub, int gsh,
                                       int64_t idx, float depth_scale) {
  const float vs = a.voxel_size;
  const bool on = valid && hit;
  const float P[3] = {o[0] + t * dl[0], o[1] + t * dl[1], o[2] + t * dl[2]};
  if (valid && sub == 0) {
    a.depth[idx] = hit ? t * depth_scale : 0.0f;
    if (a.hit) a.hit[idx] = hit ? 1 : 0;
  }
  if (COLOR) {
    // the colour voxel that contains P, found as the march finds its TSDF voxel.  No layer-flag load: the colour pool of a slot without a colour
    // block is all-zero (nvbx_internal.h, "lookups without a layer-flag check"), and weight 0 is "no colour" -- grey 127, the mesh's rule
    const bool mine = sub == RL - 1;
    const int32_t gx = voxel_of(P[0], vs), gy = voxel_of(P[1], vs), gz = voxel_of(P[2], vs);
    const int32_t bx = gx >> 3, by = gy >> 3, bz = gz >> 3;
    const bool need = on && mine;
    const uint32_t h = need ? table_pos(m, bx, by, bz) : 0u;
    const uint4 e = ld_entry(m, h);
    const uint32_t slot = need ? resolve_any(m, pack_key(bx, by, bz), h, e) : SLOT_NONE;
    const uint2 cv = m.color[slot_ok(slot) ? (size_t)slot * 512 + (gz & 7) + 8 * (gy & 7) + 64 * (gx & 7) : 0];
    if (valid && mine) {
      uint32_t rgb = 0u;
      if (hit) rgb = (slot_ok(slot) && __uint_as_float(cv.y) > 0.0f) ? (cv.x & 0x00FFFFFFu) : (127u | (127u << 8) | (127u << 16));
      uint8_t* out = a.color + 3 * idx;
      out[0] = (uint8_t)(rgb & 0xFFu); out[1] = (uint8_t)((rgb >> 8) & 0xFFu); out[2] = (uint8_t)((rgb >> 16) & 0xFFu);
    }
  }
  if (NORMAL) {
    constexpr int NW = 8 / RL;                 // blocks a lane probes
    constexpr int PL = RL < 4 ? RL : 4;        // lanes that fetch corner pairs ...
    constexpr int NP = 4 / PL;                 // ... and pairs each of them fetches
    int32_t b[3] = {0, 0, 0}; float tt[3] = {0.0f, 0.0f, 0.0f};
    const bool ok = on && nvbx_interp_axis(P[0], vs, &b[0], &tt[0]) && nvbx_interp_axis(P[1], vs, &b[1], &tt[1]) && nvbx_interp_axis(P[2], vs, &b[2], &tt[2]);
    const int32_t bx = b[0] >> 3, by = b[1] >> 3, bz = b[2] >> 3;
    const int vx = b[0] & 7, vy = b[1] & 7, vz = b[2] & 7;
    const int cx = vx == 7, cy = vy == 7, cz = vz == 7;
    const int cross = cx | (cy << 1) | (cz << 2);
    // one probe per distinct block: lane `sub` takes blocks sub, sub + RL, ...; first probes of all of them in flight together
    uint32_t sl[NW], hh[NW]; uint4 ee[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const int ob = sub + RL * w;
      const bool need = ok && (ob & ~cross) == 0;
      hh[w] = need ? table_pos(m, bx + (ob & 1), by + ((ob >> 1) & 1), bz + (ob >> 2)) : 0u;
      ee[w] = ld_entry(m, hh[w]);
    }
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const int ob = sub + RL * w;
      const bool need = ok && (ob & ~cross) == 0;
      sl[w] = need ? resolve_any(m, pack_key(bx + (ob & 1), by + ((ob >> 1) & 1), bz + (ob >> 2)), hh[w], ee[w]) : SLOT_NONE;
    }
    // corner pairs (i, j, 0), (i, j, 1): pair q = i + 2j is fetched by lane q % PL
    const uint2* pool = reinterpret_cast<const uint2*>(m.tsdf);
    float f0[NP], f1[NP];
    bool okl = true;
#pragma unroll
    for (int w = 0; w < NP; w++) {
      const bool fetcher = sub < PL;
      const int q = fetcher ? sub + PL * w : 0;
      const int i_ = q & 1, j_ = q >> 1;
      const int ob = (i_ & cx) | ((j_ & cy) << 1);
      const uint32_t s0 = group_slot<RL, NW>(sl, ob, gsh), s1c = group_slot<RL, NW>(sl, ob | 4, gsh);
      const uint32_t s1 = cz ? s1c : s0;
      const int xx = (vx + i_) & 7, yy = (vy + j_) & 7;
      uint2 e0 = make_uint2(0, 0), e1 = make_uint2(0, 0);
      if (fetcher && ok) {
        const size_t v0 = (size_t)s0 * 512 + vz + 8 * yy + 64 * xx;
        if (!cz) {
          if (slot_ok(s0)) { const uint4 p2 = ld_pair(pool + v0); e0 = make_uint2(p2.x, p2.y); e1 = make_uint2(p2.z, p2.w); }
        } else {
          if (slot_ok(s0)) e0 = pool[v0];
          if (slot_ok(s1)) e1 = pool[(size_t)s1 * 512 + 8 * yy + 64 * xx];
        }
        okl = okl && slot_ok(s0) && slot_ok(s1) && __uint_as_float(e0.y) >= RENDER_MIN_WEIGHT && __uint_as_float(e1.y) >= RENDER_MIN_WEIGHT;
      }
      f0[w] = __uint_as_float(e0.x); f1[w] = __uint_as_float(e1.x);
    }
    const uint32_t bad = (uint32_t)((__ballot(!okl) >> gsh) & ((1ull << RL) - 1ull));
    const bool all = ok && bad == 0;
    float c[8];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int src = gsh + (q % PL);
      c[(q & 1) + 2 * (q >> 1)] = RL == 1 ? f0[q / PL] : __shfl(f0[q / PL], src);
      c[(q & 1) + 2 * (q >> 1) + 4] = RL == 1 ? f1[q / PL] : __shfl(f1[q / PL], src);
    }
    if (valid && sub == 0) {
      float g[3] = {0.0f, 0.0f, 0.0f}, nrm[3] = {0.0f, 0.0f, 0.0f};
      if (all) {
        (void)nvbx_interp_trilinear(c, tt[0], tt[1], tt[2], vs, g);
        const float len = NVBX_SQRT((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        if (len > 0.0f) { nrm[0] = NVBX_DIV(g[0], len); nrm[1] = NVBX_DIV(g[1], len); nrm[2] = NVBX_DIV(g[2], len); }
      }
      float* out = a.normal + 3 * idx;
      out[0] = nrm[0]; out[1] = nrm[1]; out[2] = nrm[2];
    }
  }
}

template <int SRC, int RL, bool COLOR, bool NORMAL>
__global__ __launch_bounds__(256) void k_render(DMap m, RenderArgs a) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int sub = lane & (RL - 1);              // sample index within the ray's group
  const int gsh = lane & ~(RL - 1);             // first lane of the group
  constexpr int RPW = 256 / RL;                 // rays per workgroup
  int n_rounds = 0;      // (the march reports its round trips to the occlusion image's instrumentation; not used here)
  if (SRC == SRC_VIEW) {
    // rays -> workgroups and the ray of a pixel: the colour frame's (sphere_trace_camera, nvbx_sphere_trace.h), one camera
    int r, c;
    const bool valid = trace_patch_pixel<RL>((int)blockIdx.x, tid, a.srows, a.scols, &r, &c);
    float dl[3];
    const float dcz = pinhole_ray(a.fu, a.fv, a.cu, a.cv, a.subsample, a.R_LC, valid ? r : 0, valid ? c : 0, dl);
    float t = 0.0f;
    const bool hit = sphere_trace_march<RL>(m, a.t_LC, dl, a.voxel_size, a.trunc, a.max_steps, a.max_len, a.eps_m, valid, sub, gsh, &t, &n_rounds);
    render_epilogue<RL, COLOR, NORMAL>(m, a, a.t_LC, dl, t, hit, valid, sub, gsh, (int64_t)r * a.scols + c, dcz);
  } else {
    // ray i -> lane group i, in caller order; workgroup-uniform grid stride over at most RAYS_GRID_MAX workgroups (the march needs whole wavefronts)
    for (int64_t base = (int64_t)blockIdx.x * RPW; base < a.n; base += (int64_t)gridDim.x * RPW) {
      const int64_t i = base + tid / RL;
      const bool valid = i < a.n;
      float o[3], dl[3];
#pragma unroll
      for (int k = 0; k < 3; k++) { o[k] = valid ? a.origins[3 * i + k] : 0.0f; dl[k] = valid ? a.dirs[3 * i + k] : 0.0f; }
      // a ray that cannot be marched reports "no hit": direction not finite or all-zero, origin not finite or beyond the addressable blocks
      const bool finite = fabsf(dl[0]) < INFINITY && fabsf(dl[1]) < INFINITY && fabsf(dl[2]) < INFINITY &&
                          fabsf(o[0]) < a.origin_lim && fabsf(o[1]) < a.origin_lim && fabsf(o[2]) < a.origin_lim;
      const bool marchable = valid && finite && (dl[0] != 0.0f || dl[1] != 0.0f || dl[2] != 0.0f);
      float t = 0.0f;
      const bool hit = sphere_trace_march<RL>(m, o, dl, a.voxel_size, a.trunc, a.max_steps, a.max_len, a.eps_m, marchable, sub, gsh, &t, &n_rounds);
      render_epilogue<RL, COLOR, NORMAL>(m, a, o, dl, marchable ? t : 0.0f, hit, valid, sub, gsh, valid ? i : 0, 1.0f);
    }
  }
  (void)n_rounds;
}

// Lanes per ray (8, 4, 2 or 1) by ray count, as sphere_trace_lanes() chooses for a batch of cameras (color.hip: 19 200 rays per camera there):
// a few ten thousand rays leave the chip idle and want the latency trick, hundreds of thousands fill it on their own and want fewer
// speculative samples.  NVBX_RENDER_LANES (knobs.render_lanes) forces a value (tools/render_bench.py's A/B).
int render_lanes(const nvbx_mapper* m, int64_t rays) {
  if (m->knobs.render_lanes) return m->knobs.render_lanes;
  return rays >= 6 * 19200 ? 2 : (rays >= 3 * 19200 ? 4 : 8);
}

template <int SRC, int RL>
void launch_flags(nvbx_mapper* m, dim3 grid, const RenderArgs& a) {
  const bool color = a.color != nullptr, normal = a.normal != nullptr;
  if (color && normal) NVBX_LAUNCH(m, (k_render<SRC, RL, true, true>), grid, dim3(256), m->d, a);
  else if (color) NVBX_LAUNCH(m, (k_render<SRC, RL, true, false>), grid, dim3(256), m->d, a);
  else if (normal) NVBX_LAUNCH(m, (k_render<SRC, RL, false, true>), grid, dim3(256), m->d, a);
  else NVBX_LAUNCH(m, (k_render<SRC, RL, false, false>), grid, dim3(256), m->d, a);
}
template <int SRC>
int launch_render(nvbx_mapper* m, int rl, dim3 grid, const RenderArgs& a) {
  if (rl == 8) launch_flags<SRC, 8>(m, grid, a); else if (rl == 4) launch_flags<SRC, 4>(m, grid, a);
  else if (rl == 2) launch_flags<SRC, 2>(m, grid, a); else launch_flags<SRC, 1>(m, grid, a);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

// checks common to both calls + the march's parameters (options: NULL or fields <= 0 / < 0 = the mapper's parameters)
int render_begin(nvbx_mapper* m, const nvbx_render_options* opt, float max_ray_length_m, bool with_color, const char* who, RenderArgs* a) {
  if (tsdf_reader_refused(m, who)) return NVBX_E_INVALID;
  *a = RenderArgs{};
  a->voxel_size = m->p.voxel_size;
  a->trunc = m->p.truncation_distance_vox * m->p.voxel_size;
  a->max_len = max_ray_length_m > 0.0f ? max_ray_length_m : m->p.sphere_tracing_max_ray_length_m;
  a->max_steps = (opt && opt->max_steps > 0) ? opt->max_steps : m->p.sphere_tracing_max_steps;
  a->eps_m = ((opt && opt->surface_distance_epsilon_vox >= 0.0f) ? opt->surface_distance_epsilon_vox : m->p.sphere_tracing_surface_eps_vox) * m->p.voxel_size;
  if (!std::isfinite(a->max_len)) return refuse(who, ": max_ray_length_m is not finite");
  NVBX_HIP(hipSetDevice(m->device));
  // Without a colour output the launch reads TSDF voxels only, which nothing that is held back writes: the held-back work stays held back and
  // the next integrateDepth is still a two-launch pipelined frame (as for the TSDF point query, query.hip).  A colour output reads the colour
  // layer, which a held-back integrateColor writes: that work is carried out first, so the call shows what classic order would show.
  if (with_color ? m->begin_call() : m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  return NVBX_OK;
}

}  // namespace

extern "C" int nvbx_render_view_with(nvbx_mapper* m, const nvbx_render_options* options, const float T_L_C[16], const nvbx_camera* camera, int32_t subsampling,
                                     float max_ray_length_m, float* depth_dev, uint8_t* color_rgb_dev, float* normal_xyz_dev, int64_t capacity_pixels,
                                     int32_t* rows_out, int32_t* cols_out) {
  if (!m || !T_L_C || !camera || !rows_out || !cols_out || subsampling < 0) { set_error("nvbx_render_view: invalid argument"); return NVBX_E_INVALID; }
  if (!nvbx_camera_valid(camera)) { set_error("nvbx_render_view: invalid camera"); return NVBX_E_INVALID; }
  const SubsampledSize ss = subsampled_size(m, subsampling, camera->height, camera->width);
  if (!ss.ok()) { set_error("nvbx_render_view: image too small for the subsampling"); return NVBX_E_INVALID; }
  *rows_out = ss.rows; *cols_out = ss.cols;
  if (capacity_pixels < (int64_t)ss.rows * ss.cols) { set_error("nvbx_render_view: capacity_pixels is smaller than the rendered image"); return NVBX_E_CAPACITY; }
  if (!depth_dev) { set_error("nvbx_render_view: depth_dev is NULL"); return NVBX_E_INVALID; }
  const float reach = max_ray_length_m > 0.0f ? max_ray_length_m : m->p.sphere_tracing_max_ray_length_m;
  if (!nvbx_pose_in_range(T_L_C, m->p.voxel_size * 8.0f, reach)) {
    set_error("nvbx_render_view: T_L_C is not finite or lies outside the addressable block range (+-2^20 blocks)"); return NVBX_E_INVALID; }
  RenderArgs a;
  { const int rc = render_begin(m, options, max_ray_length_m, color_rgb_dev != nullptr, "nvbx_render_view", &a); if (rc) return rc; }
  nvbx_pose_unpack(T_L_C, a.R_LC, a.t_LC);
  a.fu = camera->fu; a.fv = camera->fv; a.cu = camera->cu; a.cv = camera->cv;
  a.subsample = ss.s; a.srows = ss.rows; a.scols = ss.cols;
  a.depth = depth_dev; a.color = color_rgb_dev; a.normal = normal_xyz_dev;
  const int rl = render_lanes(m, (int64_t)ss.rows * ss.cols);
  return launch_render<SRC_VIEW>(m, rl, dim3((unsigned)trace_patch_workgroups(rl, ss.rows, ss.cols)), a);
}

extern "C" int nvbx_render_view(nvbx_mapper* m, const float T_L_C[16], const nvbx_camera* camera, int32_t subsampling, float max_ray_length_m, float* depth_dev,
                                uint8_t* color_rgb_dev, float* normal_xyz_dev, int64_t capacity_pixels, int32_t* rows_out, int32_t* cols_out) {
  return nvbx_render_view_with(m, nullptr, T_L_C, camera, subsampling, max_ray_length_m, depth_dev, color_rgb_dev, normal_xyz_dev, capacity_pixels, rows_out, cols_out);
}

extern "C" int nvbx_cast_rays_with(nvbx_mapper* m, const nvbx_render_options* options, const float* origins_xyz_dev, const float* directions_xyz_dev, int64_t n,
                                   float max_ray_length_m, float* t_dev, uint8_t* hit_dev, uint8_t* color_rgb_dev, float* normal_xyz_dev) {
  if (!m || n < 0 || (n > 0 && (!origins_xyz_dev || !directions_xyz_dev || !t_dev))) { set_error("nvbx_cast_rays: invalid argument"); return NVBX_E_INVALID; }
  if (tsdf_reader_refused(m, "nvbx_cast_rays")) return NVBX_E_INVALID;
  if (n == 0) return NVBX_OK;
  RenderArgs a;
  { const int rc = render_begin(m, options, max_ray_length_m, color_rgb_dev != nullptr, "nvbx_cast_rays", &a); if (rc) return rc; }
  a.origins = origins_xyz_dev; a.dirs = directions_xyz_dev; a.n = n;
  a.origin_lim = nvbx_pose_limit(m->p.voxel_size * 8.0f, a.max_len);        // (nvbx_pose_in_range's bound, per ray)
  if (!(a.origin_lim > 0.0f)) { set_error("nvbx_cast_rays: max_ray_length_m reaches beyond the addressable block range (+-2^20 blocks)"); return NVBX_E_INVALID; }
  a.depth = t_dev; a.hit = hit_dev; a.color = color_rgb_dev; a.normal = normal_xyz_dev;
  const int rl = render_lanes(m, n);
  const int64_t rpw = 256 / rl;
  return launch_render<SRC_RAYS>(m, rl, dim3((unsigned)std::min<int64_t>((n + rpw - 1) / rpw, RAYS_GRID_MAX)), a);
}

extern "C" int nvbx_cast_rays(nvbx_mapper* m, const float* origins_xyz_dev, const float* directions_xyz_dev, int64_t n, float max_ray_length_m, float* t_dev,
                              uint8_t* hit_dev, uint8_t* color_rgb_dev, float* normal_xyz_dev) {
  return nvbx_cast_rays_with(m, nullptr, origins_xyz_dev, directions_xyz_dev, n, max_ray_length_m, t_dev, hit_dev, color_rgb_dev, normal_xyz_dev);
}
