// tsdf.hip -- MultiMapper::integrateDepth on MI355X: the projective TSDF update and the depth-frame state machine that camera frames, camera
// batches, two mappers' pairs and LiDAR scans (lidar.hip) run through.
//
// Two launches per depth frame, no host round trip in between:
//   k_mark_view      the view calculation (nvbx_view.h): the blocks in view of the frame, allocated if new, listed once each.
//   k_integrate_tsdf one 512-thread workgroup (8 wave64) per 8^3 block, grid-striding over the device-resident view
//                    list of {slot, Index3D} records; lane = voxel in z + 8y + 64x order, so every wave reads/writes
//                    512 contiguous bytes.
// Both kernels are templated on the depth source (f32 metres / u16 millimetres) and on the sensor model.  Held-back calls ride in the two
// launches (pipelined order, DESIGN.md 2.8: k_integrate_tsdf_color); nvbx_integrate_depth_pair runs two mappers' launches in one grid each
// (k_mark_view_pair, k_integrate_tsdf_color_pair).  The LiDAR-only launches are in lidar.hip, the multi-GPU measurement exchange in measure.hip.
// Reference semantics restated: [U] ProjectiveTsdfIntegrator (call sites nvblox_ros/src/lib/nvblox_node.cpp:1062 camera, :1382-1384 LiDAR;
// knobs mapper_initialization.cpp:264-358).
#define NVBX_WGT_HERE
#include "nvbx_view.h"

// the per-workgroup time stamps of every translation unit that records (nvbx_view.h NVBX_T), in one buffer: slot i of workgroup blockIdx.x of kernel k
#ifdef NVBX_WG_TIMES
constexpr int WGT_MAX_WG = 8192, WGT_SLOTS = 8;
static unsigned long long* g_wgt_host = nullptr;
extern "C" int nvbx_debug_wg_times(unsigned long long* out_host, int64_t n_words) {
  const size_t total = (size_t)2 * WGT_MAX_WG * WGT_SLOTS;
  if (!g_wgt_host) {
    if (hipMalloc(&g_wgt_host, total * 8) != hipSuccess) return -1;
    (void)hipMemset(g_wgt_host, 0, total * 8);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wgt), &g_wgt_host, sizeof(g_wgt_host));
    (void)wgt_bind_lidar(g_wgt_host);
  }
  if (out_host) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(out_host, g_wgt_host, std::min<size_t>(total, (size_t)n_words) * 8, hipMemcpyDeviceToHost);
    (void)hipMemset(g_wgt_host, 0, total * 8);
  }
  return (int)WGT_MAX_WG;
}
#endif

// Two mappers' view-marking launches in ONE grid (nvbx_integrate_depth_pair: the background and the foreground mapper of a MultiMapper's dynamic / human
// mapping types take the same depth frame, split by a mask, one after the other -- four dependent launches of 6-8 us each for two small jobs).  A workgroup
// runs mapper a's body or mapper b's, numbered from that mapper's own 0 (n_tiles tiles, then its riders; n_wg in all); nothing is shared between the two maps.
template <typename Img> struct MarkViewArgs { DMap m; FrameSet<Img, 1> fs; int4* view_list; int32_t list_cap, reset_esdf_dirty, n_edt_wg; EsdfArgs ea; TraceRiderT<1> tr; int32_t n_tiles, n_wg; };
template <typename Img>
__global__ __launch_bounds__(CameraSensor::kThreads) void k_mark_view_pair(MarkViewArgs<Img> a, MarkViewArgs<Img> b) {
  extern __shared__ __align__(16) unsigned char smem[];
  // dispatch order [a's tiles][b's tiles][a's riders][b's riders]: the tiles are each map's longest chain (~9 us) and start first (measured against
  // [all of a][all of b]: 11.4 against 11.6 us -- within the noise; kept because it is the order a single mapper's launch has).  Every segment is a
  // multiple of 8 long.
  const int32_t g = (int32_t)blockIdx.x, at = a.n_tiles, bt = b.n_tiles, ar = a.n_wg - a.n_tiles;
  bool is_a; int32_t wg;
  if (g < at) { is_a = true; wg = g; }
  else if (g < at + bt) { is_a = false; wg = g - at; }
  else if (g < at + bt + ar) { is_a = true; wg = at + (g - at - bt); }
  else { is_a = false; wg = bt + (g - at - bt - ar); }
  if (is_a) mark_view_body<Img, CameraSensor, 1>(a.m, a.fs, CameraSensor{}, a.view_list, a.list_cap, a.reset_esdf_dirty, a.n_edt_wg, a.ea, a.tr, wg, smem);
  else mark_view_body<Img, CameraSensor, 1>(b.m, b.fs, CameraSensor{}, b.view_list, b.list_cap, b.reset_esdf_dirty, b.n_edt_wg, b.ea, b.tr, wg, smem);
}
static_assert(2 * sizeof(MarkViewArgs<DepthF32>) <= 4096, "k_mark_view_pair: kernel arguments");

// A wave-uniform value the inner loop uses as a VALU operand, parked in a vector register: the LiDAR instantiation needs ~100 scalar
// registers, the 8-waves-per-SIMD budget leaves 72, and every use of a spilled one is a v_readlane in the per-voxel path.
template <typename T> __device__ inline T in_vgpr(T x) { asm volatile("" : "+v"(x)); return x; }

// Dependent-access chain: {view count, view record} -> {depth gather, voxel} -> store.  The record of the first block
// is fetched speculatively beside the count, the voxel is fetched before the projection decides whether it is needed,
// and the flag / dirty-list atomics of lane 0 are issued first and consumed last.
// Occupancy: 8 waves per SIMD (four of these workgroups per CU) is asked for explicitly -- the kernel's ~100 scalar registers would
// otherwise cost the eighth wave, and on the LiDAR map (112 k blocks per scan) residency is throughput; the grid is exactly the 1024
// workgroups that are then resident together (tools/integ_grid_sweep.sh: 768 / 1024 workgroups at 6 waves 499 / 569 us, 1024 at 8 waves 430-470).
// Plain = every camera of the launch is frame_is_plain() (nvbx_internal.h): the occupancy / weighting-mode / decay switches fold away
// at compile time -- same arithmetic, 12 % fewer issue cycles on the LiDAR launch (tools/variant_ab.sh).
template <typename Img, typename Sensor, int NB, bool Plain>
__device__ inline void integrate_tsdf_worker(const DMap& m, const FrameSet<Img, NB>& fs, const Sensor& sensor, const int4* view_list, int32_t list_cap,
                                             int32_t mesh_list, int32_t* view_export, int32_t view_export_cap, int32_t spec_lanes, const uint8_t* view_class,
                                             const int32_t wgi, const int32_t n_wg, const int32_t* dense_list = nullptr) {
  const Frame& f0 = fs.f[0];
  const int tid = threadIdx.x, lane = tid & 63;
  // The view records are taken 64 at a time: lane j of every wavefront fetches the record of the j-th block this workgroup will
  // process next (speculatively, beside the count) and transforms that block's origin into the sensor frame; the block loop then
  // reads slot and origin out of lane j (v_readlane: scalar operands from there on).  The record fetch leaves the per-block
  // dependent chain and the 3 x 3 transform is paid once per block and wavefront instead of once per voxel.
  // Only the first `spec_lanes` lanes fetch speculatively (a host hint: the view count the GPU last reported / the grid, + 1): a camera
  // frame has ~300 blocks in view and about as many workgroups, so one record per wavefront is wanted -- 64 speculative 16-B records from
  // each of 8 x 1024 wavefronts were 8 MB of HBM traffic for 3.5 MB of work (PMC, profiles/r02z_pmc.json).  A lane the hint left out
  // fetches once the count is known (a dependent load, only when the view grew by more than the hint's margin).
  // which records this workgroup takes: runs of consecutive records (neighbouring blocks: the same patch of the depth image) stay on one XCD's L2
  // (xcd_chunked, nvbx_internal.h); the LiDAR work list is dealt out per shard already
  const int32_t wgr = dense_list ? wgi : xcd_chunked(wgi, n_wg);
  int32_t mine = wgr + lane * n_wg;
  int4 rec = (!dense_list && lane < spec_lanes && mine < list_cap) ? view_list[mine] : make_int4((int32_t)SLOT_NONE, 0, 0, 0);
  int32_t n = m.counters[C_VIEW_COUNT + (f0.frame_id & 3)];
  if (n > list_cap) n = list_cap;
  if (wgi == 0 && tid == 192) __hip_atomic_store(&m.host_mirror[2], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);     // next launch's hint (the VIEW count)
  // LiDAR behind the beam-centric launch: that launch has left the records it did NOT take as a work list (indices into the view list, one
  // region per shard) -- this launch deals THOSE out, so every workgroup gets the same number of blocks.  Dealing out the whole view list and
  // skipping the taken records (60 %) left a workgroup with Binomial(110, 0.4) blocks: 44 +- 5, the slowest of 1024 with ~60.
  int32_t dpre[NSH + 1];
  auto dense_at = [&](int32_t k) -> int32_t {          // (selects only: a dynamically indexed dpre[] would live in scratch memory)
    int sh = 0; int32_t base = 0;
#pragma unroll
    for (int q = 1; q < NSH; q++) if (k >= dpre[q]) { sh = q; base = dpre[q]; }
    return dense_list[(size_t)sh * list_cap + (k - base)];
  };
  if (dense_list) {
    int32_t c[NSH];
#pragma unroll
    for (int q = 0; q < NSH; q++) c[q] = *shc_at(m, S_LIDAR_SPARSE, q, 1);
    dpre[0] = 0;
#pragma unroll
    for (int q = 0; q < NSH; q++) dpre[q + 1] = dpre[q] + min(c[q], list_cap);
    n = dpre[NSH];
    if (mine < n) rec = view_list[dense_at(mine)];
  } else {
    if (lane >= spec_lanes && mine < n) rec = view_list[mine];
    // (LiDAR without the work list: blocks the beam-centric launch k_lidar_sparse has already updated are skipped -- their record reads as "no slot")
    if (view_class && mine < n && view_class[mine]) rec.x = (int32_t)SLOT_NONE;
  }
  // nvbx_set_view_export: the frame's block indices also go to a caller-owned packed buffer [1 + cap][3] (row 0 = count) --
  // the message of the multi-GPU exchange, written here instead of by an export launch
  if (view_export && wgi == 0 && tid == 0) { view_export[0] = min(n, view_export_cap); view_export[1] = 0; view_export[2] = 0; }
  // pool growth: the free-slot count after this frame's allocations goes to pinned host memory (not waited for)
  if (wgi == 0 && tid == 64) __hip_atomic_store(&m.host_mirror[0], m.counters[C_FREE_TOP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (wgi == 0 && tid == 128) __hip_atomic_store(&m.host_mirror[1], m.counters[C_HIGH_WATER], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const int vx = tid >> 6, vy = (tid >> 3) & 7, vz = tid & 7;
  float off0[3] = {0.0f, 0.0f, 0.0f};
  if (NB == 1) sensor_voxel_offset(f0, vx, vy, vz, off0);          // (a batch rotates the offset per camera inside the loop)
  // LiDAR: the image geometry the four-tap gather needs per voxel lives in vector registers (see in_vgpr)
  Frame fl = f0; Img img0 = fs.img[0];
  if (Sensor::kLongRays && NB == 1) { fl.cols = in_vgpr(f0.cols); fl.rows = in_vgpr(f0.rows); img0.p = in_vgpr(fs.img[0].p); }
  for (int32_t i0 = wgr; i0 < n; i0 += 64 * n_wg) {
    if (i0 != wgr) {
      mine = i0 + lane * n_wg;
      if (dense_list) rec = mine < n ? view_list[dense_at(mine)] : make_int4((int32_t)SLOT_NONE, 0, 0, 0);
      else {
        rec = mine < n ? view_list[mine] : make_int4((int32_t)SLOT_NONE, 0, 0, 0);
        if (view_class && mine < n && view_class[mine]) rec.x = (int32_t)SLOT_NONE;
      }
    }
    if (view_export && tid < 64 && mine < n && mine < view_export_cap) { int32_t* e = view_export + 3 * (1 + (int64_t)mine); e[0] = rec.y; e[1] = rec.z; e[2] = rec.w; }
    float org[3] = {0.0f, 0.0f, 0.0f};
    if (NB == 1) sensor_block_origin(f0, rec.y, rec.z, rec.w, org);
#pragma unroll 1
    for (int32_t j = 0; j < 64 && i0 + j * n_wg < n; j++) {               // (uniform)
      const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane(rec.x, j);               // pool slot (stable across hash rebuilds)
      if (!slot_ok(slot)) continue;
      float2* vp = &m.tsdf[(size_t)slot * 512 + tid];
      const float2 cur_c = *vp;
      // batch: which cameras had this block in view = the mask k_mark_view left in the entry's stamp (uniform per block)
      uint32_t cams = 1u;
      if (NB > 1) cams = __builtin_amdgcn_readfirstlane(m.table[m.slot_entry[slot]].stamp & 0xFFu);
      uint32_t old = 0;
      if (tid == 0) old = atomicOr(&m.slot_flags[slot], F_TSDF | F_DIRTY_ESDF | F_DIRTY_MESH | ((Sensor::kLongRays && (Plain || !f0.occupancy)) ? F_BAND_STALE : 0u));
      if (!Sensor::kLongRays && tid == 64) m.slot_cam[slot] = (f0.frame_id << 8) | cams;       // the camera view decayTsdfExcludeLastView<Camera> spares
      const int32_t bx = __builtin_amdgcn_readlane(rec.y, j), by = __builtin_amdgcn_readlane(rec.z, j), bz = __builtin_amdgcn_readlane(rec.w, j);
      float2 fin = cur_c;            // the voxel as this launch leaves it: the cameras' updates applied in order, exactly as separate calls would
      bool touched = false;
#pragma unroll 1
      for (int c = 0; c < (NB > 1 ? fs.n : 1); c++) {
        if (NB > 1 && !((cams >> c) & 1u)) continue;       // uniform
        const Frame& f = (Sensor::kLongRays && NB == 1) ? fl : fs.f[c];
        const Img& img = (Sensor::kLongRays && NB == 1) ? img0 : fs.img[c];
        float pc[3];
        if (NB == 1) {
          pc[0] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(org[0]), j)) + off0[0];
          pc[1] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(org[1]), j)) + off0[1];
          pc[2] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(org[2]), j)) + off0[2];
        } else {
          float o[3], d[3];
          sensor_block_origin(f, bx, by, bz, o); sensor_voxel_offset(f, vx, vy, vz, d);
          pc[0] = o[0] + d[0]; pc[1] = o[1] + d[1]; pc[2] = o[2] + d[2];
        }
        float ds = 0.0f, vd = 0.0f;
        const int got = sensor.sample(f, img, pc, &ds, &vd);
        if (Plain) {
          if (got > 0 && tsdf_fuse_plain(f, &fin, ds, vd)) touched = true;
        } else if (f.occupancy) {     // occupancy mapper: the pool holds log-odds (nvbx_internal.h occupancy_update)
          if (got > 0) { fin = make_float2(occupancy_update(f, fin.x, ds, vd), 0.0f); touched = true; }
        } else {
          if (got < 0 && f.invalid_decay >= 0.0f) { fin = make_float2(fin.x, fin.y * f.invalid_decay); touched = true; }
          if (got > 0 && tsdf_fuse(f, &fin, ds, vd)) touched = true;
        }
      }
      if (touched) *vp = fin;
      if (Plain || !f0.occupancy) {
        // band vote for the colour integrator (F_BAND, nvbx_internal.h): exact, so set AND cleared here, one bit per wavefront
        if (!Sensor::kLongRays) {      // (LiDAR: marked stale above instead)
          // one workgroup per block and a few hundred blocks: a block-wide vote and ONE atomic are cheaper here than a bit per wavefront
          const int any_band = __syncthreads_or(in_band(fin.x, fin.y, f0.trunc) ? 1 : 0);
          if (tid == 0) { if (any_band) atomicOr(&m.slot_flags[slot], F_BAND); else atomicAnd(&m.slot_flags[slot], ~F_BAND); if (old & F_BAND_STALE) atomicAnd(&m.slot_flags[slot], ~F_BAND_STALE); }
        }
      }
      if (tid == 0) {
        if (!(old & F_DIRTY_ESDF)) list_append(m, S_LIST_ESDF_DIRTY, (int32_t)slot);
        if (!(old & F_DIRTY_MESH)) list_append(m, mesh_list, (int32_t)slot);
      }
    }
  }
}
template <typename Img, typename Sensor, int NB, bool Plain>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_integrate_tsdf(DMap m, FrameSet<Img, NB> fs, Sensor sensor, const int4* view_list, int32_t list_cap,
                                                        int32_t mesh_list, int32_t* view_export, int32_t view_export_cap, int32_t spec_lanes, const uint8_t* view_class,
                                                        const int32_t* dense_list) {
  NVBX_INV_WRITER_BEGIN(m);
  integrate_tsdf_worker<Img, Sensor, NB, Plain>(m, fs, sensor, view_list, list_cap, mesh_list, view_export, view_export_cap, spec_lanes, view_class, (int32_t)blockIdx.x, (int32_t)gridDim.x, dense_list);
  NVBX_INV_WRITER_END(m);
}

// Pipelined order, fused: TSDF update of frame i + 1, colour integration of frame i (from the candidate records the riders
// of the view-marking launch discovered) and the distance transform of ESDF update i in ONE launch -- two launches per frame:
//   k_mark_view            view marking (i+1) || sphere tracing (i) || colour candidates (i) || ESDF site marking (i)
//   k_integrate_tsdf_color TSDF update (i+1)  || colour integration (i)                      || distance transform (i)
// What makes the three parts of this launch independent: the colour workers read no block flag (their candidates were fixed before the
// launch: the TSDF update rewrites F_BAND beside them) and no TSDF voxel; the distance transform reads the site masks of a marking pass that
// has finished (previous launch) and writes ESDF voxels only; the update appends to an ESDF-dirty list that pass has emptied.  Every part
// reads exactly the state separate calls would have shown it.
// Workgroups: [distance transform (512 threads = 8 wavefronts per ESDF block)][TSDF update][colour].
// (occupancy: the compiler's own register choice gives 3 of these 8-wavefront workgroups per CU -- 768 resident of the ~1 080 a frame launches, so the
//  colour workgroups, dispatched last, start late; asking for four per CU with amdgpu_waves_per_eu(8, 8) was measured in round 4: the colour part
//  starts at once but every part runs slower, the launch 9.2 -> 10.0 us -- left at the compiler's choice)
template <typename Img, typename Pix, int NB, bool Plain>
__device__ __forceinline__ void integrate_tsdf_color_body(const DMap& m, const FrameSet<Img, NB>& fs, const CameraSensor& sensor, const int4* view_list, int32_t list_cap,
                                                          int32_t mesh_list, int32_t* view_export, int32_t view_export_cap, int32_t spec_lanes, int32_t n_tsdf_wg,
                                                          const FrameSetC<Pix, NB>& fsc, const float* synth, int32_t srows, int32_t scols, const int4* cand, int32_t cand_cnt_idx,
                                                          int32_t n_edt_wg, const EsdfArgs& ea, const ImportArgs& imp, const int32_t b, const int32_t n_wg_total, unsigned char* smem) {
  NVBX_T(1, 0);
  if (b < n_edt_wg) { esdf_edt_worker<512>(m, ea, (int)b, n_edt_wg, reinterpret_cast<EdtShared*>(smem)); NVBX_T(1, 1); NVBX_T(1, 7); return; }
  if (b < n_edt_wg + n_tsdf_wg) {
    NVBX_INV_WRITER_BEGIN(m);
    integrate_tsdf_worker<Img, CameraSensor, NB, Plain>(m, fs, sensor, view_list, list_cap, mesh_list, view_export, view_export_cap, spec_lanes, nullptr, b - n_edt_wg, n_tsdf_wg);
    NVBX_INV_WRITER_END(m);
    NVBX_T(1, 2); NVBX_T(1, 7);
    return;
  }
  // (multi-GPU, imp.n_wg > 0: the LAST workgroups resolve the peers' gathered block lists into ESDF-dirty flags, nvbx_esdf_mark.h)
  const int32_t n_color_wg = n_wg_total - n_edt_wg - n_tsdf_wg - imp.n_wg;
  if (b >= n_edt_wg + n_tsdf_wg + n_color_wg) { esdf_import_dirty_worker(m, imp, (int64_t)(b - n_edt_wg - n_tsdf_wg - n_color_wg) * 512 + threadIdx.x, (int64_t)imp.n_wg * 512); return; }
  color_integrate_list_worker<Pix, NB>(m, fsc, synth, srows, scols, mesh_list, cand, cand_cnt_idx, b - n_edt_wg - n_tsdf_wg, n_color_wg);
  NVBX_T(1, 3); NVBX_T(1, 7);
}
template <typename Img, typename Pix, int NB, bool Plain>
__global__ __launch_bounds__(512) NVBX_FUSED_ATTR void k_integrate_tsdf_color(DMap m, FrameSet<Img, NB> fs, CameraSensor sensor, const int4* view_list, int32_t list_cap,
                                                              int32_t mesh_list, int32_t* view_export, int32_t view_export_cap, int32_t spec_lanes, int32_t n_tsdf_wg,
                                                              FrameSetC<Pix, NB> fsc, const float* synth, int32_t srows, int32_t scols, const int4* cand, int32_t cand_cnt_idx,
                                                              int32_t n_edt_wg, EsdfArgs ea, ImportArgs imp) {
  __shared__ __align__(16) unsigned char smem[sizeof(EdtShared)];
  integrate_tsdf_color_body<Img, Pix, NB, Plain>(m, fs, sensor, view_list, list_cap, mesh_list, view_export, view_export_cap, spec_lanes, n_tsdf_wg, fsc, synth, srows, scols, cand, cand_cnt_idx,
                                                 n_edt_wg, ea, imp, (int32_t)blockIdx.x, (int32_t)gridDim.x, smem);
}
// ... and two mappers' fused TSDF-update launches in one grid (nvbx_integrate_depth_pair, see k_mark_view_pair): mapper a's [distance transform][TSDF
// update][colour][union step] workgroups, then mapper b's, each numbered from its own 0.  The general (not "plain") arithmetic path for both.
template <typename Img, typename Pix> struct FusedArgs {
  DMap m; FrameSet<Img, 1> fs; const int4* view_list; int32_t list_cap, mesh_list; int32_t* view_export; int32_t view_export_cap, spec_lanes, n_tsdf_wg;
  FrameSetC<Pix, 1> fsc; const float* synth; int32_t srows, scols; const int4* cand; int32_t cand_cnt_idx, n_edt_wg; EsdfArgs ea; ImportArgs imp; int32_t n_wg; };
template <typename Img, typename Pix>
__global__ __launch_bounds__(512) void k_integrate_tsdf_color_pair(FusedArgs<Img, Pix> a, FusedArgs<Img, Pix> b) {
  __shared__ __align__(16) unsigned char smem[sizeof(EdtShared)];
  // dispatch order: mapper a's workgroups, then mapper b's (dealing the parts out alternately -- transforms, updates, colour -- measured slower: 9.5 -> 10.4 us;
  // about 770 of these 8-wavefront workgroups are resident at a time, so what matters is how MANY there are: the second mapper brings few, see the host side)
  const int32_t g = (int32_t)blockIdx.x;
  const bool is_a = g < a.n_wg; const int32_t wg = is_a ? g : g - a.n_wg;
  if (is_a)
    integrate_tsdf_color_body<Img, Pix, 1, false>(a.m, a.fs, CameraSensor{}, a.view_list, a.list_cap, a.mesh_list, a.view_export, a.view_export_cap, a.spec_lanes, a.n_tsdf_wg, a.fsc, a.synth, a.srows,
                                                  a.scols, a.cand, a.cand_cnt_idx, a.n_edt_wg, a.ea, a.imp, wg, a.n_wg, smem);
  else
    integrate_tsdf_color_body<Img, Pix, 1, false>(b.m, b.fs, CameraSensor{}, b.view_list, b.list_cap, b.mesh_list, b.view_export, b.view_export_cap, b.spec_lanes, b.n_tsdf_wg, b.fsc, b.synth, b.srows,
                                                  b.scols, b.cand, b.cand_cnt_idx, b.n_edt_wg, b.ea, b.imp, wg, b.n_wg, smem);
}
static_assert(2 * sizeof(FusedArgs<DepthF32, PixRgb8>) <= 4096, "k_integrate_tsdf_color_pair: kernel arguments");
// (a depth batch AND a colour batch in one argument block: the 4 KiB kernel-argument limit is why the colour path's frames are FrameCore)
static_assert(sizeof(DMap) + sizeof(FrameSet<DepthF32, MAX_BATCH>) + sizeof(FrameSetC<PixRgb8, MAX_BATCH>) + sizeof(EsdfArgs) + sizeof(ImportArgs) + 160 <= 4096, "k_integrate_tsdf_color<.., MAX_BATCH>: kernel arguments");

// ---- One depth frame's two launches, in STEPS (round 6): integrate_depth_impl runs them in order for one mapper; nvbx_integrate_depth_pair interleaves the
// steps of TWO mappers around two shared launches (k_mark_view_pair, k_integrate_tsdf_color_pair).  The steps are the former body of integrate_depth_impl, cut
// where it launches; what each step does to the mapper's host state, and in which order, is unchanged.
static bool fused_colour_applies(const nvbx_mapper* m) {
  // (knobs.fuse_colc -- A/B: 0 = three launches per frame)
  return m->knobs.fuse_colc && m->p.projective_layer_type != 1 && m->p.esdf_mode == 0 && m->p.esdf_propagation == 0 && !m->lidar_integrated && m->capacity <= (1ll << 24);
}
template <int NB> struct DepthSteps {
  int tiles = 0, edt_wg = 0; EsdfArgs ea{}; TraceRiderT<NB> tr{};                 // launch 1
  bool plain = true, has_color = false, pipelined = false, fused = false;
  HeldColorFrames<NB> col{};      // launch 2 (fused form): the held-back colour frame(s), if any
  int grid = 8; int32_t spec_lanes = 1;
  int32_t n_edt = 0; EsdfArgs ea_edt{}; const int4* cand = nullptr; int32_t cand_idx = 0; int cgrid = 0; ImportArgs imp{};
  nvbx_mapper::ModeScope pipelined_order;      // the mapper's flag: on in step 1, off in step 2 -- or wherever the frame is given up in between
};
// step 1: everything in front of the view-marking launch (ray grid, riders of the held-back calls, the fence report)
template <typename Img, typename Sensor, int NB>
static int depth_step_before_mark_view(nvbx_mapper* m, FrameSet<Img, NB>& fs, DepthSteps<NB>& st) {
  size_ray_grid(fs);
  const Frame& f = fs.f[0];
  st.tiles = mark_view_tile_wgs<Sensor>(f) * fs.n;       // tile workgroups (padded: the groups of one XCD are a contiguous band, k_mark_view); camera after camera
  // a held-back EDT rides in this launch (camera: 256-thread workgroups); the LiDAR launch is 64 threads wide, so flush first
  st.edt_wg = 0; st.ea = m->held.edt_args;
  if (m->held.edt_pending) {
    if (Sensor::kRiders) { st.edt_wg = 256; m->held.edt_pending = false; }        // (256 .. 1024 riders measured: no difference, profiles/r02x_kernel_isolation.txt)
    else if (m->flush_edt()) return NVBX_E_DEVICE;
  }
  // Colour deferral: a held-back integrateColor (and an updateEsdf behind it) is carried out in PIPELINED order -- its sphere tracing rides
  // in this view-marking launch, its colour integration + ESDF marking follow, then this frame's TSDF update: three launches per frame.
  // Or TWO (fused, k_integrate_tsdf_color above): the colour frame's candidate blocks are discovered and the ESDF marking pass runs as
  // riders of this view-marking launch too, and colour integration, the update's distance transform and this frame's TSDF update share
  // the second launch.
  // A held-back updateEsdf with NO colour frame in front (depth-only hosts, occupancy mappers) is carried the same way: marking pass here,
  // distance transform in the second launch, no colour workgroups.
  st.tr = TraceRiderT<NB>{};
  st.plain = true;
  for (int c = 0; c < fs.n; c++) st.plain = st.plain && frame_is_plain(fs.f[c]);
  st.has_color = m->held.color_pending.on;
  // (one frame carries a frame, a batch a batch; a held-back updateEsdf WITHOUT a colour frame -- depth-only and occupancy mappers -- is carried by
  //  any camera launch: integrate_cameras has checked that the two-launch order applies, nvbx_mapper::esdf_only_carry)
  st.pipelined = Sensor::kRiders && (st.has_color ? m->held.color_pending.carried_by(NB) : m->held.esdf_update_pending);
  st.fused = false;
  if (st.pipelined) {
    // TSDF mapper (with or without a freespace layer), 2-D ESDF by the exact transform (the marking pass / distance transform that ride are the
    // 2-D ones), no multi-GPU union step waiting for the colour launch, and no block that may be F_BAND_STALE (the candidate riders read the
    // band flags only)
    st.fused = st.has_color ? fused_colour_applies(m)
                            : true;      // (no colour: no candidates, no band flags -- esdf_only_carry has checked the rest)
    // (a distance transform armed outside the pipeline must precede the marking pass that rides in this launch: its own launch, rare)
    if (st.fused && st.edt_wg) { m->held.edt_pending = true; st.edt_wg = 0; if (m->flush_edt()) return NVBX_E_DEVICE; }
    st.pipelined_order.enter(m->pipelined_order);
    if (st.has_color) { const int rc = m->pending_color_trace_rider<NB>(&st.tr); if (rc) return rc; }
    // riders before or after the tiles (A/B: NVBX_MARK_TILES_FIRST = 0 / 1).  One frame: tiles first (15.2 vs 15.8 us).  A batch of 8: riders first
    // (32.4 vs 42.0 us) -- its 2 688 single-wavefront tile workgroups, each holding its LDS key set, take most of the workgroup slots, and
    // sphere-tracing workgroups dispatched behind them start when the tiles are done: the launch took the SUM of its parts.
    const bool tiles_first = m->knobs.mark_tiles_first >= 0 ? m->knobs.mark_tiles_first != 0 : NB == 1;
    if (tiles_first) st.tr.n_tile_wg = st.tiles;
    if (st.fused && !st.has_color) m->pending_marking_args(&st.tr.n_mark_wg, &st.ea, NB == 1);
    if (st.fused && st.has_color) {
      if (m->color_cand.ensure(m->stream, (size_t)m->capacity * 2 * sizeof(int4))) return NVBX_E_DEVICE;      // (the capacity only grows: the buffer is [2][capacity])
      const int64_t hw_seen = std::max<int64_t>(1, __atomic_load_n(&m->h_mirror[1], __ATOMIC_RELAXED));
      st.tr.n_scan_wg = (int32_t)std::min<int64_t>(256, 8 * ((hw_seen + hw_seen / 4 + 64 + 2047) / 2048));      // 256 slots per workgroup and pass; a hint only (the riders grid-stride)
      st.tr.cand = m->color_cand.as<int4>() + (size_t)m->cand_parity * (size_t)m->capacity;
      st.tr.cand_cnt_idx = C_CAND_COUNT + m->cand_parity; st.tr.cand_reset_idx = C_CAND_COUNT + (1 - m->cand_parity);
      m->cand_parity ^= 1;      // (the next fused launch resets THIS count, whether or not the colour launch below is reached: an error return in between leaves no stale candidates behind)
      m->pending_marking_args(&st.tr.n_mark_wg, &st.ea, NB == 1);        // (the held-back integrateColor's marking pass, in call order: before its colour integration below)
    }
  }
  st.tr.fence_report = m->next_fence_report();
  return NVBX_OK;
}
// a launch grid sized from the count the GPU last reported keeps a margin over it: 25 % + 64 is what a view that grows while exploring needs
// (NVBX_GRID_MARGIN="percent,blocks": A/B only -- tools/env_ab.sh)
static int64_t with_grid_margin(const nvbx_mapper* m, int64_t n) { return n + n * m->knobs.grid_margin_pct / 100 + m->knobs.grid_margin_blocks; }
// step 2: between the two launches -- the host-side steps of the held-back calls, then the sizes of the TSDF-update part
template <typename Sensor, int NB>
static int depth_step_between(nvbx_mapper* m, DepthSteps<NB>& st) {
  if (st.pipelined) {
    // the host-side steps of the held-back calls, in call order: integrateColor (its marking pass empties the dirty list itself, the EDT
    // of the update keeps it -- EsdfArgs), then updateEsdf (which only arms the next held-back EDT: the marking pass has been launched)
    if (!st.fused) m->premark_consumed = false;
    int rc = NVBX_OK;
    if (st.fused) { if (st.has_color) rc = m->pending_color_fused_args<NB>(&st.col); }
    else rc = m->launch_pending_color_after_trace();
    if (rc == NVBX_OK && m->held.esdf_update_pending) { m->held.esdf_update_pending = false; rc = nvbx_update_esdf(m); }
    st.pipelined_order.leave();
    if (rc) return rc;
  }
  m->premark_consumed = false; m->dirty_since_mark = true;
  // grid-stride over the view list: exactly the 1024 workgroups that are resident together (4 per CU)
  // (a camera BATCH: 512 -- its fused launch is residency-bound, 1 024 eight-wavefront workgroups resident, and 1 024 TSDF workgroups in front kept the colour
  //  part waiting: 4 / 8 cameras 0.0382 / 0.0560 -> 0.0365 / 0.0547 ms per step, tools/fused_grid_sweep.sh)
  const int grid_cap = m->knobs.integ_grid > 0 ? m->knobs.integ_grid : (NB > 1 ? 512 : 1024);    // (NVBX_INTEG_GRID: tools/integ_grid_sweep.sh, tools/fused_grid_sweep.sh)
  // ... or fewer when the view is smaller: sized from the view count of the last launch the GPU has finished (pinned host memory, not
  // waited for) + 25 % + 64; a hint only -- the kernel grid-strides over whatever the count turns out to be
  // (no launch finished yet -- a new or just cleared map: the full grid; sized for 64 blocks, the first scans of a LiDAR map, enqueued faster
  //  than the first finishes, took 1.7 ms each for their 112 k blocks: the whole of round 4's first "exploring" LiDAR figure)
  const int64_t n_hint = std::max<int64_t>(0, __atomic_load_n(&m->h_mirror[2], __ATOMIC_RELAXED));
  const int64_t n_want = with_grid_margin(m, n_hint);
  const int64_t want = n_hint == 0 ? (int64_t)grid_cap : ((n_want + 7) / 8) * 8;
  st.grid = (int)std::max<int64_t>(8, std::min<int64_t>(std::min<int64_t>(m->capacity, grid_cap), want));
  st.spec_lanes = (int32_t)std::min<int64_t>(64, (n_want + st.grid - 1) / st.grid);
  return NVBX_OK;
}
// step 3 (fused form): the riders of the TSDF-update launch
// [distance transform the held-back updateEsdf has just armed][TSDF update of this frame][colour integration of the held-back frame]
template <int NB>
static void depth_step_fused_riders(nvbx_mapper* m, DepthSteps<NB>& st) {
  st.n_edt = 0; st.ea_edt = m->held.edt_args;
  if (m->held.edt_pending) { st.n_edt = m->knobs.edt_riders; m->held.edt_pending = false; }      // (NVBX_EDT_RIDERS -- A/B; a multiple of 8, at least 8)
  st.cand = st.tr.cand;
  st.cand_idx = st.tr.cand_cnt_idx;
  const int64_t c_hint = std::max<int64_t>(0, __atomic_load_n(&m->h_mirror[3], __ATOMIC_RELAXED));         // candidates of the last colour frame the GPU has finished
  // (no colour frame: update + distance transform only; no colour launch finished yet -- a new or just cleared map: as many as the TSDF part)
  const int color_cap = m->knobs.color_grid;      // (NVBX_COLOR_GRID -- A/B: workgroups of the colour part, tools/fused_grid_sweep.sh)
  st.cgrid = !st.has_color ? 0 : (int)std::max<int64_t>(8, std::min<int64_t>(std::min<int64_t>(m->capacity, color_cap), c_hint == 0 ? (int64_t)st.grid : ((with_grid_margin(m, c_hint) + 7) / 8) * 8));
  // a held-back union step of the multi-GPU exchange (nvbx_mark_esdf_dirty_gathered_deferred) rides here in eight workgroups: the peers'
  // blocks become ESDF-dirty for the NEXT marking pass (its own marking launch, or a ride in the colour launch, would be a third launch;
  // beside this frame's view marking it would meet blocks that launch is just allocating -- DESIGN.md 6.1)
  st.imp = ImportArgs{};
  if (m->held.import_pending) {
    st.imp.g = m->held.import_ptr; st.imp.world = m->held.import_world; st.imp.self_rank = m->held.import_rank; st.imp.max_count = m->held.import_max; st.imp.n_wg = 8;
    m->held.import_pending = false;
  }
}
// step 4: behind the TSDF-update launch
template <typename Sensor>
static int depth_step_after(nvbx_mapper* m, int n_frames) {
  NVBX_HIP(hipGetLastError());
  m->last_view_frame = m->frame_id;
  if (!Sensor::kLongRays) { m->last_camera_view_frame = m->frame_id; m->last_camera_view_mask = 1u << (n_frames - 1); }   // (a batch: the LAST camera's view, as separate calls would leave it)
  m->last_view_batch = n_frames;
  if (m->p.projective_layer_type == 2 && m->update_freespace()) return NVBX_E_DEVICE;     // TSDF with freespace (dynamic mapping)
  return NVBX_OK;
}

// (frames of a held-back colour image a depth call carries out: let go of on every way out, behind the launches that read them)
struct ReleaseFrames { nvbx_mapper* m; ~ReleaseFrames() { m->release_consumed_frames(); } };
template <typename Img, typename Sensor, int NB>
static int integrate_depth_impl(nvbx_mapper* m, FrameSet<Img, NB> fs, const Sensor& sensor) {
  ReleaseFrames release_frames{m};
  DepthSteps<NB> st;
  { const int rc = depth_step_before_mark_view<Img, Sensor, NB>(m, fs, st); if (rc) return rc; }
  bool grid_view = false;
  if constexpr (Sensor::kLongRays) { const int rc = launch_view_grid(m, fs, sensor, st.tiles, st.tr.fence_report, &grid_view); if (rc) return rc; }
  if (!grid_view)
  NVBX_LAUNCH_SMEM(m, (k_mark_view<Img, Sensor, NB>), dim3(st.tiles + st.edt_wg + st.tr.n_wg + st.tr.n_scan_wg + st.tr.n_mark_wg), dim3(Sensor::kThreads), mark_view_smem<Sensor>(st.edt_wg > 0), m->d, fs, sensor, (int4*)m->view_list, (int32_t)m->capacity,
              (int32_t)(m->premark_consumed ? 1 : 0), (int32_t)st.edt_wg, st.ea, st.tr);
  { const int rc = depth_step_between<Sensor, NB>(m, st); if (rc) return rc; }
  const int grid = st.grid; const int32_t spec_lanes = st.spec_lanes; const bool plain = st.plain;
  uint8_t* view_class = nullptr; int32_t* dense_list = nullptr;
  if constexpr (Sensor::kLongRays) { const int rc = launch_lidar_sparse(m, fs, sensor, plain, &view_class, &dense_list); if (rc) return rc; }
  if (Sensor::kLongRays && m->p.projective_layer_type != 1) m->lidar_integrated = true;      // (blocks may be F_BAND_STALE from here on)
  if (st.fused) {
    if constexpr (Sensor::kRiders) {
      depth_step_fused_riders<NB>(m, st);
      const dim3 g((unsigned)(st.n_edt + grid + st.cgrid + st.imp.n_wg));
#define NVBX_FUSED_LAUNCH(PIX, PLAIN) NVBX_LAUNCH(m, (k_integrate_tsdf_color<Img, PIX, NB, PLAIN>), g, dim3(512), m->d, fs, sensor, (const int4*)m->view_list, (int32_t)m->capacity, \
        m->mesh_list_live(), m->view_export, (int32_t)m->view_export_cap, spec_lanes, (int32_t)grid, fsc, m->synth.as<const float>(), st.col.srows, st.col.scols, st.cand, st.cand_idx, st.n_edt, st.ea_edt, st.imp)
      std::visit([&](const auto& fsc) {      // (each instantiation named in source text: that text is its name in the profile, NVBX_LAUNCH)
        if constexpr (std::is_same_v<decltype(pix_of(fsc)), PixRgb8>) { if (plain) NVBX_FUSED_LAUNCH(PixRgb8, true); else NVBX_FUSED_LAUNCH(PixRgb8, false); }
        else { if (plain) NVBX_FUSED_LAUNCH(PixBgra8, true); else NVBX_FUSED_LAUNCH(PixBgra8, false); }
      }, st.col.fs);
#undef NVBX_FUSED_LAUNCH
    }
  } else
  if (plain) NVBX_LAUNCH(m, (k_integrate_tsdf<Img, Sensor, NB, true>), dim3(grid), dim3(512), m->d, fs, sensor, (const int4*)m->view_list, (int32_t)m->capacity,
                         m->mesh_list_live(), m->view_export, (int32_t)m->view_export_cap, spec_lanes, (const uint8_t*)view_class, (const int32_t*)dense_list);
  else NVBX_LAUNCH(m, (k_integrate_tsdf<Img, Sensor, NB, false>), dim3(grid), dim3(512), m->d, fs, sensor, (const int4*)m->view_list, (int32_t)m->capacity,
                   m->mesh_list_live(), m->view_export, (int32_t)m->view_export_cap, spec_lanes, (const uint8_t*)view_class, (const int32_t*)dense_list);
  return depth_step_after<Sensor>(m, fs.n);
}

// Two mappers, one depth frame each (same image size, same stream), in TWO launches instead of four: defined as equal to integrate_depth_impl(ma) followed by
// integrate_depth_impl(mb) -- the maps share nothing, so running each launch's two halves side by side changes no result (tests/test_gpu_round6.py).  Both
// frames are camera frames that have passed integrate_cameras' own preparation (pair_prepare below).
template <typename Img>
static int integrate_depth_pair_impl(nvbx_mapper* ma, FrameSet<Img, 1> fa, nvbx_mapper* mb, FrameSet<Img, 1> fb) {
  ReleaseFrames release_a{ma}, release_b{mb};
  DepthSteps<1> sa, sb;
  { const int rc = depth_step_before_mark_view<Img, CameraSensor, 1>(ma, fa, sa); if (rc) return rc; }
  { const int rc = depth_step_before_mark_view<Img, CameraSensor, 1>(mb, fb, sb); if (rc) return rc; }
  // (a distance transform armed in classic order would ride with the LDS of an EdtShared: launched on its own first -- rare, a mapper that has just left the classic order)
  if (sa.edt_wg) { ma->held.edt_pending = true; sa.edt_wg = 0; if (ma->flush_edt()) return NVBX_E_DEVICE; }
  if (sb.edt_wg) { mb->held.edt_pending = true; sb.edt_wg = 0; if (mb->flush_edt()) return NVBX_E_DEVICE; }
  // (tiles-first layout inside each mapper's numbering, whether or not it has riders: the pair kernel deals the tiles of both out first)
  sa.tr.n_tile_wg = sa.tiles; sb.tr.n_tile_wg = sb.tiles;
  MarkViewArgs<Img> A{ma->d, fa, (int4*)ma->view_list, (int32_t)ma->capacity, (int32_t)(ma->premark_consumed ? 1 : 0), 0, sa.ea, sa.tr, sa.tiles, sa.tiles + sa.tr.n_wg + sa.tr.n_scan_wg + sa.tr.n_mark_wg};
  MarkViewArgs<Img> B{mb->d, fb, (int4*)mb->view_list, (int32_t)mb->capacity, (int32_t)(mb->premark_consumed ? 1 : 0), 0, sb.ea, sb.tr, sb.tiles, sb.tiles + sb.tr.n_wg + sb.tr.n_scan_wg + sb.tr.n_mark_wg};
  mb->enqueue_seq++;
  NVBX_LAUNCH_SMEM(ma, (k_mark_view_pair<Img>), dim3((unsigned)(A.n_wg + B.n_wg)), dim3(CameraSensor::kThreads), mark_view_smem<CameraSensor>(false), A, B);
  { const int rc = depth_step_between<CameraSensor, 1>(ma, sa); if (rc) return rc; }
  { const int rc = depth_step_between<CameraSensor, 1>(mb, sb); if (rc) return rc; }
  // the TSDF-update launch in its fused form for both (a mapper with nothing held back: no riders -- the same worker as k_integrate_tsdf)
  if (sa.fused) depth_step_fused_riders<1>(ma, sa);      // (else: zero riders, DepthSteps' defaults)
  if (sb.fused) depth_step_fused_riders<1>(mb, sb);
  // (the second mapper of a pair is the foreground mapper: a few blocks.  Its distance transform gets 64 workers instead of 256 -- they grid-stride, and the
  //  launch is residency-bound: every idle 8-wavefront workgroup holds a slot for ~1.5 us)
  if (sb.n_edt > mb->knobs.pair_b_edt_riders) sb.n_edt = mb->knobs.pair_b_edt_riders;      // (NVBX_PAIR_B_EDT_RIDERS, the second mapper's)
  // ONE pixel type for the pair: whichever mapper holds a colour frame, else rgb8; a mapper that holds none passes an empty set of that type
  if (sa.has_color && sb.has_color && sa.col.fs.index() != sb.col.fs.index()) { set_error("nvbx_integrate_depth_pair: colour frames of two encodings"); return NVBX_E_INVALID; }
  auto fused_args = [&](nvbx_mapper* m, const FrameSet<Img, 1>& f, const DepthSteps<1>& st, const auto& lead_fs) {
    FusedArgs<Img, decltype(pix_of(lead_fs))> x{}; x.m = m->d; x.fs = f; x.view_list = (const int4*)m->view_list; x.list_cap = (int32_t)m->capacity; x.mesh_list = m->mesh_list_live(); x.view_export = m->view_export;
    x.view_export_cap = (int32_t)m->view_export_cap; x.spec_lanes = st.spec_lanes; x.n_tsdf_wg = (int32_t)st.grid; if (auto* fsc = std::get_if<std::decay_t<decltype(lead_fs)>>(&st.col.fs)) x.fsc = *fsc;
    x.synth = m->synth.as<const float>(); x.srows = st.col.srows; x.scols = st.col.scols; x.cand = st.cand; x.cand_cnt_idx = st.cand_idx; x.n_edt_wg = st.n_edt; x.ea = st.ea_edt; x.imp = st.imp;
    x.n_wg = st.n_edt + st.grid + st.cgrid + st.imp.n_wg;
    return x;
  };
  mb->enqueue_seq++;
  std::visit([&](const auto& lead_fs) {
    const auto FA_ = fused_args(ma, fa, sa, lead_fs), FB_ = fused_args(mb, fb, sb, lead_fs);
    if constexpr (std::is_same_v<decltype(pix_of(lead_fs)), PixRgb8>) NVBX_LAUNCH(ma, (k_integrate_tsdf_color_pair<Img, PixRgb8>), dim3((unsigned)(FA_.n_wg + FB_.n_wg)), dim3(512), FA_, FB_);
    else NVBX_LAUNCH(ma, (k_integrate_tsdf_color_pair<Img, PixBgra8>), dim3((unsigned)(FA_.n_wg + FB_.n_wg)), dim3(512), FA_, FB_);
  }, (sa.has_color ? sa.col : sb.col).fs);
  { const int rc = depth_step_after<CameraSensor>(ma, 1); if (rc) return rc; }
  return depth_step_after<CameraSensor>(mb, 1);
}
// the 24-bit view frame id of Entry::stamp: before it would wrap, every stamp is reset (once per 16.7 M depth frames)
__global__ void k_reset_stamps(DMap m) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= m.mask; i += gridDim.x * blockDim.x) m.table[i].stamp = STAMP_NEVER;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m.capacity; i += gridDim.x * blockDim.x) m.slot_cam[i] = STAMP_NEVER;
  if (blockIdx.x == 0 && threadIdx.x < 4) m.counters[C_VIEW_COUNT + threadIdx.x] = 0;
}
int next_frame_id(nvbx_mapper* m) {
  if (m->frame_id >= STAMP_FRAME_MAX) {
    if (m->begin_call()) return NVBX_E_DEVICE;
    NVBX_LAUNCH(m, k_reset_stamps, dim3(1024), dim3(256), m->d);
    NVBX_HIP(hipGetLastError());
    m->frame_id = 0; m->last_view_frame = 0; m->last_camera_view_frame = 0;
  }
  m->frame_id++;
  return NVBX_OK;
}

// [U] DepthPreprocessor (do_depth_preprocessing, depth_preprocessing_num_dilations): invalid-depth regions grow by n pixels.
// One thread per pixel; the (2n+1)^2 window is read through L1/L2 (the image is 1.2 MB).  Output in metres (f32).
template <typename Img>
__global__ void k_dilate_invalid(Img in, int32_t rows, int32_t cols, int32_t n, float* out) {
  const int64_t total = (int64_t)rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
    bool bad = false;
    for (int dr = -n; dr <= n && !bad; dr++) {
      const int rr = r + dr; if (rr < 0 || rr >= rows) continue;
      for (int dc = -n; dc <= n; dc++) {
        const int cc = c + dc; if (cc < 0 || cc >= cols) continue;
        if (!(in(pix(rr, cc, cols)) > 0.0f)) { bad = true; break; }
      }
    }
    out[i] = bad ? 0.0f : in(i);
  }
}

// what a camera integrateDepth does before it enqueues anything of its own frame: argument check, the held-back calls it cannot carry, pool growth
template <int NB>
static int cameras_prepare(nvbx_mapper* m, int32_t n, const float* T_L_C /* n x 16 */) {
  for (int c = 0; c < n; c++)
    if (!nvbx_pose_in_range(T_L_C + 16 * c, m->p.voxel_size * 8.0f, m->p.max_integration_distance_m + 2.0f * m->p.truncation_distance_vox * m->p.voxel_size)) {
      set_error("integrate depth: T_L_C is not finite or lies outside the addressable block range (+-2^20 blocks)"); return NVBX_E_INVALID; }
  NVBX_HIP(hipSetDevice(m->device));
  const bool dilate_first = m->p.do_depth_preprocessing && m->p.depth_preprocessing_num_dilations > 0;
  // held-back integrateColor / updateEsdf that this call cannot carry out in pipelined order are replayed NOW (the replayed calls launch / re-arm the EDT)
  const bool carry = !dilate_first && (m->held.color_pending.on ? m->held.color_pending.carried_by(NB) : m->esdf_only_carry());      // this call can carry the held-back calls out in pipelined order
  if (!carry && m->replay_deferred()) return NVBX_E_DEVICE;
  // (begin_call would launch a held-back EDT / union step; the EDT rides in k_mark_view instead, the union step stays held back for the next
  //  integrateColor -- it belongs to the NEXT ESDF update and touches nothing this launch reads.  What else is still held back, this call carries out)
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  { const int rc = m->maybe_grow(); if (rc) return rc; }          // (before anything of this frame is enqueued)
  return NVBX_OK;
}
// n camera frames (n = 1: MultiMapper::integrateDepth; n > 1: nvbx_integrate_depth_batch) of one image size -> one launch set
template <typename Img, int NB>
static int integrate_cameras(nvbx_mapper* m, int32_t n, const Img* imgs, int32_t rows, int32_t cols, const float* T_L_C /* n x 16 */, const nvbx_camera* cameras) {
  { const int rc = cameras_prepare<NB>(m, n, T_L_C); if (rc) return rc; }
  const bool dilate = m->p.do_depth_preprocessing && m->p.depth_preprocessing_num_dilations > 0;
  if (dilate && m->flush_edt()) return NVBX_E_DEVICE;   // first launch is the dilation
  { const int rc = next_frame_id(m); if (rc) return rc; }
  FrameSet<Img, NB> fs{}; fs.n = n;
  for (int c = 0; c < n; c++) { fs.f[c] = m->make_frame(T_L_C + 16 * c, cameras + c, rows, cols, m->p.raycast_subsampling_factor); fs.img[c] = imgs[c]; }
  if (dilate) {             // (single frames only: nvbx_integrate_depth_batch falls back to separate calls)
    const int64_t npx = (int64_t)rows * cols;
    if (m->depth_pre.ensure(m->stream, (size_t)npx * 4)) return NVBX_E_DEVICE;
    NVBX_LAUNCH(m, (k_dilate_invalid<Img>), dim3((unsigned)std::min<int64_t>((npx + 255) / 256, 4096)), dim3(256), imgs[0], rows, cols,
                m->p.depth_preprocessing_num_dilations, m->depth_pre.as<float>());
    FrameSet<DepthF32, 1> fd{}; fd.n = 1; fd.f[0] = fs.f[0]; fd.img[0] = DepthF32{m->depth_pre.as<float>()};
    return integrate_depth_impl<DepthF32, CameraSensor, 1>(m, fd, CameraSensor{});
  }
  return integrate_depth_impl<Img, CameraSensor, NB>(m, fs, CameraSensor{});
}

extern "C" int nvbx_integrate_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const float T_L_C[16],
                                    const nvbx_camera* camera) {
  if (const int rc = nvbx_camera_frame_refused("nvbx_integrate_depth", m && depth_dev && T_L_C && camera, "", rows, cols, camera)) return rc;
  const DepthF32 img{depth_dev};
  return integrate_cameras<DepthF32, 1>(m, 1, &img, rows, cols, T_L_C, camera);
}
extern "C" int nvbx_integrate_depth_u16mm(nvbx_mapper* m, const uint16_t* depth_mm_dev, int32_t rows, int32_t cols, const float T_L_C[16],
                                          const nvbx_camera* camera) {
  if (const int rc = nvbx_camera_frame_refused("nvbx_integrate_depth_u16mm", m && depth_mm_dev && T_L_C && camera, "", rows, cols, camera)) return rc;
  const DepthU16mm img{depth_mm_dev};
  return integrate_cameras<DepthU16mm, 1>(m, 1, &img, rows, cols, T_L_C, camera);
}
// Up to NVBX_MAX_BATCH camera frames (same image size) in ONE launch set: see include/nvblox_hip.h
extern "C" int nvbx_integrate_depth_batch(nvbx_mapper* m, int32_t n, const float* const* depth_dev, int32_t rows, int32_t cols, const float* T_L_C,
                                          const nvbx_camera* cameras) {
  if (const int rc = nvbx_camera_frame_refused("nvbx_integrate_depth_batch", m && n >= 1 && n <= MAX_BATCH && depth_dev && T_L_C && cameras, "1 <= n <= 8, ", rows, cols, cameras, n, reinterpret_cast<const void* const*>(depth_dev))) return rc;
  // what a batch cannot express falls back to the separate calls it is defined by: per-frame freespace time stamps, depth dilation
  if (n == 1 || m->p.projective_layer_type == 2 || (m->p.do_depth_preprocessing && m->p.depth_preprocessing_num_dilations > 0)) {
    for (int c = 0; c < n; c++) { const int rc = nvbx_integrate_depth(m, depth_dev[c], rows, cols, T_L_C + 16 * c, cameras + c); if (rc) return rc; }
    return NVBX_OK;
  }
  DepthF32 imgs[MAX_BATCH];
  for (int c = 0; c < n; c++) imgs[c] = DepthF32{depth_dev[c]};
  return integrate_cameras<DepthF32, MAX_BATCH>(m, n, imgs, rows, cols, T_L_C, cameras);
}

// One depth frame each for TWO mappers on one stream -- MultiMapper::integrateDepth of the dynamic and the human mapping types: the background mapper takes the
// unmasked part of the depth image, the foreground (occupancy) mapper the masked part, nvblox_node.cpp:1057-1062 -- in two launches instead of four.
// See include/nvblox_hip.h; whatever the pair cannot express falls back to the two calls it is defined by.
static bool pair_can_fuse(const nvbx_mapper* m) {
  if (m->capacity > (1ll << 24)) return false;
  if (m->p.do_depth_preprocessing && m->p.depth_preprocessing_num_dilations > 0) return false;          // (a dilation launch in front)
  if (m->held.color_pending.on && (m->held.color_pending.n != 1 || !fused_colour_applies(m))) return false;      // (its colour frame would be carried in three launches)
  return true;
}
// (the pair launch decodes ONE pixel type -- that of whichever mapper holds a colour frame: two held-back frames in different encodings, rgb8 and bgra8,
//  cannot share it.  Checked before either mapper's preparation, which consumes host state)
static bool pair_colour_encodings_differ(const nvbx_mapper* ma, const nvbx_mapper* mb) {
  return ma->held.color_pending.on && mb->held.color_pending.on && ma->held.color_pending.enc != mb->held.color_pending.enc;
}
extern "C" int nvbx_integrate_depth_pair(nvbx_mapper* ma, const float* depth_a_dev, nvbx_mapper* mb, const float* depth_b_dev, int32_t rows, int32_t cols,
                                         const float T_L_C[16], const nvbx_camera* camera) {
  if (const int rc = nvbx_camera_frame_refused("nvbx_integrate_depth_pair", ma && mb && ma != mb && depth_a_dev && depth_b_dev && T_L_C && camera, "two different mappers, ", rows, cols, camera)) return rc;
  const bool pair_on = ma->knobs.depth_pair && mb->knobs.depth_pair;       // (NVBX_DEPTH_PAIR -- A/B: 0 in either mapper = always the two separate calls)
  if (!pair_on || ma->device != mb->device || ma->stream != mb->stream || !pair_can_fuse(ma) || !pair_can_fuse(mb) ||
      pair_colour_encodings_differ(ma, mb)) {
    const int rc = nvbx_integrate_depth(ma, depth_a_dev, rows, cols, T_L_C, camera); if (rc) return rc;
    return nvbx_integrate_depth(mb, depth_b_dev, rows, cols, T_L_C, camera);
  }
  // each mapper's own preparation, in call order (held-back calls it cannot carry are replayed, pools grow), then the frame ids
  { const int rc = cameras_prepare<1>(ma, 1, T_L_C); if (rc) return rc; }
  { const int rc = cameras_prepare<1>(mb, 1, T_L_C); if (rc) return rc; }
  { const int rc = next_frame_id(ma); if (rc) return rc; }
  { const int rc = next_frame_id(mb); if (rc) return rc; }
  FrameSet<DepthF32, 1> fa{}, fb{}; fa.n = 1; fb.n = 1;
  fa.f[0] = ma->make_frame(T_L_C, camera, rows, cols, ma->p.raycast_subsampling_factor); fa.img[0] = DepthF32{depth_a_dev};
  fb.f[0] = mb->make_frame(T_L_C, camera, rows, cols, mb->p.raycast_subsampling_factor); fb.img[0] = DepthF32{depth_b_dev};
  return integrate_depth_pair_impl<DepthF32>(ma, fa, mb, fb);
}

// ------------------------------------------------------------------------------------------------ for measure.hip and lidar.hip
// (behind the camera entry points: the order in which the file instantiates its kernels steers the compiler's inlining order, and so their code)
// The view marking of one camera frame, no riders, no TSDF update behind it (nvbx_measure_depth): blocks looked up / allocated as integrateDepth would.
void launch_mark_view_camera(nvbx_mapper* m, const FrameSet<DepthF32, 1>& fs) {
  TraceRider no_riders{}; no_riders.fence_report = m->next_fence_report();
  NVBX_LAUNCH_SMEM(m, (k_mark_view<DepthF32, CameraSensor, 1>), dim3(mark_view_tile_wgs<CameraSensor>(fs.f[0])), dim3(CameraSensor::kThreads), mark_view_smem<CameraSensor>(false), m->d, fs, CameraSensor{},
              (int4*)m->view_list, (int32_t)m->capacity, (int32_t)(m->premark_consumed ? 1 : 0), (int32_t)0, m->held.edt_args, no_riders);
  m->premark_consumed = false;
}
int integrate_lidar_frame(nvbx_mapper* m, FrameSet<DepthF32, 1> fs, const LidarSensor& sensor) {
  return integrate_depth_impl<DepthF32, LidarSensor, 1>(m, fs, sensor);
}
