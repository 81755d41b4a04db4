// nvbx_mapper.h -- host-side state of one mapper (one GPU, one stream).  Host code only, but for nvbx_index_in_range, which kernels call too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <cmath>
#include <algorithm>
#include <vector>
#include "../../include/nvblox_hip.h"
#include "nvbx_internal.h"
#include "nvbx_knobs.h"       // the NVBX_* environment knobs, validated
#include "nvbx_devbuf.h"      // DevBuf (scratch memory that grows on demand), PoolArr (the table of capacity-sized arrays)

namespace nvbx {

struct EsdfArgs {
  int32_t kz_min, kz_max, kz_out;   // global voxel z range of the TSDF band, output plane
  int32_t bz_lo, bz_hi, bz_out, vz_out;
  int32_t ri;                       // integer search radius (voxels)
  int32_t rb;                       // ceil(ri / 8) blocks
  float max_sq, site_dist_m, min_weight, voxel_size;
  int32_t site_rule;
  uint32_t epoch;
  uint32_t mark_pass;               // stamp of this marking pass (column de-duplication within one pass)
  int32_t rec;                      // C_ESDF_UPD + 8 * (epoch & 1)
  int32_t rec_next;                 // record of the next epoch (reset by this update)
  // Who empties the ESDF-dirty list a marking pass has consumed.  Classic order: the next k_mark_view or the EDT does (the consumed list still names
  // "the blocks dirtied since the last updateEsdf" for nvbx_esdf_dirty_list until then).  Pipelined order (held.hip): nothing runs between the marking
  // pass and the next appends, so the pass empties the list itself -- its last worker, counted in C_MARK_DONE (self_reset) -- and the EDT of that
  // update, which then runs AFTER those appends, must not (keep_list).
  int32_t self_reset, keep_list;
  // [U] ground-plane-relative slice (nvbx_mapper_params::esdf_use_ground_plane): the z band of column (x, y) is [h + above, h + above + thick],
  // h = height of the plane {n, d} at the column's centre (esdf_plane_height); 0 = the fixed band kz_min .. kz_max above
  int32_t plane_on; float pl[4], above, thick;
};

struct MeshRecord { int32_t x, y, z, vbase, nvert, tbase, ntri, pad; };
enum class ColorEnc { rgb8, bgra8 };      // a colour image's encoding
template <int NB> struct TraceRiderT; template <int NB> struct HeldColorFrames;      // what color.hip hands to tsdf.hip of a held-back colour call (nvbx_sphere_trace.h, nvbx_color_worker.h)

float log_odds(float p);
// frames.hip: library-owned, reference-counted device frames (ownership transfer of input images)
bool frame_retain_if_frame(const void* p, size_t need_bytes, bool* too_small);
void frame_release_fenced(void* p, const volatile int32_t* progress, int32_t seq, const volatile int32_t* reports_enqueued, hipStream_t reader, const void* owner);
void frames_register_stream(int device, hipStream_t stream);
void frames_forget_owner(const void* owner, int device, hipStream_t stream);
void set_error(const char* what, hipError_t e);
void set_error(const char* what);
// THE refusal of a C-ABI argument check: the error becomes who + why (why carries its own ": "), the call returns NVBX_E_INVALID
inline int refuse(const char* who, const char* why) { set_error((std::string(who) + why).c_str()); return NVBX_E_INVALID; }
// segment.hip.  nvbx_label_components' refusals in their order, for every call that ends in it; volume_why: what the caller found wrong with its
// block arrays (their count, their pointers), null = nothing -- the one refusal whose condition and text differ between the callers
int seg_check(const char* who, int32_t connectivity, int32_t min_voxels, const char* volume_why, const void* comps, int64_t cap, const void* count);
// layers.hip.  API layer id -> internal slot flag (0 = this mapper cannot hold that layer); bytes of one voxel in the reference's struct layout
uint32_t internal_layer(const nvbx_mapper* m, uint32_t layer);
size_t ref_voxel_bytes(uint32_t layer);
// API layer ids by what can be done with them: written block by block (nvbx_set_blocks, map files) / read block by block / listed
static inline bool layer_writable(uint32_t l) { return l == F_TSDF || l == F_COLOR || l == F_ESDF || l == NVBX_LAYER_OCCUPANCY; }
static inline bool layer_readable(uint32_t l) { return layer_writable(l) || l == F_FREESPACE; }
static inline bool layer_listable(uint32_t l) { return layer_readable(l) || l == F_MESH || l == F_FEATURE; }      // (feature blocks are read by nvbx_get_feature_blocks)

}  // namespace nvbx

// the camera model must describe the image that is handed over with it: the kernels bound projections by (width, height) and
// address pixels by (rows, cols)
static inline bool nvbx_camera_matches(const nvbx_camera* c, int32_t rows, int32_t cols) {
  return c && c->width == cols && c->height == rows && c->fu > 0.0f && c->fv > 0.0f;
}
// THE two refusals of a camera-frame entry point `who`, in their order; 0 = go on.  args_ok: the entry's own conditions on its pointers and counts; hint: what its first refusal says in
// parentheses ahead of the image sides (null: no parentheses).  images: a batch's n image pointers, each checked with its camera (a single frame: null, its image pointer is part of args_ok)
static inline int nvbx_camera_frame_refused(const char* who, bool args_ok, const char* hint, int32_t rows, int32_t cols, const nvbx_camera* cameras, int32_t n = 1, const void* const* images = nullptr) {
  if (!args_ok || !nvbx::image_dims_ok(rows, cols)) return nvbx::refuse(who, hint ? (std::string(": invalid argument (") + hint + "image sides 1 .. 32768)").c_str() : ": invalid argument");
  for (int c = 0; c < n; c++)
    if ((images && !images[c]) || !nvbx_camera_matches(cameras + c, rows, cols))
      return nvbx::refuse(who, images ? ": every camera's width/height must equal the images' cols/rows, focal lengths > 0"
                                      : ": camera width/height must equal the image's cols/rows, focal lengths > 0");
  return 0;
}
// ... and one that comes without an image (rendering, view gain, feature frames) must describe an image the C-ABI would accept
static inline bool nvbx_camera_valid(const nvbx_camera* c) {
  return c && c->fu > 0.0f && c->fv > 0.0f && nvbx::image_dims_ok(c->height, c->width);
}

// Block indices are 21 bits per axis in the hash key (pack_key): a sensor pose is accepted only if it is finite and everything
// within `reach` metres of it stays inside [-2^20, 2^20) blocks (419 km at 0.05 m voxels) -- beyond that keys would alias.
// nvbx_pose_limit: the bound on |translation| per axis, also handed to the kernels that test ray origins and candidate poses on the device.
static inline float nvbx_pose_limit(float block_size, float reach) { return ((float)(1 << 20) - 2.0f) * block_size - reach; }
static inline bool nvbx_pose_in_range(const float T[16], float block_size, float reach) {
  for (int i = 0; i < 16; i++) if (!std::isfinite(T[i])) return false;
  const float lim = nvbx_pose_limit(block_size, reach);
  return std::fabs(T[3]) < lim && std::fabs(T[7]) < lim && std::fabs(T[11]) < lim;
}
// a row-major 4 x 4 pose -> its rotation, row-major 3 x 3, and its translation
static inline void nvbx_pose_unpack(const float T[16], float R[9], float t[3]) {
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R[3 * i + j] = T[4 * i + j]; t[i] = T[4 * i + 3]; }
}
__host__ __device__ static inline bool nvbx_index_in_range(int32_t x, int32_t y, int32_t z) {
  const int32_t L = 1 << 20;
  return x >= -L && x < L && y >= -L && y < L && z >= -L && z < L;
}

struct nvbx_mapper {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false, stream_registered = false;
  hipEvent_t ev_order = nullptr;     // nvbx_mapper_wait_for: this mapper's stream as the producer
  // The NVBX_* environment knobs (nvbx_knobs.h), read at nvbx_mapper_create and again by nvbx_mapper_reload_knobs: every launch-geometry and A/B
  // decision of this mapper reads them here.  max_capacity, color_deferral / color_staging and defer_edt take their value at creation only.
  nvbx_knobs knobs{};
  nvbx_plan_knobs plan_knobs{}; // ... and the cost field's two (plan.hip), read with them
  nvbx_change_knobs change_knobs{}; // ... and change detection's one (change.hip)
  nvbx_resample_knobs resample_knobs{}; // ... and resampling's one (resample.hip)
  int begin_call(bool carry_out_held = true);      // first call of every entry point (held.hip): the device is made current, held-back work is carried out (no host sync)
  nvbx_mapper_params p{};
  int64_t capacity = 0;
  // Pool growth (the reference allocates blocks on demand; here the pools double before they run out): kernels mirror the number of
  // free slots into pinned host memory (DMap::host_mirror), every integrate call looks at it first and, below half, doubles every
  // capacity-sized array + rebuilds the hash on the device (grow_map, maintenance.hip).  max_capacity == capacity: fixed pools.
  int64_t max_capacity = 0;
  int32_t* h_mirror = nullptr;       // host view of DMap::host_mirror
  int maybe_grow(int64_t extra_blocks_wanted = 0);
  int grow_map(int64_t new_capacity);
  // THE list of the map's device arrays, with their sizes at `cap` blocks (mapper.hip): creation, pool growth and destruction all walk it
  std::vector<nvbx::PoolArr> pool_arrays(int64_t cap);
  static uint64_t hash_slots(int64_t cap) { uint64_t tsz = 1; while (tsz < (uint64_t)cap * 2) tsz <<= 1; return tsz; }      // hash table entries: a power of two, load <= 1/2
  static int64_t mesh_verts(int64_t cap) { return std::min<int64_t>(cap * 192, 48ll << 20); }                              // mesh arena: vertices (triangles: twice as many)
  int64_t growths = 0;
  nvbx::DMap d{};
  // lists (device)
  int32_t* view_list = nullptr;      // int4 {slot, x, y, z} of the blocks in view of the last depth frame
  // (the ESDF-dirty / mesh-dirty / colour work lists are sharded and live in d.lists / d.shc, nvbx_internal.h)
  int32_t* export_idx = nullptr;     // int32[capacity][3] scratch for multi-GPU export of the dirty list
  int32_t* export_count = nullptr;
  int32_t* cleared_idx = nullptr;    // int32[capacity][3]: Index3D of projective-layer blocks deallocated since nvbx_take_cleared_blocks
  // LiDAR beam direction tables (float2 {sin, cos}: rows elevations then cols azimuths), rebuilt when the model changes
  nvbx::DevBuf lidar_tab; nvbx_lidar lidar_cached{}; std::vector<float> lidar_host;
  // mask splitting scratch: nearest depth (in the mask camera) that landed on each mask pixel
  nvbx::DevBuf mask_zmin;
  // depth preprocessing scratch (dilated depth image)
  nvbx::DevBuf depth_pre;
  // colour scratch
  nvbx::DevBuf synth; int32_t synth_rows = 0, synth_cols = 0, synth_last = 0;
  // feature layer (features.hip): null / 0 until nvbx_enable_features.  feat_val: capacity x (channels / 8) x 512 x 8 halfs, feat_w: capacity x 512 f32;
  // both in pool_arrays (pool growth carries them), handed to the feature kernels in their own argument structs.  feat_synth: the synthetic depth of
  // the last feature frame -- the colour path's `synth` stays the last colour frame's.
  void* feat_val = nullptr; float* feat_w = nullptr; int32_t feat_channels = 0;
  nvbx::DevBuf feat_synth;
  // feature segmentation (segment.hip): the entry table, parent[n][512] and count[n][512] of the largest block list labelled so far
  nvbx::DevBuf seg_scratch;
  // pose alignment (align.hip): the f64 pose state and the 256 x 29 partial sums of the accumulate launches, about 60 KB
  nvbx::DevBuf align_buf;
  // relocalisation (relocalize.hip): the lattice tables (4 KB) and, where the caller wants no scores, the lattice's 24-byte records; the tables' host copy
  nvbx::DevBuf reloc_buf; std::vector<float> reloc_host;
  // map merging and resampling (merge.hip, resample.hip), as the destination: a 64-byte head of counters and the key set that counts the distinct candidate blocks
  nvbx::DevBuf merge_buf;
  // change detection (change.hip), as the map that is scanned: 64 bytes of counters, allocated with the map
  nvbx::DevBuf change_buf;
  // surface points (surface.hip), as the mapper whose stream runs the call: a 64-byte head (the count of nvbx_align_map / nvbx_relocalize_map), the
  // crossing count and the three neighbour slots of every slot of the scanned map and the sums and offsets of the scan's tiles; and, apart from it (a growth keeps no contents),
  // the points and colours those two calls hand to the alignment
  nvbx::DevBuf surface_buf, surface_pts;
  // cost field (plan.hip) and cost volume (plan3d.hip), sized and carved up by nvbx_plan_grid.h's plan_grid_setup alone: a 64-byte head of counters, the class word of every cell and the two sets of active-tile flags of the largest input so far
  nvbx::DevBuf plan_scratch;
  // traversability (elevation.hip): one bit row of HAZARD flags, ceil(cols / 64) 64-bit words, per row of the largest image so far
  nvbx::DevBuf terrain_scratch;
  // mesh arena
  float* mesh_vert = nullptr; float* mesh_nrm = nullptr; uint8_t* mesh_col = nullptr; int32_t* mesh_tri = nullptr;
  nvbx::MeshRecord* mesh_rec = nullptr;
  int64_t mesh_vert_cap = 0, mesh_tri_cap = 0;
  // staging
  nvbx::DevBuf staging;
  // nvbx_esdf_slice_to_host: pinned, device-mapped [16-int header][image] that k_esdf_slice_rows writes directly (one wait per host slice)
  float* slice_pinned = nullptr; float* slice_pinned_dev = nullptr; int64_t slice_pinned_elems = 0;
  // every kernel launch bumps enqueue_seq (NVBX_LAUNCH*); nvbx_esdf_slice_size remembers it: a slice_to_image right behind it re-uses the counters
  uint64_t enqueue_seq = 1, slice_size_seq = 0;
  int32_t* h_counters = nullptr;     // pinned
  uint32_t frame_id = 0;
  uint32_t esdf_epoch = 0;
  uint32_t mark_pass = 0;            // ESDF marking passes launched so far
  // ESDF marking state: `dirty_since_mark` = TSDF changed since the last marking pass; `premark_consumed` = the dirty list
  // was processed by a pass that no EDT followed yet, so it must be emptied before anything is appended to it
  bool dirty_since_mark = false, premark_consumed = false;
  void reset_marking() { dirty_since_mark = false; premark_consumed = false; mark_pass = 0; unresolved_marks = false; pass_at_last_edt = 0; }      // (a cleared map)
  // `unresolved_marks` = a marking pass ran that no distance transform has followed yet (its columns are only PENDING):
  // an operation that deallocates blocks takes such passes back first (undo_marks, esdf.hip), so that the ESDF update that
  // eventually runs sees exactly the dirty set the reference semantics define at that moment.  `pass_at_last_edt` =
  // mark_pass when the last distance transform was enqueued (passes above it are the unresolved ones).
  bool unresolved_marks = false; uint32_t pass_at_last_edt = 0;
  int undo_marks();
  // nvbx_tsdf_zero_crossings: the sorted result of the last call, valid until any other entry point runs (begin_call) -- serves the
  // "count, then data" pair of calls with one launch, one download and one sort
  bool zc_valid = false; float zc_min = 0.0f, zc_max = 0.0f; std::vector<float> zc_points;
  // dynamic mapping (dynamics.hip)
  int64_t time_ms = 0;               // update_time_ms of the next integrateDepth
  int ensure_freespace_pool();
  int update_freespace();            // after the TSDF update of a depth frame (projective_layer_type 2)
  nvbx::DevBuf apply_postab;         // nvbx_apply_measurements: per slot, the record position of each rank (+1)
  nvbx::DevBuf cc_scratch;           // connected components: label[n], size[2][n]
  int64_t cc_ready_n = 0; int cc_parity = 0;                         // image size the arrays are initialised for; which size array the next call uses
  nvbx::DevBuf dyn_scratch;          // nvbx_dynamic_depth_split: label[2][n], size[2][n], nearest depth[2][n] (by call parity)
  int64_t dyn_ready_n = 0; int dyn_parity = 0;
  // EsdfMode::k3D (esdf3d.hip)
  int update_esdf_3d();
  nvbx::DevBuf esdf3_scratch; int64_t esdf3_blocks_marked = 0, esdf3_window_voxels = 0;
  bool defer_edt = true;             // the EDT of an updateEsdf is held back (NVBX_DEFER_EDT=0 disables): see nvbx_update_esdf
  int flush_edt(); int flush_import();      // esdf.hip: launch the held-back EDT / union step now
  // (n = 1: integrateColor, rgb8 or bgra8; n > 1: nvbx_integrate_color_batch, rgb8 -- nvbx::with_color_types turns {enc, n} into the kernels' types.
  //  frames[i] != nullptr: imgs[i] lives in a library-owned frame this mapper has RETAINED, let go of with a fence once the launches that read it are enqueued: frames.hip)
  struct ColorPending { bool on = false; nvbx::ColorEnc enc = nvbx::ColorEnc::rgb8; int32_t n = 1; const void* imgs[nvbx::MAX_BATCH] = {}; void* frames[nvbx::MAX_BATCH] = {}; int32_t rows = 0, cols = 0; float T[16 * nvbx::MAX_BATCH]; nvbx_camera cams[nvbx::MAX_BATCH];
    bool carried_by(int depth_frames) const { return (depth_frames == 1) == (n == 1); } };      // one depth frame carries one colour frame, a depth batch a batch
  struct Held {      // work an entry point has accepted but not launched yet: what, who carries it out and in which order -- the top of held.hip
    bool edt_pending = false; nvbx::EsdfArgs edt_args{};       // the distance transform of the last updateEsdf
    bool import_pending = false; const int32_t* import_ptr = nullptr; int32_t import_world = 0, import_rank = 0; int64_t import_max = 0;      // the union step of the multi-GPU exchange
    ColorPending color_pending;                                // an integrateColor (colour deferral) ...
    bool esdf_update_pending = false;                          // ... and an updateEsdf called behind it, or with colour deferral on and no colour at all
    bool any() const { return edt_pending || import_pending || color_pending.on || esdf_update_pending; }
    // (a cleared map) nothing is carried out, the frames of a held-back colour call are let go of with their fence
    void drop(nvbx_mapper& m) { edt_pending = false; import_pending = false; esdf_update_pending = false; (void)m.take_pending(); m.release_consumed_frames(); }
  } held;
  bool color_deferral = true;        // the switch (default: on, staged -- nvbx_mapper_create; NVBX_COLOR_DEFERRAL=0 in the environment: off)
  // nvbx_mapper_set_color_deferral(m, 2): a held-back frame is COPIED into mapper-owned staging memory when it is held back (one asynchronous copy on the
  // mapper's stream, ordered behind the launches that read the previous one), so the caller may overwrite its image as soon as integrateColor has returned
  bool color_staging = true;
  // frames of held-back colour images (frames.hip).  take_pending: the held-back call is being carried out -- its frames move to `consumed_frames`;
  // release_consumed_frames (after the launches that read them are enqueued, or abandoned): refs dropped with the fence {h_mirror[4] >= seq}.
  // h_mirror[4] is written by the next view-marking launch as its first action (TraceRiderT::fence_report = color_reads_enqueued at that time).
  std::vector<void*> consumed_frames;
  int32_t color_reads_enqueued = 0;      // fence sequence: bumped once per release_consumed_frames
  int32_t fence_reports_enqueued = 0;    // the largest fence_report any ENQUEUED launch carries
  ColorPending take_pending() { ColorPending c = held.color_pending; held.color_pending.on = false; for (int i = 0; i < nvbx::MAX_BATCH; i++) { if (c.frames[i]) consumed_frames.push_back(c.frames[i]); held.color_pending.frames[i] = nullptr; } return c; }
  void release_consumed_frames() {
    if (consumed_frames.empty()) return;
    const int32_t seq = ++color_reads_enqueued;
    for (void* f : consumed_frames) nvbx::frame_release_fenced(f, h_mirror + 4, seq, &fence_reports_enqueued, stream, this);
    consumed_frames.clear();
  }
  int32_t next_fence_report() { __atomic_store_n(&fence_reports_enqueued, color_reads_enqueued, __ATOMIC_RELEASE); return color_reads_enqueued; }
  int64_t inv_i8 = 0;                // (-DNVBX_CHECK_INVARIANTS) colour-reading launches enqueued on a library frame that nobody holds
  // The two modes of held.hip, each true for a stretch of code and false outside it, whichever way that stretch is left: set by a ModeScope only.
  bool replaying = false;            // inside replay_deferred: the calls run as usual
  bool pipelined_order = false;      // inside the pipelined integrateDepth: marking passes empty their list, EDTs keep it (EsdfArgs)
  struct ModeScope {
    bool* flag = nullptr; ModeScope() = default; explicit ModeScope(bool& f) { enter(f); } ModeScope(const ModeScope&) = delete; ~ModeScope() { leave(); }
    void enter(bool& f) { flag = &f; f = true; }
    void leave() { if (flag) *flag = false; flag = nullptr; }
  };
  int replay_deferred();
  int begin_call_keeping_held() { return begin_call(false); }      // for an entry point that touches nothing the held-back work does: it all stays held back
  // a held-back updateEsdf with NO colour frame in front of it (depth-only hosts, occupancy mappers) that the next camera launch can carry in two-launch order
  bool esdf_only_carry() const { return held.esdf_update_pending && !held.color_pending.on && p.esdf_mode == 0 && p.esdf_propagation == 0 && !held.import_pending && defer_edt; }
  template <int NB> int pending_color_trace_rider(nvbx::TraceRiderT<NB>* out);      // color.hip, for a depth call of NB frames (1 or MAX_BATCH; a held-back call of the other count is refused): set the held-back frame(s) up, the sphere tracing as a rider
  int launch_pending_color_after_trace();
  bool replay_pair_applies() const;  // color.hip: a held-back colour frame + updateEsdf can be replayed in two launches (replay_pair)
  int replay_pair();
// -- fused colour + TSDF launch of the pipelined order (two launches per frame)
  nvbx::DevBuf color_cand;           // int4 [2][capacity] candidate records {slot, block index} of the held-back colour frame (parity cand_parity)
  int cand_parity = 0;
  bool lidar_integrated = false;     // a LiDAR scan has been integrated since the last clear: blocks may be F_BAND_STALE -> no fused launches
  // color.hip: the marking pass that rides in the view-marking launch (0 workgroups: none), and the held-back colour frame's set-up for the fused launch, in its own pixel type
  void pending_marking_args(int32_t* mark_wg, nvbx::EsdfArgs* ea_out, bool single_frame);
  template <int NB> int pending_color_fused_args(nvbx::HeldColorFrames<NB>* out);
  void* table_spare = nullptr; void* table_dirty = nullptr; uint32_t table_mask_extra = 0xFFFFFFFFu;       // decay's rotating hash tables: the all-empty one k_decay builds the next table in, and the one it empties for the call after (maintenance.hip, round 6)
  nvbx::DevBuf view_class;           // LiDAR: per view record, 1 = updated by the beam-centric launch (lidar.hip k_lidar_sparse)
  // LiDAR view calculation over a dense grid (lidar.hip k_mark_view_grid): one byte per block of the box around the sensor (cell-major, 64 B per
  // 4 x 4 x 4 cell) + one byte per cell; all-zero between scans (k_scan_view_grid puts back what the scan set).  `view_grid_dirty`: a scan's
  // launches were not all enqueued (an error return in between) -- the next scan clears the arrays first.
  nvbx::DevBuf view_grid_fine; int64_t view_grid_cells = 0; bool view_grid_dirty = false;      // (view_grid_cells: the cell count the arrays are laid out for)
  int32_t* view_export = nullptr; int64_t view_export_cap = 0;      // nvbx_set_view_export
  int reset_consumed_list();         // empty a consumed dirty list (tiny launch; rare paths only)
  int begin_dirtying() { const int rc = reset_consumed_list(); dirty_since_mark = true; return rc; }
  uint32_t mesh_epoch = 0;
  int mesh_list_live() const { return nvbx::S_LIST_MESH_DIRTY + (int)(mesh_epoch & 1); }   // mesh-dirty list being filled
  int32_t* h_shc = nullptr;          // pinned mirror of d.shc
  int64_t shc_sum(int id, int field) const { int64_t t = 0; for (int s = 0; s < nvbx::NSH; s++) t += h_shc[(id * nvbx::NSH + s) * nvbx::SH_STRIDE + field]; return t; }
  uint32_t last_view_frame = 0;
  // frame stamp of the last CAMERA depth frame: decayTsdfExcludeLastView<Camera> spares the camera's view only -- a LiDAR scan in
  // between must not take its place (nvblox_node.cpp:931-936: 'lidar views are not excluded')
  uint32_t last_camera_view_frame = 0;
  uint32_t last_camera_view_mask = 1;  // camera bit (Entry::stamp) of the last camera of that frame / batch
  int32_t last_view_batch = 1;         // frames in the last depth launch set
  // C-ABI helpers implemented across the .hip files
  nvbx::Frame make_frame(const float T_L_C[16], const nvbx_camera* cam, int32_t rows, int32_t cols, int32_t subsample) const;
  nvbx::EsdfArgs make_esdf_args() const;
  int fetch_counters();              // D2H of all counters + stream sync
  // wait until the mapper's stream has done everything enqueued so far (queries: the slice for a host, counters, nvbx_synchronize)
  int wait_stream();
  // optional per-kernel timing (hipEvent pairs on the mapper stream), used by bench.py for the roofline line
  bool profiling = false;
  struct Span { const char* name; hipEvent_t a, b; };
  std::vector<Span> spans;
  std::vector<hipEvent_t> event_pool;
  hipEvent_t get_event();
  void span_begin(const char* name, hipStream_t s);
  void span_end(hipStream_t s);
};

// every call that reads the TSDF layer refuses an occupancy mapper: -> 0, or NVBX_E_INVALID with the error set
static inline int tsdf_reader_refused(const nvbx_mapper* m, const char* who) {
  return m->p.projective_layer_type == 1 ? nvbx::refuse(who, ": an occupancy mapper has no TSDF layer") : 0;
}

// THE refusals of a call that writes a sparse voxel volume of its own scan (nvbx_find_frontiers, nvbx_find_changes), in their order: its
// capacity, its count and block arrays, its box -> 0, or NVBX_E_INVALID with the error set
constexpr int64_t NVBX_VOLUME_MAX_BLOCKS = 1ll << 22;      // nvbx_label_components' limit: 2^22 x 512 voxel ids fill int32
static inline int sparse_volume_refused(const char* who, const int32_t* box, const void* block_idx, const void* label, int64_t capacity, const void* count) {
  if (capacity < 0 || capacity > NVBX_VOLUME_MAX_BLOCKS) return nvbx::refuse(who, ": capacity_blocks must be 0 .. 2^22");
  if (!count) return nvbx::refuse(who, ": the block count pointer is required");
  if (capacity > 0 && (!block_idx || !label)) return nvbx::refuse(who, ": block_idx_dev and label_dev are required with capacity_blocks > 0");
  if (box && (box[0] > box[3] || box[1] > box[4] || box[2] > box[5])) return nvbx::refuse(who, ": box_min_max_vox has min > max on an axis");
  return 0;
}

// every kernel launch of the library goes through this macro (name = the kernel's name in rocprof output)
#define NVBX_LAUNCH(m, kernel, grid, block, ...) NVBX_LAUNCH_SMEM(m, kernel, grid, block, 0, __VA_ARGS__)
// (... with `smem` bytes of dynamic LDS per workgroup)
#define NVBX_LAUNCH_SMEM(m, kernel, grid, block, smem, ...)                          \
  do {                                                                               \
    if ((m)->profiling) (m)->span_begin(#kernel, (m)->stream);                       \
    (m)->enqueue_seq++;                                                              \
    hipLaunchKernelGGL(kernel, grid, block, (smem), (m)->stream, __VA_ARGS__);       \
    if ((m)->profiling) (m)->span_end((m)->stream);                                  \
  } while (0)

#define NVBX_HIP(call)                                                 \
  do {                                                                 \
    hipError_t e_ = (call);                                            \
    if (e_ != hipSuccess) { nvbx::set_error(#call, e_); return NVBX_E_DEVICE; } \
  } while (0)
