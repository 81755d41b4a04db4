/* nvbx_knobs.h -- the environment knobs of the launch geometry and the A/B switches, parsed in one place (plain C: the host code includes it, and
 * tests/test_knobs.py compiles THIS file with gcc and checks the mapping on the CPU).  Each nvbx_knob_* function takes the variable's value (NULL when
 * unset) and returns what the library uses.  A missing, malformed or out-of-range value gives the default, so no setting can size a launch at zero
 * or drop work; rider counts are rounded up to a multiple of 8.  No knob changes a result, only which workgroup does what.
 * struct nvbx_knobs holds one mapper's settings; nvbx_knobs_read fills it, and names every variable there and nowhere else.  The cost field's two
 * knobs have a struct and a read of their own in front of it (nvbx_plan_knobs), and so have change detection's one (nvbx_change_knobs) and
 * resampling's one (nvbx_resample_knobs). */
#ifndef NVBX_KNOBS_H_
#define NVBX_KNOBS_H_
#include <errno.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#define NVBX_KNOB_GRID_MAX (1 << 20)      /* workgroups of one part of a launch */
#define NVBX_KNOB_RIDERS_MAX (1 << 16)    /* rider workgroups of one held-back pass */
#define NVBX_KNOB_SCORE_CHUNKS_MAX 1024   /* point chunks of a pose (relocalize.hip: SCORE_MAX_CHUNKS) */

/* s as a whole decimal integer in [lo, hi]; anything else: def */
static inline int nvbx_knob_int(const char* s, int def, int lo, int hi) {
  if (!s || !*s) return def;
  char* end = NULL;
  errno = 0;
  const long v = strtol(s, &end, 10);
  if (errno || end == s || *end || v < lo || v > hi) return def;
  return (int)v;
}
/* a rider count: at least 8, rounded up to a multiple of 8 */
static inline int nvbx_knob_riders(const char* s, int def) {
  const int v = nvbx_knob_int(s, def, 8, NVBX_KNOB_RIDERS_MAX);
  return (v + 7) / 8 * 8;
}
/* an A/B switch: 0 or 1, default on */
static inline int nvbx_knob_switch(const char* s) { return nvbx_knob_int(s, 1, 0, 1); }

/* NVBX_INTEG_GRID: cap on the TSDF update's workgroups; 0 = the built-in cap (1024 for one camera, 512 for a batch) */
static inline int nvbx_knob_integ_grid(const char* s) { return nvbx_knob_int(s, 0, 1, NVBX_KNOB_GRID_MAX); }
/* NVBX_GRID_MARGIN = "percent[,blocks]": a grid sized from a reported count n covers n + n * percent / 100 + blocks; each part falls back on its own */
static inline void nvbx_knob_grid_margin(const char* s, int* pct, int* blocks) {
  char head[24];
  const char* comma = s ? strchr(s, ',') : NULL;
  *pct = 25; *blocks = 64;
  if (!s) return;
  if (!comma) { *pct = nvbx_knob_int(s, 25, 0, 10000); return; }
  if ((size_t)(comma - s) < sizeof(head)) {
    memcpy(head, s, (size_t)(comma - s)); head[comma - s] = 0;
    *pct = nvbx_knob_int(head, 25, 0, 10000);
  }
  *blocks = nvbx_knob_int(comma + 1, 64, 0, NVBX_KNOB_GRID_MAX);
}
/* NVBX_COLOR_GRID: cap on the colour part's workgroups in the fused launch */
static inline int nvbx_knob_color_grid(const char* s) { return nvbx_knob_int(s, 1024, 1, NVBX_KNOB_GRID_MAX); }
/* NVBX_EDT_RIDERS: distance-transform riders of the fused launch (a held-back updateEsdf) */
static inline int nvbx_knob_edt_riders(const char* s) { return nvbx_knob_riders(s, 256); }
/* NVBX_PAIR_B_EDT_RIDERS: at most this many for the second mapper of a depth pair */
static inline int nvbx_knob_pair_b_edt_riders(const char* s) { return nvbx_knob_riders(s, 64); }
/* NVBX_MARK_RIDERS: marking-pass riders, rounded up to a multiple of 8; 0 = sized from the view count the GPU last reported */
static inline int nvbx_knob_mark_riders(const char* s) { const int v = nvbx_knob_int(s, 0, 1, NVBX_KNOB_RIDERS_MAX); return (v + 7) / 8 * 8; }
/* NVBX_MARK_TILES_FIRST: 1 = tile workgroups before the riders of the view-marking launch, 0 = after; -1 = by batch size */
static inline int nvbx_knob_mark_tiles_first(const char* s) { return nvbx_knob_int(s, -1, 0, 1); }
/* NVBX_DECAY_GRID: cap on k_decay's decaying workgroups */
static inline int nvbx_knob_decay_grid(const char* s) { return nvbx_knob_int(s, 4096, 1, NVBX_KNOB_GRID_MAX); }
/* NVBX_ST_LANES: lanes per ray of a batch's sphere tracing, 1 / 2 / 4 / 8; 0 = by camera count */
static inline int nvbx_knob_st_lanes(const char* s) {
  const int v = nvbx_knob_int(s, 0, 1, 8);
  return (v == 1 || v == 2 || v == 4 || v == 8) ? v : 0;
}
/* NVBX_RENDER_LANES: lanes per ray of nvbx_render_view / nvbx_cast_rays, 1 / 2 / 4 / 8; 0 = by ray count */
static inline int nvbx_knob_render_lanes(const char* s) { return nvbx_knob_st_lanes(s); }
/* NVBX_FUSED_TRACE_LANES: lanes per ray of one frame's riding sphere tracing, 4 or 8 */
static inline int nvbx_knob_fused_trace_lanes(const char* s) { return nvbx_knob_int(s, 8, 4, 8) == 4 ? 4 : 8; }
/* NVBX_LIDAR_SPARSE_GRID: workgroups of the beam-centric LiDAR launch */
static inline int nvbx_knob_lidar_sparse_grid(const char* s) { return nvbx_knob_int(s, 2048, 1, NVBX_KNOB_GRID_MAX); }
/* NVBX_COLOR_DEFERRAL: a new mapper's colour deferral, 0 off / 1 zero-copy / 2 staged; -1 = unset (the library's default, staged) */
static inline int nvbx_knob_color_deferral(const char* s) { return nvbx_knob_int(s, -1, 0, 2); }
/* NVBX_SCORE_CHUNKS: point chunks per pose of k_score_poses, 1 = one workgroup per pose; 0 = the launch's own choice */
static inline int nvbx_knob_score_chunks(const char* s) { return nvbx_knob_int(s, 0, 1, NVBX_KNOB_SCORE_CHUNKS_MAX); }
/* NVBX_VIEW_GRID_REACH: cap, in blocks, on the half side of the LiDAR view grid's box; 0 = no cap */
static inline int nvbx_knob_view_grid_reach(const char* s) { return nvbx_knob_int(s, 0, 1, 1 << 20); }
/* NVBX_VIEW_GRID_MAX_MB: the largest LiDAR view grid, in MiB, that is allocated */
static inline int nvbx_knob_view_grid_max_mb(const char* s) { return nvbx_knob_int(s, 128, 1, 1 << 20); }
/* NVBX_MAX_BLOCKS: bound of the pools' growth (the mapper clamps it to [initial capacity, 2^24]); 0 = the built-in bound */
static inline int nvbx_knob_max_blocks(const char* s) { return nvbx_knob_int(s, 0, 1, INT_MAX); }
/* NVBX_FRAME_POOL_MAX: frames per image size in the library's pool (process-wide, frames.hip); an integer below 2 gives 2 */
static inline int nvbx_knob_frame_pool_max(const char* s) { const int v = nvbx_knob_int(s, 8, INT_MIN, 1 << 16); return v < 2 ? 2 : v; }

/* The cost field's knobs (plan.hip), a struct and a read of their own beside the mapper's: filled where nvbx_knobs is, through the
 * same lookup.  NVBX_PLAN_ROUNDS_PER_WAIT: relaxation rounds enqueued between two reads of the changed counter; NVBX_PLAN_TILE_SWEEPS: sweeps a
 * workgroup makes over its tile before it stores it and asks for another round.  No result depends on either. */
static inline int nvbx_knob_plan_rounds_per_wait(const char* s) { return nvbx_knob_int(s, 16, 1, 1024); }
static inline int nvbx_knob_plan_tile_sweeps(const char* s) { return nvbx_knob_int(s, 64, 1, 4096); }
struct nvbx_plan_knobs { int rounds_per_wait, tile_sweeps; };
static inline void nvbx_plan_knobs_read(struct nvbx_plan_knobs* k, const char* (*lookup)(const char* name)) {
  k->rounds_per_wait = nvbx_knob_plan_rounds_per_wait(lookup("NVBX_PLAN_ROUNDS_PER_WAIT"));
  k->tile_sweeps = nvbx_knob_plan_tile_sweeps(lookup("NVBX_PLAN_TILE_SWEEPS"));
}

/* Change detection's knob (change.hip), in a struct and a read of its own like the cost field's: NVBX_CHANGE_GRID caps
 * k_find_changes' workgroups, as NVBX_DECAY_GRID caps k_decay's.  No result depends on it. */
static inline int nvbx_knob_change_grid(const char* s) { return nvbx_knob_int(s, 1024, 1, NVBX_KNOB_GRID_MAX); }      /* (256 CUs x 4 resident workgroups) */
struct nvbx_change_knobs { int grid; };
static inline void nvbx_change_knobs_read(struct nvbx_change_knobs* k, const char* (*lookup)(const char* name)) {
  k->grid = nvbx_knob_change_grid(lookup("NVBX_CHANGE_GRID"));
}

/* Resampling's knob (resample.hip), likewise: NVBX_RESAMPLE_GRID caps k_resample_fuse's workgroups (the default is the cap
 * k_merge_fuse has built in).  No result depends on it. */
static inline int nvbx_knob_resample_grid(const char* s) { return nvbx_knob_int(s, 2048, 1, NVBX_KNOB_GRID_MAX); }
struct nvbx_resample_knobs { int grid; };
static inline void nvbx_resample_knobs_read(struct nvbx_resample_knobs* k, const char* (*lookup)(const char* name)) {
  k->grid = nvbx_knob_resample_grid(lookup("NVBX_RESAMPLE_GRID"));
}

/* One mapper's knobs: filled at nvbx_mapper_create and again by nvbx_mapper_reload_knobs.  Three of them shape the mapper at creation and are
 * not applied to a live one: max_blocks, color_deferral, defer_edt (include/nvblox_hip.h). */
struct nvbx_knobs {
  /* A/B switches */
  int fuse_colc, depth_pair, lidar_sparse, lidar_dense_list, lidar_view_grid, defer_edt, replay_pair, esdf_only_carry;      /* default on */
  int color_deferral, mark_tiles_first;                                                                                    /* -1 = unset */
  /* launch geometry */
  int integ_grid, color_grid, decay_grid, lidar_sparse_grid, grid_margin_pct, grid_margin_blocks;
  int edt_riders, pair_b_edt_riders, mark_riders;
  int st_lanes, fused_trace_lanes, render_lanes, score_chunks;
  /* sizes */
  int view_grid_reach, view_grid_max_mb, max_blocks;
};
/* lookup(name): the variable's value, or NULL when it is unset (the library hands in the environment's, the test a table) */
static inline void nvbx_knobs_read(struct nvbx_knobs* k, const char* (*lookup)(const char* name)) {
  k->fuse_colc = nvbx_knob_switch(lookup("NVBX_FUSE_COLC"));
  k->depth_pair = nvbx_knob_switch(lookup("NVBX_DEPTH_PAIR"));
  k->lidar_sparse = nvbx_knob_switch(lookup("NVBX_LIDAR_SPARSE"));
  k->lidar_dense_list = nvbx_knob_switch(lookup("NVBX_LIDAR_DENSE_LIST"));
  k->lidar_view_grid = nvbx_knob_switch(lookup("NVBX_LIDAR_VIEW_GRID"));
  k->defer_edt = nvbx_knob_switch(lookup("NVBX_DEFER_EDT"));
  k->replay_pair = nvbx_knob_switch(lookup("NVBX_REPLAY_PAIR"));
  k->esdf_only_carry = nvbx_knob_switch(lookup("NVBX_ESDF_ONLY_CARRY"));
  k->color_deferral = nvbx_knob_color_deferral(lookup("NVBX_COLOR_DEFERRAL"));
  k->mark_tiles_first = nvbx_knob_mark_tiles_first(lookup("NVBX_MARK_TILES_FIRST"));
  k->integ_grid = nvbx_knob_integ_grid(lookup("NVBX_INTEG_GRID"));
  k->color_grid = nvbx_knob_color_grid(lookup("NVBX_COLOR_GRID"));
  k->decay_grid = nvbx_knob_decay_grid(lookup("NVBX_DECAY_GRID"));
  k->lidar_sparse_grid = nvbx_knob_lidar_sparse_grid(lookup("NVBX_LIDAR_SPARSE_GRID"));
  nvbx_knob_grid_margin(lookup("NVBX_GRID_MARGIN"), &k->grid_margin_pct, &k->grid_margin_blocks);
  k->edt_riders = nvbx_knob_edt_riders(lookup("NVBX_EDT_RIDERS"));
  k->pair_b_edt_riders = nvbx_knob_pair_b_edt_riders(lookup("NVBX_PAIR_B_EDT_RIDERS"));
  k->mark_riders = nvbx_knob_mark_riders(lookup("NVBX_MARK_RIDERS"));
  k->st_lanes = nvbx_knob_st_lanes(lookup("NVBX_ST_LANES"));
  k->fused_trace_lanes = nvbx_knob_fused_trace_lanes(lookup("NVBX_FUSED_TRACE_LANES"));
  k->render_lanes = nvbx_knob_render_lanes(lookup("NVBX_RENDER_LANES"));
  k->score_chunks = nvbx_knob_score_chunks(lookup("NVBX_SCORE_CHUNKS"));
  k->view_grid_reach = nvbx_knob_view_grid_reach(lookup("NVBX_VIEW_GRID_REACH"));
  k->view_grid_max_mb = nvbx_knob_view_grid_max_mb(lookup("NVBX_VIEW_GRID_MAX_MB"));
  k->max_blocks = nvbx_knob_max_blocks(lookup("NVBX_MAX_BLOCKS"));
}
#endif
