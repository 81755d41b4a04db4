/* nvbx_knobs.h -- the environment knobs of the launch geometry and the A/B switches, parsed in one place (plain C: the host code includes it, and
 * tests/test_knobs.py compiles THIS file with gcc and checks the mapping on the CPU).  Each function takes the variable's value (getenv's result, NULL
 * when unset) and returns what the library uses.  A missing, malformed or out-of-range value gives the default, so no setting can size a launch at zero
 * or drop work; rider counts are rounded up to a multiple of 8.  No knob changes a result, only which workgroup does what. */
#ifndef NVBX_KNOBS_H_
#define NVBX_KNOBS_H_
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#define NVBX_KNOB_GRID_MAX (1 << 20)      /* workgroups of one part of a launch */
#define NVBX_KNOB_RIDERS_MAX (1 << 16)    /* rider workgroups of one held-back pass */

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
/* NVBX_FUSE_COLC, NVBX_DEPTH_PAIR, NVBX_LIDAR_SPARSE, NVBX_LIDAR_DENSE_LIST, NVBX_DEFER_EDT: nvbx_knob_switch */
#endif
