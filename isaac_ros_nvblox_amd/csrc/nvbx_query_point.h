// nvbx_query_point.h -- one lane's interpolated point query: the block probes, the eight-corner fetch and the interpolant with its gradient.
// Device code shared by k_query_points (query.hip), k_align_accumulate (align.hip) and k_score_poses (relocalize.hip), so the three agree bit
// for bit by construction; the arithmetic itself is the inline code of include/nvblox_hip_device.h.  q_color, at the end, is the colour layer's
// interpolant on the same lattice, shared by k_query_colors (color_query.hip) and the colour term of k_align_accumulate.
#pragma once
#include "nvbx_internal.h"
#include "../../include/nvblox_hip_device.h"

namespace nvbx {

enum { Q_TSDF = 0, Q_ESDF3 = 1, Q_ESDF2 = 2 };

// slot of block (x, y, z) if it carries `flag`, else SLOT_NONE -- one 16-B entry load per probe (the table is not written while a
// query runs: every writer is stream-ordered before it)
__device__ inline uint32_t q_probe(const DMap& m, int32_t x, int32_t y, int32_t z, uint32_t flag) {
  const u64 key = pack_key(x, y, z);
  uint32_t h = table_pos(m, x, y, z);
  for (uint32_t probe = 0; probe <= m.mask; ++probe) {
    const uint4 e = ld_entry(m, h);
    const u64 k = ((u64)e.y << 32) | (u64)e.x;
    if (k == key) return (slot_ok(e.z) && (m.slot_flags[e.z] & flag)) ? e.z : SLOT_NONE;
    if (k == KEY_EMPTY) return SLOT_NONE;
    h = (h + 1) & m.mask;
  }
  return SLOT_NONE;
}

// the probe of a lane that needs the block, SLOT_NONE for one that does not (every lane probes on its own: a wave-level de-duplication of the
// probes was measured slower on coherent and uniform batches alike)
__device__ inline uint32_t q_lookup(const DMap& m, bool need, int32_t x, int32_t y, int32_t z, uint32_t flag) {
  uint32_t s = SLOT_NONE;
  if (need) s = q_probe(m, x, y, z, flag);
  return s;
}

// DIST_ONLY's memory of the lane's last base block: a lane that walks neighbouring points probes the hash only when the base corner leaves
// that block (k_view_gain's scheme).  A missing block is remembered as well.  (bx = INT32_MIN: nothing yet -- no block has that index.)
struct QBlockCache { int32_t bx = INT32_MIN, by = 0, bz = 0; uint32_t slot = SLOT_NONE; };

// The query at p: returns valid; *d = the interpolant or `unknown`, g = its gradient per metre or 0.  `pool` = the layer's voxels (TSDF: m.tsdf as
// uint2).  Corner (i, j, k) of the lane: block offset o = (i & cx) | (j & cy) << 1 | (k & cz) << 2 from the base block.
// DIST_ONLY (a further instantiation; the others compile to what they were): the distance alone -- g is not touched and may be null, the gradient's
// arithmetic is dead code, *d_out has the same bits -- and the base block's slot comes from `cache` while the base corner stays in one block.
// slots_out (null in every caller but the colour alignment; a constant after inlining): the eight block slots sl[o] the lane resolved, for q_color.
template <int KIND, bool DIST_ONLY = false>
__device__ inline bool q_point(const DMap& m, const uint2* pool, const float p[3], float vs, float min_weight, float unknown, int32_t plane_vz,
                               float* d_out, float g[3], QBlockCache* cache = nullptr, uint32_t* slots_out = nullptr) {
  constexpr uint32_t FLAG = KIND == Q_TSDF ? F_TSDF : F_ESDF;
  constexpr int NC = KIND == Q_ESDF2 ? 4 : 8;
  int32_t b[3] = {0, 0, plane_vz}; float t[3] = {0.0f, 0.0f, 0.0f};
  bool ok = nvbx_interp_axis(p[0], vs, &b[0], &t[0]) && nvbx_interp_axis(p[1], vs, &b[1], &t[1]);
  if (KIND != Q_ESDF2) ok = ok && nvbx_interp_axis(p[2], vs, &b[2], &t[2]);
  const int32_t bx = b[0] >> 3, by = b[1] >> 3, bz = b[2] >> 3;
  const int vx = b[0] & 7, vy = b[1] & 7, vz = b[2] & 7;
  const int cx = vx == 7, cy = vy == 7, cz = KIND != Q_ESDF2 && vz == 7;
  const int cross = cx | (cy << 1) | (cz << 2);
  // slots of the blocks the corners lie in (o: constant index -> registers)
  uint32_t sl[8];
#pragma unroll
  for (int o = 0; o < 8; o++) {
    sl[o] = SLOT_NONE;
    if (KIND == Q_ESDF2 && (o & 4)) continue;
    const bool need = ok && (o & ~cross) == 0;
    if (DIST_ONLY && o == 0) {
      if (need) {
        if (cache->bx != bx || cache->by != by || cache->bz != bz) { cache->slot = q_probe(m, bx, by, bz, FLAG); cache->bx = bx; cache->by = by; cache->bz = bz; }
        sl[0] = cache->slot;
      }
      continue;
    }
    sl[o] = q_lookup(m, need, bx + (o & 1), by + ((o >> 1) & 1), bz + (o >> 2), FLAG);
  }
  if (slots_out) {
#pragma unroll
    for (int o = 0; o < 8; o++) slots_out[o] = sl[o];
  }
  // corner values; the pair along the layout's fastest axis (TSDF z, ESDF x) is one 16-B load when it stays inside a block
  float c[8];
  bool all = ok;
#pragma unroll
  for (int q = 0; q < NC / 2; q++) {
    uint2 e0, e1; uint32_t s0, s1;
    if (KIND == Q_TSDF) {          // q = i + 2j: corners (i, j, 0) and (i, j, 1)
      const int i_ = q & 1, j_ = q >> 1;
      const int o = (i_ & cx) | ((j_ & cy) << 1);
      s0 = o == 0 ? sl[0] : o == 1 ? sl[1] : o == 2 ? sl[2] : sl[3];
      s1 = cz ? (o == 0 ? sl[4] : o == 1 ? sl[5] : o == 2 ? sl[6] : sl[7]) : s0;
      const int xx = (vx + i_) & 7, yy = (vy + j_) & 7;
      const size_t v0 = (size_t)s0 * 512 + vz + 8 * yy + 64 * xx;
      if (!cz) {
        if (slot_ok(s0)) { const uint4 w = ld_pair(pool + v0); e0 = make_uint2(w.x, w.y); e1 = make_uint2(w.z, w.w); } else { e0 = e1 = make_uint2(0, 0); }
      } else {
        e0 = slot_ok(s0) ? pool[v0] : make_uint2(0, 0);
        e1 = slot_ok(s1) ? pool[(size_t)s1 * 512 + 8 * yy + 64 * xx] : make_uint2(0, 0);
      }
      const float2 f0 = make_float2(__uint_as_float(e0.x), __uint_as_float(e0.y)), f1 = make_float2(__uint_as_float(e1.x), __uint_as_float(e1.y));
      all = all && slot_ok(s0) && slot_ok(s1) && f0.y >= min_weight && f1.y >= min_weight;
      c[i_ + 2 * j_] = f0.x; c[i_ + 2 * j_ + 4] = f1.x;
    } else {                       // q = j + 2k: corners (0, j, k) and (1, j, k)
      const int j_ = q & 1, k_ = q >> 1;
      const int o = ((j_ & cy) << 1) | ((k_ & cz) << 2);
      s0 = o == 0 ? sl[0] : o == 2 ? sl[2] : o == 4 ? sl[4] : sl[6];
      s1 = cx ? (o == 0 ? sl[1] : o == 2 ? sl[3] : o == 4 ? sl[5] : sl[7]) : s0;
      const int yy = (vy + j_) & 7, zz = (vz + k_) & 7;
      const size_t v0 = (size_t)s0 * 512 + vx + 8 * yy + 64 * zz;
      if (!cx) {
        if (slot_ok(s0)) { const uint4 w = ld_pair(pool + v0); e0 = make_uint2(w.x, w.y); e1 = make_uint2(w.z, w.w); } else { e0 = e1 = make_uint2(0, 0); }
      } else {
        e0 = slot_ok(s0) ? pool[v0] : make_uint2(0, 0);
        e1 = slot_ok(s1) ? pool[(size_t)s1 * 512 + 8 * yy + 64 * zz] : make_uint2(0, 0);
      }
      float d0 = 0.0f, d1 = 0.0f;
      const bool o0 = nvbx_interp_esdf_value(e0, vs, &d0), o1 = nvbx_interp_esdf_value(e1, vs, &d1);
      all = all && slot_ok(s0) && slot_ok(s1) && o0 && o1;
      c[2 * j_ + 4 * k_] = d0; c[2 * j_ + 4 * k_ + 1] = d1;
    }
  }
  float d = unknown;
  float g_unused[3];
  if (DIST_ONLY) g = g_unused; else g[0] = g[1] = g[2] = 0.0f;
  if (all) d = KIND == Q_ESDF2 ? nvbx_interp_bilinear(c, t[0], t[1], vs, g) : nvbx_interp_trilinear(c, t[0], t[1], t[2], vs, g);
  *d_out = d;
  return all;
}

// luminance of a colour voxel's packed rgba8 word (r in the low byte), in levels
__device__ inline float q_luma(uint32_t rgba) { return luma_levels(rgba & 0xFFu, (rgba >> 8) & 0xFFu, (rgba >> 16) & 0xFFu); }

// The colour interpolant at p (k_query_colors, color_query.hip; k_align_accumulate<.., true>, align.hip): the TSDF query's lattice and its inline
// interpolant over the luminance of the eight colour voxels.  A corner counts when its block carries F_COLOR and its voxel's weight is
// >= min_color_weight; returns valid, *y_out = Y(p) in levels or 0, gy = dY/dp per metre or 0; RGB: rgb[ch] = the same interpolant of channel ch.
// tsdf_slots: what q_point<Q_TSDF> left in slots_out for this p, or null.  A slot found there needs one flag load and no probe; a corner block
// without one (or every block, when null) is probed for F_COLOR.
template <bool RGB>
__device__ inline bool q_color(const DMap& m, const float p[3], float vs, float min_color_weight, const uint32_t* tsdf_slots, float* y_out,
                               float gy[3], float rgb[3]) {
  int32_t b[3] = {0, 0, 0}; float t[3] = {0.0f, 0.0f, 0.0f};
  const bool ok = nvbx_interp_axis(p[0], vs, &b[0], &t[0]) && nvbx_interp_axis(p[1], vs, &b[1], &t[1]) && nvbx_interp_axis(p[2], vs, &b[2], &t[2]);
  const int32_t bx = b[0] >> 3, by = b[1] >> 3, bz = b[2] >> 3;
  const int vx = b[0] & 7, vy = b[1] & 7, vz = b[2] & 7;
  const int cx = vx == 7, cy = vy == 7, cz = vz == 7;
  const int cross = cx | (cy << 1) | (cz << 2);
  uint32_t sl[8];
#pragma unroll
  for (int o = 0; o < 8; o++) {
    uint32_t s = SLOT_NONE;
    if (ok && (o & ~cross) == 0) {
      s = tsdf_slots ? tsdf_slots[o] : SLOT_NONE;
      if (!slot_ok(s)) s = q_probe(m, bx + (o & 1), by + ((o >> 1) & 1), bz + (o >> 2), F_COLOR);
      else if (!(m.slot_flags[s] & F_COLOR)) s = SLOT_NONE;
    }
    sl[o] = s;
  }
  const uint2* pool = m.color;
  float c[8], cr[8], cg[8], cb[8];
  bool all = ok;
#pragma unroll
  for (int q = 0; q < 4; q++) {          // q = i + 2j: corners (i, j, 0) and (i, j, 1), as the TSDF path of q_point
    const int i_ = q & 1, j_ = q >> 1;
    const int o = (i_ & cx) | ((j_ & cy) << 1);
    const uint32_t s0 = o == 0 ? sl[0] : o == 1 ? sl[1] : o == 2 ? sl[2] : sl[3];
    const uint32_t s1 = cz ? (o == 0 ? sl[4] : o == 1 ? sl[5] : o == 2 ? sl[6] : sl[7]) : s0;
    const int xx = (vx + i_) & 7, yy = (vy + j_) & 7;
    const size_t v0 = (size_t)s0 * 512 + vz + 8 * yy + 64 * xx;
    uint2 e0, e1;
    if (!cz) {
      if (slot_ok(s0)) { const uint4 w = ld_pair(pool + v0); e0 = make_uint2(w.x, w.y); e1 = make_uint2(w.z, w.w); } else { e0 = e1 = make_uint2(0, 0); }
    } else {
      e0 = slot_ok(s0) ? pool[v0] : make_uint2(0, 0);
      e1 = slot_ok(s1) ? pool[(size_t)s1 * 512 + 8 * yy + 64 * xx] : make_uint2(0, 0);
    }
    all = all && slot_ok(s0) && slot_ok(s1) && __uint_as_float(e0.y) >= min_color_weight && __uint_as_float(e1.y) >= min_color_weight;
    c[q] = q_luma(e0.x); c[q + 4] = q_luma(e1.x);
    if (RGB) {
      cr[q] = (float)(e0.x & 0xFFu); cg[q] = (float)((e0.x >> 8) & 0xFFu); cb[q] = (float)((e0.x >> 16) & 0xFFu);
      cr[q + 4] = (float)(e1.x & 0xFFu); cg[q + 4] = (float)((e1.x >> 8) & 0xFFu); cb[q + 4] = (float)((e1.x >> 16) & 0xFFu);
    }
  }
  float y = 0.0f;
  gy[0] = gy[1] = gy[2] = 0.0f;
  if (RGB) rgb[0] = rgb[1] = rgb[2] = 0.0f;
  if (all) {
    y = nvbx_interp_trilinear(c, t[0], t[1], t[2], vs, gy);
    if (RGB) {
      float g_unused[3];
      rgb[0] = nvbx_interp_trilinear(cr, t[0], t[1], t[2], vs, g_unused);
      rgb[1] = nvbx_interp_trilinear(cg, t[0], t[1], t[2], vs, g_unused);
      rgb[2] = nvbx_interp_trilinear(cb, t[0], t[1], t[2], vs, g_unused);
    }
  }
  *y_out = y;
  return all;
}

}  // namespace nvbx
