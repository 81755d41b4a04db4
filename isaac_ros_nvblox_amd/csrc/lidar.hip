// lidar.hip -- the spinning LiDAR's own launches (range image; nvblox_ros/src/lib/nvblox_node.cpp:1382-1384): the view calculation over a
// dense "seen in this scan" grid (k_mark_view_grid, k_scan_view_grid, k_resolve_view), the beam-centric far-field TSDF update (k_lidar_sparse),
// the beam direction tables, nvbx_integrate_lidar_depth and nvbx_depth_image_from_pointcloud.  A scan runs through the depth-frame state machine
// of tsdf.hip (integrate_lidar_frame), which calls launch_view_grid / launch_lidar_sparse below where a camera frame has nothing to launch; the
// fallback view marking (k_mark_view<.., LidarSensor, 1>) and the dense TSDF update of a scan are launched there.
#define NVBX_WGT_HERE
#include "nvbx_view.h"

#ifdef NVBX_WG_TIMES
int wgt_bind_lidar(unsigned long long* buf) { return hipMemcpyToSymbol(HIP_SYMBOL(g_wgt), &buf, sizeof(buf)) == hipSuccess ? 0 : -1; }
#endif

// ------------------------------------------------------------------------------------------------ LiDAR view calculation over a dense "seen in this scan" grid
// A 200 m scan walks its 16 k (sub-sampled) rays through ~10^6 blocks to find the ~112 k distinct ones.  k_mark_view<Lidar> (nvbx_view.h) decides "first
// ray through this block?" with one compare-and-swap per key on the hash entry's stamp; a first version of this path decided it with one returning
// atomicOr per key on a bit of a dense grid.  Both take ~58 us, and the per-bundle time stamps (tools/wg_timeline_lidar_grid.py) say why: a bundle
// with ONE far key waits 30-40 us for its atomic like a bundle with 500 -- ~10^5 returning atomics on scattered addresses are served at ~3 G/s by the
// memory side, whoever issues them.  So the marking launch issues NO atomic at all:
//   k_mark_view_grid : the walk (same code as k_mark_view: view_ray_setup, dda_jump, dda_step); a visited block is a plain STORE of 1 to its byte of a
//                      dense grid around the sensor (idempotent: any number of rays may visit) + a store of 1 to the byte of its 4 x 4 x 4 cell in
//                      a coarse map.  The grid is cell-major -- the 64 bytes of a cell are one 64-B line.  (Every visit stores: ~700 k redundant byte
//                      stores around the sensor cost less than looking first -- VG_NEAR > 0 builds the look-before-store variant, measured slower.)
//   k_scan_view_grid : reads the coarse map (0.8 MB for a 200 m box at 0.8 m blocks), the lines of the touched cells, and appends {tag, x, y, z} per
//                      set byte to the view list -- one reservation per wavefront -- and puts every byte it found back to 0: the grid is all-zero
//                      again when the scan's launches are done.
//   k_resolve_view   : one lane per tagged record: hash lookup or insert (the wavefront's new blocks pop their slots together), entry stamp, slot
//                      written into the record.
// Blocks outside the box (none, if the box was sized from the sensor's range: a ray then ends inside by construction) take mark_block directly.
// Same block set as k_mark_view<Lidar>; only the de-duplication differs.
struct ViewGrid {
  uint8_t* fine;           // byte cell * 64 + (lx & 3) + 4 (ly & 3) + 16 (lz & 3), cell = ((lz >> 2) * ncy + (ly >> 2)) * ncx + (lx >> 2), l = block - o
  uint8_t* coarse;         // byte per cell (padded to a multiple of 4)
  int32_t ox, oy, oz;      // block index of the box's minimum corner
  int32_t ncx, ncy, ncz;   // cells per axis (<= 256: local block coordinates are 10 bits)
  int32_t cx, cy, cz;      // the sensor's block
  uint32_t tag;            // slot field of a record waiting for k_resolve_view: 0x80000000 | view frame id (never a slot: capacity <= 2^24)
};
#ifndef NVBX_VG_NEAR
#define NVBX_VG_NEAR 0              // (0: every visit stores.  24 / 48: 19.3 / 19.9 us for the launch instead of 16.6 -- the stores were never what waited)
#define NVBX_VG_CHUNK 16
#endif
constexpr int VG_NEAR = NVBX_VG_NEAR, VG_CHUNK = NVBX_VG_CHUNK;
constexpr uint32_t VG_NONE = 0xFFFFFFFFu;

#ifndef NVBX_VIEW_GRID_ATTR
#define NVBX_VIEW_GRID_ATTR
#endif
template <typename Img>
__global__ __launch_bounds__(64) NVBX_VIEW_GRID_ATTR void k_mark_view_grid(DMap m, FrameSet<Img, 1> fs, LidarSensor sensor, int4* view_list, int32_t list_cap,
                                                       int32_t reset_esdf_dirty, int32_t fence_report, ViewGrid vg) {
  constexpr int TR = LidarSensor::kTileRows, TC = LidarSensor::kTileCols, NSEG = LidarSensor::kSegments, C = VG_CHUNK;
  static_assert(TR * TC * NSEG <= 64, "one wavefront per bundle of rays");
  const int lane = (int)threadIdx.x;
  const Frame& f = fs.f[0];
  const Img& depth = fs.img[0];
  NVBX_T(0, 0);
  if (blockIdx.x == 0 && lane == 0) __hip_atomic_store(&m.host_mirror[4], fence_report, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);    // (k_mark_view: frames.hip's fence)
  // XCD-aware numbering, as k_mark_view: the bundles of one XCD are a contiguous band of ray rows
  const int tiles_x = (f.n_ray_cols + TC - 1) / TC, tiles_y = (f.n_ray_rows + TR - 1) / TR;
  const int n_tiles = tiles_x * tiles_y, per_xcd = (n_tiles + NSH - 1) / NSH;
  const int wg = (int)blockIdx.x;
  const int tile = (wg & (NSH - 1)) * per_xcd + (wg >> 3);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int ray = lane / NSEG, seg = lane % NSEG;
  const int ri = ty * TR + ray / TC, ci = tx * TC + ray % TC;
  bool active = (wg >> 3) < per_xcd && tile < n_tiles && ray < TR * TC && ri < f.n_ray_rows && ci < f.n_ray_cols;
  int prow = ri * f.subsample; if (prow >= f.rows) prow = f.rows - 1;
  int pcol = ci * f.subsample; if (pcol >= f.cols) pcol = f.cols - 1;
  const float d = active ? depth(pix(prow, pcol, f.cols)) : 0.0f;
  if (wg == 0 && lane == 0) m.counters[C_VIEW_COUNT + ((f.frame_id + 1) & 3)] = 0;   // next frame's counter
  if (wg == 0 && lane < NSH) { *shc_at(m, S_LIDAR_SPARSE, lane, 0) = 0; *shc_at(m, S_LIDAR_SPARSE, lane, 1) = 0; }
  if (reset_esdf_dirty && wg == 0 && lane < NSH) *shc_at(m, S_LIST_ESDF_DIRTY, lane, 0) = 0;
  Dda dd{};
  float inv_dt[3] = {0.0f, 0.0f, 0.0f};
  const int32_t nsteps = view_ray_setup(f, sensor, active, d, prow, pcol, dd, inv_dt);
  NVBX_TV(0, 1, wall_clock64() + (unsigned long long)(nsteps & 0));       // (the depth pixel has arrived, the ray is set up)
  int32_t k0 = 0, k1 = nsteps;
  if (NSEG > 1 && nsteps >= 0) {
    const int32_t q = (nsteps + NSEG) / NSEG;
    k0 = seg * q; k1 = min(nsteps, k0 + q - 1);
    if (k0 > nsteps) k1 = -1;
    else if (k0 > 0) dda_jump(dd, k0, inv_dt);
  }
  NVBX_TV(0, 2, wall_clock64() + (unsigned long long)(dd.cur[0] & 0));    // (this lane stands at the start of its segment)
  int32_t* cnt = &m.counters[C_VIEW_COUNT + (f.frame_id & 3)];
  const uint32_t NX = 4u * (uint32_t)vg.ncx, NY = 4u * (uint32_t)vg.ncy, NZ = 4u * (uint32_t)vg.ncz;
  for (int32_t base = k0; __ballot(base <= k1) != 0ull; base += C) {
    uint32_t code[VG_NEAR > 0 ? C : 1], w[VG_NEAR > 0 ? C : 1];
#pragma unroll
    for (int i = 0; i < C; i++) {
      if (VG_NEAR > 0) code[i] = VG_NONE;
      bool spill = false; u64 key = KEY_EMPTY;
      if (base + i <= k1) {
        const int32_t bx = dd.cur[0], by = dd.cur[1], bz = dd.cur[2];
        if (block_in_workspace(f, bx, by, bz)) {
          const uint32_t lx = (uint32_t)(bx - vg.ox), ly = (uint32_t)(by - vg.oy), lz = (uint32_t)(bz - vg.oz);
          if (lx < NX && ly < NY && lz < NZ) {
            const uint32_t cell = ((lz >> 2) * (uint32_t)vg.ncy + (ly >> 2)) * (uint32_t)vg.ncx + (lx >> 2);
            const uint32_t at = cell * 64u + ((lx & 3u) | ((ly & 3u) << 2) | ((lz & 3u) << 4));
            const uint32_t nx = (uint32_t)(bx - vg.cx + VG_NEAR), ny = (uint32_t)(by - vg.cy + VG_NEAR), nz = (uint32_t)(bz - vg.cz + VG_NEAR);
            if (VG_NEAR > 0 && nx < 2u * VG_NEAR && ny < 2u * VG_NEAR && nz < 2u * VG_NEAR) code[VG_NEAR > 0 ? i : 0] = at;      // (looked at first, below)
            else { vg.fine[at] = 1; vg.coarse[cell] = 1; }
          } else { spill = true; key = pack_key(bx, by, bz); }
        }
        dda_step(dd);
      }
      if (__ballot(spill)) {                     // outside the box (a box sized from the sensor's range holds every ray): the hash decides
        int4 rec = make_int4(0, 0, 0, 0);
        const bool first = spill && mark_block(m, key, f.frame_id, f.cam_bit, &rec);
        view_append(cnt, view_list, list_cap, first, rec, lane);
      }
    }
    if (base == k0) NVBX_TV(0, 3, wall_clock64());
    if (VG_NEAR > 0) {
      // near the sensor: the chunk's bytes are loaded together and stored only where they read 0 (a stale 0 costs a store, nothing else)
#pragma unroll
      for (int i = 0; i < C; i++) { w[i] = 1u; if (code[i] != VG_NONE) w[i] = (uint32_t)vg.fine[code[i]]; }
#pragma unroll
      for (int i = 0; i < C; i++) if (code[i] != VG_NONE && !w[i]) { vg.fine[code[i]] = 1; vg.coarse[code[i] >> 6] = 1; }
      if (base == k0) NVBX_TV(0, 4, wall_clock64() + (unsigned long long)(w[0] & 0u));
    }
  }
  NVBX_T(0, 7);
}

// Up to K keys per lane -> pool slots, the dependent round trips taken together: the first PD probe positions of every key, then the inserts of
// the blocks that are new (compare-and-swap on the entries; the wavefront's winners pop their slots with ONE atomicSub on the free-stack top and
// one atomicMax on the high-water mark -- flush_set's B'), then whatever is left (a longer probe chain, a lost insert) by hash_insert.  The caller
// OWNS these keys for the launch (nobody else looks them up or stamps them), so the entry stamp is a plain store.  Whole wavefront must call.
template <int K, int PD, bool STAMP = true>
__device__ inline void resolve_keys(const DMap& m, const u64 (&key)[K], const bool (&valid)[K], uint32_t want, uint32_t (&slot)[K], int lane) {
  uint32_t h[K]; uint4 e[K][PD];
#pragma unroll
  for (int k = 0; k < K; k++) { int32_t x, y, z; unpack_key(key[k], &x, &y, &z); h[k] = valid[k] ? table_pos(m, x, y, z) : 0u; }
#pragma unroll
  for (int k = 0; k < K; k++) if (valid[k]) {
#pragma unroll
    for (int q = 0; q < PD; q++) e[k][q] = ld_entry(m, (h[k] + q) & m.mask);
  }
  bool done[K], ins[K], won[K]; uint32_t hpos[K];
  bool any_ins = false;
#pragma unroll
  for (int k = 0; k < K; k++) {
    done[k] = false; ins[k] = false; won[k] = false; hpos[k] = 0u; slot[k] = SLOT_NONE;
    if (valid[k]) {
      bool open = true; int qe = -1;
#pragma unroll
      for (int q = 0; q < PD; q++) {
        const u64 kq = ((u64)e[k][q].y << 32) | (u64)e[k][q].x;
        if (open && !done[k] && kq == key[k]) { slot[k] = e[k][q].z; hpos[k] = (h[k] + q) & m.mask; done[k] = true; }
        if (open && kq == KEY_EMPTY) { open = false; if (!done[k]) qe = q; }
      }
      if (done[k] && slot[k] == SLOT_INVALID) done[k] = false;            // (being inserted by somebody else right now: hash_insert below waits)
      else if (!done[k] && qe >= 0) { ins[k] = true; any_ins = true; hpos[k] = (h[k] + qe) & m.mask; }
    }
  }
  if (__ballot(any_ins)) {
    u64 oldk[K];
#pragma unroll
    for (int k = 0; k < K; k++) if (ins[k]) oldk[k] = atomicCAS(&m.table[hpos[k]].key, KEY_EMPTY, key[k]);
    int32_t wtotal = 0, wpre[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      won[k] = ins[k] && oldk[k] == KEY_EMPTY;
      const u64 mask = __ballot(won[k]);
      wpre[k] = wtotal + (int32_t)__popcll(mask & ((1ull << lane) - 1ull));
      wtotal += (int32_t)__popcll(mask);
    }
    if (wtotal) {
      int32_t top = 0;
      if (lane == 0) {
        top = atomicSub(&m.counters[C_FREE_TOP], wtotal);
        if (top < wtotal) { atomicAdd(&m.counters[C_FREE_TOP], wtotal - (top > 0 ? top : 0)); atomicExch(&m.counters[C_OVERFLOW], 1); }     // pool exhausted: give back what was not there
      }
      top = __shfl(top, 0);
      int32_t hwm = 0;
#pragma unroll
      for (int k = 0; k < K; k++) if (won[k]) {
        const int32_t idx = top - 1 - wpre[k];
        slot[k] = idx >= 0 ? m.free_stack[idx] : SLOT_NONE;
        if (slot_ok(slot[k])) {
          int32_t x, y, z; unpack_key(key[k], &x, &y, &z);
          m.slot_index[3 * slot[k]] = x; m.slot_index[3 * slot[k] + 1] = y; m.slot_index[3 * slot[k] + 2] = z;
          m.slot_entry[slot[k]] = hpos[k];
          atomicOr(&m.slot_flags[slot[k]], F_TSDF);
          hwm = max(hwm, (int32_t)slot[k] + 1);
        }
        __hip_atomic_store(&m.table[hpos[k]].slot, slot[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        done[k] = true;
      }
#pragma unroll
      for (int o = 32; o; o >>= 1) hwm = max(hwm, __shfl_xor(hwm, o));
      if (lane == 0 && hwm) atomicMax(&m.counters[C_HIGH_WATER], hwm);
    }
  }
#pragma unroll
  for (int k = 0; k < K; k++) if (valid[k]) {
    if (!done[k]) {
      int32_t x, y, z; unpack_key(key[k], &x, &y, &z);
      bool is_new;
      const int32_t hi = hash_insert(m, x, y, z, F_TSDF, &is_new);
      if (hi < 0) { slot[k] = SLOT_NONE; continue; }
      hpos[k] = (uint32_t)hi;
      uint32_t s = SLOT_INVALID;
      while (s == SLOT_INVALID) s = ld_slot_acquire(&m.table[hi]);
      slot[k] = s;
    }
    if (STAMP) m.table[hpos[k]].stamp = want;
  }
}

// The launches behind k_mark_view_grid.  k_scan_view_grid: a wavefront takes four 64-B lines of the coarse map (256 cells; the four lines from
// four far-apart places: the cells around the sensor are all touched and lie in a few hundred neighbouring lines -- taken as consecutive lines they
// gave a few wavefronts 60 cells each and the launch 28 us), lists the touched cells in LDS, reads their lines (four lanes x 16 bytes per cell,
// sixteen cells per round) once to count and once more -- from the L2 -- to write {tag, x, y, z} per set byte behind ONE reservation; whatever it
// found set goes back to 0.
__device__ inline int32_t vg_nonzero_bytes(uint32_t b) { return (int32_t)((b & 0xFFu) != 0u) + (int32_t)((b & 0xFF00u) != 0u) + (int32_t)((b & 0xFF0000u) != 0u) + (int32_t)((b >> 24) != 0u); }
constexpr int VG_SCAN_WAVES = 8;          // wavefronts per scanning workgroup: ONE reservation per workgroup (3 000 per-wavefront reservations on the
                                          // view counter were most of a 15 us launch: returning atomics on one address are served one after the other)
__global__ __launch_bounds__(64 * VG_SCAN_WAVES) void k_scan_view_grid(DMap m, uint32_t frame_id, int4* view_list, int32_t list_cap, ViewGrid vg) {
  __shared__ uint32_t s_cells[VG_SCAN_WAVES][256];
  __shared__ int32_t s_total[VG_SCAN_WAVES], s_base;
  int32_t* cnt = &m.counters[C_VIEW_COUNT + (frame_id & 3)];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int32_t n_cells = vg.ncx * vg.ncy * vg.ncz, n_words = (n_cells + 3) >> 2, n_lines = (n_words + 15) >> 4;
  const int32_t n_waves = (int32_t)gridDim.x * VG_SCAN_WAVES, me = (int32_t)blockIdx.x * VG_SCAN_WAVES + wave;       // (4 n_waves >= n_lines: one pass)
  uint32_t* cw = reinterpret_cast<uint32_t*>(vg.coarse);
  uint4* fq = reinterpret_cast<uint4*>(vg.fine);
  uint32_t* cells = s_cells[wave];
  const int32_t line = me + (lane >> 4) * n_waves;
  const int32_t i = line * 16 + (lane & 15);
  const uint32_t v = (line < n_lines && i < n_words) ? cw[i] : 0u;
  if (v) cw[i] = 0u;
  int32_t n = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const bool t = ((v >> (8 * k)) & 0xFFu) != 0u;
    const u64 mask = __ballot(t);
    if (t) cells[n + (int32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)(4 * i + k);
    n += (int32_t)__popcll(mask);
  }
  const int sub = lane >> 2, part = lane & 3;             // sixteen cells per round, four lanes (16 bytes each) per cell
  int32_t mine = 0;
  for (int32_t it = 0; it < n; it += 16) {
    uint4 b = make_uint4(0u, 0u, 0u, 0u);
    if (it + sub < n) b = fq[(size_t)cells[it + sub] * 4 + part];
    mine += vg_nonzero_bytes(b.x) + vg_nonzero_bytes(b.y) + vg_nonzero_bytes(b.z) + vg_nonzero_bytes(b.w);
  }
  int32_t total = mine;
#pragma unroll
  for (int o = 32; o; o >>= 1) total += __shfl_xor(total, o);
  if (lane == 0) s_total[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t all = 0;
#pragma unroll
    for (int w = 0; w < VG_SCAN_WAVES; w++) all += s_total[w];
    s_base = all ? atomicAdd(cnt, all) : 0;
  }
  __syncthreads();
  if (!total) return;
  int32_t pos = s_base;
#pragma unroll
  for (int w = 0; w < VG_SCAN_WAVES; w++) if (w < wave) pos += s_total[w];
  for (int32_t it = 0; it < n; it += 16) {
    const bool have = it + sub < n;
    const uint32_t cell = have ? cells[it + sub] : 0u;
    uint4 b = make_uint4(0u, 0u, 0u, 0u);
    if (have) b = fq[(size_t)cell * 4 + part];
    if (b.x | b.y | b.z | b.w) fq[(size_t)cell * 4 + part] = make_uint4(0u, 0u, 0u, 0u);
    const int32_t cxi = (int32_t)(cell % (uint32_t)vg.ncx), cyi = (int32_t)((cell / (uint32_t)vg.ncx) % (uint32_t)vg.ncy), czi = (int32_t)(cell / ((uint32_t)vg.ncx * (uint32_t)vg.ncy));
    const uint32_t bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (__ballot(bw[q] != 0u) == 0ull) continue;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool t = ((bw[q] >> (8 * k)) & 0xFFu) != 0u;
        const u64 mask = __ballot(t);
        if (t) {
          const int32_t at = pos + (int32_t)__popcll(mask & ((1ull << lane) - 1ull));
          const int j = part * 16 + q * 4 + k;               // byte of the cell: lx & 3 | (ly & 3) << 2 | (lz & 3) << 4
          if (at < list_cap) view_list[at] = make_int4((int32_t)vg.tag, vg.ox + 4 * cxi + (j & 3), vg.oy + 4 * cyi + ((j >> 2) & 3), vg.oz + 4 * czi + (j >> 4));
        }
        pos += (int32_t)__popcll(mask);
      }
    }
  }
}
// k_resolve_view: the records the scan left tagged, one per lane -- the slot replaces the tag (records of blocks outside the box carry their slot already)
__global__ __launch_bounds__(256) void k_resolve_view(DMap m, uint32_t frame_id, int4* view_list, int32_t list_cap, uint32_t tag) {
  const int32_t n = min(m.counters[C_VIEW_COUNT + (frame_id & 3)], list_cap);
  const uint32_t want = (frame_id << 8) | 1u;
  const int lane = (int)(threadIdx.x & 63);
  for (int32_t i0 = (int32_t)blockIdx.x * 256 + (int32_t)(threadIdx.x & ~63u); i0 < n; i0 += (int32_t)gridDim.x * 256) {
    const int32_t i = i0 + lane;
    int4 rec = make_int4(0, 0, 0, 0);
    if (i < n) rec = view_list[i];
    u64 key[1]; bool valid[1]; uint32_t slot[1];
    valid[0] = i < n && (uint32_t)rec.x == tag;
    key[0] = pack_key(rec.y, rec.z, rec.w);
    if (__ballot(valid[0]) == 0ull) continue;
    // (no entry stamp: Entry::stamp de-duplicates the tiles of a CAMERA frame and carries a batch's camera masks; a scan's view is its view list --
    //  nothing reads the stamp of a LiDAR frame, and 112 k scattered 4-byte stores are 112 k lines written back)
    resolve_keys<1, 2, false>(m, key, valid, want, slot, lane);
    if (valid[0]) view_list[i].x = (int32_t)slot[0];
  }
}

// ------------------------------------------------------------------------------------------------ LiDAR, far field: beam-centric update
// Measured on a configs[4] scan (an instrumented copy of the CPU checker): 78 % of the voxels of the blocks in view run the nearest-beam rule
// -- the four beams around them do not agree, as on a ground plane seen at a grazing angle -- and only 6 % pass it: at 0.10 m voxels a beam's
// acceptance tube is one voxel wide while the beams are 0.6 m x 1.2 m apart at 100 m.  One lane per voxel pays the projection, four taps, the
// nearest tap and the point-to-ray distance 512 times per block to update ~20 voxels.  This launch turns the question round for the blocks
// where ONLY the nearest-beam rule can apply: ONE WAVEFRONT PER BLOCK
//   (1) projects the block's 8 corners: its footprint in the range image (+ 0.75 px: the elevation of a box is not extremal at its corners);
//       a block whose corner fails to project, that straddles the azimuth seam, or whose footprint exceeds 64 pixels is left to the dense launch;
//   (2) tests every 2 x 2 beam quad a voxel of the block could interpolate in ("four returns that agree"): one valid quad -> dense launch;
//   (3) otherwise walks every beam of the footprint that has a return through the block: in block voxel coordinates the beam is a line, along its
//       major axis it crosses 8 voxel slices, and a voxel centre within (0.5 + 0.01) voxel of the line lies within 0.51 / 0.577 = 0.88 < 1 voxel of
//       the crossing point inside its slice, i.e. among the 2 x 2 cells around that point -- 32 candidate voxels per beam instead of 512 per block;
//   (4) evaluates every candidate with the SAME per-voxel code as the dense launch (LidarSensor::sample_px, tsdf_fuse_plain; the voxel centre is
//       block origin + rotated offset, exactly as there) and updates it iff the rule's nearest beam is the beam that enumerated it (so a voxel
//       near two tubes is updated once).  A voxel that is not a candidate of its nearest beam fails that beam's distance test: untouched, as in the
//       dense launch.  Result: bit-identical maps (tests/test_gpu_full_size.py compares all 112 k blocks of two scans with the CPU checker).
// The class of every record (1 = updated here) goes to view_class[]; the dense launch that follows skips those.  Requires the plain integrator
// configuration (constant weighting, TSDF) and a nearest-beam acceptance radius <= 0.55 voxel (the 2 x 2 argument); the host falls back otherwise.
#ifndef NVBX_SPARSE_WAVES
#define NVBX_SPARSE_WAVES 6      // (81 VGPRs were one register away from six wavefronts per SIMD: 5 / 6 / 7 / 8 asked for = 116.6 / 110.0 / 111.1 / 114.4 us)
#endif
template <typename Img>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NVBX_SPARSE_WAVES, NVBX_SPARSE_WAVES))) void k_lidar_sparse(DMap m, FrameSet<Img, 1> fs, LidarSensor sensor, const int4* view_list, int32_t list_cap,
                                                      int32_t mesh_list, uint8_t* view_class, int32_t* dense_list) {
  // per wavefront: the crossing beams {line in block voxel coordinates ob[3], db[3]; pixel; range; direction[3]; major axis} and the
  // candidate voxels that survive the geometric pre-filter {beam << 9 | voxel}
  __shared__ float s_beam[4][64][12];
  __shared__ uint16_t s_item[4][512];
  const Frame& f = fs.f[0];
  const Img& img = fs.img[0];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t n_waves = (int32_t)gridDim.x * 4;
  int32_t n = m.counters[C_VIEW_COUNT + (f.frame_id & 3)];
  if (n > list_cap) n = list_cap;
  const float vs = f.voxel_size, bs = f.block_size;
  const int rows = f.rows, cols = f.cols;
  // Dependent-access chain per block: {record (fetched one block ahead)} -> {quad taps || footprint taps || beam tables || flag atomic} ->
  // {voxels of the candidates that pass} -> store.  The candidates' arithmetic needs no image access at all: their beam's range and direction
  // travel with the beam.
  // Records are taken EIGHT at a time: lanes 8 j .. 8 j + 7 project the eight corners of block j, so the footprints of eight blocks cost one
  // pass of the projection code (with one block per pass 56 of the 64 lanes idled through it); the blocks are then walked one after the other.
  const int grp = lane >> 3;
  int32_t n_mine = 0;                                        // blocks this wavefront updated (one counter atomic per wavefront, at the end)
  // pass p of G = ceil(n / 8) takes records p, G + p, 2 G + p, ...: eight far-apart places of the list (a pass's cost is the sum of its
  // blocks' footprints; neighbours in the list have footprints of one size -- eight consecutive records per pass: 126.5 instead of 116.4 us, EXPERIMENTS.md)
  const int32_t G = (n + 7) >> 3;
  auto ridx = [&](int32_t p, int g) -> int32_t { return g * G + p; };
  int32_t pass = (int32_t)blockIdx.x * 4 + wv;
  int4 rec_next = (pass < G && ridx(pass, grp) < n) ? view_list[ridx(pass, grp)] : make_int4((int32_t)SLOT_NONE, 0, 0, 0);
  for (; pass < G; pass += n_waves) {
    const int4 rec_g = rec_next;
    if (pass + n_waves < G && ridx(pass + n_waves, grp) < n) rec_next = view_list[ridx(pass + n_waves, grp)]; else rec_next = make_int4((int32_t)SLOT_NONE, 0, 0, 0);
    // (1) corners of the group's block
    bool sparse_g = ridx(pass, grp) < n && slot_ok((uint32_t)rec_g.x);
    float org_g[3];
    sensor_block_origin(f, rec_g.y, rec_g.z, rec_g.w, org_g);
    int c0_g = 0, r0_g = 0, w_g = 0, h_g = 0;
    {
      float off[3], pc[3], u = 0.0f, v = 0.0f;
      rotate(f.R_CL, (float)(lane & 1) * bs, (float)((lane >> 1) & 1) * bs, (float)((lane >> 2) & 1) * bs, off);
      pc[0] = org_g[0] + off[0]; pc[1] = org_g[1] + off[1]; pc[2] = org_g[2] + off[2];
      const bool okc = nvbx_lidar_project(&sensor.l, pc, nvbx_lidar_range(pc), &u, &v) != 0;
      const u64 bad = __ballot(!okc);
      if ((bad >> (8 * grp)) & 0xFFull) sparse_g = false;
      float umin = u, umax = u, vmin = v, vmax = v;
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        umin = fminf(umin, __shfl_xor(umin, o)); umax = fmaxf(umax, __shfl_xor(umax, o));
        vmin = fminf(vmin, __shfl_xor(vmin, o)); vmax = fmaxf(vmax, __shfl_xor(vmax, o));
      }
      if (sparse_g) {
        if (umax - umin > (float)cols * 0.5f) sparse_g = false;               // straddles the azimuth seam
        c0_g = (int)floorf(umin - 0.75f); r0_g = (int)floorf(vmin - 0.75f);
        w_g = (int)floorf(umax + 0.75f) - c0_g + 1; h_g = (int)floorf(vmax + 0.75f) - r0_g + 1;
        if (w_g < 1 || h_g < 1 || w_g * h_g > 64) sparse_g = false;           // one lane per footprint pixel
      }
    }
    const u64 sparse_groups = __ballot(sparse_g);
    uint32_t dmask = 0;                                                         // records of this pass left to the dense launch (uniform)
#pragma unroll 1
    for (int j = 0; j < 8; j++) {
    const int32_t i = ridx(pass, j);
    if (i >= n) continue;                                                       // (uniform)
    bool sparse = ((sparse_groups >> (8 * j)) & 1ull) != 0;
    const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane(rec_g.x, 8 * j);
    if (!sparse) { if (lane == 0) view_class[i] = 0; if (slot_ok(slot)) dmask |= 1u << j; continue; }               // (uniform)
    const float org[3] = {__int_as_float(__builtin_amdgcn_readlane(__float_as_int(org_g[0]), 8 * j)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(org_g[1]), 8 * j)),
                          __int_as_float(__builtin_amdgcn_readlane(__float_as_int(org_g[2]), 8 * j))};
    const int c0 = __builtin_amdgcn_readlane(c0_g, 8 * j), r0 = __builtin_amdgcn_readlane(r0_g, 8 * j), w = __builtin_amdgcn_readlane(w_g, 8 * j), h = __builtin_amdgcn_readlane(h_g, 8 * j);
    // footprint pixel of this lane: its range and its beam's direction tables are requested together with the quad taps below
    // (lane -> (column, row) of a w-wide grid without an integer division: exact for lane < 2^10)
    const int ly = (int)(((float)lane + 0.5f) * (1.0f / (float)w)), lx = lane - ly * w;
    const int bc = c0 + lx, brr = r0 + ly;
    const bool in_img = ly < h && bc >= 0 && brr >= 0 && bc < cols && brr < rows;
    const float bd = in_img ? img(pix(brr, bc, cols)) : 0.0f;
    const float2 te = sensor.el_tab[in_img ? brr : 0], ta = sensor.az_tab[in_img ? bc : 0];
    // (2) quads x0 in [c0 - 1, c0 + w - 1], y0 in [r0 - 1, r0 + h - 1]: (w + 1) x (h + 1) <= 130 of them, up to three per lane
    bool anyq = false;
    const int nq = (w + 1) * (h + 1);
    const float iw1 = 1.0f / (float)(w + 1);
    for (int qi = lane; qi < nq; qi += 64) {
      const int qy = (int)(((float)qi + 0.5f) * iw1), qx = qi - qy * (w + 1);
      const int x0 = c0 - 1 + qx, y0 = r0 - 1 + qy;
      if (!(x0 < 0 || y0 < 0 || x0 + 1 > cols - 1 || y0 + 1 > rows - 1)) {
        const int32_t i00 = pix(y0, x0, cols);
        const float f00 = img(i00), f10 = img(i00 + 1), f01 = img(i00 + cols), f11 = img(i00 + cols + 1);
        if (depth_valid4(f00, f10, f01, f11)) {
          const float mx = fmaxf(fmaxf(f00, f10), fmaxf(f01, f11)), mn = fminf(fminf(f00, f10), fminf(f01, f11));
          if (mx - mn <= sensor.max_diff_m) anyq = true;
        }
      }
    }
    if (__ballot(anyq)) sparse = false;
    if (!sparse) { if (lane == 0) view_class[i] = 0; dmask |= 1u << j; continue; }               // (uniform)
    // (3) the beams of the footprint that have a return, one per lane: line in block voxel coordinates q = R_LC (P - org) / vs (sensor origin: P = 0)
    float ob[3] = {0.0f, 0.0f, 0.0f}, db[3] = {1.0f, 0.0f, 0.0f};
    const float dir[3] = {te.y * ta.y, te.y * ta.x, te.x};                   // == LidarSensor::beam_dir(brr, bc)
    bool crossing = false; int axis = 0;
    if (in_img && depth_valid(bd)) {
      float t3[3];
      rotate(f.R_LC, org[0], org[1], org[2], t3);
      const float ivs = 1.0f / vs;
      ob[0] = -t3[0] * ivs; ob[1] = -t3[1] * ivs; ob[2] = -t3[2] * ivs;    // (enumeration geometry only: a slack of 0.1 voxel, no exactness needed)
      rotate(f.R_LC, dir[0], dir[1], dir[2], db);
      int a = 0; if (fabsf(db[1]) > fabsf(db[a])) a = 1; if (fabsf(db[2]) > fabsf(a == 0 ? db[0] : db[1])) a = 2;
      axis = a;
      const float oa = a == 0 ? ob[0] : (a == 1 ? ob[1] : ob[2]), da = a == 0 ? db[0] : (a == 1 ? db[1] : db[2]);
      const float obb = a == 0 ? ob[1] : (a == 1 ? ob[2] : ob[0]), dbb = a == 0 ? db[1] : (a == 1 ? db[2] : db[0]);     // axes (a + 1) % 3, (a + 2) % 3
      const float occ = a == 0 ? ob[2] : (a == 1 ? ob[0] : ob[1]), dcc = a == 0 ? db[2] : (a == 1 ? db[0] : db[1]);
      const float ida = 1.0f / da;
      // the line's crossing points of slice 0 and slice 7 bound those of the slices between: the tube meets the block iff the interval of
      // crossing points (+- one cell) meets [0, 7] in both perpendicular axes
      const float t0 = (0.5f - oa) * ida, t7 = (7.5f - oa) * ida;
      const float b0 = obb + t0 * dbb - 0.5f, b7 = obb + t7 * dbb - 0.5f, cc0 = occ + t0 * dcc - 0.5f, cc7 = occ + t7 * dcc - 0.5f;
      crossing = fmaxf(b0, b7) >= -1.0f && fminf(b0, b7) <= 8.0f && fmaxf(cc0, cc7) >= -1.0f && fminf(cc0, cc7) <= 8.0f;
    }
    const u64 cross = __ballot(crossing);
    const int nb = (int)__popcll(cross);
    if (crossing) {
      const int k = (int)__popcll(cross & ((1ull << lane) - 1ull));
      float* q = s_beam[wv][k];
      q[0] = ob[0]; q[1] = ob[1]; q[2] = ob[2]; q[3] = db[0]; q[4] = db[1]; q[5] = db[2];
      q[6] = __int_as_float(pix(brr, bc, cols)); q[7] = bd; q[8] = dir[0]; q[9] = dir[1]; q[10] = dir[2]; q[11] = __int_as_float(axis);
    }
    __threadfence_block();                                  // (the wavefront's own LDS writes, read by its other lanes below: no workgroup barrier -- the four wavefronts run independent loops)
    __builtin_amdgcn_wave_barrier();
    // (4a) candidates: item = (beam, slice, cell) -> 32 per beam; a candidate survives the PRE-FILTER if its centre lies within the acceptance radius + 0.02 voxel of the
    // beam's line in block coordinates (the exact test below is this distance in the sensor frame, to ~1e-4 voxel); survivors are compacted
    int32_t ns = 0;                                           // survivors (wave-uniform)
    const float pre = sensor.max_ray_dist_m / vs + 0.02f, pre2 = pre * pre;     // acceptance radius of the exact test, in voxels, + slack
    for (int it0 = 0; it0 < nb * 32; it0 += 64) {
      const int item = it0 + lane;
      const int kb = item >> 5, sl = (item >> 2) & 7, cell = item & 3;
      bool keep = false; int vox = 0;
      if (kb < nb) {
        const float* q = s_beam[wv][kb];
        const float o0 = q[0], o1 = q[1], o2 = q[2], d0 = q[3], d1 = q[4], d2 = q[5];
        const int a = __float_as_int(q[11]);
        const float oa = a == 0 ? o0 : (a == 1 ? o1 : o2), da = a == 0 ? d0 : (a == 1 ? d1 : d2);
        const float obb = a == 0 ? o1 : (a == 1 ? o2 : o0), dbb = a == 0 ? d1 : (a == 1 ? d2 : d0);
        const float occ = a == 0 ? o2 : (a == 1 ? o0 : o1), dcc = a == 0 ? d2 : (a == 1 ? d0 : d1);
        const float t = ((float)sl + 0.5f - oa) / da;
        const int jb = (int)floorf(obb + t * dbb - 0.5f) + (cell & 1), jc = (int)floorf(occ + t * dcc - 0.5f) + (cell >> 1);
        if (jb >= 0 && jb <= 7 && jc >= 0 && jc <= 7) {
          const int vx = a == 0 ? sl : (a == 1 ? jc : jb), vy = a == 0 ? jb : (a == 1 ? sl : jc), vz = a == 0 ? jc : (a == 1 ? jb : sl);
          const float px = (float)vx + 0.5f - o0, py = (float)vy + 0.5f - o1, pz = (float)vz + 0.5f - o2;
          const float cx = py * d2 - pz * d1, cy = pz * d0 - px * d2, cz = px * d1 - py * d0;     // |(p - o) x d|^2 = squared distance to the line (|d| = 1)
          keep = (cx * cx + cy * cy) + cz * cz <= pre2;
          vox = vz + 8 * vy + 64 * vx;
        }
      }
      const u64 km = __ballot(keep);
      if (keep) { const int pos = ns + (int)__popcll(km & ((1ull << lane) - 1ull)); if (pos < 512) s_item[wv][pos] = (uint16_t)((kb << 9) | vox); }
      ns += (int32_t)__popcll(km);
    }
    if (ns > 512) sparse = false;                             // more survivors than the list holds (dense beams at close range): the dense launch takes the block
    if (lane == 0) view_class[i] = sparse ? 1 : 0;
    if (!sparse) { dmask |= 1u << j; __builtin_amdgcn_wave_barrier(); continue; }                // (uniform)
    // the block's books, as the dense launch keeps them (lane 0; the returning atomic is consumed after the update)
    uint32_t old = 0;
    if (lane == 0) old = atomicOr(&m.slot_flags[slot], F_TSDF | F_DIRTY_ESDF | F_DIRTY_MESH | F_BAND_STALE);
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    // (4b) the survivors, 64 at a time.  In a block of this class the four-tap rule cannot measure (no valid quad in reach), so a candidate goes
    // straight to the nearest-beam rule -- the same operations, in the same order, as the tail of LidarSensor::sample_px, with the beam's range and
    // direction taken from the beam instead of from the image and the tables.
    for (int it0 = 0; it0 < ns; it0 += 64) {
      if (it0 + lane >= ns) continue;
      const int code = s_item[wv][it0 + lane];
      const float* q = s_beam[wv][code >> 9];
      const int vox = code & 511, vx = vox >> 6, vy = (vox >> 3) & 7, vz = vox & 7;
      float off[3], pc[3];
      sensor_voxel_offset(f, vx, vy, vz, off);
      pc[0] = org[0] + off[0]; pc[1] = org[1] + off[1]; pc[2] = org[2] + off[2];
      const float r = nvbx_lidar_range(pc);
      if (f.max_dist > 0.0f && r > f.max_dist) continue;
      float u, v;
      if (!nvbx_lidar_project(&sensor.l, pc, r, &u, &v)) continue;
      const int c = (int)floorf(u), rr = (int)floorf(v);
      if (c < 0 || rr < 0 || c >= cols || rr >= rows) continue;
      if (pix(rr, c, cols) != __float_as_int(q[6])) continue;   // the rule's nearest beam is another one: that beam's walk takes the voxel (if it can)
      const float d = q[7];
      const float bdx = q[8], bdy = q[9], bdz = q[10];
      const float dot = __builtin_fmaf(pc[2], bdz, __builtin_fmaf(pc[1], bdy, pc[0] * bdx));
      const float ex = __builtin_fmaf(-dot, bdx, pc[0]), ey = __builtin_fmaf(-dot, bdy, pc[1]), ez = __builtin_fmaf(-dot, bdz, pc[2]);
      if (__builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)) > sensor.max_ray_dist_m * sensor.max_ray_dist_m) continue;
      float2* vp = &m.tsdf[(size_t)slot * 512 + vox];
      float2 fin = *vp;
      if (tsdf_fuse_plain(f, &fin, d, r)) *vp = fin;
    }
    if (lane == 0) {
      if (!(old & F_DIRTY_ESDF)) list_append(m, S_LIST_ESDF_DIRTY, (int32_t)slot);
      if (!(old & F_DIRTY_MESH)) list_append(m, mesh_list, (int32_t)slot);
    }
    n_mine++;
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    }
    // the dense launch's work list: the view-list indices of the records left to it, one reservation per pass in this workgroup's shard
    if (dense_list && dmask) {
      const int sh = my_shard();
      int32_t base0 = 0;
      if (lane == 0) base0 = atomicAdd(shc_at(m, S_LIDAR_SPARSE, sh, 1), (int32_t)__popc(dmask));
      base0 = __shfl(base0, 0);
      if (lane < 8 && ((dmask >> lane) & 1u)) {
        const int32_t pos = base0 + (int32_t)__popc(dmask & ((1u << lane) - 1u));
        if (pos < list_cap) dense_list[(size_t)sh * list_cap + pos] = ridx(pass, lane);
      }
    }
  }
  if (lane == 0 && n_mine) atomicAdd(shc_at(m, S_LIDAR_SPARSE, my_shard(), 0), n_mine);
}

// the beam-centric far-field launch; view_class = nullptr: everything goes to the dense launch
int launch_lidar_sparse(nvbx_mapper* m, const FrameSet<DepthF32, 1>& fs, const LidarSensor& sensor, bool plain, uint8_t** view_class, int32_t** dense_list) {
  *view_class = nullptr; *dense_list = nullptr;
  // (knobs.lidar_sparse -- A/B: 0 = dense launch only)
  if (!m->knobs.lidar_sparse || !plain || !(m->p.lidar_nearest_interpolation_max_allowable_dist_to_ray_vox <= 0.55f)) return NVBX_OK;
  // [capacity class bytes][NSH x capacity view-list indices: the dense launch's work list, one region per shard]
  const size_t class_bytes = ((size_t)m->capacity + 15) & ~(size_t)15;
  if (m->view_class.ensure(m->stream, class_bytes + (size_t)NSH * (size_t)m->capacity * 4)) return NVBX_E_DEVICE;
  uint8_t* vc = m->view_class.as<uint8_t>();
  const int sparse_grid = m->knobs.lidar_sparse_grid;    // (NVBX_LIDAR_SPARSE_GRID; six resident wavefronts per SIMD = 1536 workgroups; 1536 / 2048 / 2560 / 3072 / 3584 / 4096 / 8192 workgroups: 111.1 / 109.5 / 110.5 / 111.0 / 114.8 / 115.3 / 114.3 us with strided passes and the work list)
  // (with an exchange buffer registered -- nvbx_set_view_export -- the dense launch walks the whole view list, as it writes every record's index there)
  // (knobs.lidar_dense_list -- A/B: 0 = the dense launch skips the taken records of the whole list)
  int32_t* dense = (m->knobs.lidar_dense_list && !m->view_export) ? reinterpret_cast<int32_t*>(vc + class_bytes) : nullptr;
  NVBX_LAUNCH(m, (k_lidar_sparse<DepthF32>), dim3(sparse_grid), dim3(256), m->d, fs, sensor, (const int4*)m->view_list, (int32_t)m->capacity, m->mesh_list_live(), vc, dense);
  *dense_list = dense;
  *view_class = vc;
  return NVBX_OK;
}

// LiDAR view calculation over the dense grid (k_mark_view_grid, k_scan_view_grid, k_resolve_view) instead of k_mark_view; *used = false: the caller
// launches k_mark_view (a scan without a range limit or with a box beyond the grid's addressing / memory cap; NVBX_LIDAR_VIEW_GRID=0)
int launch_view_grid(nvbx_mapper* m, const FrameSet<DepthF32, 1>& fs, const LidarSensor& sensor, int tiles, int32_t fence_report, bool* used) {
  *used = false;
  const Frame& f = fs.f[0];
  // (knobs.lidar_view_grid -- A/B: 0 = k_mark_view<Lidar>)
  if (!m->knobs.lidar_view_grid || !(f.max_dist > 0.0f) || m->capacity > (1ll << 24)) return NVBX_OK;
  // the box: every ray ends within max_dist of the sensor; along z the beams' elevation range bounds it (|world z of a unit beam| <=
  // hypot(R20, R21) cos(el) + |R22 sin(el)|, elevation table rows on the host: ensure_lidar_tables)
  const double reach = (double)f.max_dist / (double)f.block_size;
  double wz = 0.0;
  const double hxy = std::hypot((double)f.R_LC[6], (double)f.R_LC[7]);
  for (int k = 0; k < sensor.l.rows; k++) wz = std::max(wz, hxy * std::fabs((double)m->lidar_host[2 * (size_t)k + 1]) + std::fabs((double)f.R_LC[8] * (double)m->lidar_host[2 * (size_t)k]));
  int64_t H = (int64_t)std::ceil(reach) + 2, Hz = std::min<int64_t>(H, (int64_t)std::ceil(reach * std::min(1.0, wz)) + 2);
  // (tests: a box SMALLER than the sensor's range -- the blocks beyond it take the hash path, block by block; tests/test_gpu_round5.py)
  const int64_t reach_cap = m->knobs.view_grid_reach;      // (NVBX_VIEW_GRID_REACH; 0 = no cap)
  if (reach_cap > 0) { H = std::min(H, reach_cap); Hz = std::min(Hz, reach_cap); }
  const int64_t ncx = (2 * H + 1 + 3) / 4, ncz = (2 * Hz + 1 + 3) / 4;
  const int64_t cells = ncx * ncx * ncz;
  const int64_t cap_mb = m->knobs.view_grid_max_mb;      // (NVBX_VIEW_GRID_MAX_MB: 1 .. 2^20, default 128)
  if (ncx > 256 || ncz > 256 || cells * 64 > (cap_mb << 20)) return NVBX_OK;
  const size_t coarse_bytes = ((size_t)cells + 3) & ~(size_t)3;
  bool grew = false;
  if (m->view_grid_fine.ensure(m->stream, (size_t)cells * 64 + coarse_bytes, &grew)) return NVBX_E_DEVICE;      // [fine: 64 B per cell][coarse: 1 B per cell]
  if (grew) { m->view_grid_cells = cells; m->view_grid_dirty = true; }
  if (m->view_grid_dirty) NVBX_HIP(hipMemsetAsync(m->view_grid_fine.p, 0, m->view_grid_fine.bytes, m->stream));
  m->view_grid_dirty = true;                 // until all three launches are enqueued
  ViewGrid vg{};
  vg.fine = m->view_grid_fine.as<uint8_t>(); vg.coarse = vg.fine + (size_t)m->view_grid_cells * 64;
  vg.cx = (int32_t)std::floor(f.t_LC[0] / f.block_size); vg.cy = (int32_t)std::floor(f.t_LC[1] / f.block_size); vg.cz = (int32_t)std::floor(f.t_LC[2] / f.block_size);
  vg.ox = vg.cx - (int32_t)H; vg.oy = vg.cy - (int32_t)H; vg.oz = vg.cz - (int32_t)Hz;
  vg.ncx = (int32_t)ncx; vg.ncy = (int32_t)ncx; vg.ncz = (int32_t)ncz;
  vg.tag = 0x80000000u | f.frame_id;
  NVBX_LAUNCH(m, (k_mark_view_grid<DepthF32>), dim3(tiles), dim3(64), m->d, fs, sensor, (int4*)m->view_list, (int32_t)m->capacity, (int32_t)(m->premark_consumed ? 1 : 0), fence_report, vg);
  // the resolving launch: one tagged record per lane -- as many as the last finished scan had in view (+ 25 %; a hint only, it grid-strides)
  // the scan: a wavefront per four lines (256 cells) of the coarse map, VG_SCAN_WAVES wavefronts per workgroup, everything in one pass
  const int64_t coarse_lines = ((cells + 3) / 4 + 15) / 16;
  const int64_t scan_wg = (coarse_lines + 4 * VG_SCAN_WAVES - 1) / (4 * VG_SCAN_WAVES);
  NVBX_LAUNCH(m, k_scan_view_grid, dim3((unsigned)scan_wg), dim3(64 * VG_SCAN_WAVES), m->d, f.frame_id, (int4*)m->view_list, (int32_t)m->capacity, vg);
  const int64_t n_hint = std::max<int64_t>(0, __atomic_load_n(&m->h_mirror[2], __ATOMIC_RELAXED));
  const int64_t rec_wg = n_hint == 0 ? 512 : std::max<int64_t>(8, std::min<int64_t>(2048, (n_hint + n_hint / 4 + 255) / 256));
  NVBX_LAUNCH(m, k_resolve_view, dim3((unsigned)rec_wg), dim3(256), m->d, f.frame_id, (int4*)m->view_list, (int32_t)m->capacity, vg.tag);
  NVBX_HIP(hipGetLastError());
  m->view_grid_dirty = false;
  *used = true;
  return NVBX_OK;
}

// ------------------------------------------------------------------------------------------------ LiDAR entry points
static bool same_lidar(const nvbx_lidar& a, const nvbx_lidar& b) { return memcmp(&a, &b, sizeof(a)) == 0; }

// beam direction tables: sin / cos evaluated in double on the host from the float model parameters, rounded to float
// (the oracle builds the same tables the same way, so view rays are bit-identical)
static int ensure_lidar_tables(nvbx_mapper* m, const nvbx_lidar* ld, const nvbx_lidar_model& l) {
  if (m->lidar_tab.p && same_lidar(m->lidar_cached, *ld)) return NVBX_OK;
  const size_t n = (size_t)l.rows + (size_t)l.cols;
  if (m->lidar_tab.ensure(m->stream, n * sizeof(float2))) return NVBX_E_DEVICE;
  m->lidar_host.resize(n * 2);
  for (int k = 0; k < l.rows; k++) {
    const double el = (double)l.max_el - (double)k * (double)l.rpp_el;
    m->lidar_host[2 * (size_t)k] = (float)sin(el); m->lidar_host[2 * (size_t)k + 1] = (float)cos(el);
  }
  for (int j = 0; j < l.cols; j++) {
    const double az = -(double)NVBX_PI_F + (double)j * (double)l.rpp_az;
    m->lidar_host[2 * ((size_t)l.rows + j)] = (float)sin(az); m->lidar_host[2 * ((size_t)l.rows + j) + 1] = (float)cos(az);
  }
  NVBX_HIP(hipMemcpyAsync(m->lidar_tab.p, m->lidar_host.data(), n * sizeof(float2), hipMemcpyHostToDevice, m->stream));
  NVBX_HIP(hipStreamSynchronize(m->stream));    // once per sensor model
  m->lidar_cached = *ld;
  return NVBX_OK;
}

static bool lidar_ok(const nvbx_lidar* ld) {
  return ld && ld->num_azimuth_divisions >= 2 && ld->num_elevation_divisions >= 2 && ld->max_elevation_rad > ld->min_elevation_rad &&
         image_dims_ok(ld->num_elevation_divisions, ld->num_azimuth_divisions);
}

extern "C" int nvbx_integrate_lidar_depth(nvbx_mapper* m, const float* range_dev, int32_t rows, int32_t cols, const float T_L_C[16],
                                          const nvbx_lidar* lidar) {
  if (!m || !range_dev || !T_L_C || !lidar_ok(lidar) || rows != lidar->num_elevation_divisions || cols != lidar->num_azimuth_divisions) {
    set_error("nvbx_integrate_lidar_depth: invalid argument (range image must be elevation x azimuth divisions)"); return NVBX_E_INVALID;
  }
  if (!nvbx_pose_in_range(T_L_C, m->p.voxel_size * 8.0f, m->p.lidar_max_integration_distance_m + 2.0f * m->p.truncation_distance_vox * m->p.voxel_size)) {
    set_error("nvbx_integrate_lidar_depth: T_L_C is not finite or lies outside the addressable block range (+-2^20 blocks)"); return NVBX_E_INVALID; }
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call()) return NVBX_E_DEVICE;
  const nvbx_lidar_model l = nvbx_lidar_make(cols, rows, lidar->min_valid_range_m, lidar->min_elevation_rad, lidar->max_elevation_rad);
  const int rc = ensure_lidar_tables(m, lidar, l); if (rc) return rc;
  { const int rcg = m->maybe_grow(); if (rcg) return rcg; }
  { const int rc2 = next_frame_id(m); if (rc2) return rc2; }
  nvbx_camera none{1.f, 1.f, 0.f, 0.f, cols, rows};
  FrameSet<DepthF32, 1> fs{}; fs.n = 1; fs.img[0] = DepthF32{range_dev};
  fs.f[0] = m->make_frame(T_L_C, &none, rows, cols, m->p.raycast_subsampling_factor);
  fs.f[0].max_dist = m->p.lidar_max_integration_distance_m;
  LidarSensor s{l, m->lidar_tab.as<const float2>(), m->lidar_tab.as<const float2>() + rows,
                m->p.lidar_linear_interpolation_max_allowable_difference_vox * m->p.voxel_size,
                m->p.lidar_nearest_interpolation_max_allowable_dist_to_ray_vox * m->p.voxel_size};
  return integrate_lidar_frame(m, fs, s);
}

// depthImageFromPointcloudKernel (conversions/pointcloud_conversions.cu:118-150): last writer wins
__global__ void k_depth_from_points(const float* pts, int64_t n, nvbx_lidar_model l, float* img) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    if (isnan(p[0]) || isnan(p[1]) || isnan(p[2])) continue;
    const float r = nvbx_lidar_range(p);
    float u, v;
    if (!nvbx_lidar_project(&l, p, r, &u, &v)) continue;
    const int c = (int)floorf(u), rr = (int)floorf(v);
    if (c < 0 || rr < 0 || c >= l.cols || rr >= l.rows) continue;
    img[(int64_t)rr * l.cols + c] = r;
  }
}
extern "C" int nvbx_depth_image_from_pointcloud(nvbx_mapper* m, const float* points_xyz_dev, int64_t n_points, const nvbx_lidar* lidar,
                                                float* range_dev) {
  if (!m || !points_xyz_dev || n_points < 0 || !lidar_ok(lidar) || !range_dev) { set_error("nvbx_depth_image_from_pointcloud: invalid argument"); return NVBX_E_INVALID; }
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call()) return NVBX_E_DEVICE;
  const nvbx_lidar_model l = nvbx_lidar_make(lidar->num_azimuth_divisions, lidar->num_elevation_divisions, lidar->min_valid_range_m,
                                             lidar->min_elevation_rad, lidar->max_elevation_rad);
  NVBX_HIP(hipMemsetAsync(range_dev, 0, (size_t)l.rows * l.cols * sizeof(float), m->stream));
  if (n_points > 0)
    NVBX_LAUNCH(m, k_depth_from_points, dim3((unsigned)std::min<int64_t>((n_points + 255) / 256, 4096)), dim3(256), points_xyz_dev, n_points, l, range_dev);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}
