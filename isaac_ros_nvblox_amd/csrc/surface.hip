// surface.hip -- the TSDF's surface as a device-resident point cloud, and one map registered against another over it (nvbx_surface_points /
// nvbx_align_map / nvbx_relocalize_map; SEMANTICS.md "Surface points", "Registering two maps").
// [U] nothing of the kind is readable in the reference tree; the per-edge arithmetic is nvbx_surface_math.h.
//
// The output order is specified (slot, voxel, axis), so nothing is appended through an atomic counter: count, scan, emit, in stream order, and no
// workgroup waits for another inside a launch.
//   k_surface_count      one 512-thread workgroup per pool slot below the high-water mark (grid-stride), lane = voxel t = vz + 8 vy + 64 vx.  The
//                        block's 512 {d, w} pairs go to LDS with the three neighbour FACES (+x, +y, +z, 64 voxels each): three lanes probe the
//                        hash once each, three wavefronts load a face each.  Every lane forms the 3-bit crossing mask of its voxel; the
//                        workgroup's total goes to counts[slot] (0 for a slot without a TSDF block), the three neighbour slots to fslots[slot].
//   k_surface_tile_sums  one workgroup per tile of SF_TILE slots: the tile's sum.
//   k_surface_scan_tiles one workgroup: the exclusive prefix of the tile sums (64-bit), the total into *count_dev.
//   k_surface_emit       the same tile and masks again, recomputed (a block without a crossing ends after one 4-byte load); the neighbour slots are
//                        read back, 12 bytes, not probed for again (with the probe loop this kernel spilled SGPRs).  The "add" of the scan is
//                        done here: the block's first row = its tile's offset + the counts of the tile's slots below it (at most SF_TILE - 1
//                        coalesced loads, one reduction).  A crossing's rank inside the block, in (t, axis) order, comes from three ballots and
//                        population counts per wavefront and the wavefronts' totals in order; the crossings are compacted into LDS by rank, and
//                        lane r takes crossing r, r + 512, ..: the point and the colour voxel (the neighbour's slot is the face's: no further probe,
//                        one flag load) are formed on full wavefronts and the rows are written coalesced.
//   k_surface_normals    only where normals are asked for: one lane per written row, the point read back, the query (q_point, nvbx_query_point.h:
//                        nvbx_query_points' inline code) and the division by the length.  Inside k_surface_emit the query cost that kernel 10 to
//                        14 spilled SGPRs, whichever way its loop was cut; on its own neither kernel spills.
// nvbx_align_map / nvbx_relocalize_map: the same launches on dst's stream over src's map, the rows into scratch of dst, one host wait for the
// count, then nvbx_align_points' / nvbx_relocalize_points' own launches (nvbx_align.h).
#include <algorithm>
#include <cmath>
#include "nvbx_align.h"
#include "nvbx_query_point.h"
#include "nvbx_surface_math.h"

using namespace nvbx;

constexpr int SF_TPB = 512;
constexpr int SF_TILE = 256;                 // slots per tile of the scan (tests/test_gpu_surface.py crosses its borders)
constexpr int SF_SCAN_TPB = 1024;
constexpr int64_t SF_MAX_POINTS = 1ll << 30;
constexpr size_t SF_HEAD_BYTES = 64;         // nvbx_mapper::surface_buf: the head, then counts, tile sums, tile offsets
static_assert(sizeof(nvbx_surface_options) == 40, "C-ABI layout");

struct SurfaceArgs {
  float vs, min_weight;
  int32_t stride, use_box, require_color, pad;
  int32_t box[6];
  uint32_t* counts; uint32_t* fslots; uint32_t* tile_sum; u64* tile_off; int32_t ntiles;
  float* points; uint8_t* colors; float* normals;
  int64_t capacity; long long* count;
};

struct SurfaceTile { float2 v[512]; float2 face[3][64]; uint32_t fslot[3]; };

// the neighbour of voxel t along axis ax: its {d, w} from the tile; *ns = its block's slot, *nt = its voxel index there
__device__ inline float2 surface_neighbour(const SurfaceTile& s, uint32_t slot, int t, int ax, uint32_t* ns, int* nt) {
  const int vx = t >> 6, vy = (t >> 3) & 7, vz = t & 7;
  const int v = ax == 0 ? vx : ax == 1 ? vy : vz;
  const int step = ax == 0 ? 64 : ax == 1 ? 8 : 1;
  if (v < 7) { *ns = slot; *nt = t + step; return s.v[t + step]; }
  const int fi = ax == 0 ? vy * 8 + vz : ax == 1 ? vx * 8 + vz : vx * 8 + vy;
  *ns = s.fslot[ax]; *nt = t - 7 * step;
  return s.face[ax][fi];
}

// the colour of an edge: the colour voxel of the endpoint nearer the surface -> has one; *rgba = its packed word or 0
__device__ inline bool surface_color(const DMap& m, uint32_t slot, int t, uint32_t ns, int nt, float d0, float d1, uint32_t* rgba) {
  const bool far_end = nvbx_surface_color_end(d0, d1) != 0;
  const uint32_t cs = far_end ? ns : slot;
  const int ct = far_end ? nt : t;
  *rgba = 0u;
  if (!slot_ok(cs) || !(m.slot_flags[cs] & F_COLOR)) return false;
  const uint2 c = m.color[(size_t)cs * 512 + ct];
  if (!(__uint_as_float(c.y) > 0.0f)) return false;
  *rgba = c.x;
  return true;
}

// Loads the tile of the TSDF block in `slot` (all 512 lanes, two barriers) -> the lane's crossing mask, bit a = the edge along axis a.
// PROBE: the three neighbour blocks are looked up in the hash and their slots left in a.fslots[slot] (k_surface_count); else they are read from
// there (k_surface_emit: no second probe, and without the probe loop that kernel spills no SGPR).
template <bool PROBE>
__device__ inline uint32_t surface_tile(const DMap& m, const SurfaceArgs& a, uint32_t slot, SurfaceTile& s, int tid) {
  const int32_t bx = m.slot_index[3 * slot], by = m.slot_index[3 * slot + 1], bz = m.slot_index[3 * slot + 2];
  s.v[tid] = m.tsdf[(size_t)slot * 512 + tid];
  if (tid < 3) {
    const int32_t nx = bx + (tid == 0), ny = by + (tid == 1), nz = bz + (tid == 2);
    uint32_t fs = SLOT_NONE;
    if (PROBE) {
      if (nvbx_index_in_range(nx, ny, nz)) fs = q_probe(m, nx, ny, nz, F_TSDF);
      a.fslots[3 * (size_t)slot + tid] = fs;
    } else fs = a.fslots[3 * (size_t)slot + tid];
    s.fslot[tid] = fs;
  }
  __syncthreads();
  if (tid < 192) {
    const int f = tid >> 6, i = tid & 63;
    const uint32_t fs = s.fslot[f];
    const int idx = f == 0 ? i : f == 1 ? (i >> 3) * 64 + (i & 7) : i * 8;
    float2 v = make_float2(__uint_as_float(0x7FC00000u), 0.0f);      // no block: never observed, whatever min_weight is
    if (slot_ok(fs)) v = m.tsdf[(size_t)fs * 512 + idx];
    s.face[f][i] = v;
  }
  __syncthreads();
  const int vx = tid >> 6, vy = (tid >> 3) & 7, vz = tid & 7;
  if (!nvbx_surface_origin_kept(8 * bx + vx, 8 * by + vy, 8 * bz + vz, a.stride, a.use_box, a.box)) return 0u;
  const float2 v0 = s.v[tid];
  uint32_t mask = 0u;
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    uint32_t ns; int nt;
    const float2 v1 = surface_neighbour(s, slot, tid, ax, &ns, &nt);
    bool c = nvbx_surface_crosses(v0.x, v0.y, v1.x, v1.y, a.min_weight);
    if (c && a.require_color) { uint32_t rgba; c = surface_color(m, slot, tid, ns, nt, v0.x, v1.x, &rgba); }
    mask |= c ? (1u << ax) : 0u;
  }
  return mask;
}

__global__ __launch_bounds__(SF_TPB) void k_surface_count(DMap m, SurfaceArgs a) {
  __shared__ SurfaceTile s;
  __shared__ uint32_t s_w[SF_TPB / 64];
  const int tid = threadIdx.x;
  const int32_t hw = min(m.counters[C_HIGH_WATER], (int32_t)m.capacity);
  for (int32_t slot = blockIdx.x; slot < hw; slot += gridDim.x) {
    if (!(m.slot_flags[slot] & F_TSDF)) { if (tid == 0) a.counts[slot] = 0u; continue; }      // uniform
    __syncthreads();                                   // the previous block's readers of the tile and of s_w are done
    const uint32_t mask = surface_tile<true>(m, a, (uint32_t)slot, s, tid);
    const uint32_t wt = __popcll(__ballot(mask & 1u)) + __popcll(__ballot(mask & 2u)) + __popcll(__ballot(mask & 4u));
    if ((tid & 63) == 0) s_w[tid >> 6] = wt;
    __syncthreads();
    if (tid == 0) {
      uint32_t t = 0u;
      for (int w = 0; w < SF_TPB / 64; w++) t += s_w[w];
      a.counts[slot] = t;
    }
  }
}

__global__ __launch_bounds__(SF_TILE) void k_surface_tile_sums(DMap m, SurfaceArgs a) {
  __shared__ uint32_t s_w[SF_TILE / 64];
  const int tid = threadIdx.x;
  const int32_t hw = min(m.counters[C_HIGH_WATER], (int32_t)m.capacity);
  const int64_t slot = (int64_t)blockIdx.x * SF_TILE + tid;
  uint32_t c = slot < hw ? a.counts[slot] : 0u;
#pragma unroll
  for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
  if ((tid & 63) == 0) s_w[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0u;
    for (int w = 0; w < SF_TILE / 64; w++) t += s_w[w];
    a.tile_sum[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(SF_SCAN_TPB) void k_surface_scan_tiles(SurfaceArgs a) {
  __shared__ u64 s_w[SF_SCAN_TPB / 64];
  __shared__ u64 s_carry;
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_carry = 0ull;
  __syncthreads();
  for (int32_t base = 0; base < a.ntiles; base += SF_SCAN_TPB) {
    const int32_t i = base + tid;
    const u64 own = i < a.ntiles ? (u64)a.tile_sum[i] : 0ull;
    u64 inc = own;                                     // inclusive prefix inside the wavefront
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u64 up = __shfl_up(inc, o); if (lane >= o) inc += up; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 before = s_carry;
    for (int w = 0; w < wave; w++) before += s_w[w];
    if (i < a.ntiles) a.tile_off[i] = before + (inc - own);
    __syncthreads();                                   // every lane has read s_carry and s_w
    if (tid == SF_SCAN_TPB - 1) s_carry = before + inc;
    __syncthreads();
  }
  if (tid == 0) *a.count = (long long)s_carry;
}

// crossing `code` = t << 2 | axis of the tile's block (bx, by, bz) -> t; p = its point, *d0 / *d1 = the edge's distances, *ns / *nt = the neighbour's slot and voxel
__device__ inline int surface_row_point(const SurfaceTile& s, uint32_t slot, int code, int32_t bx, int32_t by, int32_t bz, float vs, uint32_t* ns, int* nt,
                                        float* d0, float* d1, float p[3]) {
  const int t = code >> 2, ax = code & 3;
  const int vx = t >> 6, vy = (t >> 3) & 7, vz = t & 7;
  *d0 = s.v[t].x;
  *d1 = surface_neighbour(s, slot, t, ax, ns, nt).x;
  p[0] = nvbx_surface_center(bx, vx, vs); p[1] = nvbx_surface_center(by, vy, vs); p[2] = nvbx_surface_center(bz, vz, vs);
  const float off = vs * NVBX_DIV(-*d0, *d1 - *d0);
  p[0] = ax == 0 ? p[0] + off : p[0]; p[1] = ax == 1 ? p[1] + off : p[1]; p[2] = ax == 2 ? p[2] + off : p[2];
  return t;
}

__global__ __launch_bounds__(SF_TPB) void k_surface_emit(DMap m, SurfaceArgs a) {
  __shared__ SurfaceTile s;
  __shared__ uint32_t s_w[SF_TPB / 64], s_b[SF_TPB / 64];
  __shared__ uint16_t s_list[3 * 512];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t hw = min(m.counters[C_HIGH_WATER], (int32_t)m.capacity);
  for (int32_t slot = blockIdx.x; slot < hw; slot += gridDim.x) {
    if (!(m.slot_flags[slot] & F_TSDF)) continue;      // uniform
    const uint32_t total = a.counts[slot];
    if (total == 0u) continue;                         // uniform: no crossing, nothing of the block is read
    __syncthreads();                                   // the previous block's readers of the tile, s_w, s_b and s_list are done
    // the scan's add: the block's first row
    const int32_t tile = slot / SF_TILE, first = tile * SF_TILE;
    uint32_t below = (tid < slot - first) ? a.counts[first + tid] : 0u;
#pragma unroll
    for (int o = 32; o; o >>= 1) below += __shfl_xor(below, o);
    if (lane == 0) s_b[wave] = below;
    const uint32_t mask = surface_tile<false>(m, a, (uint32_t)slot, s, tid);      // (its barriers publish s_b as well)
    u64 row0 = a.tile_off[tile];
    for (int w = 0; w < SF_TPB / 64; w++) row0 += s_b[w];
    if ((long long)row0 >= a.capacity) continue;       // uniform: counted, written nowhere
    // ranks in (t, axis) order
    const unsigned long long b0 = __ballot(mask & 1u), b1 = __ballot(mask & 2u), b2 = __ballot(mask & 4u);
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (lane == 0) s_w[wave] = __popcll(b0) + __popcll(b1) + __popcll(b2);
    __syncthreads();
    uint32_t rank = __popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt);
    for (int w = 0; w < wave; w++) rank += s_w[w];
#pragma unroll
    for (int ax = 0; ax < 3; ax++)
      if (mask & (1u << ax)) { s_list[rank] = (uint16_t)((tid << 2) | ax); rank++; }
    __syncthreads();
    const int32_t bx = m.slot_index[3 * slot], by = m.slot_index[3 * slot + 1], bz = m.slot_index[3 * slot + 2];
    // rows r, r + 512, ..: the point and its colour
    const uint32_t rows = (uint32_t)min((long long)total, a.capacity - (long long)row0);
    for (uint32_t r = tid; r < rows; r += SF_TPB) {
      const size_t row = (size_t)row0 + r;
      uint32_t ns; int nt; float d0, d1, p[3];
      const int t = surface_row_point(s, (uint32_t)slot, s_list[r], bx, by, bz, a.vs, &ns, &nt, &d0, &d1, p);
      a.points[3 * row] = p[0]; a.points[3 * row + 1] = p[1]; a.points[3 * row + 2] = p[2];
      if (a.colors) {
        uint32_t rgba;
        surface_color(m, (uint32_t)slot, t, ns, nt, d0, d1, &rgba);
        a.colors[3 * row] = (uint8_t)(rgba & 0xFFu); a.colors[3 * row + 1] = (uint8_t)((rgba >> 8) & 0xFFu); a.colors[3 * row + 2] = (uint8_t)((rgba >> 16) & 0xFFu);
      }
    }
  }
}

// one lane per written row: the normal at the point k_surface_emit left there
__global__ __launch_bounds__(256) void k_surface_normals(DMap m, SurfaceArgs a) {
  const uint2* pool = reinterpret_cast<const uint2*>(m.tsdf);
  const long long rows = min(*a.count, (long long)a.capacity);
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < rows; row += (long long)gridDim.x * blockDim.x) {
    const float p[3] = {a.points[3 * row], a.points[3 * row + 1], a.points[3 * row + 2]};
    float d, g[3], n[3] = {0.0f, 0.0f, 0.0f};
    if (q_point<Q_TSDF>(m, pool, p, a.vs, a.min_weight, 0.0f, 0, &d, g)) {
      const float len = NVBX_SQRT((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
      if (len > 0.0f) { n[0] = NVBX_DIV(g[0], len); n[1] = NVBX_DIV(g[1], len); n[2] = NVBX_DIV(g[2], len); }
    }
    a.normals[3 * row] = n[0]; a.normals[3 * row + 1] = n[1]; a.normals[3 * row + 2] = n[2];
  }
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" void nvbx_default_surface_options(nvbx_surface_options* o) {
  if (!o) return;
  o->min_weight = 1e-4f; o->stride = 1; o->use_box = 0; o->require_color = 0;
  for (int k = 0; k < 3; k++) { o->box_min_max_vox[k] = INT32_MIN; o->box_min_max_vox[3 + k] = INT32_MAX; }
}

namespace {

// the refusals of nvbx_surface_points in their order (m is not null); *o = the options with the defaults filled in
int surface_check(const char* who, const nvbx_mapper* m, const nvbx_surface_options* options, const void* points, int64_t capacity, const void* count,
                  nvbx_surface_options* o) {
  if (!count) return refuse(who, ": count_dev is required");
  if (options) *o = *options; else nvbx_default_surface_options(o);
  if (capacity < 0 || capacity > SF_MAX_POINTS) return refuse(who, ": capacity must be 0 .. 2^30");
  if (capacity > 0 && !points) return refuse(who, ": points_dev is required with capacity > 0");
  if (o->stride < 1) return refuse(who, ": stride must be >= 1");
  if (std::isnan(o->min_weight)) return refuse(who, ": min_weight is not a number");
  const int32_t* b = o->box_min_max_vox;
  if (o->use_box && (b[0] > b[3] || b[1] > b[4] || b[2] > b[5])) return refuse(who, ": box_min_max_vox has min > max on an axis");
  return tsdf_reader_refused(m, who);
}

// count and scan of src's surface on `on`'s stream -> `a`, with *count_dev written; both mappers' calls have begun
int surface_scan(nvbx_mapper* on, nvbx_mapper* src, const nvbx_surface_options& o, int64_t* count_dev, SurfaceArgs& a) {
  const int64_t cap = src->capacity, ntiles = (cap + SF_TILE - 1) / SF_TILE;
  const size_t counts_bytes = ((size_t)cap * 16 + 63) / 64 * 64, sums_bytes = ((size_t)ntiles * 4 + 63) / 64 * 64;
  if (on->surface_buf.ensure(on->stream, SF_HEAD_BYTES + counts_bytes + sums_bytes + (size_t)ntiles * 8)) return NVBX_E_DEVICE;
  unsigned char* base = on->surface_buf.as<unsigned char>();
  a = SurfaceArgs{};
  a.vs = src->p.voxel_size; a.min_weight = o.min_weight; a.stride = o.stride; a.use_box = o.use_box != 0; a.require_color = o.require_color != 0;
  for (int k = 0; k < 6; k++) a.box[k] = o.box_min_max_vox[k];
  a.counts = reinterpret_cast<uint32_t*>(base + SF_HEAD_BYTES);
  a.fslots = a.counts + cap;                          // [cap][3]: the slots of every block's +x, +y, +z neighbours, left by the count for the emit
  a.tile_sum = reinterpret_cast<uint32_t*>(base + SF_HEAD_BYTES + counts_bytes);
  a.tile_off = reinterpret_cast<u64*>(base + SF_HEAD_BYTES + counts_bytes + sums_bytes);
  a.ntiles = (int32_t)ntiles;
  a.count = reinterpret_cast<long long*>(count_dev ? count_dev : reinterpret_cast<int64_t*>(base));
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, 65536)));
  NVBX_LAUNCH(on, k_surface_count, grid, dim3(SF_TPB), src->d, a);
  NVBX_LAUNCH(on, k_surface_tile_sums, dim3((unsigned)ntiles), dim3(SF_TILE), src->d, a);
  NVBX_LAUNCH(on, k_surface_scan_tiles, dim3(1), dim3(SF_SCAN_TPB), a);
  return NVBX_OK;
}

int surface_emit(nvbx_mapper* on, nvbx_mapper* src, SurfaceArgs& a, float* points, uint8_t* colors, float* normals, int64_t capacity) {
  if (capacity <= 0) return NVBX_OK;
  a.points = points; a.colors = colors; a.normals = normals; a.capacity = capacity;
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(src->capacity, 65536)));
  NVBX_LAUNCH(on, k_surface_emit, grid, dim3(SF_TPB), src->d, a);
  if (normals) NVBX_LAUNCH(on, k_surface_normals, dim3((unsigned)std::min<int64_t>((capacity + 255) / 256, 2048)), dim3(256), src->d, a);
  return NVBX_OK;
}

// what nvbx_align_map and nvbx_relocalize_map refuse first
int map_pair_refused(const char* who, const nvbx_mapper* dst, const nvbx_mapper* src) {
  if (!dst || !src) return refuse(who, ": both mappers are required");
  if (src == dst) return refuse(who, ": src and dst are the same mapper");
  if (src->device != dst->device) return refuse(who, ": the mappers are on different devices");
  return NVBX_OK;
}

// src's surface points into dst's scratch, on dst's stream behind src's: -> *pts, *rgb (null unless color), *n.  Waits once, for the count.
int map_points(const char* who, nvbx_mapper* dst, nvbx_mapper* src, const nvbx_surface_options& o, bool color, float** pts, uint8_t** rgb, int64_t* n) {
  NVBX_HIP(hipSetDevice(dst->device));
  // (colour is read: src's held-back colour work is carried out, as for nvbx_query_colors; else it stays held back)
  if ((color ? src->begin_call() : src->begin_call_keeping_held()) || dst->begin_call_keeping_held()) return NVBX_E_DEVICE;
  { const int rc = nvbx_mapper_wait_for(dst, src); if (rc) return rc; }
  SurfaceArgs a;
  if (surface_scan(dst, src, o, nullptr, a)) return NVBX_E_DEVICE;
  int64_t count = 0;
  NVBX_HIP(hipMemcpyAsync(&count, a.count, sizeof(count), hipMemcpyDeviceToHost, dst->stream));
  NVBX_HIP(hipStreamSynchronize(dst->stream));         // THE wait of the call: the count sizes the scratch and the alignment's grid
  *pts = nullptr; *rgb = nullptr; *n = count;
  if (count > SF_MAX_POINTS) {
    (void)nvbx_mapper_wait_for(src, dst);
    set_error((std::string(who) + ": the source map has more than 2^30 surface points; use a stride or a box").c_str());
    return NVBX_E_CAPACITY;
  }
  if (count > 0) {
    const size_t pts_bytes = ((size_t)count * 12 + 63) / 64 * 64;
    if (dst->surface_pts.ensure(dst->stream, pts_bytes + (color ? (size_t)count * 3 : 0))) return NVBX_E_DEVICE;
    *pts = dst->surface_pts.as<float>();
    if (color) *rgb = dst->surface_pts.as<uint8_t>() + pts_bytes;
    if (surface_emit(dst, src, a, *pts, *rgb, nullptr, count)) return NVBX_E_DEVICE;
  }
  NVBX_HIP(hipGetLastError());
  return nvbx_mapper_wait_for(src, dst);               // later work on src runs behind the reads
}

}  // namespace

extern "C" int nvbx_surface_points(nvbx_mapper* m, const nvbx_surface_options* options, float* points_dev, uint8_t* colors_dev, float* normals_dev,
                                   int64_t capacity, int64_t* count_dev) {
  const char* who = "nvbx_surface_points";
  if (!m) return refuse(who, ": the mapper is required");
  nvbx_surface_options o;
  { const int rc = surface_check(who, m, options, points_dev, capacity, count_dev, &o); if (rc) return rc; }
  NVBX_HIP(hipSetDevice(m->device));
  const bool color = colors_dev || o.require_color;
  if (color ? m->begin_call() : m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  SurfaceArgs a;
  if (surface_scan(m, m, o, count_dev, a) || surface_emit(m, m, a, points_dev, colors_dev, normals_dev, capacity)) return NVBX_E_DEVICE;
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

extern "C" int nvbx_align_map(nvbx_mapper* dst, nvbx_mapper* src, const float T_D_S_guess[16], const nvbx_surface_options* surface_options,
                              const nvbx_align_options* align_options, const nvbx_align_color_options* color_options, nvbx_align_result* result_dev,
                              nvbx_align_color_result* color_result_dev) {
  const char* who = "nvbx_align_map";
  if (map_pair_refused(who, dst, src)) return NVBX_E_INVALID;
  nvbx_surface_options o;
  const bool color = color_options != nullptr;
  int rc = surface_check(who, src, surface_options, nullptr, 0, dst, &o);
  if (!rc) rc = align_points_call(who, dst, nullptr, nullptr, 0, T_D_S_guess, align_options, color, color_options, result_dev, color_result_dev, true);
  if (rc) return rc;
  if (color) o.require_color = 1;
  float* pts; uint8_t* rgb; int64_t n;
  rc = map_points(who, dst, src, o, color, &pts, &rgb, &n);
  if (rc) return rc;
  return align_points_call(who, dst, pts, rgb, n, T_D_S_guess, align_options, color, color_options, result_dev, color_result_dev, false);
}

extern "C" int nvbx_relocalize_map(nvbx_mapper* dst, nvbx_mapper* src, const float T0[16], const nvbx_search_lattice* lattice,
                                   const nvbx_surface_options* surface_options, const nvbx_score_options* score_options, int32_t min_inliers,
                                   const nvbx_align_options* align_options, nvbx_pose_score* scores_dev, nvbx_relocalize_result* result_dev) {
  const char* who = "nvbx_relocalize_map";
  if (map_pair_refused(who, dst, src)) return NVBX_E_INVALID;
  nvbx_surface_options o;
  int rc = surface_check(who, src, surface_options, nullptr, 0, dst, &o);
  if (!rc) rc = relocalize_points_call(who, dst, nullptr, 0, T0, lattice, score_options, min_inliers, align_options, scores_dev, result_dev, true);
  if (rc) return rc;
  float* pts; uint8_t* rgb; int64_t n;
  rc = map_points(who, dst, src, o, false, &pts, &rgb, &n);
  if (rc) return rc;
  return relocalize_points_call(who, dst, pts, n, T0, lattice, score_options, min_inliers, align_options, scores_dev, result_dev, false);
}
