// segment.hip -- from matched feature voxels to a table of 3-D objects (SEMANTICS.md "Feature segmentation"):
// nvbx_label_components labels the connected components of a labelled sparse voxel volume (the shape nvbx_match_features returns) and fills one
// record per component; nvbx_segment_features chains match, threshold and labelling on the mapper's stream.  Reads nothing from the map.
//
// Union-find with atomicMin, the scheme of k_cc_union (dynamics.hip) taken to the block grid: a voxel's id is entry 512 + t, a parent is always
// <= its child, so every chain is strictly decreasing and ends at the lowest voxel id of the set.  Seven launches in stream order, nothing waits
// for another workgroup inside a launch:
//   k_seg_local    a workgroup per block: inserts the block into the entry table (open addressing over entry numbers, compared by the block index
//                  the entry names -- no packed key, so no index range to respect) and resolves the components INSIDE the block in LDS (Jacobi
//                  min-propagation with one pointer jump per round, at most 512 rounds); parent = the block-local root (the lowest t), the id
//                  volume takes the local root's t for the later passes, the per-root count is zeroed
//   k_seg_border   27 table probes per workgroup (the 13 "positive" neighbour blocks; 3 under connectivity 6), then every border voxel unites with
//                  its equal-labelled neighbours in those blocks
//   k_seg_count    one find per (block, local root); the voxels are counted per local root in LDS, one atomicAdd per (block, local root) into
//                  count[root]; parent = root for every voxel
//   k_seg_compact  a root with count >= min_voxels claims an index (one atomic per wavefront) and starts its record; count[root] = the index or -1
//   k_seg_records  per (block, local root) in LDS: box (an occupancy mask per axis), sums and count (packed into one 64-bit add), the best
//                  {score, lowest t}; then 10 integer atomics into the record.  The peak goes into the record's last 16 bytes as two keys:
//                  key1 = {ordered score, inverted x}, a maximum
//   k_seg_peak     key2 = {y, z}, a minimum over the voxels that have key1's score and x (aggregated per local root in LDS as well); writes the ids
//   k_seg_finish   a thread per record: the two keys become peak_score / peak_xyz
#include <algorithm>
#include <limits.h>
#include "nvbx_mapper.h"

using namespace nvbx;

struct SegArgs {
  const int32_t* bidx; const int32_t* label; const float* score;      // the input ([n][3], [n][512], [n][512] or null)
  int64_t n; const long long* n_dev;                                  // entries: min(n, *n_dev) where n_dev is given
  int32_t conn, min_voxels;
  int32_t* table; uint32_t tmask;                                     // entry numbers, -1 = empty; tmask + 1 = a power of two >= 2 n
  int32_t* parent; int32_t* cnt;                                      // [n][512]
  int32_t* ids; nvbx_component* comps; int64_t cap; u64* count;       // the output
};
constexpr int SEG_TPB = 512;                 // a thread per voxel
constexpr int32_t SEG_BIAS = 1 << 23;        // global voxel coordinates of the addressable range as 24 unsigned bits

__device__ inline int32_t seg_n(const SegArgs& a) {
  long long n = a.n;
  if (a.n_dev) { const long long d = *a.n_dev; n = d < n ? d : n; }
  return n < 0 ? 0 : (int32_t)n;
}
__device__ inline uint32_t seg_hash(int32_t x, int32_t y, int32_t z) {
  return (((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349663u) ^ ((uint32_t)z * 83492791u)) * 0x9E3779B1u >> 7;
}
__device__ inline bool seg_is(const SegArgs& a, int32_t e, int32_t x, int32_t y, int32_t z) {
  return a.bidx[3 * (size_t)e] == x && a.bidx[3 * (size_t)e + 1] == y && a.bidx[3 * (size_t)e + 2] == z;
}
// (at most n of the >= 2 n places are ever taken: a probe sequence meets an empty one)
__device__ inline void seg_insert(const SegArgs& a, int32_t e) {
  const int32_t x = a.bidx[3 * (size_t)e], y = a.bidx[3 * (size_t)e + 1], z = a.bidx[3 * (size_t)e + 2];
  uint32_t h = seg_hash(x, y, z) & a.tmask;
  for (uint32_t probe = 0; probe <= a.tmask; probe++) {
    const int32_t v = atomicCAS(&a.table[h], -1, e);
    if (v == -1 || seg_is(a, v, x, y, z)) return;      // (a repeated block index: the first copy is the one the neighbours see)
    h = (h + 1) & a.tmask;
  }
}
__device__ inline int32_t seg_lookup(const SegArgs& a, int32_t x, int32_t y, int32_t z) {
  uint32_t h = seg_hash(x, y, z) & a.tmask;
  for (uint32_t probe = 0; probe <= a.tmask; probe++) {
    const int32_t v = a.table[h];
    if (v < 0) return -1;
    if (seg_is(a, v, x, y, z)) return v;
    h = (h + 1) & a.tmask;
  }
  return -1;
}

__device__ inline int32_t seg_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int32_t seg_find(const int32_t* parent, int32_t x) {
  int32_t p = seg_load(&parent[x]);
  while (p != x) { x = p; p = seg_load(&parent[x]); }      // (p < x: strictly decreasing)
  return x;
}
// find with path halving, as cc_find_halving: every second node on the way is re-hung under its grandparent
__device__ inline int32_t seg_find_halving(int32_t* parent, int32_t x) {
  int32_t p = seg_load(&parent[x]);
  while (p != x) {
    const int32_t gp = seg_load(&parent[p]);
    if (gp == p) return p;
    atomicMin(&parent[x], gp);
    x = gp; p = seg_load(&parent[x]);
  }
  return x;
}
// (every round either ends or continues from a strictly lower b: the atomicMin it retries after observed a change)
__device__ inline void seg_union(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = seg_find_halving(parent, a); b = seg_find_halving(parent, b);
    if (a == b) return;
    if (a > b) { const int32_t t = a; a = b; b = t; }
    const int32_t old = atomicMin(&parent[b], a);
    if (old == b) return;
    b = old;
  }
}

// offset k of the 27 (k = 13: none): dx = k / 9 - 1, dy = k / 3 % 3 - 1, dz = k % 3 - 1
#define SEG_DX(k) ((k) / 9 - 1)
#define SEG_DY(k) ((k) / 3 % 3 - 1)
#define SEG_DZ(k) ((k) % 3 - 1)
__device__ inline bool seg_offset_used(int k, int32_t conn) {
  const int s = abs(SEG_DX(k)) + abs(SEG_DY(k)) + abs(SEG_DZ(k));
  return s == 1 || (s > 1 && conn == 26);
}

__global__ __launch_bounds__(SEG_TPB) void k_seg_local(SegArgs a) {
  __shared__ int32_t s_lab[512], s_par[512];
  const int t = threadIdx.x, vx = t >> 6, vy = (t >> 3) & 7, vz = t & 7;
  const int32_t n = seg_n(a);
  for (int32_t e = blockIdx.x; e < n; e += gridDim.x) {
    if (t == 0) seg_insert(a, e);
    const size_t id = (size_t)e * 512 + t;
    const int32_t l = a.label[id];
    __syncthreads();                                   // (the previous block's readers are done)
    s_lab[t] = l; s_par[t] = l >= 0 ? t : -1;
    __syncthreads();
    uint32_t nb = 0;                                   // bit k: the voxel at offset k is inside the block and has this label
    if (l >= 0) {
#pragma unroll
      for (int k = 0; k < 27; k++) {
        if (k == 13 || !seg_offset_used(k, a.conn)) continue;
        const int x = vx + SEG_DX(k), y = vy + SEG_DY(k), z = vz + SEG_DZ(k);
        if ((unsigned)x < 8u && (unsigned)y < 8u && (unsigned)z < 8u && s_lab[t + SEG_DX(k) * 64 + SEG_DY(k) * 8 + SEG_DZ(k)] == l) nb |= 1u << k;
      }
    }
    // Jacobi rounds: the minimum over the neighbours' values, then one jump (the value at that minimum).  After round r a voxel holds at most
    // the minimum within r steps of it, a path inside a block has at most 511 steps: 512 rounds are enough, the exit is the first quiet one.
    int32_t cur = l >= 0 ? t : -1;
    for (int round = 0; round < 512; round++) {
      int32_t mn = cur;
      if (l >= 0) {
#pragma unroll
        for (int k = 0; k < 27; k++)
          if (nb & (1u << k)) mn = min(mn, s_par[t + SEG_DX(k) * 64 + SEG_DY(k) * 8 + SEG_DZ(k)]);
        mn = s_par[mn];
      }
      const int changed = mn < cur;
      __syncthreads();
      if (changed) { cur = mn; s_par[t] = mn; }
      if (!__syncthreads_or(changed)) break;
    }
    a.parent[id] = l >= 0 ? e * 512 + cur : -1;
    a.ids[id] = cur;                                   // the local root's t, until k_seg_peak writes the component's index
    a.cnt[id] = 0;
  }
}

__global__ __launch_bounds__(SEG_TPB) void k_seg_border(SegArgs a) {
  __shared__ int32_t s_nb[27];
  const int t = threadIdx.x, vx = t >> 6, vy = (t >> 3) & 7, vz = t & 7;
  const int32_t n = seg_n(a);
  for (int32_t e = blockIdx.x; e < n; e += gridDim.x) {
    __syncthreads();
    if (t < 27) {      // the neighbour blocks in the 13 positive directions (lexicographically above 0); the other side of a pair is that block's business
      const int dx = SEG_DX(t), dy = SEG_DY(t), dz = SEG_DZ(t);
      const bool positive = dx > 0 || (dx == 0 && (dy > 0 || (dy == 0 && dz > 0)));
      int32_t e2 = -1;
      if (positive && seg_offset_used(t, a.conn))
        e2 = seg_lookup(a, (int32_t)((uint32_t)a.bidx[3 * (size_t)e] + (uint32_t)dx), (int32_t)((uint32_t)a.bidx[3 * (size_t)e + 1] + (uint32_t)dy),
                        (int32_t)((uint32_t)a.bidx[3 * (size_t)e + 2] + (uint32_t)dz));
      s_nb[t] = e2;
    }
    __syncthreads();
    const int32_t id = e * 512 + t;
    const int32_t l = a.label[id];
    if (l < 0 || (((vx + 7) & 7) < 6 && ((vy + 7) & 7) < 6 && ((vz + 7) & 7) < 6)) continue;      // background, or no coordinate is 0 or 7
#pragma unroll
    for (int k = 0; k < 27; k++) {
      if (k == 13 || !seg_offset_used(k, a.conn)) continue;
      const int x = vx + SEG_DX(k), y = vy + SEG_DY(k), z = vz + SEG_DZ(k);      // -1 .. 8
      const int dk = ((x >> 3) + 1) * 9 + ((y >> 3) + 1) * 3 + ((z >> 3) + 1);   // which block that is
      if (dk == 13) continue;
      const int32_t e2 = s_nb[dk];
      if (e2 < 0) continue;
      const int32_t id2 = e2 * 512 + (x & 7) * 64 + (y & 7) * 8 + (z & 7);
      if (a.label[id2] == l) seg_union(a.parent, id, id2);
    }
  }
}

__global__ __launch_bounds__(SEG_TPB) void k_seg_count(SegArgs a) {
  __shared__ int32_t s_cnt[512], s_root[512];
  const int t = threadIdx.x;
  const int32_t n = seg_n(a);
  for (int32_t e = blockIdx.x; e < n; e += gridDim.x) {
    __syncthreads();
    s_cnt[t] = 0;
    __syncthreads();
    const int32_t id = e * 512 + t;
    const int32_t lr = a.ids[id];
    if (lr >= 0) atomicAdd(&s_cnt[lr], 1);
    __syncthreads();
    if (lr == t) {
      const int32_t r = seg_find(a.parent, id);
      s_root[t] = r;
      atomicAdd(&a.cnt[r], s_cnt[t]);
    }
    __syncthreads();
    if (lr >= 0) __hip_atomic_store(&a.parent[id], s_root[lr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (another block's find may pass through here: root or old ancestor, both lead there)
  }
}

// the record's last 16 bytes (peak_score, peak_xyz) hold the two peak keys until k_seg_finish
__device__ inline u64* seg_keys(nvbx_component* c) { return reinterpret_cast<u64*>(reinterpret_cast<unsigned char*>(c) + 56); }

__global__ __launch_bounds__(256) void k_seg_compact(SegArgs a) {
  const int64_t total = (int64_t)seg_n(a) * 512;       // (a multiple of 64: a wavefront is inside or outside as a whole)
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const bool root = a.parent[i] == (int32_t)i;
    const int32_t c = root ? a.cnt[i] : 0;
    const bool keep = root && c >= a.min_voxels;
    const u64 kept = __ballot(keep);
    if (kept) {
      const int leader = __ffsll((long long)kept) - 1;
      u64 base = 0;
      if (lane == leader) base = atomicAdd(a.count, (u64)__popcll(kept));
      base = __shfl(base, leader);
      if (keep) {
        const u64 ci = base + (u64)__popcll(kept & ((1ull << lane) - 1ull));
        a.cnt[i] = (int32_t)ci;
        if ((int64_t)ci < a.cap) {
          nvbx_component* c_out = a.comps + ci;
          c_out->label = a.label[i]; c_out->voxels = c;
          for (int k = 0; k < 3; k++) { c_out->min_xyz[k] = INT_MAX; c_out->max_xyz[k] = INT_MIN; c_out->sum_xyz[k] = 0; }
          seg_keys(c_out)[0] = 0ull; seg_keys(c_out)[1] = ~0ull;
        }
      }
    }
    if (root && !keep) a.cnt[i] = -1;
  }
}

// a score as an unsigned that orders as the float does; -0 counts as +0, a NaN as -infinity
__device__ inline uint32_t seg_ordered(float s) {
  s = (s == s) ? s + 0.0f : -INFINITY;
  const uint32_t b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float seg_unordered(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }
__device__ inline int32_t seg_global(int32_t block, int v) { return (int32_t)(8u * (uint32_t)block + (uint32_t)v); }

__global__ __launch_bounds__(SEG_TPB) void k_seg_records(SegArgs a) {
  __shared__ uint32_t s_box[512];      // bits 0-7: the x an own voxel has, 8-15: y, 16-23: z
  __shared__ u64 s_sum[512];           // count << 48 | sum vx << 32 | sum vy << 16 | sum vz (each sum <= 512 * 7)
  __shared__ u64 s_key[512];           // ordered score << 32 | 511 - t: the maximum is the best score at the lowest t
  const int t = threadIdx.x, vx = t >> 6, vy = (t >> 3) & 7, vz = t & 7;
  const int32_t n = seg_n(a);
  for (int32_t e = blockIdx.x; e < n; e += gridDim.x) {
    __syncthreads();
    s_box[t] = 0u; s_sum[t] = 0ull; s_key[t] = 0ull;
    __syncthreads();
    const int32_t id = e * 512 + t;
    const int32_t lr = a.ids[id];
    if (lr >= 0) {
      atomicOr(&s_box[lr], (1u << vx) | (1u << (8 + vy)) | (1u << (16 + vz)));
      atomicAdd(&s_sum[lr], (1ull << 48) | ((u64)vx << 32) | ((u64)vy << 16) | (u64)vz);
      atomicMax(&s_key[lr], ((u64)seg_ordered(a.score ? a.score[id] : 0.0f) << 32) | (u64)(511 - t));
    }
    __syncthreads();
    if (lr != t) continue;
    const int32_t ci = a.cnt[a.parent[id]];
    if (ci < 0 || (int64_t)ci >= a.cap) continue;
    nvbx_component* c = a.comps + ci;
    const uint32_t box = s_box[t]; const u64 sum = s_sum[t], key = s_key[t];
    const int64_t cnt = (int64_t)(sum >> 48);
    for (int k = 0; k < 3; k++) {
      const int32_t g0 = seg_global(a.bidx[3 * (size_t)e + k], 0);
      const uint32_t bits = (box >> (8 * k)) & 0xFFu;
      atomicMin(&c->min_xyz[k], seg_global(a.bidx[3 * (size_t)e + k], __ffs((int)bits) - 1));
      atomicMax(&c->max_xyz[k], seg_global(a.bidx[3 * (size_t)e + k], 31 - __clz((int)bits)));
      atomicAdd(reinterpret_cast<u64*>(&c->sum_xyz[k]), (u64)(cnt * (int64_t)g0 + (int64_t)((sum >> (32 - 16 * k)) & 0xFFFFull)));
    }
    const int tp = 511 - (int)(key & 0x1FFull);
    const uint32_t xb = (uint32_t)(seg_global(a.bidx[3 * (size_t)e], tp >> 6) + SEG_BIAS) & 0xFFFFFFu;
    atomicMax(&seg_keys(c)[0], ((key >> 32) << 24) | (u64)(0xFFFFFFu - xb));
  }
}

__global__ __launch_bounds__(SEG_TPB) void k_seg_peak(SegArgs a) {
  __shared__ u64 s_k1[512], s_k2[512];
  __shared__ int32_t s_ci[512];
  const int t = threadIdx.x, vx = t >> 6, vy = (t >> 3) & 7, vz = t & 7;
  const int32_t n = seg_n(a);
  for (int32_t e = blockIdx.x; e < n; e += gridDim.x) {
    __syncthreads();
    const int32_t id = e * 512 + t;
    const int32_t lr = a.ids[id];
    s_k2[t] = ~0ull;
    if (lr == t) {
      const int32_t ci = a.cnt[a.parent[id]];
      s_ci[t] = ci;
      s_k1[t] = (ci >= 0 && (int64_t)ci < a.cap) ? seg_keys(a.comps + ci)[0] : 0ull;      // (0: below every voxel's key, nobody is a candidate)
    }
    __syncthreads();
    int32_t ci = -1;
    if (lr >= 0) {
      ci = s_ci[lr];
      const uint32_t xb = (uint32_t)(seg_global(a.bidx[3 * (size_t)e], vx) + SEG_BIAS) & 0xFFFFFFu;
      const u64 mine = ((u64)seg_ordered(a.score ? a.score[id] : 0.0f) << 24) | (u64)(0xFFFFFFu - xb);
      if (mine == s_k1[lr]) {
        const uint32_t yb = (uint32_t)(seg_global(a.bidx[3 * (size_t)e + 1], vy) + SEG_BIAS) & 0xFFFFFFu;
        const uint32_t zb = (uint32_t)(seg_global(a.bidx[3 * (size_t)e + 2], vz) + SEG_BIAS) & 0xFFFFFFu;
        atomicMin(&s_k2[lr], ((u64)yb << 24) | (u64)zb);
      }
    }
    __syncthreads();
    if (lr == t && s_k2[t] != ~0ull) atomicMin(&seg_keys(a.comps + ci)[1], s_k2[t]);      // (a candidate exists only where the record does)
    a.ids[id] = ci;
  }
}

__global__ __launch_bounds__(256) void k_seg_finish(SegArgs a) {
  const int64_t found = (int64_t)*a.count, total = found < a.cap ? found : a.cap;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    nvbx_component* c = a.comps + i;
    const u64 k1 = seg_keys(c)[0], k2 = seg_keys(c)[1];
    c->peak_score = seg_unordered((uint32_t)(k1 >> 24));
    c->peak_xyz[0] = (int32_t)(0xFFFFFFu - (uint32_t)(k1 & 0xFFFFFFull)) - SEG_BIAS;
    c->peak_xyz[1] = (int32_t)((k2 >> 24) & 0xFFFFFFull) - SEG_BIAS;
    c->peak_xyz[2] = (int32_t)(k2 & 0xFFFFFFull) - SEG_BIAS;
  }
}

// the threshold of nvbx_segment_features, in place over the entries the match wrote
__global__ __launch_bounds__(256) void k_seg_threshold(int32_t* label, float* score, const float* min_score, int32_t n_queries, int64_t capacity, const long long* count) {
  const long long c = *count;
  const int64_t total = (c < 0 ? 0 : c < capacity ? c : capacity) * 512;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t l = label[i];
    if (l >= 0 && l < n_queries && score[i] < min_score[l]) { label[i] = -1; score[i] = 0.0f; }
  }
}

// ------------------------------------------------------------------------------------------------ C-ABI
constexpr int64_t SEG_MAX_BLOCKS = 1ll << 22;      // 2^22 x 512 voxel ids fill int32

// what is wrong with a call's n blocks of indices, labels and ids (null: nothing) -- seg_check's volume_why
static const char* seg_volume_why(const void* block_idx, const void* label, int64_t n, const void* ids) {
  if (n < 0 || n > SEG_MAX_BLOCKS) return ": the number of blocks must be 0 .. 2^22";
  if (n > 0 && (!block_idx || !label || !ids)) return ": block_idx_dev, label_dev and component_id_dev are required";
  return nullptr;
}

int nvbx::seg_check(const char* who, int32_t connectivity, int32_t min_voxels, const char* volume_why, const void* comps, int64_t cap, const void* count) {
  if (connectivity != 6 && connectivity != 26) return refuse(who, ": connectivity must be 6 or 26");
  if (min_voxels < 1) return refuse(who, ": min_voxels must be >= 1");
  if (volume_why) return refuse(who, volume_why);
  if (!count) return refuse(who, ": the component count pointer is required");
  if (cap < 0 || (cap > 0 && (!comps || ((uintptr_t)comps & 7)))) return refuse(who, ": components_dev must be 8-byte aligned memory for capacity_components >= 0 records");
  return NVBX_OK;
}

// the launches of nvbx_label_components; the arguments have been checked
static int seg_launch(nvbx_mapper* m, const nvbx_index3d* block_idx_dev, const int32_t* label_dev, const float* score_dev, int64_t n, const int64_t* n_dev,
                      int32_t connectivity, int32_t min_voxels, int32_t* ids, nvbx_component* comps, int64_t cap, int64_t* count_dev) {
  NVBX_HIP(hipMemsetAsync(count_dev, 0, sizeof(int64_t), m->stream));
  if (n == 0) return NVBX_OK;
  uint64_t tsz = 64; while (tsz < (uint64_t)n * 2) tsz <<= 1;
  const size_t table_bytes = (size_t)tsz * 4, vol_bytes = (size_t)n * 512 * 4;
  if (m->seg_scratch.ensure(m->stream, table_bytes + 2 * vol_bytes)) return NVBX_E_DEVICE;
  SegArgs a{};
  a.bidx = reinterpret_cast<const int32_t*>(block_idx_dev); a.label = label_dev; a.score = score_dev;
  a.n = n; a.n_dev = reinterpret_cast<const long long*>(n_dev); a.conn = connectivity; a.min_voxels = min_voxels;
  a.table = m->seg_scratch.as<int32_t>(); a.tmask = (uint32_t)(tsz - 1);
  a.parent = a.table + tsz; a.cnt = a.parent + (size_t)n * 512;
  a.ids = ids; a.comps = comps; a.cap = cap; a.count = reinterpret_cast<u64*>(count_dev);
  NVBX_HIP(hipMemsetAsync(a.table, 0xFF, table_bytes, m->stream));
  const dim3 per_block((unsigned)std::min<int64_t>(n, 8192)), flat((unsigned)std::min<int64_t>(n * 2, 2048));
  NVBX_LAUNCH(m, k_seg_local, per_block, dim3(SEG_TPB), a);
  NVBX_LAUNCH(m, k_seg_border, per_block, dim3(SEG_TPB), a);
  NVBX_LAUNCH(m, k_seg_count, per_block, dim3(SEG_TPB), a);
  NVBX_LAUNCH(m, k_seg_compact, flat, dim3(256), a);
  if (cap > 0) NVBX_LAUNCH(m, k_seg_records, per_block, dim3(SEG_TPB), a);
  NVBX_LAUNCH(m, k_seg_peak, per_block, dim3(SEG_TPB), a);
  if (cap > 0) NVBX_LAUNCH(m, k_seg_finish, dim3((unsigned)std::min<int64_t>((std::min<int64_t>(cap, n * 512) + 255) / 256, 2048)), dim3(256), a);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

extern "C" int nvbx_label_components(nvbx_mapper* m, const nvbx_index3d* block_idx_dev, const int32_t* label_dev, const float* score_dev, int64_t n_blocks,
                                     const int64_t* n_blocks_dev, int32_t connectivity, int32_t min_voxels, int32_t* component_id_dev,
                                     nvbx_component* components_dev, int64_t capacity_components, int64_t* count_dev) {
  if (!m) return NVBX_E_INVALID;
  const int rc = seg_check("nvbx_label_components", connectivity, min_voxels, seg_volume_why(block_idx_dev, label_dev, n_blocks, component_id_dev), components_dev,
                           capacity_components, count_dev);
  if (rc) return rc;
  NVBX_HIP(hipSetDevice(m->device));
  return seg_launch(m, block_idx_dev, label_dev, score_dev, n_blocks, n_blocks_dev, connectivity, min_voxels, component_id_dev, components_dev,
                    capacity_components, count_dev);
}

extern "C" int nvbx_segment_features(nvbx_mapper* m, const void* queries_dev, int32_t n_queries, int32_t metric, float min_weight, const float* min_score_dev,
                                     int32_t connectivity, int32_t min_voxels, nvbx_index3d* block_idx_dev, int32_t* label_dev, float* score_dev,
                                     int32_t* component_id_dev, int64_t capacity_blocks, int64_t* block_count_dev, nvbx_component* components_dev,
                                     int64_t capacity_components, int64_t* component_count_dev) {
  if (!m) return NVBX_E_INVALID;
  int rc = seg_check("nvbx_segment_features", connectivity, min_voxels, seg_volume_why(block_idx_dev, label_dev, capacity_blocks, component_id_dev), components_dev,
                     capacity_components, component_count_dev);
  if (rc) return rc;
  rc = nvbx_match_features(m, queries_dev, n_queries, metric, min_weight, block_idx_dev, label_dev, score_dev, nullptr, capacity_blocks, block_count_dev);
  if (rc) return rc;
  if (min_score_dev && capacity_blocks > 0) {
    NVBX_LAUNCH(m, k_seg_threshold, dim3((unsigned)std::min<int64_t>(capacity_blocks * 2, 2048)), dim3(256), label_dev, score_dev, min_score_dev, n_queries,
                capacity_blocks, reinterpret_cast<const long long*>(block_count_dev));
  }
  return seg_launch(m, block_idx_dev, label_dev, score_dev, capacity_blocks, block_count_dev, connectivity, min_voxels, component_id_dev, components_dev,
                    capacity_components, component_count_dev);
}
