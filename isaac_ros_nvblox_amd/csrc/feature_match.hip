// feature_match.hip -- scoring the feature layer against query embeddings (SEMANTICS.md "Feature matching"): per voxel the dot
// product or the cosine with each of Q <= 128 fp16 query vectors, over every feature block of the map (nvbx_match_features: scores, the best
// query per voxel) or at the voxels that contain given points (nvbx_match_points).  Read-only on the map.
//
// The one dense contraction of the library, and its one use of the matrix cores: v_mfma_f32_32x32x16_f16, queries on the rows (A), voxels on the
// columns (B).  The value pool's layout is the instruction's operand layout: lane l of a wavefront takes column l & 31 and the 8 channels of chunk
// 2 s + (l >> 5) in k-step s, which is the 16 bytes at val[(slot nch + chunk) 512 + voxel] -- one global load per lane is a B fragment, no LDS
// transpose.  The queries are staged once per workgroup in LDS in the same [chunk][row][8 halfs] order (a ds_read_b128 per lane is an A fragment,
// 512 B contiguous per half-wave), rows >= Q and chunks >= nch zero.  The accumulator of a 32-row tile has the voxel on the lane and the queries in
// its 16 registers (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)): the argmax over queries is in-lane plus one exchange with lane ^ 32, and
// |f|^2 is summed per lane from the fragments it loaded anyway.
//
// Two kernels, one device function (match_accumulate: NT column tiles of 32 voxels against RT row tiles of 32 queries) and one epilogue
// (match_epilogue: normalise, mask, store, argmax):
//   k_match_features  256-thread workgroups persistent over the slot range, candidates found by a ballot on the flags of 64 slots per load as
//                     k_integrate_features finds them, but strided (workgroup g owns slots g, g + grid, ...: consecutive feature slots spread over
//                     the grid); one atomic per feature block claims its output entry; wavefront w takes voxels 128 w .. 128 w + 127
//   k_match_points    a wavefront per 64 points: lane l resolves point l's slot (find_slot), the column tiles gather from there
#include <algorithm>
#include "nvbx_mapper.h"
#include "nvbx_feature.h"      // half8, feature_voxel_of

using namespace nvbx;

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct MatchArgs {
  const half8* val; const float* w;      // the pools
  const half8* q;                        // [Q][nch] chunks, row-major
  int32_t nch, Q, metric;
  int32_t vec4;                          // the score matrix takes 16-byte stores (Q a multiple of 4, base 16-byte aligned)
  float min_weight;
};

// LDS of both kernels: [nch2][32 RT] query chunks (nch2 = nch rounded up to even), then 32 RT query norms |q|^2
__device__ inline int match_nch2(int nch) { return (nch + 1) & ~1; }
template <int RT> __device__ inline void stage_queries(const MatchArgs& a, half8* qs, float* qn) {
  constexpr int QP = 32 * RT;
  const int nch2 = match_nch2(a.nch);
  half8 z;
#pragma unroll
  for (int j = 0; j < 8; j++) z[j] = (_Float16)0.0f;
  for (int i = threadIdx.x; i < nch2 * QP; i += blockDim.x) {
    const int k = i / QP, r = i - k * QP;
    qs[i] = (r < a.Q && k < a.nch) ? a.q[(size_t)r * a.nch + k] : z;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < QP; r += blockDim.x) {
    float s = 0.0f;
    for (int k = 0; k < a.nch; k++) {
      const half8 v = qs[k * QP + r];
#pragma unroll
      for (int j = 0; j < 8; j++) s += (float)v[j] * (float)v[j];
    }
    qn[r] = s;
  }
  __syncthreads();
}

// Accumulate NT column tiles against all queries.  p[c]: the lane's value of chunk (lane >> 5) for tile c's column (lane & 31) -- chunk k of the same
// voxel lies 512 k further on; ok[c] false: a column without a voxel (zero fragments).  acc[c][r]: tile c x row tile r; nf[c]: the lane's share of |f|^2.
template <int RT, int NT>
__device__ inline void match_accumulate(const half8* const (&p)[NT], const bool (&ok)[NT], int nch, const half8* qs, floatx16 (&acc)[NT][RT], float (&nf)[NT]) {
  constexpr int QP = 32 * RT;
  const int lane = threadIdx.x & 63, h = lane >> 5;
  half8 z;
#pragma unroll
  for (int j = 0; j < 8; j++) z[j] = (_Float16)0.0f;
#pragma unroll
  for (int c = 0; c < NT; c++) {
    nf[c] = 0.0f;
#pragma unroll
    for (int r = 0; r < RT; r++)
#pragma unroll
      for (int j = 0; j < 16; j++) acc[c][r][j] = 0.0f;
  }
  // KU k-steps' fragments are loaded together (KU NT loads in flight per lane), then multiplied: a tile costs ceil(ks / KU) memory round trips, not ks
  constexpr int KU = 4;
  const int ks = (nch + 1) >> 1;
  for (int s0 = 0; s0 < ks; s0 += KU) {
    half8 b[KU][NT];
#pragma unroll
    for (int u = 0; u < KU; u++)
#pragma unroll
      for (int c = 0; c < NT; c++) b[u][c] = (ok[c] && 2 * (s0 + u) + h < nch) ? p[c][(size_t)(2 * (s0 + u)) * 512] : z;      // (a chunk at or beyond nch: a zero fragment)
#pragma unroll
    for (int u = 0; u < KU; u++) {
      if (s0 + u >= ks) break;                         // uniform
      const half8* qa = qs + (2 * (s0 + u) + h) * QP + (lane & 31);
#pragma unroll
      for (int r = 0; r < RT; r++) {
        const half8 av = qa[32 * r];
#pragma unroll
        for (int c = 0; c < NT; c++) acc[c][r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b[u][c], acc[c][r], 0, 0, 0);
      }
#pragma unroll
      for (int c = 0; c < NT; c++)
#pragma unroll
        for (int j = 0; j < 8; j++) nf[c] += (float)b[u][c][j] * (float)b[u][c][j];
    }
  }
}

// One column tile's results.  counts: the lane's voxel counts (both halves of the wavefront agree); row: where the voxel's Q scores go, or null;
// label / score: where its best query goes (half 0 writes), or null.  A voxel that does not count: zeros, label -1.
template <int RT>
__device__ inline void match_epilogue(const MatchArgs& a, floatx16 (&acc)[RT], float nf_lane, bool counts, const float* qn, float* row, int32_t* label, float* score) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const float nf = nf_lane + __shfl_xor(nf_lane, 32);
  float best = 0.0f; int32_t bi = -1;
#pragma unroll
  for (int r = 0; r < RT; r++) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int q0 = 32 * r + 8 * g + 4 * h;           // registers 4 g .. 4 g + 3 of the tile: queries q0 .. q0 + 3
      if (q0 >= a.Q) continue;
      float s[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float v = acc[r][4 * g + j];
        if (a.metric == NVBX_MATCH_COSINE) {
          const float nq = qn[q0 + j];
          v = (nf > 0.0f && nq > 0.0f) ? NVBX_DIV(v, NVBX_SQRT(nf * nq)) : 0.0f;
        }
        s[j] = counts ? v : 0.0f;
        if (counts && q0 + j < a.Q && (bi < 0 || s[j] > best)) { best = s[j]; bi = q0 + j; }      // (rows in rising order: the lowest index keeps a tie)
      }
      if (row) {
        if (a.vec4) *reinterpret_cast<float4*>(row + q0) = make_float4(s[0], s[1], s[2], s[3]);
        else {
#pragma unroll
          for (int j = 0; j < 4; j++) if (q0 + j < a.Q) row[q0 + j] = s[j];
        }
      }
    }
  }
  if (label) {
    const float ob = __shfl_xor(best, 32); const int32_t oi = __shfl_xor(bi, 32);
    if (oi >= 0 && (bi < 0 || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    if (counts && bi < 0) { bi = 0; best = acc[0][0]; }      // (every score a NaN: query 0, whose score half 0 holds)
    if (h == 0) { *label = counts ? bi : -1; *score = counts ? best : 0.0f; }
  }
}

struct MatchScanArgs {
  MatchArgs a;
  int32_t* block_idx; int32_t* label; float* score; float* all;
  int64_t capacity; unsigned long long* count;
};

template <int RT> __global__ __launch_bounds__(256) void k_match_features(DMap m, MatchScanArgs sa) {
  constexpr int NT = RT > 2 ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const MatchArgs& a = sa.a;
  half8* qs = reinterpret_cast<half8*>(smem);
  float* qn = reinterpret_cast<float*>(qs + match_nch2(a.nch) * 32 * RT);
  long long* s_e = reinterpret_cast<long long*>(qn + 32 * RT);
  stage_queries<RT>(a, qs, qn);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const int32_t cap = (int32_t)m.capacity;
  const int32_t n_wg = (int32_t)gridDim.x, wg = (int32_t)blockIdx.x;
  const int32_t hw = min(m.counters[C_HIGH_WATER], cap);
  // workgroup wg owns the slots wg, wg + n_wg, wg + 2 n_wg, ...: 64 of them per flag load (lane j: the j-th), so that a run of consecutive feature
  // slots -- frames allocate their blocks together -- spreads over as many workgroups instead of queueing in one
  for (int32_t base = wg; base < hw; base += 64 * n_wg) {
    const int64_t ls = (int64_t)base + (int64_t)lane * n_wg;
    const uint32_t lflags = ls < hw ? m.slot_flags[ls] : 0u;
    u64 cand = __ballot((lflags & F_FEATURE) != 0u);      // (the same in all four wavefronts: nobody writes these bits here)
    while (cand) {
      const int cj = __ffsll((long long)cand) - 1;
      cand &= cand - 1ull;
      const int32_t slot = base + cj * n_wg;
      __syncthreads();
      if (tid == 0) *s_e = (long long)atomicAdd(sa.count, 1ull);
      __syncthreads();
      const long long e = *s_e;
      if (e >= sa.capacity) continue;                  // uniform: counted, not written anywhere
      if (tid < 3) sa.block_idx[3 * e + tid] = m.slot_index[3 * slot + tid];
      const half8* vb = a.val + ((size_t)slot * a.nch + h) * 512;
      const float* wb = a.w + (size_t)slot * 512;
#pragma unroll 1
      for (int t0 = 128 * wave; t0 < 128 * wave + 128; t0 += 32 * NT) {
        const half8* p[NT]; bool ok[NT]; float wv[NT];
#pragma unroll
        for (int c = 0; c < NT; c++) { const int t = t0 + 32 * c + (lane & 31); p[c] = vb + t; ok[c] = true; wv[c] = wb[t]; }
        floatx16 acc[NT][RT]; float nf[NT];
        match_accumulate<RT, NT>(p, ok, a.nch, qs, acc, nf);
#pragma unroll
        for (int c = 0; c < NT; c++) {
          const size_t v = (size_t)e * 512 + t0 + 32 * c + (lane & 31);
          const bool counts = wv[c] > 0.0f && wv[c] >= a.min_weight;
          match_epilogue<RT>(a, acc[c], nf[c], counts, qn, sa.all ? sa.all + v * a.Q : nullptr, sa.label + v, sa.score + v);
        }
      }
    }
  }
}

template <int RT> __global__ __launch_bounds__(256) void k_match_points(DMap m, MatchArgs a, const float* __restrict__ pts, int64_t n, float vs,
                                                                        float* __restrict__ scores, float* __restrict__ w_out) {
  constexpr int NT = RT > 2 ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  half8* qs = reinterpret_cast<half8*>(smem);
  float* qn = reinterpret_cast<float*>(qs + match_nch2(a.nch) * 32 * RT);
  stage_queries<RT>(a, qs, qn);
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t p0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64; p0 < n; p0 += n_waves * 64) {
    // lane l: point p0 + l -> its slot, voxel and weight
    const int64_t pi = p0 + lane;
    uint32_t slot = SLOT_NONE; int32_t t = 0; float wv = 0.0f;
    if (pi < n) {
      int32_t g[3] = {0, 0, 0};
      if (feature_voxel_of(pts[3 * pi], pts[3 * pi + 1], pts[3 * pi + 2], vs, g)) slot = find_slot(m, g[0] >> 3, g[1] >> 3, g[2] >> 3, F_FEATURE);
      if (slot_ok(slot)) { t = (g[2] & 7) + 8 * (g[1] & 7) + 64 * (g[0] & 7); wv = a.w[(size_t)slot * 512 + t]; }
      w_out[pi] = wv;
    }
#pragma unroll 1
    for (int c0 = 0; c0 < 2; c0 += NT) {
      const half8* p[NT]; bool ok[NT]; float cw[NT];
#pragma unroll
      for (int c = 0; c < NT; c++) {
        const int src = 32 * (c0 + c) + (lane & 31);
        const uint32_t cs = __shfl(slot, src); const int32_t ct = __shfl(t, src); cw[c] = __shfl(wv, src);
        ok[c] = slot_ok(cs);
        p[c] = a.val + ((size_t)(ok[c] ? cs : 0u) * a.nch + h) * 512 + ct;
      }
      floatx16 acc[NT][RT]; float nf[NT];
      match_accumulate<RT, NT>(p, ok, a.nch, qs, acc, nf);
#pragma unroll
      for (int c = 0; c < NT; c++) {
        const int64_t cp = p0 + 32 * (c0 + c) + (lane & 31);
        match_epilogue<RT>(a, acc[c], nf[c], cw[c] > 0.0f, qn, cp < n ? scores + cp * a.Q : nullptr, nullptr, nullptr);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ C-ABI
static int match_common(nvbx_mapper* m, const char* who, const void* queries_dev, int32_t n_queries, int32_t metric, MatchArgs* a, size_t* smem, int* rt) {
  if (!m) return NVBX_E_INVALID;
  if (!m->feat_channels) return refuse(who, ": call nvbx_enable_features first");
  if (n_queries < 1 || n_queries > 128) return refuse(who, ": n_queries must be 1 .. 128");
  if (metric != NVBX_MATCH_DOT && metric != NVBX_MATCH_COSINE) return refuse(who, ": unknown metric");
  if (!queries_dev || ((uintptr_t)queries_dev & 15)) return refuse(who, ": queries_dev is NULL or not 16-byte aligned");
  a->val = static_cast<const half8*>(m->feat_val); a->w = m->feat_w; a->q = static_cast<const half8*>(queries_dev);
  a->nch = m->feat_channels / 8; a->Q = n_queries; a->metric = metric; a->vec4 = 0; a->min_weight = 0.0f;
  *rt = n_queries <= 32 ? 1 : n_queries <= 64 ? 2 : 4;
  *smem = (size_t)((a->nch + 1) & ~1) * 32 * *rt * 16 + (size_t)32 * *rt * 4 + 16;
  return NVBX_OK;
}
// up to 64 KiB of queries + their norms: above the default limit of dynamic LDS
template <typename K> static int match_allow_smem(K kernel, size_t smem) {
  if (smem <= 48u * 1024) return NVBX_OK;
  NVBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  return NVBX_OK;
}

extern "C" int nvbx_match_features(nvbx_mapper* m, const void* queries_dev, int32_t n_queries, int32_t metric, float min_weight, nvbx_index3d* block_idx_dev,
                                   int32_t* label_dev, float* score_dev, float* all_scores_dev, int64_t capacity_blocks, int64_t* count_dev) {
  MatchScanArgs sa{}; size_t smem = 0; int rt = 1;
  const int rc = match_common(m, "nvbx_match_features", queries_dev, n_queries, metric, &sa.a, &smem, &rt);
  if (rc) return rc;
  if (capacity_blocks < 0 || !count_dev || (capacity_blocks > 0 && (!block_idx_dev || !label_dev || !score_dev))) {
    set_error("nvbx_match_features: count_dev and, with capacity_blocks > 0, block_idx_dev / label_dev / score_dev are required"); return NVBX_E_INVALID; }
  if (m->begin_call()) return NVBX_E_DEVICE;
  sa.a.min_weight = min_weight;
  sa.a.vec4 = (all_scores_dev && !(n_queries & 3) && !((uintptr_t)all_scores_dev & 15)) ? 1 : 0;
  sa.block_idx = reinterpret_cast<int32_t*>(block_idx_dev); sa.label = label_dev; sa.score = score_dev; sa.all = all_scores_dev;
  sa.capacity = capacity_blocks; sa.count = reinterpret_cast<unsigned long long*>(count_dev);
  const int grid = (int)std::min<int64_t>(m->capacity, 1024);
  NVBX_HIP(hipMemsetAsync(count_dev, 0, sizeof(int64_t), m->stream));
  if (rt == 1) { if (match_allow_smem(k_match_features<1>, smem)) return NVBX_E_DEVICE; NVBX_LAUNCH_SMEM(m, k_match_features<1>, dim3((unsigned)grid), dim3(256), smem, m->d, sa); }
  else if (rt == 2) { if (match_allow_smem(k_match_features<2>, smem)) return NVBX_E_DEVICE; NVBX_LAUNCH_SMEM(m, k_match_features<2>, dim3((unsigned)grid), dim3(256), smem, m->d, sa); }
  else { if (match_allow_smem(k_match_features<4>, smem)) return NVBX_E_DEVICE; NVBX_LAUNCH_SMEM(m, k_match_features<4>, dim3((unsigned)grid), dim3(256), smem, m->d, sa); }
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

extern "C" int nvbx_match_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const void* queries_dev, int32_t n_queries, int32_t metric,
                                 float* scores_dev, float* weight_dev) {
  MatchArgs a{}; size_t smem = 0; int rt = 1;
  const int rc = match_common(m, "nvbx_match_points", queries_dev, n_queries, metric, &a, &smem, &rt);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!points_xyz_dev || !scores_dev || !weight_dev))) { set_error("nvbx_match_points: n >= 0; points, scores_dev and weight_dev are required"); return NVBX_E_INVALID; }
  if (n == 0) return NVBX_OK;
  if (m->begin_call()) return NVBX_E_DEVICE;
  a.vec4 = (!(n_queries & 3) && !((uintptr_t)scores_dev & 15)) ? 1 : 0;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
  const float vs = m->p.voxel_size;
  if (rt == 1) { if (match_allow_smem(k_match_points<1>, smem)) return NVBX_E_DEVICE; NVBX_LAUNCH_SMEM(m, k_match_points<1>, dim3(grid), dim3(256), smem, m->d, a, points_xyz_dev, n, vs, scores_dev, weight_dev); }
  else if (rt == 2) { if (match_allow_smem(k_match_points<2>, smem)) return NVBX_E_DEVICE; NVBX_LAUNCH_SMEM(m, k_match_points<2>, dim3(grid), dim3(256), smem, m->d, a, points_xyz_dev, n, vs, scores_dev, weight_dev); }
  else { if (match_allow_smem(k_match_points<4>, smem)) return NVBX_E_DEVICE; NVBX_LAUNCH_SMEM(m, k_match_points<4>, dim3(grid), dim3(256), smem, m->d, a, points_xyz_dev, n, vs, scores_dev, weight_dev); }
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}
