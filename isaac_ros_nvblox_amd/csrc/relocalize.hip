// relocalize.hip -- where in the map is the sensor, roughly: scoring pose hypotheses against the TSDF and the search that ends in the
// alignment (nvbx_score_poses_points / _depth, nvbx_relocalize_points / _depth; SEMANTICS.md "Relocalisation").
// [U] Nothing of the kind is readable in the reference tree; scan-to-map branch-and-bound matchers and KinectFusion-style relocalisers
// answer the same question.
//
//   k_score_poses   one workgroup = one pose x one chunk of the points: 256 points, one per lane, up to 1 024 chunks.  Beyond that -- and
//                   in the one-workgroup-per-pose variant, which measured slower -- a lane takes `per_lane` CONSECUTIVE points
//                   (neighbouring pixels or scan points lie in neighbouring voxels: the lane keeps the slot of the last base block,
//                   q_point<.., DIST_ONLY>, and probes the hash only when the base corner leaves that block).  A lane fetches its point
//                   (point_source_fetch), transforms it (apply_rt, f32), takes the TSDF distance of k_query_points (the same inline code)
//                   and classifies it.  The three counts are ballots and pop-counts
//                   per wavefront, kept in scalar registers; |d| in 2^-20 m is summed per lane in 64 bits, once across the wavefront
//                   with shuffles, once across the four wavefronts through LDS.  With one chunk the workgroup stores the record; with
//                   more it adds to a record zeroed on the stream with vector integer atomics -- integer sums, so any order gives the
//                   same bits.  The pose comes from the caller's list, from the lattice tables (workgroups ordered yaw-major, so that
//                   neighbours in the launch are spatial neighbours of one yaw and read neighbouring voxels), or from the result record
//                   of a relocalisation in flight.  No per-pose copy of the points exists anywhere.
//   k_select_pose   one workgroup: arg-max of (inliers - conflicts, inliers, -h) over the lattice's records, the result record's head,
//                   and the state record the alignment's iterations start from (align.hip, nvbx_align.h).
// nvbx_relocalize_*: tables (host, nvbx_relocalize_math.h) -> upload -> k_score_poses -> k_select_pose -> the alignment's launches ->
// k_score_poses of the refined pose, all enqueued at once.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "nvbx_align.h"
#include "nvbx_knobs.h"
#include "nvbx_query_point.h"
#include "nvbx_relocalize_math.h"

using namespace nvbx;

constexpr int SCORE_TPB = 256, SCORE_WAVES = SCORE_TPB / 64;
constexpr int64_t SCORE_MAX_CHUNKS = NVBX_KNOB_SCORE_CHUNKS_MAX;   // 1024 point chunks of a pose (gridDim.y): 262 144 points at one per lane
constexpr float Q20 = 1048576.0f;
enum { POSE_LIST = 0, POSE_LATTICE = 1, POSE_REFINED = 2 };

struct LatticeArgs { const nvbx_lattice_tables* tab; float t0[3]; int32_t ny, nz, nyaw, nspatial; };

struct ScoreArgs {
  PointSource src;
  int64_t per_lane;
  int32_t source, split;
  const float* poses;                                           // POSE_LIST: [gridDim.x][16]
  LatticeArgs lat;                                              // POSE_LATTICE
  const nvbx_relocalize_result* from;                           // POSE_REFINED: align.T_L_S, if status is NVBX_RELOC_OK
  float vs, min_weight, inlier, conflict, pose_lim;
  nvbx_pose_score* out;
};

// the lattice's pose h = sp nyaw + iw: table entries and three additions (nvbx_lattice_pose on the host)
__device__ inline void lattice_pose(const LatticeArgs& l, int32_t sp, int32_t iw, float R[9], float t[3]) {
  const int32_t iz = sp % l.nz, iy = (sp / l.nz) % l.ny, ix = sp / (l.nz * l.ny);
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = l.tab->R[iw][k];
  t[0] = l.t0[0] + l.tab->off[0][ix]; t[1] = l.t0[1] + l.tab->off[1][iy]; t[2] = l.t0[2] + l.tab->off[2][iz];
}

template <bool DEPTH>
__global__ __launch_bounds__(SCORE_TPB) void k_score_poses(DMap m, ScoreArgs a) {
  __shared__ int32_t s_cnt[SCORE_WAVES][4];
  __shared__ long long s_res[SCORE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t h = (int32_t)blockIdx.x;
  float R[9], t[3];
  bool ok = true;
  if (a.source == POSE_LATTICE) {
    const int32_t iw = h / a.lat.nspatial, sp = h - iw * a.lat.nspatial;      // yaw-major launch order
    lattice_pose(a.lat, sp, iw, R, t);
    h = sp * a.lat.nyaw + iw;
  } else {
    if (a.source == POSE_REFINED && a.from->status != NVBX_RELOC_OK) return;      // (uniform: the whole grid leaves)
    const float* T = a.source == POSE_REFINED ? a.from->align.T_L_S : a.poses + 16 * (size_t)h;
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float x = T[4 * i + j];
        ok = ok && fabsf(x) < INFINITY;
        if (i < 3) { if (j < 3) R[3 * i + j] = x; else t[i] = x; }
      }
    }
  }
  // nvbx_pose_in_range on the device: finite (a NaN fails the comparison), and inside the addressable blocks
  ok = ok && fabsf(t[0]) < a.pose_lim && fabsf(t[1]) < a.pose_lim && fabsf(t[2]) < a.pose_lim;
  nvbx_pose_score* rec = a.out + h;
  if (!ok) {                                                    // uniform
    if (blockIdx.y == 0 && tid == 0) { rec->points = -1; rec->valid = 0; rec->inliers = 0; rec->conflicts = 0; rec->abs_residual_q20 = 0; }
    return;
  }
  const uint2* pool = reinterpret_cast<const uint2*>(m.tsdf);
  const int64_t start = ((int64_t)blockIdx.y * SCORE_TPB + tid) * a.per_lane;
  QBlockCache cache;
  int32_t n_pts = 0, n_valid = 0, n_inl = 0, n_conf = 0;       // wave-uniform
  long long res = 0;
  for (int64_t j = 0; j < a.per_lane; j++) {                    // (a uniform trip count: every lane of the wavefront reaches the ballots)
    const int64_t i = start + j;
    float x[3] = {0.0f, 0.0f, 0.0f};
    const bool take = i < a.src.n && point_source_fetch<DEPTH>(a.src, i, x);
    bool valid = false;
    float d = 0.0f;
    if (take) {
      float p[3];
      apply_rt(R, t, x[0], x[1], x[2], p);
      valid = q_point<Q_TSDF, true>(m, pool, p, a.vs, a.min_weight, 0.0f, 0, &d, nullptr, &cache);
    }
    const float ad = fabsf(d);
    n_pts += __popcll(__ballot(take));
    n_valid += __popcll(__ballot(valid));
    n_inl += __popcll(__ballot(valid && ad <= a.inlier));
    n_conf += __popcll(__ballot(valid && d > a.conflict));
    if (valid) res += (long long)rintf(ad * Q20);
  }
  for (int off = 32; off >= 1; off >>= 1) res += __shfl_down(res, off);
  if (lane == 0) { s_cnt[wave][0] = n_pts; s_cnt[wave][1] = n_valid; s_cnt[wave][2] = n_inl; s_cnt[wave][3] = n_conf; s_res[wave] = res; }
  __syncthreads();
  if (tid != 0) return;
  int32_t c[4] = {0, 0, 0, 0};
  long long rs = 0;
  for (int w = 0; w < SCORE_WAVES; w++) {
    for (int k = 0; k < 4; k++) c[k] += s_cnt[w][k];
    rs += s_res[w];
  }
  if (!a.split) {
    rec->points = c[0]; rec->valid = c[1]; rec->inliers = c[2]; rec->conflicts = c[3]; rec->abs_residual_q20 = rs;
  } else {
    if (c[0]) atomicAdd(&rec->points, c[0]);
    if (c[1]) atomicAdd(&rec->valid, c[1]);
    if (c[2]) atomicAdd(&rec->inliers, c[2]);
    if (c[3]) atomicAdd(&rec->conflicts, c[3]);
    if (rs) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->abs_residual_q20), (unsigned long long)rs);
  }
}

struct SelectArgs {
  const nvbx_pose_score* scores; int32_t n_poses, min_inliers;
  LatticeArgs lat;
  nvbx_relocalize_result* res; AlignState* st;
};
constexpr int SELECT_TPB = 256;

// (key, inliers, h): a larger key wins, then more inliers, then the lower h
__device__ inline bool select_better(int32_t ka, int32_t ia, int32_t ha, int32_t kb, int32_t ib, int32_t hb) {
  return ka != kb ? ka > kb : ia != ib ? ia > ib : ha < hb;
}

__global__ __launch_bounds__(SELECT_TPB) void k_select_pose(SelectArgs a) {
  __shared__ int32_t s_key[SELECT_TPB], s_inl[SELECT_TPB], s_h[SELECT_TPB];
  const int tid = threadIdx.x;
  uint32_t* words = reinterpret_cast<uint32_t*>(a.res);
  for (int i = tid; i < (int)(sizeof(nvbx_relocalize_result) / 4); i += SELECT_TPB) words[i] = 0;
  int32_t bk = INT32_MIN, bi = INT32_MIN, bh = INT32_MAX;       // (loses against every record)
  for (int32_t h = tid; h < a.n_poses; h += SELECT_TPB) {
    const int32_t inl = a.scores[h].inliers, key = inl - a.scores[h].conflicts;
    if (select_better(key, inl, h, bk, bi, bh)) { bk = key; bi = inl; bh = h; }
  }
  s_key[tid] = bk; s_inl[tid] = bi; s_h[tid] = bh;
  __syncthreads();
  for (int off = SELECT_TPB / 2; off >= 1; off >>= 1) {
    if (tid < off && select_better(s_key[tid + off], s_inl[tid + off], s_h[tid + off], s_key[tid], s_inl[tid], s_h[tid])) {
      s_key[tid] = s_key[tid + off]; s_inl[tid] = s_inl[tid + off]; s_h[tid] = s_h[tid + off];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const int32_t h = s_h[0];                                     // (n_poses >= 1: a record was seen)
  float R[9], t[3];
  lattice_pose(a.lat, h / a.lat.nyaw, h % a.lat.nyaw, R, t);
  nvbx_relocalize_result* o = a.res;
  const bool found = s_inl[0] >= a.min_inliers;
  o->status = found ? NVBX_RELOC_OK : NVBX_RELOC_NO_CANDIDATE;
  o->best_index = h;
  o->coarse = a.scores[h];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) o->T_coarse[4 * i + j] = R[3 * i + j];
    o->T_coarse[4 * i + 3] = t[i];
  }
  o->T_coarse[15] = 1.0f;
  for (int k = 0; k < 9; k++) a.st->R[k] = (double)R[k];
  for (int k = 0; k < 3; k++) a.st->t[k] = (double)t[k];
  a.st->status = found ? 0 : NVBX_ALIGN_TOO_FEW;                // (not 0: the alignment's launches return at once and write nothing)
  a.st->iterations = 0;
}

// ------------------------------------------------------------------------------------------------ C-ABI
namespace {

struct ScoreOptions { float min_weight, inlier, conflict, max_d; int32_t s; };

int score_options_check(const char* who, const nvbx_mapper* m, const nvbx_score_options* options, ScoreOptions* o) {
  nvbx_score_options in;
  if (options) in = *options; else nvbx_default_score_options(&in);
  if (std::isnan(in.min_weight) || std::isnan(in.inlier_distance_m) || std::isnan(in.conflict_distance_m) || std::isnan(in.max_depth_m))
    return refuse(who, ": min_weight / inlier_distance_m / conflict_distance_m / max_depth_m is not a number");
  if (in.subsampling < 1) return refuse(who, ": subsampling must be >= 1");
  o->min_weight = in.min_weight > 0.0f ? in.min_weight : 1e-4f;
  o->inlier = in.inlier_distance_m > 0.0f ? in.inlier_distance_m : m->p.voxel_size;
  o->conflict = in.conflict_distance_m > 0.0f ? in.conflict_distance_m : 0.5f * (m->p.truncation_distance_vox * m->p.voxel_size);
  o->max_d = in.max_depth_m; o->s = in.subsampling;
  return NVBX_OK;
}

// One launch over n_poses poses; the arguments have been checked, the mapper's stream is ready.  Chunks: a workgroup per 256 points, one point per
// lane, for every pose count -- measured faster than one workgroup per pose even where the poses alone fill the device (DESIGN.md 2.20,
// EXPERIMENTS.md); beyond SCORE_MAX_CHUNKS x 256 points the lanes take runs of consecutive points.  (A/B, tools/relocalize_bench.py:
// NVBX_SCORE_CHUNKS = c forces c chunks where the points allow, 1 = one workgroup per pose; nvbx_mapper_reload_knobs lets one process measure both.)
int score_launch(nvbx_mapper* m, ScoreArgs a, const ScoreOptions& o, int64_t n_poses, bool records_are_zero) {
  const int forced = m->knobs.score_chunks;      // (0: unset, malformed or out of range)
  const int64_t full = std::max<int64_t>((a.src.n + SCORE_TPB - 1) / SCORE_TPB, 1);
  const int64_t chunks_wanted = forced > 0 ? forced : SCORE_MAX_CHUNKS;
  int64_t chunks = std::min(std::min(chunks_wanted, full), SCORE_MAX_CHUNKS);
  a.per_lane = (a.src.n + SCORE_TPB * chunks - 1) / (SCORE_TPB * chunks);
  if (a.per_lane > 0) chunks = (a.src.n + SCORE_TPB * a.per_lane - 1) / (SCORE_TPB * a.per_lane);      // (no empty chunk)
  a.split = chunks > 1;
  a.vs = m->p.voxel_size; a.min_weight = o.min_weight; a.inlier = o.inlier; a.conflict = o.conflict;
  a.pose_lim = nvbx_pose_limit(m->p.voxel_size * 8.0f, 0.0f);
  if (a.split && !records_are_zero) NVBX_HIP(hipMemsetAsync(a.out, 0, sizeof(nvbx_pose_score) * (size_t)n_poses, m->stream));
  const dim3 grid((unsigned)n_poses, (unsigned)chunks);
  if (a.src.depth) NVBX_LAUNCH(m, k_score_poses<true>, grid, dim3(SCORE_TPB), m->d, a);
  else NVBX_LAUNCH(m, k_score_poses<false>, grid, dim3(SCORE_TPB), m->d, a);
  return NVBX_OK;
}

int score_run(const char* who, nvbx_mapper* m, const float* pts, int64_t n, const float* depth, int32_t rows, int32_t cols, const nvbx_camera* cam,
              const float* poses, int32_t n_poses, const nvbx_score_options* options, nvbx_pose_score* scores) {
  if (!m) return NVBX_E_INVALID;
  if (tsdf_reader_refused(m, who)) return NVBX_E_INVALID;
  if (n_poses < 0) return refuse(who, ": n_poses must be >= 0");
  if (n_poses > 0 && (!poses || !scores)) return refuse(who, ": the poses and scores_dev are required with n_poses > 0");
  if ((uintptr_t)scores & 7) return refuse(who, ": scores_dev must be 8-byte aligned");
  ScoreOptions o;
  ScoreArgs a{};
  if (score_options_check(who, m, options, &o) || point_source_check(who, pts, n, depth, rows, cols, cam, o.s, o.max_d, &a.src)) return NVBX_E_INVALID;
  if (n_poses == 0) return NVBX_OK;
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;      // TSDF voxels and flags only: held-back colour and ESDF work stays held back (query.hip)
  a.source = POSE_LIST; a.poses = poses; a.out = scores;
  if (score_launch(m, a, o, n_poses, false)) return NVBX_E_DEVICE;
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

int relocalize_run(const char* who, nvbx_mapper* m, const float* pts, int64_t n, const float* depth, int32_t rows, int32_t cols, const nvbx_camera* cam,
                   const float T0[16], const nvbx_search_lattice* lattice, const nvbx_score_options* score_options, int32_t min_inliers,
                   const nvbx_align_options* align_options, nvbx_pose_score* scores, nvbx_relocalize_result* res, bool check_only = false) {
  if (!m) return NVBX_E_INVALID;
  if (tsdf_reader_refused(m, who)) return NVBX_E_INVALID;
  if (!T0 || !lattice || !res) return refuse(who, ": T0, the lattice and result_dev are required");
  if (((uintptr_t)res & 7) || ((uintptr_t)scores & 7)) return refuse(who, ": result_dev and scores_dev must be 8-byte aligned");
  if (!nvbx_lattice_ok(lattice)) return refuse(who, ": lattice steps must be 1 .. 64 with a product <= 2^20, the half-extents finite and >= 0");
  if (!nvbx_pose_in_range(T0, m->p.voxel_size * 8.0f, 0.0f)) return refuse(who, ": T0 is not finite or out of range");
  ScoreOptions o;
  ScoreArgs a{};
  if (score_options_check(who, m, score_options, &o) || point_source_check(who, pts, n, depth, rows, cols, cam, o.s, o.max_d, &a.src)) return NVBX_E_INVALID;
  AlignArgs al;
  const int rc = align_check_from_state(who, m, pts, n, depth, rows, cols, cam, align_options, &res->align, al);
  if (rc || check_only) return rc;
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;
  // buffers first: a growth waits for the stream
  const int64_t K = nvbx_lattice_count(lattice);
  constexpr size_t TAB_BYTES = (sizeof(nvbx_lattice_tables) + 255) / 256 * 256;
  if (m->reloc_buf.ensure(m->stream, TAB_BYTES + (scores ? 0 : sizeof(nvbx_pose_score) * (size_t)K))) return NVBX_E_DEVICE;
  if (align_buffers(m, al)) return NVBX_E_DEVICE;
  // the tables: made here, uploaded from memory that outlives the call
  m->reloc_host.resize(sizeof(nvbx_lattice_tables) / sizeof(float));
  nvbx_lattice_tables* tab_host = reinterpret_cast<nvbx_lattice_tables*>(m->reloc_host.data());
  nvbx_lattice_make_tables(T0, lattice, tab_host);
  NVBX_HIP(hipMemcpyAsync(m->reloc_buf.p, tab_host, sizeof(nvbx_lattice_tables), hipMemcpyHostToDevice, m->stream));
  LatticeArgs lat{};
  lat.tab = m->reloc_buf.as<nvbx_lattice_tables>();
  for (int i = 0; i < 3; i++) lat.t0[i] = T0[4 * i + 3];
  lat.ny = lattice->steps[1]; lat.nz = lattice->steps[2]; lat.nyaw = lattice->steps[3];
  lat.nspatial = lattice->steps[0] * lattice->steps[1] * lattice->steps[2];
  nvbx_pose_score* rec = scores ? scores : reinterpret_cast<nvbx_pose_score*>(m->reloc_buf.as<unsigned char>() + TAB_BYTES);
  // 1: the lattice
  ScoreArgs sa = a;
  sa.source = POSE_LATTICE; sa.lat = lat; sa.out = rec;
  if (score_launch(m, sa, o, K, false)) return NVBX_E_DEVICE;
  // 2: the selection; it zeroes the result record and leaves the state the iterations start from
  SelectArgs se{};
  se.scores = rec; se.n_poses = (int32_t)K; se.min_inliers = min_inliers > 0 ? min_inliers : 50; se.lat = lat; se.res = res; se.st = al.st;
  NVBX_LAUNCH(m, k_select_pose, dim3(1), dim3(SELECT_TPB), se);
  // 3: the alignment's iterations
  if (align_launch(m, al)) return NVBX_E_DEVICE;
  // 4: the refined pose's record (zeroed by the selection)
  ScoreArgs sr = a;
  sr.source = POSE_REFINED; sr.from = res; sr.out = &res->refined;
  if (score_launch(m, sr, o, 1, true)) return NVBX_E_DEVICE;
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

}  // namespace

// nvbx_relocalize_map (surface.hip, described in nvbx_align.h)
int nvbx::relocalize_points_call(const char* who, nvbx_mapper* m, const float* pts, int64_t n, const float T0[16], const nvbx_search_lattice* lattice,
                                 const nvbx_score_options* score_options, int32_t min_inliers, const nvbx_align_options* align_options, nvbx_pose_score* scores,
                                 nvbx_relocalize_result* res, bool check_only) {
  return relocalize_run(who, m, pts, n, nullptr, 0, 0, nullptr, T0, lattice, score_options, min_inliers, align_options, scores, res, check_only);
}

extern "C" void nvbx_default_score_options(nvbx_score_options* o) {
  if (!o) return;
  o->min_weight = 0.0f; o->inlier_distance_m = 0.0f; o->conflict_distance_m = 0.0f; o->max_depth_m = 0.0f; o->subsampling = 4;
}

extern "C" int nvbx_score_poses_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const float* T_L_S_dev, int32_t n_poses,
                                       const nvbx_score_options* options, nvbx_pose_score* scores_dev) {
  return score_run("nvbx_score_poses_points", m, points_xyz_dev, n, nullptr, 0, 0, nullptr, T_L_S_dev, n_poses, options, scores_dev);
}

extern "C" int nvbx_score_poses_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const nvbx_camera* camera, const float* T_L_C_dev,
                                      int32_t n_poses, const nvbx_score_options* options, nvbx_pose_score* scores_dev) {
  if (depth_entry_refused("nvbx_score_poses_depth", m, depth_dev, camera)) return NVBX_E_INVALID;
  return score_run("nvbx_score_poses_depth", m, nullptr, 0, depth_dev, rows, cols, camera, T_L_C_dev, n_poses, options, scores_dev);
}

extern "C" int nvbx_search_lattice_poses(const float T0[16], const nvbx_search_lattice* lattice, float* T_out_host) {
  const char* who = "nvbx_search_lattice_poses";
  if (!T0 || !lattice || !T_out_host) return refuse(who, ": T0, the lattice and the output are required");
  if (!nvbx_lattice_ok(lattice)) return refuse(who, ": lattice steps must be 1 .. 64 with a product <= 2^20, the half-extents finite and >= 0");
  for (int i = 0; i < 16; i++) if (!std::isfinite(T0[i])) return refuse(who, ": T0 is not finite");
  nvbx_lattice_tables tab;
  nvbx_lattice_make_tables(T0, lattice, &tab);
  const int64_t K = nvbx_lattice_count(lattice);
  for (int64_t h = 0; h < K; h++) nvbx_lattice_pose(T0, lattice, &tab, h, T_out_host + 16 * h);
  return (int)K;
}

extern "C" int nvbx_relocalize_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const float T0[16], const nvbx_search_lattice* lattice,
                                      const nvbx_score_options* score_options, int32_t min_inliers, const nvbx_align_options* align_options,
                                      nvbx_pose_score* scores_dev, nvbx_relocalize_result* result_dev) {
  return relocalize_run("nvbx_relocalize_points", m, points_xyz_dev, n, nullptr, 0, 0, nullptr, T0, lattice, score_options, min_inliers, align_options,
                        scores_dev, result_dev);
}

extern "C" int nvbx_relocalize_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const nvbx_camera* camera, const float T0[16],
                                     const nvbx_search_lattice* lattice, const nvbx_score_options* score_options, int32_t min_inliers,
                                     const nvbx_align_options* align_options, nvbx_pose_score* scores_dev, nvbx_relocalize_result* result_dev) {
  if (depth_entry_refused("nvbx_relocalize_depth", m, depth_dev, camera)) return NVBX_E_INVALID;
  return relocalize_run("nvbx_relocalize_depth", m, nullptr, 0, depth_dev, rows, cols, camera, T0, lattice, score_options, min_inliers, align_options,
                        scores_dev, result_dev);
}
