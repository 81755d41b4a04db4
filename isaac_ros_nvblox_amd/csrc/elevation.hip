// elevation.hip -- how high the ground is, whether the robot can stand there and how far the next place is where it cannot (SEMANTICS.md
// "Elevation and traversability"): nvbx_elevation_map scans the TSDF columns of a z band into a height and a status image that
// lie pixel for pixel on the slice image's grid, nvbx_traversability turns such a pair into classes, step, squared slope and the distance to
// the nearest hazard, in the form nvbx_cost_field reads.  Both read only; the voxel test, the gradient selection and the classes are
// nvbx_terrain_math.h's, shared with the host.  No workgroup waits for another, every loop is bounded.
// k_elevation_scan: column-centric.  A wavefront per 8 x 8 block column that meets the image, lane = (vy, vx); four block columns adjacent in x
//   per workgroup.  The lanes first resolve the column's blocks of the band, one find_slot each (up to 64 at a time: one probe latency for the
//   whole column), then the wavefront walks the blocks from the band's top downwards with the slot broadcast: a lane's eight z voxels are 64
//   contiguous bytes, four float4 loads, the wavefront reads the 4 KiB block in four instructions.  Each lane carries {observed, d} of the voxel
//   above in registers, also across the block boundary; a missing block is all-unobserved and costs nothing but its probe.  The wavefront stops
//   when a ballot says every lane has found its topmost solid voxel.  The four wavefronts hand their 8 x 8 results through 1.3 KB of LDS, so that
//   the workgroup stores rows of 32 pixels (128 B of heights) instead of 8.
// k_terrain_classify: a wavefront per 64 consecutive columns of a row: the 3 x 3 stencil from global memory (the nine reads of neighbouring lanes
//   and rows hit the L1 / L2), class, step and slope2 out, and the HAZARD flags of the wavefront as ONE ballot word into the mapper's scratch: one
//   bit row of ceil(cols / 64) words per image row, every word written in full.
// k_terrain_distance: the same lanes.  For |dr| = 0, 1, .. R a lane reads the three words around its column of rows r - |dr| and r + |dr| (the
//   same three for the whole wavefront), shifts them into "hazards at c, c + 1, .." and "hazards at c, c - 1, ..", and takes the nearest set bit
//   of each with a count of trailing / leading zeros; it stops once dr * dr reaches the best sum so far.  At most 65 rows x 3 words per pixel.
#include <algorithm>
#include <cmath>
#include "nvbx_mapper.h"
#include "nvbx_terrain_math.h"

using namespace nvbx;

constexpr int EL_TPB = 256;               // four wavefronts
constexpr int EL_BX = EL_TPB / 64;        // block columns along x per workgroup

struct ElevArgs {
  int32_t x0, y0, rows, cols, z_lo, z_hi;
  float min_weight, unknown_value, vs;
  float* height; uint8_t* status;
  int32_t bx0, by0, ngx;                  // first block column of the image, workgroups along x
};

__global__ __launch_bounds__(EL_TPB) void k_elevation_scan(DMap m, ElevArgs a) {
  __shared__ float s_h[8][8 * EL_BX];
  __shared__ uint8_t s_s[8][8 * EL_BX];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, vx = lane & 7, vy = lane >> 3;
  const int32_t wy = (int32_t)blockIdx.x / a.ngx, wx = (int32_t)blockIdx.x - wy * a.ngx;
  const int32_t bx = a.bx0 + wx * EL_BX + wave, by = a.by0 + wy;
  const int32_t c = 8 * bx + vx - a.x0, r = 8 * by + vy - a.y0;
  const bool inside = r >= 0 && c >= 0 && r < a.rows && c < a.cols;
  const int32_t hb = a.z_hi >> 3, nblk = hb - (a.z_lo >> 3) + 1;      // at most (z_hi - z_lo) / 8 + 2 blocks
  bool done = !inside, any_obs = false, up_obs = false;               // up_*: the voxel above the one looked at, if it lies in the band
  float up_d = 0.0f, h = a.unknown_value;
  int status = -1;
  bool more = __ballot(!done) != 0ull;                                // (a wavefront past the image's last block column probes nothing)
  for (int32_t base = 0; base < nblk && more; base += 64) {
    uint32_t mine = SLOT_NONE;
    if (base + lane < nblk) mine = find_slot(m, bx, by, hb - base - lane, F_TSDF);
    const int n = min(64, nblk - base);
    for (int i = 0; i < n && more; i++) {
      const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)mine, i));
      const int32_t bz = hb - base - i;
      if (!slot_ok(slot)) { up_obs = false; continue; }               // uniform: all eight voxels unobserved
      const float4* col = reinterpret_cast<const float4*>(&m.tsdf[(size_t)slot * 512 + 64 * vx + 8 * vy]);
      float d[8], w[8];
#pragma unroll
      for (int q = 0; q < 4; q++) { const float4 v = col[q]; d[2 * q] = v.x; w[2 * q] = v.y; d[2 * q + 1] = v.z; w[2 * q + 1] = v.w; }
#pragma unroll
      for (int z = 7; z >= 0; z--) {
        const int32_t gz = 8 * bz + z;
        if (gz > a.z_hi || gz < a.z_lo) continue;                     // uniform
        const bool obs = nvbx_elev_observed(d[z], w[z], a.min_weight);
        any_obs |= obs;
        if (!done && obs && d[z] <= 0.0f) {                           // the topmost solid voxel of the band
          done = true;
          status = up_obs ? NVBX_ELEV_SURFACE : NVBX_ELEV_BLOCKED;
          if (up_obs) h = voxel_center(bz, z, a.vs * 8.0f, a.vs) + a.vs * NVBX_DIV(-d[z], up_d - d[z]);
        }
        up_obs = obs; up_d = d[z];
      }
      more = __ballot(!done) != 0ull;
    }
  }
  if (status < 0) status = any_obs ? NVBX_ELEV_VOID : NVBX_ELEV_UNKNOWN;
  s_h[vy][8 * wave + vx] = h; s_s[vy][8 * wave + vx] = (uint8_t)status;
  __syncthreads();
  const int ly = t >> 5, lx = t & 31;                                 // a row of 32 pixels per half wavefront
  const int32_t orow = 8 * by + ly - a.y0, ocol = 8 * (a.bx0 + wx * EL_BX) + lx - a.x0;
  if (orow >= 0 && ocol >= 0 && orow < a.rows && ocol < a.cols) {
    const int64_t g = (int64_t)orow * a.cols + ocol;
    a.height[g] = s_h[ly][lx]; a.status[g] = s_s[ly][lx];
  }
}

struct TerrainArgs {
  const float* h; const uint8_t* st; int32_t rows, cols, words;      // words: 64-bit words per bit row
  nvbx_terrain_options o; float vs;
  uint8_t* cls; float* step; float* slope2; float* dist;
  u64* bits;                                                          // [rows][words] HAZARD flags; NULL: no distance wanted
};

__global__ __launch_bounds__(EL_TPB) void k_terrain_classify(TerrainArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * (EL_TPB / 64) + (threadIdx.x >> 6);
  if (wid >= (int64_t)a.rows * a.words) return;                       // uniform
  const int32_t r = (int32_t)(wid / a.words), cw = (int32_t)(wid - (int64_t)r * a.words), c = cw * 64 + lane;
  bool hazard = false;
  if (c < a.cols) {
    const int64_t g = (int64_t)r * a.cols + c;
    const uint8_t s = a.st[g];
    float step = 0.0f, slope2 = 0.0f;
    int n_known = 0;
    if (s == NVBX_ELEV_SURFACE) {
      const float h = a.h[g];
      bool k[3][3]; float q[3][3];
#pragma unroll
      for (int dr = -1; dr <= 1; dr++)
#pragma unroll
        for (int dc = -1; dc <= 1; dc++) {
          const int32_t rr = r + dr, cc = c + dc;
          const bool in = rr >= 0 && cc >= 0 && rr < a.rows && cc < a.cols;
          const bool kn = in && a.st[in ? (int64_t)rr * a.cols + cc : g] == NVBX_ELEV_SURFACE;
          k[dr + 1][dc + 1] = kn; q[dr + 1][dc + 1] = kn ? a.h[(int64_t)rr * a.cols + cc] : 0.0f;
          n_known += kn;
          if (kn && (dr || dc)) { const float v = fabsf(h - q[dr + 1][dc + 1]); if (v > step) step = v; }
        }
      const float gx = nvbx_terrain_grad(k[1][0], k[1][2], q[1][0], h, q[1][2], a.vs);
      const float gy = nvbx_terrain_grad(k[0][1], k[2][1], q[0][1], h, q[2][1], a.vs);
      slope2 = gx * gx + gy * gy;
    }
    const uint8_t cl = nvbx_terrain_class(s, step, slope2, n_known, &a.o);
    a.cls[g] = cl;
    if (a.step) a.step[g] = step;
    if (a.slope2) a.slope2[g] = slope2;
    hazard = cl == NVBX_TERRAIN_HAZARD;
  }
  const u64 mask = __ballot(hazard);
  if (a.bits && lane == 0) a.bits[(int64_t)r * a.words + cw] = mask;
}

__global__ __launch_bounds__(EL_TPB) void k_terrain_distance(TerrainArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * (EL_TPB / 64) + (threadIdx.x >> 6);
  if (wid >= (int64_t)a.rows * a.words) return;
  const int32_t r = (int32_t)(wid / a.words), cw = (int32_t)(wid - (int64_t)r * a.words), c = cw * 64 + lane;
  if (c >= a.cols) return;
  const int64_t g = (int64_t)r * a.cols + c;
  const uint8_t cl = a.cls[g];
  float out = 0.0f;
  if (cl == NVBX_TERRAIN_UNKNOWN) out = a.o.unknown_value;
  else if (cl == NVBX_TERRAIN_OK) {
    const int32_t R = a.o.distance_radius_px, R2 = R * R;
    int32_t best = R2 + 1;                                            // the least dr * dr + dc * dc so far; R2 + 1: none within the radius
    for (int32_t k = 0; k <= R && k * k < best; k++) {                // rows r - k and r + k
      for (int side = 0; side < (k ? 2 : 1); side++) {
        const int32_t rr = side ? r + k : r - k;
        if (rr < 0 || rr >= a.rows) continue;
        const u64* row = a.bits + (int64_t)rr * a.words;
        const u64 w0 = row[cw], wl = cw > 0 ? row[cw - 1] : 0ull, wr = cw + 1 < a.words ? row[cw + 1] : 0ull;
        const u64 right = (w0 >> lane) | (lane ? wr << (64 - lane) : 0ull);          // bit i: a hazard at column c + i
        const u64 left = (w0 << (63 - lane)) | (lane < 63 ? wl >> (lane + 1) : 0ull);  // bit 63 - i: a hazard at column c - i
        const int32_t dr_ = right ? __builtin_ctzll(right) : 64, dl = left ? __builtin_clzll(left) : 64;
        const int32_t dc = min(dr_, dl);
        if (dc < 64) best = min(best, k * k + dc * dc);               // (a sum above R2 is above `best` too: never taken)
      }
    }
    out = best <= R2 ? a.vs * NVBX_SQRT((float)best) : a.vs * (float)(R + 1);
  }
  a.dist[g] = out;
}

// ------------------------------------------------------------------------------------------------ C-ABI
namespace {

int image_size_refused(const char* who, int32_t rows, int32_t cols) {
  if (rows <= 0 || cols <= 0 || (int64_t)rows * cols > NVBX_ELEV_MAX_PIXELS) return refuse(who, ": rows and cols must be > 0 and rows x cols <= 2^22");
  return NVBX_OK;
}

}  // namespace

extern "C" void nvbx_default_terrain_options(nvbx_terrain_options* o) {
  if (!o) return;
  o->max_step_m = 0.10f; o->max_slope_tan = 0.5f; o->unknown_value = 1000.0f;
  o->min_known = 5; o->void_is_hazard = 0; o->distance_radius_px = 15; o->pad[0] = 0; o->pad[1] = 0;
}

extern "C" int nvbx_elevation_map(nvbx_mapper* m, int32_t x0, int32_t y0, int32_t rows, int32_t cols, int32_t z_lo, int32_t z_hi, float min_weight,
                                  float unknown_value, float* height_dev, uint8_t* status_dev) {
  const char* who = "nvbx_elevation_map";
  if (!m) return refuse(who, ": the mapper is NULL");
  if (!height_dev || !status_dev) return refuse(who, ": height_dev and status_dev are required");
  if (tsdf_reader_refused(m, who)) return NVBX_E_INVALID;
  if (image_size_refused(who, rows, cols)) return NVBX_E_INVALID;
  if (z_hi < z_lo || (int64_t)z_hi - z_lo >= NVBX_ELEV_MAX_BAND) return refuse(who, ": the band must have z_lo <= z_hi and z_hi - z_lo < 1024");
  const int64_t L = NVBX_ELEV_VOXEL_LIMIT;
  if (x0 < -L || y0 < -L || z_lo < -L || (int64_t)x0 + cols > L || (int64_t)y0 + rows > L || z_hi >= L)
    return refuse(who, ": the box leaves the addressable voxels [-2^23, 2^23)");
  if (std::isnan(min_weight) || std::isnan(unknown_value)) return refuse(who, ": min_weight / unknown_value is not a number");
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;      // TSDF voxels and flags only: everything held back stays held back
  ElevArgs a{};
  a.x0 = x0; a.y0 = y0; a.rows = rows; a.cols = cols; a.z_lo = z_lo; a.z_hi = z_hi;
  a.min_weight = min_weight; a.unknown_value = unknown_value; a.vs = m->p.voxel_size; a.height = height_dev; a.status = status_dev;
  a.bx0 = x0 >> 3; a.by0 = y0 >> 3;
  const int32_t nbx = ((x0 + cols - 1) >> 3) - a.bx0 + 1, nby = ((y0 + rows - 1) >> 3) - a.by0 + 1;
  a.ngx = (nbx + EL_BX - 1) / EL_BX;
  NVBX_LAUNCH(m, k_elevation_scan, dim3((unsigned)((int64_t)a.ngx * nby)), dim3(EL_TPB), m->d, a);      // at most 2^19 + 1 workgroups
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}

extern "C" int nvbx_traversability(nvbx_mapper* m, const float* height_dev, const uint8_t* status_dev, int32_t rows, int32_t cols,
                                   const nvbx_terrain_options* options, uint8_t* class_dev, float* step_dev, float* slope2_dev, float* distance_dev) {
  const char* who = "nvbx_traversability";
  if (!m) return refuse(who, ": the mapper is NULL");
  if (!height_dev || !status_dev || !options || !class_dev) return refuse(who, ": height_dev, status_dev, options and class_dev are required");
  if (image_size_refused(who, rows, cols)) return NVBX_E_INVALID;
  if (const char* why = nvbx_terrain_options_problem(options)) return refuse(who, why);
  NVBX_HIP(hipSetDevice(m->device));
  if (m->begin_call_keeping_held()) return NVBX_E_DEVICE;      // the two images only: everything held back stays held back
  TerrainArgs a{};
  a.h = height_dev; a.st = status_dev; a.rows = rows; a.cols = cols; a.words = (cols + 63) / 64;
  a.o = *options; a.vs = m->p.voxel_size; a.cls = class_dev; a.step = step_dev; a.slope2 = slope2_dev; a.dist = distance_dev;
  const int64_t waves = (int64_t)rows * a.words;               // at most 2^22: one per 64 columns of a row
  if (distance_dev) {
    if (m->terrain_scratch.ensure(m->stream, (size_t)waves * sizeof(u64))) return NVBX_E_DEVICE;      // (grows with the largest image so far)
    a.bits = m->terrain_scratch.as<u64>();
  }
  const dim3 grid((unsigned)((waves + EL_TPB / 64 - 1) / (EL_TPB / 64)));
  NVBX_LAUNCH(m, k_terrain_classify, grid, dim3(EL_TPB), a);
  if (distance_dev) NVBX_LAUNCH(m, k_terrain_distance, grid, dim3(EL_TPB), a);
  NVBX_HIP(hipGetLastError());
  return NVBX_OK;
}
