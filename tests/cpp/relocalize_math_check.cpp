// relocalize_math_check -- the host arithmetic of the search lattice (isaac_ros_nvblox_amd/csrc/nvbx_relocalize_math.h) as a stand-alone program:
// tests/test_relocalize_math.py feeds it lattices and compares what it prints, bit for bit, with numpy tables; the same source is built with
// AddressSanitizer and UBSan and run as a program.  No HIP, no GPU.
// stdin, one case per line: 16 T0 entries, 3 half-extents and the half yaw as float32 bit patterns (hex), then the 4 step counts (decimal).
// stdout per case: "0" for a refused lattice, else "1 K", a line per offset table (its steps[a] entries), a line per yaw matrix, a line per pose
// -- float32 bit patterns in hex.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "nvbx_relocalize_math.h"

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static void print_row(const float* v, int n) {
  for (int i = 0; i < n; i++) std::printf("%s%08" PRIx32, i ? " " : "", bits(v[i]));
  std::printf("\n");
}

int main() {
  for (;;) {
    uint32_t w[20];
    int got = 0;
    for (int i = 0; i < 20; i++) got += std::scanf("%" SCNx32, &w[i]) == 1;
    if (got == 0) break;
    nvbx_search_lattice l;
    if (got != 20 || std::scanf("%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32, &l.steps[0], &l.steps[1], &l.steps[2], &l.steps[3]) != 4) return 2;
    float T0[16];
    for (int i = 0; i < 16; i++) T0[i] = from_bits(w[i]);
    for (int a = 0; a < 3; a++) l.half_extent_m[a] = from_bits(w[16 + a]);
    l.half_yaw_rad = from_bits(w[19]);
    if (!nvbx_lattice_ok(&l)) { std::printf("0\n"); continue; }
    const int64_t K = nvbx_lattice_count(&l);
    std::printf("1 %" PRId64 "\n", K);
    std::vector<nvbx_lattice_tables> tab(1);
    nvbx_lattice_make_tables(T0, &l, &tab[0]);
    for (int a = 0; a < 3; a++) print_row(tab[0].off[a], l.steps[a]);
    for (int k = 0; k < l.steps[3]; k++) print_row(tab[0].R[k], 9);
    std::vector<float> T((size_t)K * 16);
    for (int64_t h = 0; h < K; h++) nvbx_lattice_pose(T0, &l, &tab[0], h, T.data() + 16 * h);
    for (int64_t h = 0; h < K; h++) print_row(T.data() + 16 * h, 16);
  }
  return 0;
}
