// resample_math_check.cpp -- stand-alone host program over csrc/nvbx_resample_math.h (tests/test_resample_math.py drives it; also built with
// -fsanitize=address,undefined).  Reads commands from stdin, one per line, numbers as C hex floats; answers one line per command.
//   ratio <vs_d> <vs_s> <taps>                         ->  ratio <ok> <r> <n> <N>      (n = 0: taps refused; N only for ok and n > 0, else 0)
//   off <n>                                            ->  off <o_0> .. <o_(n-1)>
//   box <vs_s> <vs_d> <T x 16> <n> <s x 3>             ->  box <ok> <lo x 3> <hi x 3>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nvbx_resample_math.h"

static bool read_floats(char*& p, float* out, int n) {
  for (int i = 0; i < n; i++) {
    char* end = nullptr;
    out[i] = strtof(p, &end);
    if (end == p) return false;
    p = end;
  }
  return true;
}

static bool read_ints(char*& p, long* out, int n) {
  for (int i = 0; i < n; i++) {
    char* end = nullptr;
    out[i] = strtol(p, &end, 10);
    if (end == p) return false;
    p = end;
  }
  return true;
}

int main() {
  std::vector<char> line(1 << 12);
  while (fgets(line.data(), (int)line.size(), stdin)) {
    char* p = line.data();
    char cmd[16] = {0};
    int used = 0;
    if (sscanf(p, "%15s%n", cmd, &used) != 1) continue;
    p += used;
    if (!strcmp(cmd, "ratio")) {
      float v[2]; long taps = 0;
      if (!read_floats(p, v, 2) || !read_ints(p, &taps, 1)) { fprintf(stderr, "bad ratio line\n"); return 2; }
      double r = 0.0;
      const int ok = nvbx_resample_ratio(v[0], v[1], &r);
      const int n = ok ? nvbx_resample_taps(r, (int32_t)taps) : 0;
      printf("ratio %d %a %d %d\n", ok, r, n, ok && n ? nvbx_resample_reach(r, n) : 0);
    } else if (!strcmp(cmd, "off")) {
      long n = 0;
      if (!read_ints(p, &n, 1) || n < 1 || n > NVBX_RESAMPLE_MAX_TAPS) { fprintf(stderr, "bad off line\n"); return 2; }
      printf("off");
      for (int i = 0; i < (int)n; i++) printf(" %a", (double)nvbx_resample_tap_offset(i, (int)n));
      printf("\n");
    } else if (!strcmp(cmd, "box")) {
      float in[18], R_DS[9], t_DS[3], R_SD[9], t_SD[3];
      long k[4];
      if (!read_floats(p, in, 18) || !read_ints(p, k, 4)) { fprintf(stderr, "bad box line\n"); return 2; }
      const int32_t s[3] = {(int32_t)k[1], (int32_t)k[2], (int32_t)k[3]};
      int32_t lo[3], hi[3];
      nvbx_merge_transforms(in + 2, R_DS, t_DS, R_SD, t_SD);
      const int ok = nvbx_resample_candidate_box(R_DS, t_DS, s, in[0], in[1], (int)k[0], lo, hi);
      printf("box %d %d %d %d %d %d %d\n", ok, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  return 0;
}
