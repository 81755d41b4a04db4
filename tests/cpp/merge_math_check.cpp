// merge_math_check.cpp -- stand-alone host program over csrc/nvbx_merge_math.h (tests/test_merge_math.py drives it; also built with
// -fsanitize=address,undefined).  Reads commands from stdin, one per line, numbers as C hex floats; answers one line per command.
//   rot <T x 16>                          ->  rot <ok> <largest |R^T R - I|> <det>
//   inv <T x 16>                          ->  inv <R_DS x 9> <t_DS x 3> <R_SD x 9> <t_SD x 3>
//   box <voxel size> <T x 16> <s x 3>     ->  box <ok> <lo x 3> <hi x 3>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nvbx_merge_math.h"

static bool read_floats(char*& p, float* out, int n) {
  for (int i = 0; i < n; i++) {
    char* end = nullptr;
    out[i] = strtof(p, &end);
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
    if (!strcmp(cmd, "rot")) {
      float T[16]; double err = 0.0, det = 0.0;
      if (!read_floats(p, T, 16)) { fprintf(stderr, "bad rot line\n"); return 2; }
      const int ok = nvbx_merge_rotation_ok(T, &err, &det);
      printf("rot %d %a %a\n", ok, err, det);
    } else if (!strcmp(cmd, "inv")) {
      float T[16], R_DS[9], t_DS[3], R_SD[9], t_SD[3];
      if (!read_floats(p, T, 16)) { fprintf(stderr, "bad inv line\n"); return 2; }
      nvbx_merge_transforms(T, R_DS, t_DS, R_SD, t_SD);
      printf("inv");
      for (int i = 0; i < 9; i++) printf(" %a", (double)R_DS[i]);
      for (int i = 0; i < 3; i++) printf(" %a", (double)t_DS[i]);
      for (int i = 0; i < 9; i++) printf(" %a", (double)R_SD[i]);
      for (int i = 0; i < 3; i++) printf(" %a", (double)t_SD[i]);
      printf("\n");
    } else if (!strcmp(cmd, "box")) {
      float in[17], R_DS[9], t_DS[3], R_SD[9], t_SD[3];
      if (!read_floats(p, in, 17)) { fprintf(stderr, "bad box line\n"); return 2; }
      int32_t s[3], lo[3], hi[3];
      for (int a = 0; a < 3; a++) { char* end = nullptr; s[a] = (int32_t)strtol(p, &end, 10); if (end == p) { fprintf(stderr, "bad box index\n"); return 2; } p = end; }
      nvbx_merge_transforms(in + 1, R_DS, t_DS, R_SD, t_SD);
      const int ok = nvbx_merge_candidate_box(R_DS, t_DS, s, in[0], lo, hi);
      printf("box %d %d %d %d %d %d %d\n", ok, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  return 0;
}
