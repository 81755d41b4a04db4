// feature_merge_math_check.cpp -- stand-alone host program over csrc/nvbx_feature_merge_math.h (tests/test_feature_merge_math.py drives it; also
// built with -fsanitize=address,undefined).  Reads commands from stdin, one per line, numbers as C hex floats; answers one line per command.
//   fbox <voxel size> <T x 16> <s x 3>    ->  fbox <ok> <lo x 3> <hi x 3>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nvbx_feature_merge_math.h"

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
    if (!strcmp(cmd, "fbox")) {
      float in[17], R_DS[9], t_DS[3], R_SD[9], t_SD[3];
      if (!read_floats(p, in, 17)) { fprintf(stderr, "bad fbox line\n"); return 2; }
      int32_t s[3], lo[3], hi[3];
      for (int a = 0; a < 3; a++) { char* end = nullptr; s[a] = (int32_t)strtol(p, &end, 10); if (end == p) { fprintf(stderr, "bad fbox index\n"); return 2; } p = end; }
      nvbx_merge_transforms(in + 1, R_DS, t_DS, R_SD, t_SD);
      const int ok = nvbx_feature_merge_candidate_box(R_DS, t_DS, s, in[0], lo, hi);
      printf("fbox %d %d %d %d %d %d %d\n", ok, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  return 0;
}
