// surface_math_check.cpp -- stand-alone host program over csrc/nvbx_surface_math.h (tests/test_surface_math.py drives it; also built with
// -fsanitize=address,undefined).  Reads commands from stdin, one per line, numbers as C hex floats; answers one line per command.
//   edge <d0> <w0> <d1> <w1> <min_weight>              ->  edge <observed 0> <observed 1> <crosses> <colour end>
//   pos <vs> <d0> <d1> <b> <v>                         ->  pos <centre> <crossing>
//   mod <g> <s>                                        ->  mod <g mod s>
//   keep <stride> <use_box> <box x 6> <g x 3>          ->  keep <kept>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nvbx_surface_math.h"

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
    if (!strcmp(cmd, "edge")) {
      float v[5];
      if (!read_floats(p, v, 5)) { fprintf(stderr, "bad edge line\n"); return 2; }
      printf("edge %d %d %d %d\n", nvbx_surface_observed(v[0], v[1], v[4]), nvbx_surface_observed(v[2], v[3], v[4]),
             nvbx_surface_crosses(v[0], v[1], v[2], v[3], v[4]), nvbx_surface_color_end(v[0], v[2]));
    } else if (!strcmp(cmd, "pos")) {
      float v[3]; long k[2];
      if (!read_floats(p, v, 3) || !read_ints(p, k, 2)) { fprintf(stderr, "bad pos line\n"); return 2; }
      printf("pos %a %a\n", (double)nvbx_surface_center((int32_t)k[0], (int32_t)k[1], v[0]),
             (double)nvbx_surface_crossing((int32_t)k[0], (int32_t)k[1], v[0], v[1], v[2]));
    } else if (!strcmp(cmd, "mod")) {
      long k[2];
      if (!read_ints(p, k, 2) || k[1] < 1) { fprintf(stderr, "bad mod line\n"); return 2; }
      printf("mod %d\n", nvbx_floor_mod((int32_t)k[0], (int32_t)k[1]));
    } else if (!strcmp(cmd, "keep")) {
      long k[11];
      if (!read_ints(p, k, 11) || k[0] < 1) { fprintf(stderr, "bad keep line\n"); return 2; }
      int32_t box[6];
      for (int i = 0; i < 6; i++) box[i] = (int32_t)k[2 + i];
      printf("keep %d\n", nvbx_surface_origin_kept((int32_t)k[8], (int32_t)k[9], (int32_t)k[10], (int32_t)k[0], (int32_t)k[1], box));
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  return 0;
}
