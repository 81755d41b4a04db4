// align_math_check.cpp -- stand-alone host program over csrc/nvbx_align_math.h (tests/test_align_math.py drives it; also built with
// -fsanitize=address,undefined).  Reads commands from stdin, one per line, numbers as C hex floats; answers one line per command.
//   solve <damping> <min_pivot_ratio> <H x 21> <b x 6>   ->  <ok> <worst pivot ratio> <x x 6>
//   exp <w x 3>                                          ->  <R x 9> <V x 9>
//   compose <k> then k lines <xi x 6>                    ->  <R x 9> <t x 3>   (k steps applied to the identity pose)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "nvbx_align_math.h"

static bool read_doubles(char*& p, double* out, int n) {
  for (int i = 0; i < n; i++) {
    char* end = nullptr;
    out[i] = strtod(p, &end);
    if (end == p) return false;
    p = end;
  }
  return true;
}
static void print_doubles(const double* v, int n) { for (int i = 0; i < n; i++) printf(" %a", v[i]); }

int main() {
  std::vector<char> line(1 << 16);
  while (fgets(line.data(), (int)line.size(), stdin)) {
    char* p = line.data();
    char cmd[16] = {0};
    int used = 0;
    if (sscanf(p, "%15s%n", cmd, &used) != 1) continue;
    p += used;
    if (!strcmp(cmd, "solve")) {
      double in[2 + 21 + 6], x[6] = {0, 0, 0, 0, 0, 0}, worst = 0.0;
      if (!read_doubles(p, in, 29)) { fprintf(stderr, "bad solve line\n"); return 2; }
      const int ok = nvbx_align_solve6(in + 2, in + 23, in[0], in[1], x, &worst);
      printf("%d", ok); print_doubles(&worst, 1); print_doubles(x, 6); printf("\n");
    } else if (!strcmp(cmd, "exp")) {
      double w[3], R[9], V[9];
      if (!read_doubles(p, w, 3)) { fprintf(stderr, "bad exp line\n"); return 2; }
      nvbx_align_exp(w, R, V);
      printf("exp"); print_doubles(R, 9); print_doubles(V, 9); printf("\n");
    } else if (!strcmp(cmd, "compose")) {
      const long k = strtol(p, nullptr, 10);
      double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
      for (long i = 0; i < k; i++) {
        double xi[6];
        if (!fgets(line.data(), (int)line.size(), stdin)) { fprintf(stderr, "compose: missing step\n"); return 2; }
        char* q = line.data();
        if (!read_doubles(q, xi, 6)) { fprintf(stderr, "bad step line\n"); return 2; }
        nvbx_align_apply(R, t, xi);
      }
      printf("pose"); print_doubles(R, 9); print_doubles(t, 3); printf("\n");
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  return 0;
}
