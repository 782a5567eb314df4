// A ray table of csrc/depth_rays.h (the arithmetic k_depth_rays runs on the GPU) from a plain host build, for
// tests/test_depth_rays_host.py:  depth_rays_print lattice width height  with the lens on stdin as 12 doubles in C99 hex (D 8, fx, fy,
// cx, cy; exact).  Prints the bit patterns of x and y of every entry as hex words, row by row.
// Build: g++ -std=c++17 -O2 -ffp-contract=off
#include "../../moving_object_detector_amd/csrc/depth_rays.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const int lattice = atoi(argv[1]), width = atoi(argv[2]), height = atoi(argv[3]);
  if (lattice != MOD_DEPTH_RAYS_CENTRES && lattice != MOD_DEPTH_RAYS_CORNERS) return 2;
  double v[12];
  char word[64];
  for (double &d : v) {
    if (scanf("%63s", word) != 1) return 3;
    d = strtod(word, nullptr);
  }
  depth_rays::Lens lens{};
  for (int i = 0; i < 8; i++) lens.D[i] = v[i];
  lens.fx = v[8]; lens.fy = v[9]; lens.cx = v[10]; lens.cy = v[11];
  const double offset = lattice == MOD_DEPTH_RAYS_CORNERS ? -0.5 : 0.0;
  for (int j = 0; j < height + lattice; j++)
    for (int i = 0; i < width + lattice; i++) {
      double r[2];
      depth_rays::entry(lens, (double)i + offset, (double)j + offset, r[0], r[1]);
      unsigned long long b[2];
      memcpy(b, r, sizeof b);
      printf("%llx %llx\n", b[0], b[1]);
    }
  return 0;
}
