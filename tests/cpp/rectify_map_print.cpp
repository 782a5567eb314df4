// The rectification map of csrc/rectify_map.h (the arithmetic k_rectify_map runs on the GPU) from a plain host build, for
// tests/test_rectify_map_host.py:  rectify_map_print model x0 y0 W H  with the calibration on stdin as 38 doubles in C99 hex
// (K 9, D 8, R 9, P 12; exact).  Prints "qx qy" for every window pixel, row by row.
// Build: g++ -std=c++17 -O2 -ffp-contract=off
#include "../../moving_object_detector_amd/csrc/rectify_map.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
  if (argc != 6) return 2;
  const int model = atoi(argv[1]), x0 = atoi(argv[2]), y0 = atoi(argv[3]), W = atoi(argv[4]), H = atoi(argv[5]);
  if (model != MOD_DISTORTION_RATIONAL && model != MOD_DISTORTION_EQUIDISTANT) return 2;
  ModRectifyCamera cam{};
  double v[38];
  char word[64];
  for (double &d : v) {
    if (scanf("%63s", word) != 1) return 3;
    d = strtod(word, nullptr);
  }
  int k = 0;
  for (double &d : cam.K) d = v[k++];
  for (double &d : cam.D) d = v[k++];
  for (double &d : cam.R) d = v[k++];
  for (double &d : cam.P) d = v[k++];
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      int32_t qx, qy;
      rectify_map::entry(model, cam, (double)(x + x0), (double)(y + y0), qx, qy);
      printf("%d %d\n", qx, qy);
    }
  return 0;
}
