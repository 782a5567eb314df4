// bayer_region.h — what the host paths stage of a Bayer message (host_api.hip); plain C++, no HIP (tests/test_bayer_abi.py builds it
// with the host compiler).
#pragma once
#include <algorithm>

// A Bayer window is staged with what its demosaic reads: the window and its one-pixel apron, clamped to the message (or pane) — where
// the apron is cut the region's edge IS the message's edge, so k_bayer_to_mono on the region gives debayer-then-crop of the whole
// message.  A window's pixel in the message's frame copies column (row) 1 or width - 2, whose own neighbours the region holds too:
// a window ONE pixel wide in the frame therefore stages three columns, one more than "window + apron".
struct BayerRegion { int ax, ay, rw, rh; };   // the region's origin in the message and its size: 3 <= rw <= W + 2, 3 <= rh <= H + 2
// the window W x H at (x0, y0) of a width x height message, width, height >= 3
inline BayerRegion bayer_region(int width, int height, int x0, int y0, int W, int H) {
  const auto in = [](int v, int n) { return std::min(std::max(v, 1), n - 2); };
  const int ax = in(x0, width) - 1, ay = in(y0, height) - 1;
  return {ax, ay, in(x0 + W - 1, width) + 2 - ax, in(y0 + H - 1, height) + 2 - ay};
}
