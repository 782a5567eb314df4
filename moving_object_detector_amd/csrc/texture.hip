// texture.hip — the texture measure of a grey plane and the rejection rule on it (mod_set_texture_filter, mod_texture_dev,
// mod_texture_reject_dev; include/mod_sf.h states the rule, DESIGN.md §3.4d where it sits; tests/models/texture_model.py restates it):
//   g(x, y) = min(|I(min(x + 1, W - 1), y) - I(max(x - 1, 0), y)|, cap)      T(x, y) = sum of g over the w x w window, 0 outside the image
//
// k_texture<OUT>: one workgroup (4 waves) per 64 x 16 tile, frames in grid.z, r = (w - 1) / 2 a runtime value in 1..7.
//   A  the grey tile with r + 1 halo columns and r halo rows into LDS (at most 30 rows of 80 bytes = 2400 bytes).  Rows and columns
//      are CLAMPED into the image before the load: every load is inside the plane, at W = 1 and H = 1 too, and the clamped columns are
//      exactly the rule's min / max.
//   B  the capped differences, once per tile position, as bytes in LDS; 0 where the position lies outside the image.
//   C  row sums (2 r + 1 bytes each, at most 15 * 255) as uint16 in LDS: one wave per row, one lane per column.
//   D  column sums: a lane owns one column and four rows; the first row is summed, the next three slide (+ row entering, - row leaving).
// Lanes of a wave read consecutive bytes (A, B, C) or consecutive uint16 (D) of LDS: lanes that share a dword share its bank AND its
// address, which is a broadcast, not a conflict.  The loads of A are bytes, consecutive across lanes: a row of the plane starts at
// any byte (W need not be a multiple of 4).
// OUT: kTexPlane stores T (2 bytes per pixel).  The reject forms (bit 1: disparity, bit 2: flow; both: one launch) store ONLY where
// T < threshold and read neither plane: their traffic is the grey bytes and the rejected pixels.  Plain vector stores, no atomics.
#include "mod_launch.h"

namespace {

constexpr int kTexTileW = 64, kTexTileH = 16, kTexMaxR = 7;
constexpr int kTexCols = kTexTileW + 2 * (kTexMaxR + 1);   // 80: grey columns x0 - r - 1 .. x0 + 63 + r + 1 at r = 7
constexpr int kTexRows = kTexTileH + 2 * kTexMaxR;         // 30
constexpr int kTexPlane = 0, kTexDisparity = MOD_TEXTURE_DISPARITY, kTexFlow = MOD_TEXTURE_FLOW;

struct TexArgs {
  int W, H, r, cap, threshold;
  const uint8_t *grey;      // [F][H][W]
  uint16_t *texture;        // [F][H][W]     (kTexPlane)
  float *disparity;         // [F][H][W]     (kTexDisparity): rejected pixels become `invalid`
  float invalid;
  float2 *flow;             // [F][H][W][2]  (kTexFlow): rejected pixels become (NaN, NaN), both words 0x7fc00000
};

template <int OUT>
__global__ __launch_bounds__(256) void k_texture(TexArgs a) {
  __shared__ uint8_t sI[kTexRows][kTexCols];
  __shared__ uint8_t sg[kTexRows][kTexCols];
  __shared__ uint16_t sR[kTexRows][kTexTileW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = a.r, rows = kTexTileH + 2 * r, cols = kTexTileW + 2 * r;
  const int x0 = blockIdx.x * kTexTileW, y0 = blockIdx.y * kTexTileH;
  const size_t fN = (size_t)blockIdx.z * a.W * a.H;
  const uint8_t *I = a.grey + fN;
  // ---- A: sI[j][k] = I(x0 - r - 1 + k, y0 - r + j), both clamped into the image, k < cols + 2 ------------------------------------
  for (int i = tid; i < rows * kTexCols; i += 256) {
    const int j = i / kTexCols, k = i - j * kTexCols;
    if (k >= cols + 2) continue;
    const int x = min(max(x0 - r - 1 + k, 0), a.W - 1), y = min(max(y0 - r + j, 0), a.H - 1);
    sI[j][k] = I[(size_t)y * a.W + x];
  }
  __syncthreads();
  // ---- B: sg[j][k] = g(x0 - r + k, y0 - r + j), k < cols: the neighbours of sI column k + 1 --------------------------------------
  for (int i = tid; i < rows * kTexCols; i += 256) {
    const int j = i / kTexCols, k = i - j * kTexCols;
    if (k >= cols) continue;
    const int x = x0 - r + k, y = y0 - r + j;
    const bool in = x >= 0 && x < a.W && y >= 0 && y < a.H;
    const int d = (int)sI[j][k + 2] - (int)sI[j][k];
    sg[j][k] = in ? (uint8_t)min(abs(d), a.cap) : (uint8_t)0;
  }
  __syncthreads();
  // ---- C: sR[j][lane] = sum of g(x0 + lane - r .. x0 + lane + r, y0 - r + j) --------------------------------------------------------
  for (int j = wv; j < rows; j += 4) {
    int s = 0;
    for (int i = 0; i <= 2 * r; i++) s += sg[j][lane + i];
    sR[j][lane] = (uint16_t)s;
  }
  __syncthreads();
  // ---- D: T(x0 + lane, y0 + 4 wv + i) = sR[4 wv + i .. 4 wv + i + 2 r][lane] ---------------------------------------------------------
  const int x = x0 + lane, ly = wv * (kTexTileH / 4);
  int T = 0;
  for (int j = 0; j <= 2 * r; j++) T += sR[ly + j][lane];
#pragma unroll
  for (int i = 0; i < kTexTileH / 4; i++) {
    const int y = y0 + ly + i;
    if (x < a.W && y < a.H) {
      const size_t p = fN + (size_t)y * a.W + x;
      if constexpr (OUT == kTexPlane) {
        a.texture[p] = (uint16_t)T;
      } else if (T < a.threshold) {
        if constexpr ((OUT & kTexDisparity) != 0) a.disparity[p] = a.invalid;
        if constexpr ((OUT & kTexFlow) != 0) a.flow[p] = make_float2(__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u));
      }
    }
    if (i + 1 < kTexTileH / 4) T += (int)sR[ly + i + 1 + 2 * r][lane] - (int)sR[ly + i][lane];
  }
}

}  // namespace

void launch_texture(int W, int H, int frames, int window, int cap, int threshold, const uint8_t *grey, uint16_t *texture, float *disparity,
                    float invalid, float *flow, hipStream_t s) {
  const TexArgs a{W, H, (window - 1) / 2, cap, threshold, grey, texture, disparity, invalid, reinterpret_cast<float2 *>(flow)};
  const dim3 grid((W + kTexTileW - 1) / kTexTileW, (H + kTexTileH - 1) / kTexTileH, frames);
  if (texture) hipLaunchKernelGGL(k_texture<kTexPlane>, grid, dim3(256), 0, s, a);
  else if (disparity && flow) hipLaunchKernelGGL(k_texture<(kTexDisparity | kTexFlow)>, grid, dim3(256), 0, s, a);
  else if (disparity) hipLaunchKernelGGL(k_texture<kTexDisparity>, grid, dim3(256), 0, s, a);
  else if (flow) hipLaunchKernelGGL(k_texture<kTexFlow>, grid, dim3(256), 0, s, a);
}
