// flow_fill.hip — the disparity-gated hole fill of a finished flow (mod_set_flow_fill, mod_flow_fill_dev; include/mod_sf.h states the
// rule, DESIGN.md §3.5d where it sits; tests/models/flow_fill_model.py restates it):
//   a flow pixel is VALID when both components are finite; a disparity word d is valid when it is finite and d > 0
//   g(p) = tol_abs + tol_rel * d_p, a multiply and then an add, each rounded to float32
//   S = the pixels q != p of the w x w square round p, clipped to the image, with a valid flow, a valid disparity and
//       fabsf(d_q - d_p) <= g(p); n = |S|
//   p valid, p's disparity invalid, or n < min_valid: out = in, bit for bit
//   else out.x / out.y = the element (n - 1) / 2, in ascending order of the key k(b) = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000), of the
//   x / y words of S, each component on its own
//
// k_flow_fill<WINDOW>: one workgroup (4 waves) per 64 x 16 tile, frames in grid.z, r = (WINDOW - 1) / 2 — k_flow_median's shape.
//   A  the flow tile with r halo columns and rows, read as float2, into LDS as the two KEYS of every cell, and the disparity word of the
//      cell in a third plane ((64 + 2 r) x (16 + 2 r) x 12 bytes: 14256 / 16320 / 18480 at window 3 / 5 / 7).  A cell with an invalid flow and a cell outside the
//      image hold kSentinel in both key planes, as in k_flow_median; a cell with an invalid disparity and a cell outside the image hold
//      a NaN in the disparity plane, so that the gate's one comparison refuses them whatever the centre is.  No load leaves the planes:
//      a cell outside the image is not loaded.
//   B  a lane owns one column and four rows.  A valid centre, the common case, stores the inverse of its own two keys: its input words.
//   C  a hole reads the WINDOW^2 disparity words and keys of its window into a bit mask of the cells of S (its own cell holds the
//      sentinel and is never one) and n is the mask's population count.  The selection is a RANK COUNT over the LDS cells, not a network:
//      for every cell i of S the lane counts the cells j of S with k_j < k_i and with k_j <= k_i; the cell whose two counts enclose the
//      rank (less <= rank < less_or_equal) holds the answer.  Equal keys are equal words (the key is a bijection), so whichever of
//      them is met gives the same bits.  Both loops run over the window's cells with wave-uniform addresses (consecutive lanes,
//      consecutive dwords); lanes that are no hole, and cells that are not in a lane's S, are masked.  A wave without a hole skips it all.
//   D  a hole that is not filled needs the input's own bits: its lane reads them again from the input plane.
// Input and output are different planes (checked by the caller); every pixel of the output is stored, 8 bytes, plain vector stores.
#include "mod_launch.h"

namespace {

constexpr int kFillTileW = 64, kFillTileH = 16;
constexpr uint32_t kSentinel = 0xFFFFFFFFu, kNanBits = 0x7fc00000u;

struct FillArgs {
  int W, H, min_valid;
  float tol_abs, tol_rel;
  const float2 *in;         // [F][H][W]
  const float *disparity;   // [F][H][W]
  float2 *out;              // [F][H][W], not `in`
};

__device__ inline uint32_t flow_key(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ inline uint32_t flow_unkey(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
__device__ inline bool finite_bits(uint32_t b) { return (b & 0x7F800000u) != 0x7F800000u; }
// finite and > 0: the sign bit clear, not zero, the exponent not all ones
__device__ inline bool disparity_valid(uint32_t b) { return b - 1u < 0x7F7FFFFFu; }

template <int WINDOW>
__global__ __launch_bounds__(256) void k_flow_fill(FillArgs a) {
  constexpr int R = (WINDOW - 1) / 2, kCols = kFillTileW + 2 * R, kRows = kFillTileH + 2 * R, N = WINDOW * WINDOW;
  __shared__ uint32_t sx[kRows][kCols], sy[kRows][kCols];
  __shared__ float sd[kRows][kCols];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int x0 = blockIdx.x * kFillTileW, y0 = blockIdx.y * kFillTileH;
  const size_t fN = (size_t)blockIdx.z * a.W * a.H;
  const uint2 *const in = reinterpret_cast<const uint2 *>(a.in) + fN;
  const uint32_t *const disp = reinterpret_cast<const uint32_t *>(a.disparity) + fN;
  // ---- A: (sx, sy, sd)[j][k] = the keys and the disparity of (x0 - R + k, y0 - R + j) ------------------------------------------------
  for (int i = tid; i < kRows * kCols; i += 256) {
    const int j = i / kCols, k = i - j * kCols;
    const int x = x0 - R + k, y = y0 - R + j;
    uint32_t kx = kSentinel, ky = kSentinel, d = kNanBits;
    if (x >= 0 && x < a.W && y >= 0 && y < a.H) {
      const size_t q = (size_t)y * a.W + x;
      const uint2 w = in[q];
      const uint32_t dq = disp[q];
      if (finite_bits(w.x) && finite_bits(w.y)) { kx = flow_key(w.x); ky = flow_key(w.y); }
      if (disparity_valid(dq)) d = dq;
    }
    sx[j][k] = kx;
    sy[j][k] = ky;
    sd[j][k] = __uint_as_float(d);
  }
  __syncthreads();
  // ---- B .. D: pixels (x0 + lane, y0 + 4 wv + i) -------------------------------------------------------------------------------------
  const int x = x0 + lane;
  if (x >= a.W) return;
#pragma unroll 1
  for (int i = 0; i < kFillTileH / 4; i++) {
    const int ly = wv * (kFillTileH / 4) + i, y = y0 + ly;
    if (y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    const uint32_t cx = sx[ly + R][lane + R];
    uint2 o;
    if (cx != kSentinel) {
      o = make_uint2(flow_unkey(cx), flow_unkey(sy[ly + R][lane + R]));
    } else {
      const float dp = sd[ly + R][lane + R];
      // a NaN d_p (invalid) makes g a NaN, and every comparison below false: n = 0
      const float g = __fadd_rn(a.tol_abs, __fmul_rn(a.tol_rel, dp));
      uint64_t mask = 0;
#pragma unroll
      for (int j = 0; j < WINDOW; j++)
#pragma unroll
        for (int k = 0; k < WINDOW; k++) {
          const bool in_s = sx[ly + j][lane + k] != kSentinel && fabsf(__fsub_rn(sd[ly + j][lane + k], dp)) <= g;
          mask |= (uint64_t)in_s << (j * WINDOW + k);
        }
      const int n = __popcll(mask);
      if (n == 0 || n < a.min_valid) {
        o = in[p];
      } else {
        const int rank = (n - 1) >> 1;
        uint32_t ox = 0, oy = 0;
#pragma unroll 1
        for (int c = 0; c < N; c++) {
          if (!((mask >> c) & 1)) continue;
          const int cj = c / WINDOW, ck = c - cj * WINDOW;
          const uint32_t kx = sx[ly + cj][lane + ck], ky = sy[ly + cj][lane + ck];
          int less_x = 0, leq_x = 0, less_y = 0, leq_y = 0;
#pragma unroll
          for (int j = 0; j < WINDOW; j++)
#pragma unroll
            for (int k = 0; k < WINDOW; k++) {
              // a cell outside S counts as the sentinel, which is above every key of S: it is in neither count
              const bool in_s = (mask >> (j * WINDOW + k)) & 1;
              const uint32_t qx = in_s ? sx[ly + j][lane + k] : kSentinel, qy = in_s ? sy[ly + j][lane + k] : kSentinel;
              less_x += qx < kx; leq_x += qx <= kx;
              less_y += qy < ky; leq_y += qy <= ky;
            }
          if (less_x <= rank && rank < leq_x) ox = kx;
          if (less_y <= rank && rank < leq_y) oy = ky;
        }
        o = make_uint2(flow_unkey(ox), flow_unkey(oy));
      }
    }
    reinterpret_cast<uint2 *>(a.out)[fN + p] = o;
  }
}

}  // namespace

void launch_flow_fill(int W, int H, int frames, int window, int min_valid, float tol_abs, float tol_rel, const float *in, const float *disparity,
                      float *out, hipStream_t s) {
  const FillArgs a{W, H, min_valid, tol_abs, tol_rel, reinterpret_cast<const float2 *>(in), disparity, reinterpret_cast<float2 *>(out)};
  const dim3 grid((W + kFillTileW - 1) / kFillTileW, (H + kFillTileH - 1) / kFillTileH, frames);
  if (window == 3) hipLaunchKernelGGL(k_flow_fill<3>, grid, dim3(256), 0, s, a);
  else if (window == 5) hipLaunchKernelGGL(k_flow_fill<5>, grid, dim3(256), 0, s, a);
  else if (window == 7) hipLaunchKernelGGL(k_flow_fill<7>, grid, dim3(256), 0, s, a);
}
