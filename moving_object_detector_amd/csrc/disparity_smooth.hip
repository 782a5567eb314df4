// disparity_smooth.hip — the edge-preserving smoother of a finished disparity (mod_set_disparity_smooth, mod_disparity_smooth_dev;
// include/mod_sf.h states the rule, DESIGN.md §3.4f where it sits; tests/models/disparity_smooth_model.py restates it):
//   a word w is VALID when it is finite and w >= lo
//   an invalid pixel: out = in, bit for bit
//   a valid pixel with word d: its members are the valid words q of its window x window square (clipped to its own frame) with
//   fabsf(q - d) <= tol; n = their number (the pixel is one of them)
//   n < min_members: out = in, bit for bit;  else out = fmaxf(sum / (float)n, lo), sum = 0.0f + q + q ... in row-major order of the window
//
// k_disparity_smooth<Window>: k_depth_spatial's scheme (depth_spatial.hip) for contiguous float planes, 4 + 4 algorithmic bytes a pixel;
// the window's 9 .. 49 reads come from LDS:
//   * A workgroup of 256 lanes makes a tile of 32 runs x 8 rows.  A lane owns one run: the 4 consecutive words of one row that lie between
//     two 16-byte boundaries of the OUTPUT row, so a row interior is one aligned 16-byte store.  `head`, the words in front of a row's first
//     boundary, is per row (a width that is no multiple of 4), and the ends of a row take the element path.
//   * Rows V0 - R .. V0 + 7 + R of the tile, with R columns either side, are staged once per workgroup as F32 words: the word itself where
//     it is valid, NaN where it is not or lies outside the frame (a NaN is never a member and has no members: every gate compares false).
//   * The tile is stored residue-major: word i of a staged row lies at (i % 4) * kSlots + i / 4, so the 32 lanes of a row, which read the
//     same residue of consecutive runs, read consecutive LDS words: conflict-free ds_read_b32.
//   * A lane reads its own 4 words once more from global memory (L1 / L2 hits), as one 16-byte load where the source address allows, so
//     a copied word is the input word itself.
//   * A lane keeps 4 running sums and counts in registers and walks the window row by row, column by column: the order of the rule.
// LDS: (8 + 2 R) rows x 4 kSlots words: 5.3 KiB (window 3) to 7.7 KiB (window 7); no atomics; frames in blockIdx.z.  Input and output are
// different planes (checked by the caller); every word of the output is stored once, plain vector stores.
#include "mod_launch.h"

namespace {

constexpr int kRuns = 32, kRows = 8, kBlock = kRuns * kRows, S = 4;

__device__ __forceinline__ bool smooth_valid(uint32_t b, float lo) { return (b & 0x7F800000u) != 0x7F800000u && __uint_as_float(b) >= lo; }

//   runs  runs per row: (W + 3) / 4 + 1 (run r covers x in [head + 4 (r - 1), head + 4 r))
template <int Win>
__global__ __launch_bounds__(kBlock) void k_disparity_smooth(int W, int H, int runs, float lo, float tol, int min_members,
                                                             const uint32_t *__restrict__ src, uint32_t *__restrict__ dst) {
  constexpr int R = Win / 2;
  constexpr int kSlots = kRuns + 1 + (2 * R + S - 1) / S;   // runs a staged row spans: the tile's 32, one for the rows' differing heads, the two aprons'
  constexpr int kTileW = S * (kRuns + 1) + 2 * R;           // words of a staged row that are filled: x in [xb, xb + kTileW)
  constexpr int kPitch = S * kSlots;                        // words of a staged row
  static_assert(kTileW <= kPitch, "a staged row must fit its slots");
  const int r0 = blockIdx.x * kRuns, V0 = blockIdx.y * kRows;
  const size_t fN = (size_t)blockIdx.z * W * H;
  const uint32_t *const in = src + fN;
  uint32_t *const out_plane = dst + fN;
  const int xb = S * (r0 - 1) - R;

  __shared__ float tile[(kRows + 2 * R) * kPitch];
  for (int i = threadIdx.x; i < (kRows + 2 * R) * kTileW; i += kBlock) {
    const int ly = i / kTileW, lx = i - ly * kTileW;
    const int x = xb + lx, y = V0 - R + ly;
    float v = __builtin_nanf("");
    if (x >= 0 && x < W && y >= 0 && y < H) {               // no load leaves the frame
      const uint32_t b = in[(size_t)y * W + x];
      if (smooth_valid(b, lo)) v = __uint_as_float(b);
    }
    tile[ly * kPitch + (lx % S) * kSlots + lx / S] = v;
  }
  __syncthreads();

  const int lr = threadIdx.x % kRuns, lv = threadIdx.x / kRuns;
  const int r = r0 + lr, V = V0 + lv;
  if (r >= runs || V >= H) return;
  const uint32_t *const row = in + (size_t)V * W;
  uint32_t *const out = out_plane + (size_t)V * W;
  const int head = (int)((0u - (uint32_t)(uintptr_t)out) & 15u) / 4;
  const int xs = head + (r - 1) * S;
  if (xs >= W || xs + S <= 0) return;
  const bool whole = xs >= 0 && xs + S <= W;

  uint32_t w[S];
  if (whole && ((uintptr_t)(row + xs) & 15u) == 0) {
    const uint4 q = *reinterpret_cast<const uint4 *>(row + xs);
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < S; k++) {
      const int x = xs + k;
      w[k] = x >= 0 && x < W ? row[x] : 0u;
    }
  }

  // the lane's strip of the tile: rows lv .. lv + 2 R, words xs - R .. xs + 3 + R, which is staged word lx0 + j, j = 0 .. 3 + 2 R
  const int lx0 = xs - R - xb;    // = 4 lr + head: in 0 .. 4 kRuns - 1
  float dc[S], sum[S];            // the lane's own words as staged: NaN = invalid, and then n stays 0
  int n[S];
#pragma unroll
  for (int k = 0; k < S; k++) {
    const int i = lx0 + R + k;
    dc[k] = tile[(lv + R) * kPitch + (i % S) * kSlots + i / S];
    sum[k] = 0.0f;
    n[k] = 0;
  }
#pragma unroll
  for (int dy = 0; dy < Win; dy++) {            // rows top to bottom ...
    float q[S + 2 * R];
#pragma unroll
    for (int j = 0; j < S + 2 * R; j++) {
      const int i = lx0 + j;
      q[j] = tile[(lv + dy) * kPitch + (i % S) * kSlots + i / S];
    }
#pragma unroll
    for (int k = 0; k < S; k++)
#pragma unroll
      for (int dx = 0; dx < Win; dx++) {        // ... then left to right: the rule's order, not to be reassociated
        const bool member = fabsf(q[k + dx] - dc[k]) <= tol;   // false where either is NaN
        sum[k] = member ? sum[k] + q[k + dx] : sum[k];
        n[k] += member ? 1 : 0;
      }
  }
  uint32_t o[S];
#pragma unroll
  for (int k = 0; k < S; k++)     // (a valid pixel is its own member, n >= 1; min_members >= 1 keeps the invalid ones, n = 0, as they are)
    o[k] = n[k] >= min_members ? __float_as_uint(fmaxf(sum[k] / (float)n[k], lo)) : w[k];

  if (whole) {
    *reinterpret_cast<uint4 *>(__builtin_assume_aligned(out + xs, 16)) = uint4{o[0], o[1], o[2], o[3]};
    return;
  }
#pragma unroll
  for (int k = 0; k < S; k++) {
    const int x = xs + k;
    if (x >= 0 && x < W) out[x] = o[k];
  }
}

template <int Win>
void launch(int W, int H, int frames, float lo, float tol, int min_members, const float *in, float *out, hipStream_t s) {
  const int runs = (W + S - 1) / S + 1;
  const dim3 grid((runs + kRuns - 1) / kRuns, (H + kRows - 1) / kRows, frames);
  hipLaunchKernelGGL(k_disparity_smooth<Win>, grid, dim3(kBlock), 0, s, W, H, runs, lo, tol, min_members, reinterpret_cast<const uint32_t *>(in),
                     reinterpret_cast<uint32_t *>(out));
}

}  // namespace

void launch_disparity_smooth(int W, int H, int frames, float lo, int window, float tol, int min_members, const float *in, float *out, hipStream_t s) {
  if (window == 3) launch<3>(W, H, frames, lo, tol, min_members, in, out, s);
  else if (window == 5) launch<5>(W, H, frames, lo, tol, min_members, in, out, s);
  else launch<7>(W, H, frames, lo, tol, min_members, in, out, s);
}
