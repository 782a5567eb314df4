// depth_spatial.hip — the opt-in edge-preserving smoother and hole fill of the depth path, behind k_depth_filter and in front of
// k_depth_temporal (mod_set_depth_spatial).
//
// k_depth_spatial<Encoding, Window> maps `frames` depth messages (width x height samples, row pitch `step`, frames step * height bytes
// apart) to messages of the same layout by the rule of include/mod_sf.h: a valid sample (z > 0 and finite) becomes the mean of the raw
// values of its window's valid samples within t = tol_abs + tol_rel * z of it (a gated box mean, summed in row-major order); a sample
// without a reading becomes the mean of the valid samples of its window within t of the FARTHEST of them, where at least fill_min lie
// there; every other sample is copied bit for bit.  Both rules read the INPUT only: one pass, no cascade.
//
// k_depth_filter's scheme (depth_filter.hip), 2 + 2 (16UC1) or 4 + 4 (32FC1) algorithmic bytes a sample; the window's 9 .. 49 reads
// come from LDS:
//   * A workgroup of 256 lanes makes a tile of 32 runs x 8 rows.  A lane owns one run: the 16 / B consecutive samples of one row that
//     lie between two 16-byte boundaries of the OUTPUT row (8 of 16UC1, 4 of 32FC1), so a row interior is one aligned 16-byte store.
//     `head`, the samples in front of a row's first boundary, is per row (a step that is no multiple of 16), and the ends of a row take
//     the element path.
//   * Rows V0 - R .. V0 + 7 + R of the tile, with R columns either side, are staged once per workgroup as F32 words: x, the raw value,
//     where the sample has valid0, NaN where it has not or lies outside the message (a NaN is never a member: every gate compares
//     false).  z = x * unit is formed at the read, one multiply per staged word a lane reads: one plane, not two.
//   * The tile is stored residue-major: sample i of a staged row lies at word (i % S) * kSlots + i / S (S = samples per run), so the 64
//     lanes of a wave, which read the same residue of consecutive runs, read consecutive words: conflict-free ds_read_b32.
//   * A lane reads its own S raw words once more from global memory (L1 / L2 hits), as one 16-byte load where the source address
//     allows, so a copied sample is the input word itself.
//   * The smoother keeps S running sums in registers and walks the window row by row, column by column: the order of the rule, which
//     is what makes 32FC1 reproducible.  The hole fill is a branch of its own, two rolled passes over the window (the anchor, then the
//     members): holes are rare, and the branch costs lanes without one nothing but the test.
// LDS: (8 + 2 R) rows x S * kSlots words: 10.6 KiB (16UC1, window 3) to 14.9 KiB (16UC1, window 7), ten workgroups a CU at the least;
// no atomics; frames in blockIdx.z.
#include "mod_launch.h"

namespace {

constexpr int kRuns = 32, kRows = 8, kBlock = kRuns * kRows;

template <int Enc> constexpr int kBytes = Enc == MOD_DEPTH_16UC1 ? 2 : 4;
template <int Enc> struct Word { using type = uint32_t; };
template <> struct Word<MOD_DEPTH_16UC1> { using type = uint16_t; };

template <int Enc>
__device__ __forceinline__ float word_x(typename Word<Enc>::type w) {
  if constexpr (Enc == MOD_DEPTH_16UC1) return (float)w;
  else return __uint_as_float(w);
}

// k_depth_temporal's enc
template <int Enc>
__device__ __forceinline__ typename Word<Enc>::type enc(float m) {
  if constexpr (Enc == MOD_DEPTH_16UC1) return (uint16_t)fminf(fmaxf(rintf(m), 1.0f), 65535.0f);
  else return __float_as_uint(m);
}

__device__ __forceinline__ bool valid0(float z) { return z > 0.0f && z < __builtin_inff(); }

struct SpatialArgs { float tol_abs, tol_rel; int smooth, fill_min; };

// The hole rule for the pixel whose window begins at staged row `ly0`, staged sample `i0`: true and *m = the mean where it fills.
template <int S, int Win, int kSlots>
__device__ __forceinline__ bool fill_hole(const float *tile, int ly0, int i0, float unit, const SpatialArgs &a, float *m) {
  constexpr int kPitch = S * kSlots;
  float anchor = -__builtin_inff();      // the anchor: the largest z of the window's valid samples
#pragma unroll 1
  for (int dy = 0; dy < Win; dy++)
#pragma unroll 1
    for (int dx = 0; dx < Win; dx++) {
      const int i = i0 + dx;
      const float zq = tile[(ly0 + dy) * kPitch + (i % S) * kSlots + i / S] * unit;
      anchor = zq > anchor ? zq : anchor;      // (a NaN compares false)
    }
  if (!(anchor > 0.0f)) return false;    // no valid neighbour
  const float t = a.tol_abs + a.tol_rel * anchor;
  float sum = 0.0f;
  int n = 0;
#pragma unroll 1
  for (int dy = 0; dy < Win; dy++)
#pragma unroll 1
    for (int dx = 0; dx < Win; dx++) {
      const int i = i0 + dx;
      const float xq = tile[(ly0 + dy) * kPitch + (i % S) * kSlots + i / S];
      const float zq = xq * unit;
      if (anchor - zq <= t) { sum = sum + xq; n++; }
    }
  if (n < a.fill_min) return false;
  *m = sum / (float)n;
  return true;
}

//   runs         runs per row: (width + S - 1) / S + 1 (run r covers x in [head + S (r - 1), head + S r))
//   frame_bytes  step * height
template <int Enc, int Win>
__global__ __launch_bounds__(kBlock) void k_depth_spatial(int width, int height, int runs, const uint8_t *__restrict__ src, size_t frame_bytes, int step,
                                                          float unit, SpatialArgs a, uint8_t *__restrict__ dst) {
  using T = typename Word<Enc>::type;
  constexpr int B = kBytes<Enc>, S = 16 / B, R = Win / 2;
  constexpr int kSlots = kRuns + 1 + (2 * R + S - 1) / S;   // runs a staged row spans: the tile's 32, one for the rows' differing heads, the two aprons'
  constexpr int kTileW = S * (kRuns + 1) + 2 * R;           // samples of a staged row: x in [xb, xb + kTileW)
  constexpr int kPitch = S * kSlots;                        // words of a staged row
  static_assert(kTileW <= kPitch, "a staged row must fit its slots");
  static_assert((kRows + 2 * R) * kPitch * 4 <= 16 * 1024, "the tile must leave room for many workgroups a CU");
  const int r0 = blockIdx.x * kRuns, V0 = blockIdx.y * kRows, f = blockIdx.z;
  const uint8_t *msg = src + (size_t)f * frame_bytes;
  uint8_t *out_msg = dst + (size_t)f * frame_bytes;
  const int xb = S * (r0 - 1) - R;

  __shared__ float tile[(kRows + 2 * R) * kPitch];
  for (int i = threadIdx.x; i < (kRows + 2 * R) * kTileW; i += kBlock) {
    const int ly = i / kTileW, lx = i - ly * kTileW;
    const int x = xb + lx, y = V0 - R + ly;
    float xv = __builtin_nanf("");
    if (x >= 0 && x < width && y >= 0 && y < height) {
      const float xq = word_x<Enc>(*reinterpret_cast<const T *>(msg + (size_t)y * step + (size_t)x * B));
      if (valid0(xq * unit)) xv = xq;
    }
    tile[ly * kPitch + (lx % S) * kSlots + lx / S] = xv;
  }
  __syncthreads();

  const int lr = threadIdx.x % kRuns, lv = threadIdx.x / kRuns;
  const int r = r0 + lr, V = V0 + lv;
  if (r >= runs || V >= height) return;
  const uint8_t *row = msg + (size_t)V * step;
  uint8_t *out = out_msg + (size_t)V * step;
  const int head = (int)((0u - (uint32_t)(uintptr_t)out) & 15u) / B;
  const int xs = head + (r - 1) * S;
  if (xs >= width || xs + S <= 0) return;
  const bool whole = xs >= 0 && xs + S <= width;

  T w[S];
  if (whole && ((uintptr_t)(row + (size_t)xs * B) & 15u) == 0) {
    const uint4 q = *reinterpret_cast<const uint4 *>(row + (size_t)xs * B);
    const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < S; k++) {
      if constexpr (B == 2) w[k] = (T)(d[k >> 1] >> ((k & 1) * 16));
      else w[k] = d[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < S; k++) {
      const int x = xs + k;
      w[k] = x >= 0 && x < width ? *reinterpret_cast<const T *>(row + (size_t)x * B) : (T)0;
    }
  }

  // the lane's strip of the tile: rows lv .. lv + 2 R, samples xs - R .. xs + S - 1 + R, which is staged sample lx0 + j, j = 0 .. S + 2 R - 1
  const int lx0 = xs - R - xb;    // = S * lr + head: in 0 .. S * kRuns - 1
  float xc[S];                    // the lane's own samples as staged: NaN = no valid0
#pragma unroll
  for (int k = 0; k < S; k++) {
    const int i = lx0 + R + k;
    xc[k] = tile[(lv + R) * kPitch + (i % S) * kSlots + i / S];
  }

  T o[S];
#pragma unroll
  for (int k = 0; k < S; k++) o[k] = w[k];

  if (a.smooth) {
    float zc[S], t[S], sum[S];
    int n[S];
#pragma unroll
    for (int k = 0; k < S; k++) {
      zc[k] = xc[k] * unit;
      t[k] = a.tol_abs + a.tol_rel * zc[k];
      sum[k] = 0.0f;
      n[k] = 0;
    }
#pragma unroll
    for (int dy = 0; dy < Win; dy++) {          // V ascending ...
      float xq[S + 2 * R], zq[S + 2 * R];
#pragma unroll
      for (int j = 0; j < S + 2 * R; j++) {
        const int i = lx0 + j;
        xq[j] = tile[(lv + dy) * kPitch + (i % S) * kSlots + i / S];
        zq[j] = xq[j] * unit;
      }
#pragma unroll
      for (int k = 0; k < S; k++)
#pragma unroll
        for (int dx = 0; dx < Win; dx++) {      // ... then U ascending: the rule's order, not to be reassociated
          const bool member = fabsf(zq[k + dx] - zc[k]) <= t[k];   // false where either is NaN
          sum[k] = member ? sum[k] + xq[k + dx] : sum[k];
          n[k] += member ? 1 : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < S; k++)
      if (xc[k] == xc[k]) o[k] = enc<Enc>(sum[k] / (float)n[k]);   // (p is a member of its own window: n >= 1)
  }

  if (a.fill_min > 0) {
#pragma unroll
    for (int k = 0; k < S; k++) {
      float m;
      if (xc[k] != xc[k] && xs + k >= 0 && xs + k < width && fill_hole<S, Win, kSlots>(tile, lv, lx0 + k, unit, a, &m)) o[k] = enc<Enc>(m);
    }
  }

  if (whole) {
    uint4 q;
    if constexpr (B == 2) {
      q.x = (uint32_t)o[0] | (uint32_t)o[1] << 16; q.y = (uint32_t)o[2] | (uint32_t)o[3] << 16;
      q.z = (uint32_t)o[4] | (uint32_t)o[5] << 16; q.w = (uint32_t)o[6] | (uint32_t)o[7] << 16;
    } else {
      q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
    }
    *reinterpret_cast<uint4 *>(__builtin_assume_aligned(out + (size_t)xs * B, 16)) = q;
    return;
  }
#pragma unroll
  for (int k = 0; k < S; k++) {
    const int x = xs + k;
    if (x >= 0 && x < width) *reinterpret_cast<T *>(out + (size_t)x * B) = o[k];
  }
}

template <int Enc, int Win>
void launch(int width, int height, int frames, const void *src, int step, float unit, const SpatialArgs &a, void *dst, hipStream_t s) {
  constexpr int S = 16 / kBytes<Enc>;
  const int runs = (width + S - 1) / S + 1;
  const dim3 grid((runs + kRuns - 1) / kRuns, (height + kRows - 1) / kRows, frames);
  hipLaunchKernelGGL((k_depth_spatial<Enc, Win>), grid, dim3(kBlock), 0, s, width, height, runs, static_cast<const uint8_t *>(src),
                     (size_t)step * height, step, unit, a, static_cast<uint8_t *>(dst));
}

template <int Enc>
void launch_enc(int window, int width, int height, int frames, const void *src, int step, float unit, const SpatialArgs &a, void *dst, hipStream_t s) {
  if (window == 3) launch<Enc, 3>(width, height, frames, src, step, unit, a, dst, s);
  else if (window == 5) launch<Enc, 5>(width, height, frames, src, step, unit, a, dst, s);
  else launch<Enc, 7>(width, height, frames, src, step, unit, a, dst, s);
}

}  // namespace

void launch_depth_spatial(int encoding, int width, int height, int frames, const void *src, int step, float unit, const ModDepthSpatial &sp,
                          void *dst, hipStream_t s) {
  const SpatialArgs a{sp.tol_abs, sp.tol_rel, sp.smooth, sp.fill_min};
  if (encoding == MOD_DEPTH_16UC1) launch_enc<MOD_DEPTH_16UC1>(sp.window, width, height, frames, src, step, unit, a, dst, s);
  else launch_enc<MOD_DEPTH_32FC1>(sp.window, width, height, frames, src, step, unit, a, dst, s);
}
