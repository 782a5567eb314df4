// depth_filter.hip — the opt-in range and flying-pixel filter in front of the depth path (mod_set_depth_filter).
//
// k_depth_filter<Encoding, Window> maps `frames` depth messages (width x height samples, row pitch `step`, frames step * height bytes
// apart) to messages of the same layout: a sample that is valid (z > 0 and finite) and fails the range rule or the support rule of
// include/mod_sf.h becomes the encoding's "no reading" word, every other sample is copied bit for bit.  Support is counted on the INPUT
// after the range rule alone, so the filter is one pass.
//
// Memory-bound by design: one sample read and one written per pixel, 2 + 2 (16UC1) or 4 + 4 (32FC1) algorithmic bytes a sample.  The 8
// or 24 neighbour reads come from LDS:
//   * A workgroup of 256 lanes makes a tile of 32 runs x 8 rows.  A lane owns one run: the 16 / B consecutive samples of one row that
//     lie between two 16-byte boundaries of the OUTPUT row (8 of 16UC1, 4 of 32FC1), so a row interior is one aligned 16-byte store.
//     The rows of a message whose step is no multiple of 16 start at different offsets of that grid: `head`, the samples in front of a
//     row's first boundary, is per row, and the ends of a row take the element path.
//   * Rows V0 - R .. V0 + 7 + R of the tile, with R columns either side, are staged once per workgroup as F32 words: z where the sample
//     passes the range rule, NaN where it does not or lies outside the message (a NaN never supports: |NaN - z| <= t is false).  The
//     staging reads are element loads, consecutive lanes on consecutive samples; each input row is read (8 + 2 R) / 8 times, from L2
//     after the first.
//   * The tile is stored residue-major: sample i of a staged row lies at word (i % S) * kSlots + i / S (S = samples per run), so the 64
//     lanes of a wave, which read the same residue of consecutive runs, read consecutive words: conflict-free ds_read_b32, where the
//     row-major image would put lanes 8 (or 4) words apart.
//   * A lane reads its own S raw words once more from global memory (L1 / L2 hits: the workgroup has just staged them) as one 16-byte
//     load where the source address allows, so a kept sample is the input word itself.
// Window 0 (the range rule alone, and the copy while the filter is off) is the same kernel without the tile.
// LDS: (8 + 2 R) rows x S * 34 words: 10.6 KiB (16UC1, window 3) to 12.75 KiB (16UC1, window 5); no atomics; frames in blockIdx.z.
#include "mod_launch.h"

namespace {

constexpr int kRuns = 32, kRows = 8, kBlock = kRuns * kRows;
constexpr int kSlots = kRuns + 2;   // runs a staged row spans: the tile's 32, one for the rows' differing heads, one for the two aprons

template <int Enc> constexpr int kBytes = Enc == MOD_DEPTH_16UC1 ? 2 : 4;
template <int Enc> struct Word { using type = uint32_t; };
template <> struct Word<MOD_DEPTH_16UC1> { using type = uint16_t; };

template <int Enc>
__device__ __forceinline__ float word_z(typename Word<Enc>::type w, float unit) {
  if constexpr (Enc == MOD_DEPTH_16UC1) return (float)w * unit;
  else return __uint_as_float(w) * unit;
}

__device__ __forceinline__ bool valid0(float z) { return z > 0.0f && z < __builtin_inff(); }
__device__ __forceinline__ bool in_range(float z, float z_min, float z_max) {
  return valid0(z) && (z_min == 0.0f || z >= z_min) && (z_max == 0.0f || z <= z_max);
}

struct FilterArgs { float z_min, z_max, tol_abs, tol_rel; int min_support; };

//   runs         runs per row: (width + S - 1) / S + 1 (run r covers x in [head + S (r - 1), head + S r))
//   frame_bytes  step * height
template <int Enc, int Win>
__global__ __launch_bounds__(kBlock) void k_depth_filter(int width, int height, int runs, const uint8_t *__restrict__ src, size_t frame_bytes, int step,
                                                         float unit, FilterArgs a, uint8_t *__restrict__ dst) {
  using T = typename Word<Enc>::type;
  constexpr int B = kBytes<Enc>, S = 16 / B, R = Win / 2;
  constexpr int kTileW = S * (kRuns + 1) + 2 * R;    // samples of a staged row: x in [xb, xb + kTileW)
  constexpr int kPitch = S * kSlots;                 // words of a staged row
  static_assert(kTileW <= kPitch, "a staged row must fit its slots");
  constexpr T kNoReading = Enc == MOD_DEPTH_16UC1 ? (T)0 : (T)0x7fc00000u;
  const int r0 = blockIdx.x * kRuns, V0 = blockIdx.y * kRows, f = blockIdx.z;
  const uint8_t *msg = src + (size_t)f * frame_bytes;
  uint8_t *out_msg = dst + (size_t)f * frame_bytes;
  const int xb = S * (r0 - 1) - R;

  __shared__ float tile[Win ? (kRows + 2 * R) * kPitch : 1];
  if constexpr (Win != 0) {
    for (int i = threadIdx.x; i < (kRows + 2 * R) * kTileW; i += kBlock) {
      const int ly = i / kTileW, lx = i - ly * kTileW;
      const int x = xb + lx, y = V0 - R + ly;
      float z = __builtin_nanf("");
      if (x >= 0 && x < width && y >= 0 && y < height) {
        const float zq = word_z<Enc>(*reinterpret_cast<const T *>(msg + (size_t)y * step + (size_t)x * B), unit);
        if (in_range(zq, a.z_min, a.z_max)) z = zq;
      }
      tile[ly * kPitch + (lx % S) * kSlots + lx / S] = z;
    }
    __syncthreads();
  }

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

  T o[S];
  if constexpr (Win == 0) {
#pragma unroll
    for (int k = 0; k < S; k++) {
      const float z = word_z<Enc>(w[k], unit);
      o[k] = valid0(z) && !in_range(z, a.z_min, a.z_max) ? kNoReading : w[k];
    }
  } else {
    // the lane's strip of the tile: rows lv .. lv + 2 R, samples xs - R .. xs + S - 1 + R, which is staged sample lx0 + j, j = 0 .. S + 2 R - 1
    const int lx0 = xs - R - xb;    // = S * lr + head: in 0 .. S * kRuns - 1
    int n[S];
#pragma unroll
    for (int k = 0; k < S; k++) n[k] = 0;
    float zc[S], t[S];
#pragma unroll
    for (int k = 0; k < S; k++) {
      const int i = lx0 + R + k;
      zc[k] = tile[(lv + R) * kPitch + (i % S) * kSlots + i / S];   // NaN: not in range (n stays 0, and the sample is decided below)
      t[k] = a.tol_abs + a.tol_rel * zc[k];
    }
#pragma unroll
    for (int dy = 0; dy < Win; dy++) {
      float q[S + 2 * R];
#pragma unroll
      for (int j = 0; j < S + 2 * R; j++) {
        const int i = lx0 + j;
        q[j] = tile[(lv + dy) * kPitch + (i % S) * kSlots + i / S];
      }
#pragma unroll
      for (int k = 0; k < S; k++)
#pragma unroll
        for (int dx = 0; dx < Win; dx++)
          if (dy != R || dx != R) n[k] += fabsf(q[k + dx] - zc[k]) <= t[k] ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < S; k++) {
      const bool v0 = valid0(word_z<Enc>(w[k], unit));
      const bool keep = zc[k] == zc[k] && n[k] >= a.min_support;
      o[k] = v0 && !keep ? kNoReading : w[k];
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
void launch(int width, int height, int frames, const void *src, int step, float unit, const FilterArgs &a, void *dst, hipStream_t s) {
  constexpr int S = 16 / kBytes<Enc>;
  const int runs = (width + S - 1) / S + 1;
  const dim3 grid((runs + kRuns - 1) / kRuns, (height + kRows - 1) / kRows, frames);
  hipLaunchKernelGGL((k_depth_filter<Enc, Win>), grid, dim3(kBlock), 0, s, width, height, runs, static_cast<const uint8_t *>(src),
                     (size_t)step * height, step, unit, a, static_cast<uint8_t *>(dst));
}

template <int Enc>
void launch_enc(int window, int width, int height, int frames, const void *src, int step, float unit, const FilterArgs &a, void *dst, hipStream_t s) {
  if (window == 3) launch<Enc, 3>(width, height, frames, src, step, unit, a, dst, s);
  else if (window == 5) launch<Enc, 5>(width, height, frames, src, step, unit, a, dst, s);
  else launch<Enc, 0>(width, height, frames, src, step, unit, a, dst, s);
}

}  // namespace

void launch_depth_filter(int encoding, int width, int height, int frames, const void *src, int step, float unit, const ModDepthFilter &flt,
                         void *dst, hipStream_t s) {
  const FilterArgs a{flt.z_min, flt.z_max, flt.tol_abs, flt.tol_rel, flt.min_support};
  if (encoding == MOD_DEPTH_16UC1) launch_enc<MOD_DEPTH_16UC1>(flt.window, width, height, frames, src, step, unit, a, dst, s);
  else launch_enc<MOD_DEPTH_32FC1>(flt.window, width, height, frames, src, step, unit, a, dst, s);
}
