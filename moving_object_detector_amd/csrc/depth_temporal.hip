// depth_temporal.hip — the opt-in temporal filter with hold behind the spatial depth filter (mod_set_depth_temporal).
//
// k_depth_temporal<Encoding> maps `frames` consecutive depth messages (width x height samples, row pitch `step`, frames step * height
// bytes apart, frame 0 the oldest) to messages of the same layout by the rule of include/mod_sf.h: per pixel an exponential moving
// average `s` (F32, raw units) that restarts where the scene changed, and a counter `age` of the frames since the last reading that
// lets a pixel which dropped out repeat its average for at most `hold` frames.  The state is two packed height x width planes.
//
// Pointwise; memory-bound by design, and measured so only at one frame a call, what the stream does (at 64 frames a
// call a lane's serial frame loop, one 16-byte load in flight, reaches a third of the copy kernel's rate).  Algorithmic bytes per sample, B the bytes of a depth sample (2 for 16UC1, 4 for 32FC1): 2 B per frame
// (one word read, one written) plus 10 per call (s and age read once, 4 + 1, and written once, 4 + 1): at one frame a call 14 B of
// 16UC1 where k_depth_filter's window 0 moves 4.
//   * A workgroup of 256 lanes makes 32 runs x 8 rows, as in k_depth_filter.  A lane owns one run: the 16 / B consecutive samples of one
//     row that lie between two 16-byte boundaries of the OUTPUT row of frame 0, so a row interior is one aligned 16-byte store.  `head`,
//     the samples in front of a row's first boundary, is per row (a step that is no multiple of 16); the ends of a row take the
//     element path, and so does a later frame whose rows lie at another offset of the 16-byte grid (step * height % 16 != 0).
//   * The lane loops over the call's frames with s and age in registers: the state costs one read and one write per call, not per frame.
//     With `fresh` set the planes are not read at all: every pixel starts empty (that is how the host empties the state, in stream order).
//   * depth_out == depth_in is allowed: a lane reads its own words of a frame before it writes them, and no lane reads another's.
// The grid covers runs x rows only; no atomics, no LDS.
#include "mod_launch.h"

namespace {

constexpr int kRuns = 32, kRows = 8, kBlock = kRuns * kRows;
constexpr int kEmpty = 255;

template <int Enc> constexpr int kBytes = Enc == MOD_DEPTH_16UC1 ? 2 : 4;
template <int Enc> struct Word { using type = uint32_t; };
template <> struct Word<MOD_DEPTH_16UC1> { using type = uint16_t; };

template <int Enc>
__device__ __forceinline__ float word_x(typename Word<Enc>::type w) {
  if constexpr (Enc == MOD_DEPTH_16UC1) return (float)w;
  else return __uint_as_float(w);
}

template <int Enc>
__device__ __forceinline__ typename Word<Enc>::type enc(float s) {
  if constexpr (Enc == MOD_DEPTH_16UC1) return (uint16_t)fminf(fmaxf(rintf(s), 1.0f), 65535.0f);
  else return __float_as_uint(s);
}

__device__ __forceinline__ bool valid0(float z) { return z > 0.0f && z < __builtin_inff(); }

struct TemporalArgs { float alpha, delta_abs, delta_rel; int hold; };

//   runs         runs per row: (width + S - 1) / S + 1 (run r covers x in [head + S (r - 1), head + S r))
//   frame_bytes  step * height
template <int Enc>
__global__ __launch_bounds__(kBlock) void k_depth_temporal(int width, int height, int runs, int frames, const uint8_t *src, size_t frame_bytes, int step,
                                                           float unit, TemporalArgs a, int fresh, float *__restrict__ state_s,
                                                           uint8_t *__restrict__ state_age, uint8_t *dst) {
  using T = typename Word<Enc>::type;
  constexpr int B = kBytes<Enc>, S = 16 / B;
  const int r = blockIdx.x * kRuns + threadIdx.x % kRuns, V = blockIdx.y * kRows + threadIdx.x / kRuns;
  if (r >= runs || V >= height) return;
  const size_t row_off = (size_t)V * step;
  const int head = (int)((0u - (uint32_t)(uintptr_t)(dst + row_off)) & 15u) / B;
  const int xs = head + (r - 1) * S;
  if (xs >= width || xs + S <= 0) return;
  const bool whole = xs >= 0 && xs + S <= width;

  // the run's state: element i of the planes is pixel (i % width, i / width)
  float *const ps = state_s + ((size_t)V * width + xs);       // (formed, not dereferenced, where xs < 0)
  uint8_t *const pa = state_age + ((size_t)V * width + xs);
  const bool s_vec = whole && ((uintptr_t)ps & 15u) == 0, a_vec = whole && ((uintptr_t)pa & (S - 1)) == 0;
  float s[S];
  int age[S];
#pragma unroll
  for (int k = 0; k < S; k++) { s[k] = 0.0f; age[k] = kEmpty; }
  if (!fresh) {
    if (s_vec) {
#pragma unroll
      for (int k = 0; k < S; k += 4) {
        const float4 q = *reinterpret_cast<const float4 *>(ps + k);
        s[k] = q.x; s[k + 1] = q.y; s[k + 2] = q.z; s[k + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < S; k++) if (xs + k >= 0 && xs + k < width) s[k] = ps[k];
    }
    if (a_vec) {
      uint32_t d[S / 4];
      if constexpr (S == 8) { const uint2 q = *reinterpret_cast<const uint2 *>(pa); d[0] = q.x; d[1] = q.y; }
      else d[0] = *reinterpret_cast<const uint32_t *>(pa);
#pragma unroll
      for (int k = 0; k < S; k++) age[k] = (int)(d[k >> 2] >> ((k & 3) * 8) & 255u);
    } else {
#pragma unroll
      for (int k = 0; k < S; k++) if (xs + k >= 0 && xs + k < width) age[k] = pa[k];
    }
  }

  for (int f = 0; f < frames; f++) {
    const uint8_t *in = src + (size_t)f * frame_bytes + row_off + (ptrdiff_t)xs * B;
    uint8_t *out = dst + (size_t)f * frame_bytes + row_off + (ptrdiff_t)xs * B;
    T w[S];
    if (whole && ((uintptr_t)in & 15u) == 0) {
      const uint4 q = *reinterpret_cast<const uint4 *>(in);
      const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < S; k++) {
        if constexpr (B == 2) w[k] = (T)(d[k >> 1] >> ((k & 1) * 16));
        else w[k] = d[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < S; k++) w[k] = xs + k >= 0 && xs + k < width ? *reinterpret_cast<const T *>(in + (ptrdiff_t)k * B) : (T)0;
    }

    T o[S];
#pragma unroll
    for (int k = 0; k < S; k++) {
      const float x = word_x<Enc>(w[k]);
      const float z = x * unit;
      if (valid0(z)) {
        if (age[k] == kEmpty) {
          s[k] = x;
          o[k] = w[k];
        } else {
          const float zs = s[k] * unit;
          const float t = a.delta_abs + a.delta_rel * zs;
          if (fabsf(z - zs) <= t) {
            const float d = x - s[k];
            const float ad = a.alpha * d;
            s[k] = s[k] + ad;
          } else {
            s[k] = x;               // the scene changed: restart
          }
          o[k] = enc<Enc>(s[k]);
        }
        age[k] = 0;
      } else if (age[k] != kEmpty && age[k] < a.hold) {
        age[k] += 1;
        o[k] = enc<Enc>(s[k]);      // held
      } else {
        age[k] = kEmpty;
        s[k] = 0.0f;
        o[k] = w[k];
      }
    }

    if (whole && ((uintptr_t)out & 15u) == 0) {
      uint4 q;
      if constexpr (B == 2) {
        q.x = (uint32_t)o[0] | (uint32_t)o[1] << 16; q.y = (uint32_t)o[2] | (uint32_t)o[3] << 16;
        q.z = (uint32_t)o[4] | (uint32_t)o[5] << 16; q.w = (uint32_t)o[6] | (uint32_t)o[7] << 16;
      } else {
        q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
      }
      *reinterpret_cast<uint4 *>(out) = q;
    } else {
#pragma unroll
      for (int k = 0; k < S; k++)
        if (xs + k >= 0 && xs + k < width) *reinterpret_cast<T *>(out + (ptrdiff_t)k * B) = o[k];
    }
  }

  if (s_vec) {
#pragma unroll
    for (int k = 0; k < S; k += 4) *reinterpret_cast<float4 *>(ps + k) = make_float4(s[k], s[k + 1], s[k + 2], s[k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < S; k++) if (xs + k >= 0 && xs + k < width) ps[k] = s[k];
  }
  if (a_vec) {
    uint32_t d[S / 4];
#pragma unroll
    for (int j = 0; j < S / 4; j++)
      d[j] = (uint32_t)age[4 * j] | (uint32_t)age[4 * j + 1] << 8 | (uint32_t)age[4 * j + 2] << 16 | (uint32_t)age[4 * j + 3] << 24;
    if constexpr (S == 8) *reinterpret_cast<uint2 *>(pa) = make_uint2(d[0], d[1]);
    else *reinterpret_cast<uint32_t *>(pa) = d[0];
  } else {
#pragma unroll
    for (int k = 0; k < S; k++) if (xs + k >= 0 && xs + k < width) pa[k] = (uint8_t)age[k];
  }
}

template <int Enc>
void launch(int width, int height, int frames, const void *src, int step, float unit, const TemporalArgs &a, bool fresh, float *state_s,
            uint8_t *state_age, void *dst, hipStream_t s) {
  constexpr int S = 16 / kBytes<Enc>;
  const int runs = (width + S - 1) / S + 1;
  const dim3 grid((runs + kRuns - 1) / kRuns, (height + kRows - 1) / kRows);
  hipLaunchKernelGGL((k_depth_temporal<Enc>), grid, dim3(kBlock), 0, s, width, height, runs, frames, static_cast<const uint8_t *>(src),
                     (size_t)step * height, step, unit, a, fresh ? 1 : 0, state_s, state_age, static_cast<uint8_t *>(dst));
}

}  // namespace

void launch_depth_temporal(int encoding, int width, int height, int frames, const void *src, int step, float unit, const ModDepthTemporal &t,
                           bool fresh, float *state_s, uint8_t *state_age, void *dst, hipStream_t s) {
  const TemporalArgs a{t.alpha, t.delta_abs, t.delta_rel, t.hold};
  if (encoding == MOD_DEPTH_16UC1) launch<MOD_DEPTH_16UC1>(width, height, frames, src, step, unit, a, fresh, state_s, state_age, dst, s);
  else launch<MOD_DEPTH_32FC1>(width, height, frames, src, step, unit, a, fresh, state_s, state_age, dst, s);
}
