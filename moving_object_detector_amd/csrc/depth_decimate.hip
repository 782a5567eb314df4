// depth_decimate.hip — the opt-in decimation of depth messages, the last message-to-message stage of the depth path: behind
// k_depth_temporal and in front of k_depth_to_disparity (mod_set_depth_decimation).
//
// k_depth_decimate<Encoding, DX, DY> maps `frames` depth messages (row pitch `step`, frames frame_bytes apart) to PACKED messages of
// out_w x out_h samples of the same encoding by the rule of include/mod_sf.h: output sample (X, Y) reads the DX x DY block of message
// pixels at (x0 + DX X, y0 + DY Y) and becomes the input word of the block's lower median by (z, row-major index) over its valid samples
// (MEDIAN), of the first element of that order (MIN), enc of the mean of the raw values of the valid samples within
// t = tol_abs + tol_rel * a of the median's z (MEAN, summed in row-major order), or the block's top-left word (NEAREST); a block with
// fewer than max(min_valid, 1) valid samples becomes the encoding's "no reading" word.  DX = DY = 1 copies the window.
//
// Memory-bound: DX DY B bytes read and B written per output sample; no LDS, no atomics; frames in blockIdx.z.
//   * k_depth_filter's grid of runs: a lane owns the 16 / B consecutive output samples of one row that lie between two 16-byte
//     boundaries of the OUTPUT row (8 of 16UC1, 4 of 32FC1), so a row interior is one aligned 16-byte store; `head`, the samples in
//     front of a row's first boundary, is per row, and the ends of a row take the element path.  Consecutive lanes own consecutive
//     runs: a wave reads one contiguous span of each of its DY input rows.
//   * A run's input is DY spans of 16 DX bytes.  Where a span starts on a 16-byte boundary (packed aligned messages with x0 = 0 do) it
//     is DX 16-byte loads, else element loads; both land in the same DY x 4 DX dwords of registers.
//   * Everything is unrolled over the template's (DX, DY): the block's up to 16 samples are named registers, and the median is picked
//     by rank counting, rank(n) = #{m valid: z_m < z_n or (z_m == z_n and m < n)}, with selects: no private array is indexed at run time.
#include "mod_launch.h"

namespace {

constexpr int kRuns = 64, kRows = 4, kBlock = kRuns * kRows;   // a wave is 64 consecutive runs of one output row

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

struct DecimateArgs { int mode, min_valid; float tol_abs, tol_rel; };   // min_valid: already max(min_valid, 1)

// The rule for one block: w[n], n row-major (j ascending, then i ascending)
template <int Enc, int N>
__device__ __forceinline__ typename Word<Enc>::type decimate_block(const typename Word<Enc>::type (&w)[N], float unit, const DecimateArgs &a) {
  using T = typename Word<Enc>::type;
  constexpr T kNoReading = Enc == MOD_DEPTH_16UC1 ? (T)0 : (T)0x7fc00000u;
  if (a.mode == MOD_DEPTH_DECIMATE_NEAREST) return w[0];
  float x[N], z[N];
  bool v[N];
  int count = 0;
#pragma unroll
  for (int n = 0; n < N; n++) {
    x[n] = word_x<Enc>(w[n]);
    z[n] = x[n] * unit;
    v[n] = valid0(z[n]);
    count += v[n] ? 1 : 0;
  }
  if (count < a.min_valid) return kNoReading;
  const int target = a.mode == MOD_DEPTH_DECIMATE_MIN ? 0 : (count - 1) >> 1;
  T pick = w[0];
  float za = 0.0f;
#pragma unroll
  for (int n = 0; n < N; n++) {
    int rank = 0;
#pragma unroll
    for (int m = 0; m < N; m++) {
      if (m == n) continue;
      const bool before = m < n ? z[m] <= z[n] : z[m] < z[n];   // (z, row-major index) ascending
      rank += v[m] && before ? 1 : 0;
    }
    const bool hit = v[n] && rank == target;                    // exactly one n
    pick = hit ? w[n] : pick;
    za = hit ? z[n] : za;
  }
  if (a.mode != MOD_DEPTH_DECIMATE_MEAN) return pick;
  const float t = a.tol_abs + a.tol_rel * za;
  float sum = 0.0f;
  int members = 0;
#pragma unroll
  for (int n = 0; n < N; n++) {                                 // row-major: the rule's order, not to be reassociated
    const bool member = v[n] && fabsf(z[n] - za) <= t;
    sum = member ? sum + x[n] : sum;
    members += member ? 1 : 0;
  }
  return enc<Enc>(sum / (float)members);                        // (the median is a member: members >= 1)
}

//   runs   runs per output row: (out_w + S - 1) / S + 1 (run r covers X in [head + S (r - 1), head + S r))
//   src    message pixel (x0, y0) of frame 0: the blocks start there
template <int Enc, int DX, int DY>
__global__ __launch_bounds__(kBlock) void k_depth_decimate(int out_w, int out_h, int runs, const uint8_t *__restrict__ src, size_t frame_bytes, int step,
                                                           float unit, DecimateArgs a, uint8_t *__restrict__ dst) {
  using T = typename Word<Enc>::type;
  constexpr int B = kBytes<Enc>, S = 16 / B, N = DX * DY;
  constexpr int kPerDword = 4 / B;             // samples a dword holds
  const int r = blockIdx.x * kRuns + threadIdx.x % kRuns, Y = blockIdx.y * kRows + threadIdx.x / kRuns, f = blockIdx.z;
  if (r >= runs || Y >= out_h) return;
  const size_t out_step = (size_t)out_w * B;
  uint8_t *out = dst + ((size_t)f * out_h + Y) * out_step;
  const int head = (int)((0u - (uint32_t)(uintptr_t)out) & 15u) / B;
  const int Xs = head + (r - 1) * S;
  if (Xs >= out_w || Xs + S <= 0) return;
  const bool whole = Xs >= 0 && Xs + S <= out_w;
  const uint8_t *in = src + (size_t)f * frame_bytes + (size_t)(DY * Y) * step + (ptrdiff_t)(DX * Xs) * B;   // (read only where X is inside the row)

  // the run's input: DY spans of DX * S samples, as DX * 4 dwords each
  uint32_t raw[DY][4 * DX];
#pragma unroll
  for (int j = 0; j < DY; j++) {
    const uint8_t *span = in + (size_t)j * step;
    if (whole && ((uintptr_t)span & 15u) == 0) {
#pragma unroll
      for (int q = 0; q < DX; q++) {
        const uint4 d = reinterpret_cast<const uint4 *>(span)[q];
        raw[j][4 * q] = d.x; raw[j][4 * q + 1] = d.y; raw[j][4 * q + 2] = d.z; raw[j][4 * q + 3] = d.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4 * DX; q++) {
        uint32_t d = 0;
#pragma unroll
        for (int e = 0; e < kPerDword; e++) {
          const int X = Xs + (q * kPerDword + e) / DX;          // the output sample this input sample belongs to
          if (X >= 0 && X < out_w) d |= (uint32_t)reinterpret_cast<const T *>(span)[q * kPerDword + e] << (e * 8 * B);
        }
        raw[j][q] = d;
      }
    }
  }

  T o[S];
#pragma unroll
  for (int k = 0; k < S; k++) {
    T w[N];
#pragma unroll
    for (int j = 0; j < DY; j++)
#pragma unroll
      for (int i = 0; i < DX; i++) {
        const int s = k * DX + i;                               // sample of the span
        w[j * DX + i] = (T)(raw[j][s / kPerDword] >> ((s % kPerDword) * 8 * B));
      }
    o[k] = decimate_block<Enc, N>(w, unit, a);
  }

  if (whole) {
    uint4 q;
    if constexpr (B == 2) {
      q.x = (uint32_t)o[0] | (uint32_t)o[1] << 16; q.y = (uint32_t)o[2] | (uint32_t)o[3] << 16;
      q.z = (uint32_t)o[4] | (uint32_t)o[5] << 16; q.w = (uint32_t)o[6] | (uint32_t)o[7] << 16;
    } else {
      q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
    }
    *reinterpret_cast<uint4 *>(__builtin_assume_aligned(out + (size_t)Xs * B, 16)) = q;
    return;
  }
#pragma unroll
  for (int k = 0; k < S; k++) {
    const int X = Xs + k;
    if (X >= 0 && X < out_w) *reinterpret_cast<T *>(out + (size_t)X * B) = o[k];
  }
}

struct Launch {
  int out_w, out_h, frames, step;
  const uint8_t *src;
  size_t frame_bytes;
  float unit;
  DecimateArgs a;
  uint8_t *dst;
  hipStream_t s;
};

template <int Enc, int DX, int DY>
void launch(const Launch &l) {
  constexpr int S = 16 / kBytes<Enc>;
  const int runs = (l.out_w + S - 1) / S + 1;
  const dim3 grid((runs + kRuns - 1) / kRuns, (l.out_h + kRows - 1) / kRows, l.frames);
  hipLaunchKernelGGL((k_depth_decimate<Enc, DX, DY>), grid, dim3(kBlock), 0, l.s, l.out_w, l.out_h, runs, l.src, l.frame_bytes, l.step, l.unit, l.a, l.dst);
}

template <int Enc, int DX>
void launch_dy(int dy, const Launch &l) {
  if (dy == 1) launch<Enc, DX, 1>(l);
  else if (dy == 2) launch<Enc, DX, 2>(l);
  else if (dy == 3) launch<Enc, DX, 3>(l);
  else launch<Enc, DX, 4>(l);
}

template <int Enc>
void launch_dx(int dx, int dy, const Launch &l) {
  if (dx == 1) launch_dy<Enc, 1>(dy, l);
  else if (dx == 2) launch_dy<Enc, 2>(dy, l);
  else if (dx == 3) launch_dy<Enc, 3>(dy, l);
  else launch_dy<Enc, 4>(dy, l);
}

}  // namespace

void launch_depth_decimate(int encoding, int out_w, int out_h, int frames, const void *src, size_t frame_bytes, int step, int x0, int y0, float unit,
                           const ModDepthDecimation &d, void *dst, hipStream_t s) {
  const bool off = d.dx * d.dy == 1;             // a copy of the window: one sample a block, whatever it is
  const DecimateArgs a{off ? MOD_DEPTH_DECIMATE_NEAREST : d.mode, d.min_valid > 1 ? d.min_valid : 1, d.tol_abs, d.tol_rel};
  const uint8_t *first = static_cast<const uint8_t *>(src) + (size_t)y0 * step + (size_t)x0 * depth_bytes(encoding);
  const Launch l{out_w, out_h, frames, step, first, frame_bytes, unit, a, static_cast<uint8_t *>(dst), s};
  if (encoding == MOD_DEPTH_16UC1) launch_dx<MOD_DEPTH_16UC1>(d.dx, d.dy, l);
  else launch_dx<MOD_DEPTH_32FC1>(d.dx, d.dy, l);
}
