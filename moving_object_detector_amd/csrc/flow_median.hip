// flow_median.hip — the NaN-aware median filter of a finished flow (mod_set_flow_median, mod_flow_median_dev; include/mod_sf.h states
// the rule, DESIGN.md §3.5c where it sits; tests/models/flow_median_model.py restates it):
//   a pixel is VALID when both components are finite; S = the valid pixels of the w x w square round p, clipped to the image; n = |S|
//   p invalid: out = in, bit for bit          p valid and n < min_valid: out = (NaN, NaN), both words 0x7fc00000
//   else out.x / out.y = the element (n - 1) / 2, in ascending order of the key k(b) = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000), of the
//   x / y words of S, each component on its own
//
// k_flow_median<WINDOW>: one workgroup (4 waves) per 64 x 16 tile, frames in grid.z, r = (WINDOW - 1) / 2 — k_corner's shape.
//   A  the flow tile with r halo columns and rows, read as float2 (consecutive lanes, consecutive 8 bytes), into LDS as the two KEYS of
//      every cell, one uint32 plane per component ((64 + 2 r) x (16 + 2 r) x 4 bytes each: 9504 bytes at window 3, 10880 at window 5).
//      An invalid cell and a cell outside the image hold kSentinel = 0xFFFFFFFF in both planes: no finite float has that key (its bits
//      would be 0x7FFFFFFF, a NaN), it sorts last, and n is the number of cells of the window that do not hold it.  No load leaves the
//      plane: a cell outside the image is not loaded.
//   B  a lane owns one column and four rows.  Per pixel and component it reads the WINDOW^2 keys (consecutive lanes, consecutive
//      dwords: 32 different banks in either half of the wave), runs them through Batcher's merge-exchange network — the pairs are
//      compile-time constants, the keys stay in registers, and the compiler drops every exchange that only feeds ranks above the
//      middle, which no n can ask for — and picks rank (n - 1) / 2 with a chain of selects, never with an indexed register array.
//      The sentinels lie behind the n valid keys, so that rank of all WINDOW^2 keys is the lower median of the valid ones.
//   C  an invalid centre is the one case that needs the input's own bits: its lane reads them again from the input plane.
// Input and output are different planes (checked by the caller); every pixel of the output is stored, 8 bytes, plain vector stores.
#include "mod_launch.h"

#include <utility>

namespace {

constexpr int kMedTileW = 64, kMedTileH = 16;
constexpr uint32_t kSentinel = 0xFFFFFFFFu, kNanBits = 0x7fc00000u;

struct MedianArgs {
  int W, H, min_valid;
  const float2 *in;         // [F][H][W]
  float2 *out;              // [F][H][W], not `in`
};

__device__ inline uint32_t flow_key(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ inline bool finite_bits(uint32_t b) { return (b & 0x7F800000u) != 0x7F800000u; }

// Batcher's merge exchange (Knuth 5.2.2, algorithm M) for N keys, as a list of pairs (a < b): after exchange (a, b) wire a holds the
// smaller key.  Sorts any N; tests/test_flow_median_model.py runs this construction over every 0/1 input.
template <int N> struct Network { int a[N * N], b[N * N], count; };
template <int N> constexpr Network<N> merge_exchange() {
  Network<N> net{};
  int t = 1;
  while ((1 << t) < N) t++;
  for (int p = 1 << (t - 1); p > 0; p >>= 1) {
    int q = 1 << (t - 1), r = 0, d = p;
    while (true) {
      for (int i = 0; i < N - d; i++)
        if ((i & p) == r) { net.a[net.count] = i; net.b[net.count] = i + d; net.count++; }
      if (q == p) break;
      d = q - p; q >>= 1; r = p;
    }
  }
  return net;
}

template <int A, int B, int N> __device__ inline void exchange(uint32_t (&v)[N]) {
  const uint32_t lo = min(v[A], v[B]), hi = max(v[A], v[B]);
  v[A] = lo;
  v[B] = hi;
}

template <int N, size_t... I> __device__ inline void sort_keys(uint32_t (&v)[N], std::index_sequence<I...>) {
  constexpr Network<N> net = merge_exchange<N>();
  (exchange<net.a[I], net.b[I]>(v), ...);
}

// rank `rank` (0 .. N / 2) of the N keys of one component round (row, col) of its plane: compile-time indices only
template <int WINDOW, int COLS> __device__ inline uint32_t ranked(const uint32_t (*plane)[COLS], int row, int col, int rank) {
  constexpr int N = WINDOW * WINDOW;
  uint32_t v[N];
#pragma unroll
  for (int j = 0; j < WINDOW; j++)
#pragma unroll
    for (int i = 0; i < WINDOW; i++) v[j * WINDOW + i] = plane[row + j][col + i];
  sort_keys<N>(v, std::make_index_sequence<merge_exchange<N>().count>{});
  uint32_t k = v[0];
#pragma unroll
  for (int i = 1; i <= N / 2; i++) k = rank == i ? v[i] : k;
  return k;
}

template <int WINDOW>
__global__ __launch_bounds__(256) void k_flow_median(MedianArgs a) {
  constexpr int R = (WINDOW - 1) / 2, kCols = kMedTileW + 2 * R, kRows = kMedTileH + 2 * R;
  __shared__ uint32_t sx[kRows][kCols], sy[kRows][kCols];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int x0 = blockIdx.x * kMedTileW, y0 = blockIdx.y * kMedTileH;
  const size_t fN = (size_t)blockIdx.z * a.W * a.H;
  const uint2 *const in = reinterpret_cast<const uint2 *>(a.in) + fN;
  // ---- A: (sx, sy)[j][k] = the keys of (x0 - R + k, y0 - R + j); the sentinel where that is invalid or outside the image ------------
  for (int i = tid; i < kRows * kCols; i += 256) {
    const int j = i / kCols, k = i - j * kCols;
    const int x = x0 - R + k, y = y0 - R + j;
    uint32_t kx = kSentinel, ky = kSentinel;
    if (x >= 0 && x < a.W && y >= 0 && y < a.H) {
      const uint2 w = in[(size_t)y * a.W + x];
      if (finite_bits(w.x) && finite_bits(w.y)) { kx = flow_key(w.x); ky = flow_key(w.y); }
    }
    sx[j][k] = kx;
    sy[j][k] = ky;
  }
  __syncthreads();
  // ---- B, C: pixels (x0 + lane, y0 + 4 wv + i) -----------------------------------------------------------------------------------------
  const int x = x0 + lane;
  if (x >= a.W) return;
#pragma unroll 1
  for (int i = 0; i < kMedTileH / 4; i++) {
    const int ly = wv * (kMedTileH / 4) + i, y = y0 + ly;
    if (y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    uint2 o;
    if (sx[ly + R][lane + R] == kSentinel) {
      o = in[p];
    } else {
      int n = 0;
#pragma unroll
      for (int j = 0; j < WINDOW; j++)
#pragma unroll
        for (int k = 0; k < WINDOW; k++) n += sx[ly + j][lane + k] != kSentinel;
      if (n < a.min_valid) {
        o = make_uint2(kNanBits, kNanBits);
      } else {
        const int rank = (n - 1) >> 1;
        const uint32_t kx = ranked<WINDOW, kCols>(sx, ly, lane, rank), ky = ranked<WINDOW, kCols>(sy, ly, lane, rank);
        // the key's inverse: a key with the top bit set came from a non-negative float
        o = make_uint2(kx ^ ((kx >> 31) ? 0x80000000u : 0xFFFFFFFFu), ky ^ ((ky >> 31) ? 0x80000000u : 0xFFFFFFFFu));
      }
    }
    reinterpret_cast<uint2 *>(a.out)[fN + p] = o;
  }
}

}  // namespace

void launch_flow_median(int W, int H, int frames, int window, int min_valid, const float *in, float *out, hipStream_t s) {
  const MedianArgs a{W, H, min_valid, reinterpret_cast<const float2 *>(in), reinterpret_cast<float2 *>(out)};
  const dim3 grid((W + kMedTileW - 1) / kMedTileW, (H + kMedTileH - 1) / kMedTileH, frames);
  if (window == 3) hipLaunchKernelGGL(k_flow_median<3>, grid, dim3(256), 0, s, a);
  else if (window == 5) hipLaunchKernelGGL(k_flow_median<5>, grid, dim3(256), 0, s, a);
}
