// rectify.hip — raw camera images to rectified grey planes: what image_proc's rectifier (cv::initUndistortRectifyMap +
// cv::remap, INTER_LINEAR on the 1/32-pixel grid, BORDER_CONSTANT) and cv_bridge's MONO8 conversion do on the CPU ahead of the
// reference's constructor node.  include/mod_sf.h states the formula; tests/models/rectify_model.py restates it bit for bit.
//
// k_rectify_map (f64, the arithmetic of rectify_map.h, either distortion model): for every pixel of the context's W x H window of
// the RECTIFIED image, where it lies in the raw message, in 1/32 pixel: int32 [H][W][2], 8 B/px in HBM.
// k_rectify: one lane makes a run of 4 consecutive output pixels of one row.  Runs are placed on the OUTPUT's dword grid, so a
// row interior is one aligned dword store per lane; a run cut by a row end stores bytes.  A workgroup covers 16 runs x 16 rows
// (64 pixels x 16 rows; a wave stores 4 rows of 64 contiguous bytes).  Per pixel: the map entry, four taps of the raw message (a
// tap outside it reads 0), the bilinear weights in integers per channel, then grey.  The taps come by one of two paths:
//   direct  the two taps of a message row in one load of 2 C bytes when both lie inside the message, byte by byte where it ends;
//           the message row that is `bottom` for one output row is `top` for the next row of the same wave.  The product's path.
//   staged  a rectification map is smooth, so the taps of a tile fall into a small box of the message: the workgroup reduces the
//           box from its map entries (wave shuffles, one LDS exchange), copies it into LDS with coalesced aligned dword loads
//           (bytes singly only where a dword lies astride the message's first or last byte) and takes every tap from there; a box
//           that does not fit 16 KiB is gathered directly.  Compiled out of the product until it has been timed (kStagedDefault).
// Nothing outside the `extent` bytes of a message is loaded (height * step; for the right pane of a side-by-side message, which
// starts width * C bytes into it, that much less).  C source bytes + 8 map bytes + 1 per pixel; no atomics; frames in
// blockIdx.z.
#include "image_fmt.h"
#include "rectify_map.h"

#include <climits>
#include <cmath>
#include <cstring>

namespace {

constexpr int kRun = 4;        // output pixels per lane
constexpr int kTileRuns = 16;  // runs (lanes) of a workgroup along x ...
constexpr int kTileRows = 16;  // ... and rows
constexpr int kBlock = kTileRuns * kTileRows;

// the 2 C bytes of two neighbouring pixels at p (any byte alignment), B, G, R (or the one grey channel) of each into t0 / t1
template <int Enc, int NC>
__device__ __forceinline__ void load_pair(const uint8_t *p, uint32_t (&t0)[NC], uint32_t (&t1)[NC]) {
  using F = Fmt<Enc>;
  if constexpr (F::mono && F::C == 1) {
    uint16_t w;
    __builtin_memcpy(&w, p, 2);
    t0[0] = w & 0xffu; t1[0] = w >> 8;
  } else if constexpr (F::mono) {                  // pitch 2: the grey bytes of the pair are bytes y and 2 + y of its four
    static_assert(F::C == 2, "one grey channel at pitch 1 or 2");
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    t0[0] = (w >> (8 * F::y)) & 0xffu; t1[0] = (w >> (8 * (F::C + F::y))) & 0xffu;
  } else {
    uint64_t w = 0;
    if constexpr (F::C == 4) __builtin_memcpy(&w, p, 8);
    else { uint32_t lo; uint16_t hi; __builtin_memcpy(&lo, p, 4); __builtin_memcpy(&hi, p + 4, 2); w = lo | ((uint64_t)hi << 32); }
    t0[0] = (uint32_t)(w >> (8 * F::b)) & 0xffu; t0[1] = (uint32_t)(w >> (8 * F::g)) & 0xffu; t0[2] = (uint32_t)(w >> (8 * F::r)) & 0xffu;
    t1[0] = (uint32_t)(w >> (8 * (F::C + F::b))) & 0xffu; t1[1] = (uint32_t)(w >> (8 * (F::C + F::g))) & 0xffu;
    t1[2] = (uint32_t)(w >> (8 * (F::C + F::r))) & 0xffu;
  }
}

template <int Enc, int NC>
__device__ __forceinline__ void load_one(const uint8_t *p, uint32_t (&t)[NC]) {
  using F = Fmt<Enc>;
  if constexpr (F::mono) t[0] = p[F::y];
  else { t[0] = p[F::b]; t[1] = p[F::g]; t[2] = p[F::r]; }
}

// the bilinear weights in integers per channel, then grey; t[row][column][channel], a tap outside the message is 0
template <int Enc, int NC>
__device__ __forceinline__ uint32_t interpolate(const uint32_t (&t)[2][2][NC], uint32_t ax, uint32_t ay) {
  uint32_t v[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) {
    const uint32_t top = (32u - ax) * t[0][0][k] + ax * t[0][1][k];
    const uint32_t bot = (32u - ax) * t[1][0][k] + ax * t[1][1][k];
    v[k] = ((32u - ay) * top + ay * bot + 512u) >> 10;
  }
  if constexpr (NC == 1) return v[0];
  else return grey(v[0], v[1], v[2]);
}

// one output pixel by direct gathers: the grey value at (qx, qy) / 32 of the width x height message at msg (row pitch step)
template <int Enc>
__device__ __forceinline__ uint32_t rect_pixel(const uint8_t *__restrict__ msg, int step, int width, int height, int qx, int qy) {
  using F = Fmt<Enc>;
  constexpr int C = F::C, NC = F::mono ? 1 : 3;
  const int ix = qx >> 5, iy = qy >> 5;
  const bool in0 = (unsigned)ix < (unsigned)width, in1 = (unsigned)(ix + 1) < (unsigned)width;
  uint32_t t[2][2][NC] = {};
  if (in0 || in1) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int yy = iy + r;
      if ((unsigned)yy >= (unsigned)height) continue;
      const uint8_t *row = msg + (size_t)yy * step;
      if (in0 && in1) load_pair<Enc, NC>(row + (size_t)ix * C, t[r][0], t[r][1]);
      else if (in0) load_one<Enc, NC>(row + (size_t)ix * C, t[r][0]);
      else load_one<Enc, NC>(row + (size_t)(ix + 1) * C, t[r][1]);
    }
  }
  return interpolate<Enc, NC>(t, (uint32_t)qx & 31u, (uint32_t)qy & 31u);
}

// ---- the staged path: the workgroup's source box in LDS ------------------------------------------------------------------------
constexpr int kTileDwords = 4096;   // 16 KiB: a 64 x 16 tile of a 1080p bgra8 map with 0.8 of the focal length needs about 7

// The box of message pixels a workgroup's taps touch: columns x0 .. x1, rows y0 .. y1, all inside the message (x1 < x0: none).
struct Box { int x0, x1, y0, y1; };

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}

// B, G, R (or grey) of the pixel whose first byte is byte `at` of the 8 bytes in w
template <int Enc, int NC>
__device__ __forceinline__ void unpack(uint64_t w, int at, uint32_t (&t)[NC]) {
  using F = Fmt<Enc>;
  if constexpr (F::mono) t[0] = (uint32_t)(w >> (8 * (at + F::y))) & 0xffu;
  else {
    t[0] = (uint32_t)(w >> (8 * (at + F::b))) & 0xffu; t[1] = (uint32_t)(w >> (8 * (at + F::g))) & 0xffu;
    t[2] = (uint32_t)(w >> (8 * (at + F::r))) & 0xffu;
  }
}

// one output pixel from the staged box.  Row r of the box lies at tile + r * pitch dwords, in the byte phase of its global
// address: byte (phase0 + r * step) & 3 of the row's first dword is the first byte of column box.x0
template <int Enc>
__device__ __forceinline__ uint32_t rect_pixel_lds(const uint32_t *tile, int pitch, uint32_t phase0, int step, const Box &box, int width,
                                                   int height, int qx, int qy) {
  using F = Fmt<Enc>;
  constexpr int C = F::C, NC = F::mono ? 1 : 3;
  const int ix = qx >> 5, iy = qy >> 5;
  const bool in0 = (unsigned)ix < (unsigned)width, in1 = (unsigned)(ix + 1) < (unsigned)width;
  uint32_t t[2][2][NC] = {};
  if (in0 || in1) {
    const int xq = in0 ? ix : ix + 1;             // the first column read: inside the message, hence inside the box
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int yy = iy + r;
      if ((unsigned)yy >= (unsigned)height) continue;
      const int br = yy - box.y0;
      const uint32_t at = ((phase0 + (uint32_t)br * (uint32_t)step) & 3u) + (uint32_t)(xq - box.x0) * C;
      const uint32_t *d = tile + br * pitch + (at >> 2);
      const uint32_t sh = at & 3u;
      const uint32_t lo = __builtin_amdgcn_alignbyte(d[1], d[0], sh);
      const uint32_t hi = 2 * C <= 4 ? 0u : __builtin_amdgcn_alignbyte(d[2], d[1], sh);   // (bytes past the row's are shifted in, never used)
      const uint64_t w = lo | ((uint64_t)hi << 32);
      if (in0) unpack<Enc, NC>(w, 0, t[r][0]);
      if (in1) unpack<Enc, NC>(w, in0 ? C : 0, t[r][1]);
    }
  }
  return interpolate<Enc, NC>(t, (uint32_t)qx & 31u, (uint32_t)qy & 31u);
}

//   runs         runs per row: (W + 3) / 4 + 1 (run r covers x in [head + 4 (r - 1), head + 4 r), head = pixels of the row in front
//                of the output's first dword boundary)
//   frame_bytes  step * height, the distance between two frames;  extent: the bytes that may be loaded from a frame's first one (the
//                same, or less for a pane that starts inside the message);  width, height: of the message (pane);  map [H][W] (qx, qy)
//   Staged       the workgroup first copies the box of message bytes its taps touch into LDS with coalesced aligned dword loads
//                and samples from there; a box that does not fit kTileDwords (a map that is far from smooth) is gathered directly
template <int Enc, bool Staged>
__global__ __launch_bounds__(kBlock) void k_rectify(int W, int H, int runs, const uint8_t *__restrict__ src, size_t frame_bytes, size_t extent,
                                                    int step, int width, int height, const int2 *__restrict__ map, uint8_t *__restrict__ dst) {
  constexpr int C = Fmt<Enc>::C;
  const int r = blockIdx.x * kTileRuns + threadIdx.x % kTileRuns;
  const int y = blockIdx.y * kTileRows + threadIdx.x / kTileRuns;
  const bool live = r < runs && y < H;
  if (!Staged && !live) return;
  const uint8_t *msg = src + (size_t)blockIdx.z * frame_bytes;
  uint8_t *out = dst + ((size_t)blockIdx.z * H + (live ? y : 0)) * W;
  const int head = (int)((0u - (uint32_t)(uintptr_t)out) & (uint32_t)(kRun - 1));
  const int xs = head + (r - 1) * kRun;
  int2 q[kRun];
  bool ok[kRun];
#pragma unroll
  for (int k = 0; k < kRun; k++) {
    ok[k] = live && xs + k >= 0 && xs + k < W;
    q[k] = ok[k] ? map[(size_t)y * W + xs + k] : make_int2(0, 0);
  }
  uint32_t px[kRun];
  bool staged = false;
  if constexpr (Staged) {
    __shared__ uint32_t tile[kTileDwords];
    __shared__ int part[kBlock / 64][4];
    // the box: every tap of every pixel that lies inside the message (kept as minima: x0, -x1, y0, -y1)
    int b[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
#pragma unroll
    for (int k = 0; k < kRun; k++) {
      const int ix = q[k].x >> 5, iy = q[k].y >> 5;
      const int xa = max(ix, 0), xb = min(ix + 1, width - 1), ya = max(iy, 0), yb = min(iy + 1, height - 1);
      if (ok[k] && xa <= xb && ya <= yb) { b[0] = min(b[0], xa); b[1] = min(b[1], -xb); b[2] = min(b[2], ya); b[3] = min(b[3], -yb); }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) b[j] = wave_min(b[j]);
    if (threadIdx.x % 64 == 0)
      for (int j = 0; j < 4; j++) part[threadIdx.x / 64][j] = b[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) b[j] = min(min(part[0][j], part[1][j]), min(part[2][j], part[3][j]));
    const Box box{b[0], -b[1], b[2], -b[3]};
    if (box.x0 == INT_MAX) {                       // no tap inside the message: the whole tile is border
#pragma unroll
      for (int k = 0; k < kRun; k++) px[k] = 0;
      staged = true;
    } else {
      const int rows = box.y1 - box.y0 + 1, row_bytes = (box.x1 - box.x0 + 1) * C;
      const int nd = (row_bytes + 3) / 4 + 1;      // dwords that cover a row in any byte phase
      const int pitch = nd + 2;                    // ... and the two a sample at the row's end reads beyond them
      const uint8_t *first = msg + (size_t)box.y0 * step + (size_t)box.x0 * C;
      const uint32_t phase0 = (uint32_t)(uintptr_t)first & 3u;
      staged = (long long)rows * pitch <= kTileDwords;   // (uniform: the box is the workgroup's)
      if (staged) {
        const uint8_t *end = msg + extent;
        for (int i = threadIdx.x; i < rows * nd; i += kBlock) {
          const int br = i / nd, d = i - br * nd;
          const uint8_t *a0 = first + (size_t)br * step;                     // the row's first byte
          const uint8_t *g = a0 - ((uintptr_t)a0 & 3u) + 4 * d;              // this dword, aligned
          uint32_t w = 0;
          if (g + 4 > a0 && g < a0 + row_bytes) {                            // it holds bytes of the row
            if (g >= msg && g + 4 <= end) w = *reinterpret_cast<const uint32_t *>(__builtin_assume_aligned(g, 4));
            else {                                                           // astride the message's first or last byte
#pragma unroll
              for (int j = 0; j < 4; j++)
                if (g + j >= msg && g + j < end) w |= (uint32_t)g[j] << (8 * j);
            }
          }
          tile[br * pitch + d] = w;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kRun; k++)
          px[k] = ok[k] ? rect_pixel_lds<Enc>(tile, pitch, phase0, step, box, width, height, q[k].x, q[k].y) : 0u;
      }
    }
    if (!live) return;
  }
  if (!staged) {
#pragma unroll
    for (int k = 0; k < kRun; k++) px[k] = ok[k] ? rect_pixel<Enc>(msg, step, width, height, q[k].x, q[k].y) : 0u;
  }
  if (ok[0] && ok[kRun - 1]) {
    *reinterpret_cast<uint32_t *>(__builtin_assume_aligned(out + xs, 4)) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    return;
  }
#pragma unroll
  for (int k = 0; k < kRun; k++)
    if (ok[k]) out[xs + k] = (uint8_t)px[k];
}

// measurement builds (tools/time_rectify.py, `make EXTRA=-DMOD_RECTIFY_DIRECT OUT=...` / `EXTRA=-DMOD_RECTIFY_STAGED OUT=...`) pin the
// path; the product takes kStagedDefault
[[maybe_unused]] constexpr bool kStagedDefault = false;   // one timing so far, and it is mixed: the direct path stays
#if defined(MOD_RECTIFY_DIRECT)
constexpr bool kStaged = false;
#elif defined(MOD_RECTIFY_STAGED)
constexpr bool kStaged = true;
#else
constexpr bool kStaged = kStagedDefault;
#endif

template <int Enc>
void launch(int W, int H, int frames, const uint8_t *src, size_t frame_bytes, size_t extent, int step, int width, int height,
            const int32_t *map, uint8_t *dst, hipStream_t s) {
  const int runs = (W + kRun - 1) / kRun + 1;
  const dim3 grid((unsigned)((runs + kTileRuns - 1) / kTileRuns), (unsigned)((H + kTileRows - 1) / kTileRows), (unsigned)frames);
  hipLaunchKernelGGL((k_rectify<Enc, kStaged>), grid, dim3(kBlock), 0, s, W, H, runs, src, frame_bytes, extent, step, width, height,
                     reinterpret_cast<const int2 *>(map), dst);
}

// ---- the map itself: rectify_map.h's arithmetic, one lane per entry ----------------------------------------------------------------
// A workgroup is 64 x 4 entries: the lanes of a wave run along a row, so a wave's 8-byte (qx, qy) stores are one contiguous run of
// 512 bytes.  The calibration comes by value in the kernel arguments; pure f64 VALU work, no LDS, no atomics, nothing is loaded.
constexpr int kMapCols = 64, kMapRows = 4;

template <int Model>
__global__ __launch_bounds__(kMapCols * kMapRows) void k_rectify_map(ModRectifyCamera cam, int x0, int y0, int W, int H, int2 *__restrict__ map) {
  const int u = blockIdx.x * kMapCols + threadIdx.x, v = blockIdx.y * kMapRows + threadIdx.y;
  if (u >= W || v >= H) return;
  int32_t qx, qy;
  rectify_map::entry<Model>(cam, (double)(u + x0), (double)(v + y0), qx, qy);
  map[(size_t)v * W + u] = make_int2(qx, qy);
}

}  // namespace

void launch_rectify(int encoding, int W, int H, int frames, const uint8_t *src, size_t frame_bytes, size_t extent, int step, int width,
                    int height, const int32_t *map, uint8_t *dst, hipStream_t s) {
  switch (encoding) {
    case MOD_ENCODING_MONO8: launch<MOD_ENCODING_MONO8>(W, H, frames, src, frame_bytes, extent, step, width, height, map, dst, s); break;
    case MOD_ENCODING_BGR8:  launch<MOD_ENCODING_BGR8>(W, H, frames, src, frame_bytes, extent, step, width, height, map, dst, s); break;
    case MOD_ENCODING_RGB8:  launch<MOD_ENCODING_RGB8>(W, H, frames, src, frame_bytes, extent, step, width, height, map, dst, s); break;
    case MOD_ENCODING_BGRA8: launch<MOD_ENCODING_BGRA8>(W, H, frames, src, frame_bytes, extent, step, width, height, map, dst, s); break;
    case MOD_ENCODING_RGBA8: launch<MOD_ENCODING_RGBA8>(W, H, frames, src, frame_bytes, extent, step, width, height, map, dst, s); break;
    case MOD_ENCODING_YUV422: launch<MOD_ENCODING_YUV422>(W, H, frames, src, frame_bytes, extent, step, width, height, map, dst, s); break;
    case MOD_ENCODING_YUV422_YUY2: launch<MOD_ENCODING_YUV422_YUY2>(W, H, frames, src, frame_bytes, extent, step, width, height, map, dst, s); break;
    default: break;
  }
}

// cv::initUndistortRectifyMap (model 0) / cv::fisheye::initUndistortRectifyMap (model 1) for the W x H window at (x0, y0) of the
// rectified image, on cv::remap's 1/32-pixel grid: map [H][W] (qx, qy) on the device, enqueued on s.  Every operation in the order
// include/mod_sf.h states (the Makefile's -ffp-contract=off keeps products and sums apart), so that numpy reproduces every bit.
hipError_t launch_rectify_map(int model, const ModRectifyCamera &cam, int x0, int y0, int W, int H, int32_t *map, hipStream_t s) {
  const dim3 grid((unsigned)((W + kMapCols - 1) / kMapCols), (unsigned)((H + kMapRows - 1) / kMapRows)), block(kMapCols, kMapRows);
  int2 *q = reinterpret_cast<int2 *>(map);
  switch (model) {
    case MOD_DISTORTION_RATIONAL: hipLaunchKernelGGL(k_rectify_map<MOD_DISTORTION_RATIONAL>, grid, block, 0, s, cam, x0, y0, W, H, q); break;
    case MOD_DISTORTION_EQUIDISTANT: hipLaunchKernelGGL(k_rectify_map<MOD_DISTORTION_EQUIDISTANT>, grid, block, 0, s, cam, x0, y0, W, H, q); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

const char *check_distortion(int model, const ModRectifyCamera &cam) {
  if (model == MOD_DISTORTION_EQUIDISTANT)
    for (int i = 4; i < 8; i++)
      if (cam.D[i] != 0.0) return "rectification: the equidistant model takes D = k1 k2 k3 k4, D[4..7] must be 0";
  return nullptr;
}

const char *check_rectify_camera(const ModRectifyCamera &cam) {
  if (cam.width < 1 || cam.height < 1 || cam.width > MOD_MAX_WIDTH || cam.height > MOD_MAX_WIDTH)
    return "rectification: width and height must be in 1..MOD_MAX_WIDTH";
  for (const double v : cam.K) if (!std::isfinite(v)) return "rectification: non-finite entry in K";
  for (const double v : cam.D) if (!std::isfinite(v)) return "rectification: non-finite entry in D";
  for (const double v : cam.R) if (!std::isfinite(v)) return "rectification: non-finite entry in R";
  for (const double v : cam.P) if (!std::isfinite(v)) return "rectification: non-finite entry in P";
  if (cam.K[0] <= 0.0 || cam.K[4] <= 0.0) return "rectification: K's focal lengths must be positive";
  if (cam.P[0] <= 0.0 || cam.P[5] <= 0.0) return "rectification: P's focal lengths must be positive";
  if (cam.K[1] != 0.0) return "rectification: K's skew must be 0";
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double d = cam.R[3 * i] * cam.R[3 * j] + cam.R[3 * i + 1] * cam.R[3 * j + 1] + cam.R[3 * i + 2] * cam.R[3 * j + 2];
      if (std::fabs(d - (i == j ? 1.0 : 0.0)) > 1e-6) return "rectification: R is not a rotation (R R^T differs from I by more than 1e-6)";
    }
  return nullptr;
}
