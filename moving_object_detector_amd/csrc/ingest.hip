// ingest.hip — camera images to the grey planes the estimators read.
//
// The reference's constructor node turns every image_rect_color message into grey with cv_bridge::toCvCopy(..., MONO8)
// (scene_flow_constructor.cpp:220-221), and its ZED launch crops a centred window first (image_crop.cpp:24-40).  k_to_mono does both
// on bytes already in HBM: it reads the camera-sized window (W x H) at (x0, y0) of each 8-bit frame of a batch (row pitch `step`,
// frames stacked at step * message height bytes) and writes packed grey planes [frames][H][W].
//
// Memory-bound: C + 1 bytes per pixel (C = 1, 2, 3 or 4 bytes of a source pixel; packed YUV 4:2:2 is C = 2, grey = its Y byte).
// Each lane makes one run of 16 consecutive output pixels of one row.
// Runs are placed on the OUTPUT's 16-byte grid, so a row interior is one aligned 16-byte store; the source of a run starts at any byte
// (neither step nor x0 * C need be a multiple of 4): the run loads the dwords that cover it from the dword below its first byte and
// shifts them into place with v_alignbyte.  A run whose loads would leave the window's bytes of its row (the row ends), or whose
// pixels are cut by a row end, takes the byte path.  No LDS, no atomics; frames in blockIdx.z.
#include "image_fmt.h"

namespace {

constexpr int kRun = 16;      // output pixels per lane
constexpr int kBlock = 256;

template <int Enc>
__device__ __forceinline__ uint32_t pixel_grey(const uint8_t *p) {
  using F = Fmt<Enc>;
  if constexpr (F::mono) return p[F::y];
  else return grey(p[F::b], p[F::g], p[F::r]);
}

// byte j of a run held in dwords d[] (little-endian)
template <int J, int N>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&d)[N]) {
  return (d[J >> 2] >> ((J & 3) * 8)) & 0xffu;
}

template <int Enc, int P, int N>
__device__ __forceinline__ uint32_t run_grey(const uint32_t (&d)[N]) {
  using F = Fmt<Enc>;
  if constexpr (F::mono) return byte_of<P * F::C + F::y, N>(d);
  else return grey(byte_of<P * F::C + F::b, N>(d), byte_of<P * F::C + F::g, N>(d), byte_of<P * F::C + F::r, N>(d));
}

template <int Enc, int... P>
__device__ __forceinline__ void pack_run(const uint32_t (&d)[kRun * Fmt<Enc>::C / 4], uint32_t (&o)[4], std::integer_sequence<int, P...>) {
  using F = Fmt<Enc>;
  if constexpr (F::mono && F::C == 2) {
    // the four luma bytes of an output dword lie in two source dwords, every other byte from F::y on: one v_perm_b32 gathers them
    // (selector byte k = the index, within the eight bytes {d[2 j + 1], d[2 j]}, of output byte k)
    constexpr uint32_t sel = 0x06040200u + 0x01010101u * F::y;
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = __builtin_amdgcn_perm(d[2 * j + 1], d[2 * j], sel);
  } else {
    ((o[P >> 2] |= run_grey<Enc, P>(d) << ((P & 3) * 8)), ...);
  }
}

//   runs         runs per row: (W + 15) / 16 + 1 (run r covers x in [head + 16 (r - 1), head + 16 r), head = pixels of the row in
//                front of the output's first 16-byte boundary)
//   frame_bytes  step * message height
template <int Enc>
__global__ __launch_bounds__(kBlock) void k_to_mono(int W, int H, int runs, const uint8_t *__restrict__ src, size_t frame_bytes, int step,
                                                    int x0, int y0, uint8_t *__restrict__ dst) {
  using F = Fmt<Enc>;
  constexpr int C = F::C, NW = kRun * C / 4 + 1;   // dwords that cover 16 pixels starting at any byte
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= runs * H) return;
  const int y = i / runs, r = i - y * runs;
  const int f = blockIdx.z;
  const uint8_t *row = src + (size_t)f * frame_bytes + (size_t)(y0 + y) * step + (size_t)x0 * C;   // the window's row
  uint8_t *out = dst + ((size_t)f * H + y) * W;
  const int head = (int)((0u - (uint32_t)(uintptr_t)out) & 15u);
  const int xs = head + (r - 1) * kRun;
  const uint8_t *s = row + (ptrdiff_t)xs * C;
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
  const uint8_t *lo = s - sh;                      // the dword below the run's first byte
  if (xs >= 0 && xs + kRun <= W && lo >= row && lo + 4 * NW <= row + (size_t)W * C) {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(lo);
    uint32_t w[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) w[k] = p[k];
    uint32_t d[NW - 1];
#pragma unroll
    for (int k = 0; k < NW - 1; k++) d[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    pack_run<Enc>(d, o, std::make_integer_sequence<int, kRun>{});
    *reinterpret_cast<uint4 *>(__builtin_assume_aligned(out + xs, 16)) = make_uint4(o[0], o[1], o[2], o[3]);
    return;
  }
#pragma unroll
  for (int k = 0; k < kRun; k++) {
    const int x = xs + k;
    if (x >= 0 && x < W) out[x] = (uint8_t)pixel_grey<Enc>(row + (size_t)x * C);
  }
}

template <int Enc>
void launch(int W, int H, int frames, const uint8_t *src, size_t frame_bytes, int step, int x0, int y0, uint8_t *dst, hipStream_t s) {
  const int runs = (W + kRun - 1) / kRun + 1;
  const dim3 grid((unsigned)(((size_t)runs * H + kBlock - 1) / kBlock), 1, (unsigned)frames);
  hipLaunchKernelGGL(k_to_mono<Enc>, grid, dim3(kBlock), 0, s, W, H, runs, src, frame_bytes, step, x0, y0, dst);
}

}  // namespace

int image_channels(int encoding) {
  switch (encoding) {
    case MOD_ENCODING_MONO8: return 1;
    case MOD_ENCODING_BGR8: case MOD_ENCODING_RGB8: return 3;
    case MOD_ENCODING_BGRA8: case MOD_ENCODING_RGBA8: return 4;
    case MOD_ENCODING_YUV422: case MOD_ENCODING_YUV422_YUY2: return 2;   // bytes per pixel; one of them is the grey
    case MOD_ENCODING_BAYER_RGGB8: case MOD_ENCODING_BAYER_BGGR8: case MOD_ENCODING_BAYER_GBRG8: case MOD_ENCODING_BAYER_GRBG8:
      return 1;                                                           // one colour sample per pixel (bayer.hip converts these)
    default: return 0;
  }
}

void launch_to_mono(int encoding, int W, int H, int frames, const uint8_t *src, size_t frame_bytes, int step, int x0, int y0, uint8_t *dst,
                    hipStream_t s) {
  switch (encoding) {
    case MOD_ENCODING_MONO8: launch<MOD_ENCODING_MONO8>(W, H, frames, src, frame_bytes, step, x0, y0, dst, s); break;
    case MOD_ENCODING_BGR8:  launch<MOD_ENCODING_BGR8>(W, H, frames, src, frame_bytes, step, x0, y0, dst, s); break;
    case MOD_ENCODING_RGB8:  launch<MOD_ENCODING_RGB8>(W, H, frames, src, frame_bytes, step, x0, y0, dst, s); break;
    case MOD_ENCODING_BGRA8: launch<MOD_ENCODING_BGRA8>(W, H, frames, src, frame_bytes, step, x0, y0, dst, s); break;
    case MOD_ENCODING_RGBA8: launch<MOD_ENCODING_RGBA8>(W, H, frames, src, frame_bytes, step, x0, y0, dst, s); break;
    case MOD_ENCODING_YUV422: launch<MOD_ENCODING_YUV422>(W, H, frames, src, frame_bytes, step, x0, y0, dst, s); break;
    case MOD_ENCODING_YUV422_YUY2: launch<MOD_ENCODING_YUV422_YUY2>(W, H, frames, src, frame_bytes, step, x0, y0, dst, s); break;
    default: break;
  }
}
