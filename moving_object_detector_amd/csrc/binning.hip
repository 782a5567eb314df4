// binning.hip — grey planes reduced by an integer factor: image_proc/crop_decimate's step, behind the converters.
//
// k_bin_mono reads packed full-resolution grey planes [frames][BY H][BX W] (what k_to_mono, k_bayer_to_mono or k_rectify wrote for
// the full window, or a mono8 window as it was copied) and writes packed planes [frames][H][W]:
//   MEAN     out(X, Y) = (sum of the BX x BY block at (BX X, BY Y) + ((BX BY) >> 1)) / (BX BY)   (cv::INTER_AREA at an integer factor)
//   NEAREST  out(X, Y) = G(BX X, BY Y)                                                           (crop_decimate's default)
//
// Memory-bound: BX BY + 1 bytes per output pixel (NEAREST: BX + 1, it reads one source row per output row).
// Each lane makes one run of 16 consecutive output pixels of one row, as in ingest.hip: runs lie on the OUTPUT's 16-byte grid, so a
// row interior is one aligned 16-byte store; the 16 BX source bytes of a run start at any byte (BX W need not be a multiple of 4):
// each source row is loaded as dwords from the dword below its first byte and shifted into place with v_alignbyte.  A run cut by a
// row end, or one of whose loads would leave its source row, takes the byte path.  Horizontal sums stay packed: two 16-bit fields a
// dword for BX = 1 and 2, v_sad_u8 against 0 for BX = 3 (behind v_perm_b32) and 4; rows are accumulated one after the other (a block
// sums to at most 16 * 255), and the divisor BX BY is a compile-time constant.  No LDS, no atomics; frames in blockIdx.z.
#include "mod_launch.h"

namespace {

constexpr int kRun = 16;      // output pixels per lane
constexpr int kBlock = 256;
constexpr uint32_t kZero = 0x0cu;   // v_perm_b32 selector byte: the constant 0x00

// where the accumulators of a run keep the sum of output pixel p (MEAN): BX <= 2 two 16-bit fields a dword, else a dword each
//   BX = 1: acc[2 k] = {p(4k), p(4k + 2)}, acc[2 k + 1] = {p(4k + 1), p(4k + 3)}   (even / odd bytes of source dword k)
//   BX = 2: acc[m]   = {p(2m), p(2m + 1)}                                          (the byte pairs of source dword m)
template <int BX> constexpr int kAcc = BX <= 2 ? 8 : 16;

// the horizontal sums of one source row (d: its 16 BX bytes) added to acc
template <int BX>
__device__ __forceinline__ void add_row(const uint32_t (&d)[4 * BX], uint32_t (&acc)[kAcc<BX>]) {
  if constexpr (BX == 1) {
#pragma unroll
    for (int k = 0; k < 4; k++) { acc[2 * k] += d[k] & 0x00ff00ffu; acc[2 * k + 1] += (d[k] >> 8) & 0x00ff00ffu; }
  } else if constexpr (BX == 2) {
#pragma unroll
    for (int m = 0; m < 8; m++) acc[m] += (d[m] & 0x00ff00ffu) + ((d[m] >> 8) & 0x00ff00ffu);
  } else if constexpr (BX == 3) {
    // four pixels in three dwords A B C (bytes 0 .. 11): 0 1 2 | 3 4 5 | 6 7 8 | 9 10 11; v_perm_b32 picks from {first, second}
    // operand = bytes 7 .. 0
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t A = d[3 * k], B = d[3 * k + 1], C = d[3 * k + 2];
      acc[4 * k] = __builtin_amdgcn_sad_u8(A & 0x00ffffffu, 0u, acc[4 * k]);
      acc[4 * k + 1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_perm(B, A, (kZero << 24) | 0x050403u), 0u, acc[4 * k + 1]);
      acc[4 * k + 2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_perm(C, B, (kZero << 24) | 0x040302u), 0u, acc[4 * k + 2]);
      acc[4 * k + 3] = __builtin_amdgcn_sad_u8(C >> 8, 0u, acc[4 * k + 3]);
    }
  } else {
#pragma unroll
    for (int m = 0; m < 16; m++) acc[m] = __builtin_amdgcn_sad_u8(d[m], 0u, acc[m]);
  }
}

// (s + (DIV >> 1)) / DIV of both 16-bit fields of v; results are below 256, so they come out as bytes 0 and 2
template <int DIV>
__device__ __forceinline__ uint32_t div_fields(uint32_t v) {
  if constexpr (DIV == 1) return v;
  else if constexpr ((DIV & (DIV - 1)) == 0) return ((v + (uint32_t)(DIV >> 1) * 0x00010001u) >> __builtin_ctz(DIV)) & 0x00ff00ffu;
  else return (((v & 0xffffu) + (DIV >> 1)) / DIV) | ((((v >> 16) + (DIV >> 1)) / DIV) << 16);
}

// the 16 rounded means of a run as four dwords of bytes
template <int BX, int DIV>
__device__ __forceinline__ void means(const uint32_t (&acc)[kAcc<BX>], uint32_t (&o)[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if constexpr (BX == 1) {
      o[k] = div_fields<DIV>(acc[2 * k]) | (div_fields<DIV>(acc[2 * k + 1]) << 8);
    } else if constexpr (BX == 2) {
      o[k] = __builtin_amdgcn_perm(div_fields<DIV>(acc[2 * k + 1]), div_fields<DIV>(acc[2 * k]), 0x06040200u);
    } else {
      o[k] = 0u;
#pragma unroll
      for (int j = 0; j < 4; j++) o[k] |= ((acc[4 * k + j] + (DIV >> 1)) / DIV) << (8 * j);
    }
  }
}

// every BX-th byte of one source row
template <int BX>
__device__ __forceinline__ void gather(const uint32_t (&d)[4 * BX], uint32_t (&o)[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if constexpr (BX == 1) o[k] = d[k];
    else if constexpr (BX == 2) o[k] = __builtin_amdgcn_perm(d[2 * k + 1], d[2 * k], 0x06040200u);
    else if constexpr (BX == 3)      // bytes 0, 3, 6 of {B, A} and byte 1 of C
      o[k] = __builtin_amdgcn_perm(d[3 * k + 1], d[3 * k], (kZero << 24) | 0x060300u) | ((d[3 * k + 2] << 16) & 0xff000000u);
    else
      o[k] = __builtin_amdgcn_perm(d[4 * k + 1], d[4 * k], (kZero << 24) | (kZero << 16) | 0x0400u) |
             __builtin_amdgcn_perm(d[4 * k + 3], d[4 * k + 2], 0x04000000u | (kZero << 8) | kZero);
  }
}

//   runs  runs per output row: (W + 15) / 16 + 1 (run r covers x in [head + 16 (r - 1), head + 16 r), head = pixels of the row in
//         front of the output's first 16-byte boundary)
template <int BX, int BY, bool NEAREST>
__global__ __launch_bounds__(kBlock) void k_bin_mono(int W, int H, int runs, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst) {
  constexpr int ROWS = NEAREST ? 1 : BY, DIV = BX * BY, NW = 4 * BX + 1;   // dwords that cover 16 BX bytes starting at any byte
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= runs * H) return;
  const int y = i / runs, r = i - y * runs;
  const int f = blockIdx.z;
  const size_t pitch = (size_t)BX * W;
  const uint8_t *row = src + ((size_t)f * H + y) * BY * pitch;   // the first source row of output row y
  uint8_t *out = dst + ((size_t)f * H + y) * W;
  const int head = (int)((0u - (uint32_t)(uintptr_t)out) & 15u);
  const int xs = head + (r - 1) * kRun;
  bool fast = xs >= 0 && xs + kRun <= W;
  if (fast) {
#pragma unroll
    for (int j = 0; j < ROWS; j++) {
      const ptrdiff_t at = (ptrdiff_t)xs * BX - (ptrdiff_t)((uintptr_t)(row + j * pitch + (size_t)xs * BX) & 3);   // the dword below, from the row's start
      fast = fast && at >= 0 && at + 4 * NW <= (ptrdiff_t)pitch;
    }
  }
  if (fast) {
    [[maybe_unused]] uint32_t acc[kAcc<BX>] = {};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < ROWS; j++) {
      const uint8_t *s = row + j * pitch + (size_t)xs * BX;
      const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
      const uint32_t *p = reinterpret_cast<const uint32_t *>(s - sh);
      uint32_t w[NW];
#pragma unroll
      for (int k = 0; k < NW; k++) w[k] = p[k];
      uint32_t d[NW - 1];
#pragma unroll
      for (int k = 0; k < NW - 1; k++) d[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
      if constexpr (NEAREST) gather<BX>(d, o);
      else add_row<BX>(d, acc);
    }
    if constexpr (!NEAREST) means<BX, DIV>(acc, o);
    *reinterpret_cast<uint4 *>(__builtin_assume_aligned(out + xs, 16)) = make_uint4(o[0], o[1], o[2], o[3]);
    return;
  }
#pragma unroll 1
  for (int k = 0; k < kRun; k++) {
    const int x = xs + k;
    if (x < 0 || x >= W) continue;
    const uint8_t *b = row + (size_t)x * BX;
    uint32_t sum = 0;
    for (int j = 0; j < ROWS; j++)
      for (int q = 0; q < BX; q++) sum += b[j * pitch + q];
    out[x] = (uint8_t)(NEAREST ? b[0] : (sum + (DIV >> 1)) / DIV);
  }
}

template <int BX, int BY, bool NEAREST>
void launch(int W, int H, int frames, const uint8_t *src, uint8_t *dst, hipStream_t s) {
  const int runs = (W + kRun - 1) / kRun + 1;
  const dim3 grid((unsigned)(((size_t)runs * H + kBlock - 1) / kBlock), 1, (unsigned)frames);
  hipLaunchKernelGGL((k_bin_mono<BX, BY, NEAREST>), grid, dim3(kBlock), 0, s, W, H, runs, src, dst);
}

template <int BX, bool NEAREST>
void launch_by(int by, int W, int H, int frames, const uint8_t *src, uint8_t *dst, hipStream_t s) {
  switch (by) {
    case 1: launch<BX, 1, NEAREST>(W, H, frames, src, dst, s); break;
    case 2: launch<BX, 2, NEAREST>(W, H, frames, src, dst, s); break;
    case 3: launch<BX, 3, NEAREST>(W, H, frames, src, dst, s); break;
    case 4: launch<BX, 4, NEAREST>(W, H, frames, src, dst, s); break;
    default: break;
  }
}

template <bool NEAREST>
void launch_bx(int bx, int by, int W, int H, int frames, const uint8_t *src, uint8_t *dst, hipStream_t s) {
  switch (bx) {
    case 1: launch_by<1, NEAREST>(by, W, H, frames, src, dst, s); break;
    case 2: launch_by<2, NEAREST>(by, W, H, frames, src, dst, s); break;
    case 3: launch_by<3, NEAREST>(by, W, H, frames, src, dst, s); break;
    case 4: launch_by<4, NEAREST>(by, W, H, frames, src, dst, s); break;
    default: break;
  }
}

}  // namespace

void launch_bin_mono(const ModImageBinning &b, int W, int H, int frames, const uint8_t *src, uint8_t *dst, hipStream_t s) {
  if (b.mode == MOD_BIN_NEAREST) launch_bx<true>(b.bx, b.by, W, H, frames, src, dst, s);
  else launch_bx<false>(b.bx, b.by, W, H, frames, src, dst, s);
}
