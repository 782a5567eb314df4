// bayer.hip — 8-bit Bayer mosaics to the grey planes the estimators read.
//
// image_proc does two things to a raw camera: debayer, then rectify.  k_bayer_to_mono is the first, straight to grey: bilinear
// demosaicing and the BT.601 grey of image_fmt.h's grey() folded into ONE weighted sum with ONE rounding.  With c the pixel's own
// byte, hs / vs the sums of its two horizontal / vertical neighbours and dg the sum of its four diagonal ones,
//     v = (4 c wc + hs wh + vs wv + dg wd + 32768) >> 16
// where the weights depend on the pixel's colour site (kR = 4899, kG = 9617, kB = 1868; every set sums to 4 * 16384):
//     R site:  wc = kR, wh = wv = kG, wd = kB          G site in an R row:  wc = kG, wh = 2 kR, wv = 2 kB, wd = 0
//     B site:  wc = kB, wh = wv = kG, wd = kR          G site in a B row:   wc = kG, wh = 2 kB, wv = 2 kR, wd = 0
// (for a G site this is (2 c kG + hs kh + vs kv + 16384) >> 15 exactly: both sides of the shift are doubled).  The largest sum is
// below 2^25.  A pixel of the one-pixel frame of the region copies the nearest interior result.
//
// The kernel works on a REGION: rw x rh bytes (row pitch `step`, frames frame_bytes apart) whose byte (0, 0) lies `phase` into the
// RGGB tile (bit 0: one column, bit 1: one row), and writes the W x H window at (x0, y0) of it as packed grey planes [frames][H][W].
// A region is a whole message, one pane of a side-by-side message, or the window with its one-pixel apron as the host paths stage it.
//
// 1 byte in + 1 byte out per pixel when the two neighbour rows come from cache; as measured the kernel is VALU-bound, about half of
// it the byte path of the two row-end runs.  k_to_mono's output discipline: each
// lane makes one run of 16 consecutive output pixels of one row, runs lie on the OUTPUT's 16-byte grid (a row interior is one
// aligned 16-byte store), the 18 source bytes of each of the run's three rows start at any byte and are loaded as the six dwords
// from the dword below the first, shifted into place with v_alignbyte.  A run whose loads would leave the region's bytes of its rows,
// or whose pixels are cut by a row end or touch the region's first or last column, takes the byte path.  The region's first and
// last row cost nothing: the run's centre row is clamped.  No LDS, no atomics; frames in blockIdx.z.
#include "image_fmt.h"

namespace {

constexpr int kRun = 16;      // output pixels per lane
constexpr int kBlock = 256;
constexpr int kSrc = kRun + 2;                 // source bytes of a run in each of its three rows
constexpr int kLoad = (kSrc + 3 + 3) / 4;      // dwords that cover them from any byte: 6
constexpr uint32_t kR = 4899u, kG = 9617u, kB = 1868u;   // grey()'s weights

struct SiteWeights { uint32_t c, h, v, d; };

// (px, py): the pixel's place in the RGGB tile — R (0,0), G (1,0) / G (0,1), B (1,1)
__device__ __forceinline__ SiteWeights site_weights(uint32_t px, uint32_t py) {
  const bool green = ((px ^ py) & 1u) != 0, red_row = (py & 1u) == 0;
  const uint32_t krow = red_row ? kR : kB, kcol = red_row ? kB : kR;   // the colour that shares the row / the other one
  SiteWeights w;
  w.c = green ? kG : krow;
  w.h = green ? 2u * krow : kG;
  w.v = green ? 2u * kcol : kG;
  w.d = green ? 0u : kcol;
  return w;
}

__device__ __forceinline__ uint32_t site_grey(const SiteWeights &w, uint32_t c, uint32_t hs, uint32_t vs, uint32_t dg) {
  return (4u * c * w.c + hs * w.h + vs * w.v + dg * w.d + 32768u) >> 16;
}

// byte j of a run held in dwords d[] (little-endian)
template <int J, int N>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&d)[N]) {
  return (d[J >> 2] >> ((J & 3) * 8)) & 0xffu;
}

// the kSrc bytes at s (any address) as dwords; the caller has checked that the kLoad dwords from the one below s may be loaded
__device__ __forceinline__ void load_row(const uint8_t *s, uint32_t (&d)[kLoad - 1]) {
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
  const uint32_t *p = reinterpret_cast<const uint32_t *>(s - sh);
  uint32_t w[kLoad];
#pragma unroll
  for (int k = 0; k < kLoad; k++) w[k] = p[k];
#pragma unroll
  for (int k = 0; k < kLoad - 1; k++) d[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
}

template <int... K>
__device__ __forceinline__ void run_grey(const uint32_t (&up)[kLoad - 1], const uint32_t (&mid)[kLoad - 1], const uint32_t (&dn)[kLoad - 1],
                                         const SiteWeights &even, const SiteWeights &odd, uint32_t (&o)[4], std::integer_sequence<int, K...>) {
  // byte K + 1 of a row is pixel K of the run; col = the sums of the rows above and below, per source column
  const uint32_t col[kSrc] = {(byte_of<K, kLoad - 1>(up) + byte_of<K, kLoad - 1>(dn))..., byte_of<kRun, kLoad - 1>(up) + byte_of<kRun, kLoad - 1>(dn),
                              byte_of<kRun + 1, kLoad - 1>(up) + byte_of<kRun + 1, kLoad - 1>(dn)};
  ((o[K >> 2] |= site_grey((K & 1) ? odd : even, byte_of<K + 1, kLoad - 1>(mid), byte_of<K, kLoad - 1>(mid) + byte_of<K + 2, kLoad - 1>(mid),
                           col[K + 1], col[K] + col[K + 2])
                 << ((K & 3) * 8)),
   ...);
}

//   runs         runs per row: (W + 15) / 16 + 1 (run r covers x in [head + 16 (r - 1), head + 16 r), head = pixels of the row in
//                front of the output's first 16-byte boundary)
//   rw, rh       the region's size, both >= 3; the window (x0, y0, W, H) lies inside it
__global__ __launch_bounds__(kBlock) void k_bayer_to_mono(int W, int H, int runs, const uint8_t *__restrict__ src, size_t frame_bytes, int step,
                                                          int rw, int rh, int x0, int y0, int phase, uint8_t *__restrict__ dst) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= runs * H) return;
  const int y = i / runs, r = i - y * runs;
  const int f = blockIdx.z;
  const int Y = min(max(y0 + y, 1), rh - 2);       // the centre row: a row of the region's frame copies the nearest interior row
  const uint8_t *mid = src + (size_t)f * frame_bytes + (size_t)Y * step;   // the region's row Y
  const uint8_t *up = mid - step, *dn = mid + step;
  uint8_t *out = dst + ((size_t)f * H + y) * W;
  const int head = (int)((0u - (uint32_t)(uintptr_t)out) & 15u);
  const int xs = head + (r - 1) * kRun;
  const int X = x0 + xs;                            // the run's first pixel in the region
  const uint32_t py = (uint32_t)(Y + (phase >> 1)) & 1u, px = (uint32_t)(X + phase) & 1u;
  // a row's loads start at most 3 bytes below byte X - 1 and end at most 4 * kLoad bytes above it
  if (xs >= 0 && xs + kRun <= W && X >= 4 && X - 1 + 4 * kLoad <= rw) {
    uint32_t a[kLoad - 1], b[kLoad - 1], c[kLoad - 1];
    load_row(up + (X - 1), a);
    load_row(mid + (X - 1), b);
    load_row(dn + (X - 1), c);
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    run_grey(a, b, c, site_weights(px, py), site_weights(px ^ 1u, py), o, std::make_integer_sequence<int, kRun>{});
    *reinterpret_cast<uint4 *>(__builtin_assume_aligned(out + xs, 16)) = make_uint4(o[0], o[1], o[2], o[3]);
    return;
  }
#pragma unroll 1
  for (int k = 0; k < kRun; k++) {
    const int x = xs + k;
    if (x < 0 || x >= W) continue;
    const int Xc = min(max(x0 + x, 1), rw - 2);     // likewise for a column of the region's frame
    const SiteWeights w = site_weights((uint32_t)(Xc + phase) & 1u, py);
    const uint8_t *u = up + Xc, *m = mid + Xc, *d = dn + Xc;
    out[x] = (uint8_t)site_grey(w, m[0], (uint32_t)m[-1] + m[1], (uint32_t)u[0] + d[0], (uint32_t)u[-1] + u[1] + d[-1] + d[1]);
  }
}

}  // namespace

int bayer_phase(int encoding, int x, int y) {
  int at;                                // where the pattern's (0, 0) lies in the RGGB tile: bit 0 one column in, bit 1 one row in
  switch (encoding) {
    case MOD_ENCODING_BAYER_RGGB8: at = 0; break;
    case MOD_ENCODING_BAYER_GRBG8: at = 1; break;
    case MOD_ENCODING_BAYER_GBRG8: at = 2; break;
    case MOD_ENCODING_BAYER_BGGR8: at = 3; break;
    default: return -1;
  }
  return (((at >> 1) + y) & 1) << 1 | ((at + x) & 1);
}

void launch_bayer_to_mono(int W, int H, int frames, const uint8_t *src, size_t frame_bytes, int step, int rw, int rh, int x0, int y0, int phase,
                          uint8_t *dst, hipStream_t s) {
  const int runs = (W + kRun - 1) / kRun + 1;
  const dim3 grid((unsigned)(((size_t)runs * H + kBlock - 1) / kBlock), 1, (unsigned)frames);
  hipLaunchKernelGGL(k_bayer_to_mono, grid, dim3(kBlock), 0, s, W, H, runs, src, frame_bytes, step, rw, rh, x0, y0, phase, dst);
}
