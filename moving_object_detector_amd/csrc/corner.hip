// corner.hip — the min-eigenvalue (aperture) measure of a grey plane and the rejection rule on it for the flow (mod_set_flow_corner_filter,
// mod_flow_corner_dev, mod_flow_corner_reject_dev; include/mod_sf.h states the rule, DESIGN.md §3.5b where it sits;
// tests/models/corner_model.py restates it):
//   gx(x, y) = clamp(I(min(x + 1, W - 1), y) - I(max(x - 1, 0), y), -c, c)      gy(x, y) = clamp(I(x, min(y + 1, H - 1)) - I(x, max(y - 1, 0)), -c, c)
//   A = sum gx^2, B = sum gx gy, C = sum gy^2 over the w x w window, 0 outside the image
//   S = A + C, D = (A - C)^2 + 4 B^2, E = (S - ceil(sqrt(D))) >> 1               rejected iff E < t  iff  not (S - 2 t >= 0 and (S - 2 t)^2 >= D)
//
// k_corner<OUT>: one workgroup (4 waves) per 64 x 16 tile, frames in grid.z, r = (w - 1) / 2 a runtime value in 1..7 — k_texture's shape.
//   A  the grey tile with r + 1 halo columns and r + 1 halo rows into LDS (at most 32 rows of 80 bytes = 2560 bytes).  Rows and columns
//      are CLAMPED into the image before the load: every load is inside the plane, at W = 1 and H = 1 too, and the clamped rows and
//      columns are exactly the rule's min / max.
//   B  (gx, gy), once per tile position, as one short2 in LDS (at most 30 x 80 x 4 = 9600 bytes); (0, 0) where the position lies
//      outside the image.
//   C  the three row sums (2 r + 1 taps each; the products are formed here, no product plane is stored) as int32 in LDS
//      (3 x 30 x 64 x 4 = 23040 bytes): one wave per row, one lane per column.
//   D  column sums: a lane owns one column and four rows; the first row is summed, the next three slide (+ row entering, - row leaving).
// 35200 bytes of static LDS.  Lanes of a wave read consecutive bytes (A), consecutive dwords (B: one ds_read_b32 brings gx AND gy; C, D):
// 64 consecutive dwords are 64 different banks, no conflict in either 32-lane half.
// A, C <= 225 * 255^2 = 14630625 and |B| likewise: int32.  D < 1.1e15: int64, and below 2^53, so the plane form's double square root
// is within one of the integer root and two integer steps make it exact; the reject form needs no root.
// OUT: kCornerPlane stores E (4 bytes per pixel).  kCornerReject stores (NaN, NaN) ONLY where E < threshold and never reads the flow:
// its traffic is the grey bytes and the rejected pixels.  Plain vector stores, no atomics.
#include "mod_launch.h"

namespace {

constexpr int kCorTileW = 64, kCorTileH = 16, kCorMaxR = 7;
constexpr int kCorCols = kCorTileW + 2 * (kCorMaxR + 1);    // 80: grey columns x0 - r - 1 .. x0 + 63 + r + 1 at r = 7
constexpr int kCorRows = kCorTileH + 2 * kCorMaxR;          // 30: gradient and row-sum rows y0 - r .. y0 + 15 + r
constexpr int kCorGreyRows = kCorRows + 2;                  // 32: grey rows y0 - r - 1 .. y0 + 15 + r + 1
constexpr int kCornerPlane = 0, kCornerReject = 1;

struct CornerArgs {
  int W, H, r, cap, threshold;
  const uint8_t *grey;      // [F][H][W]
  uint32_t *strength;       // [F][H][W]     (kCornerPlane)
  float2 *flow;             // [F][H][W][2]  (kCornerReject): rejected pixels become (NaN, NaN), both words 0x7fc00000
};

// the smallest integer whose square is >= d, for 0 <= d < 2^53
__device__ inline long long ceil_sqrt(long long d) {
  long long q = (long long)sqrt((double)d);
  while (q * q < d) q++;
  while (q > 0 && (q - 1) * (q - 1) >= d) q--;
  return q;
}

template <int OUT>
__global__ __launch_bounds__(256) void k_corner(CornerArgs a) {
  __shared__ uint8_t sI[kCorGreyRows][kCorCols];
  __shared__ short2 sg[kCorRows][kCorCols];
  __shared__ int sA[kCorRows][kCorTileW], sB[kCorRows][kCorTileW], sC[kCorRows][kCorTileW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = a.r, rows = kCorTileH + 2 * r, cols = kCorTileW + 2 * r;
  const int x0 = blockIdx.x * kCorTileW, y0 = blockIdx.y * kCorTileH;
  const size_t fN = (size_t)blockIdx.z * a.W * a.H;
  const uint8_t *I = a.grey + fN;
  // ---- A: sI[j][k] = I(x0 - r - 1 + k, y0 - r - 1 + j), both clamped into the image, j < rows + 2, k < cols + 2 --------------------
  for (int i = tid; i < (rows + 2) * kCorCols; i += 256) {
    const int j = i / kCorCols, k = i - j * kCorCols;
    if (k >= cols + 2) continue;
    const int x = min(max(x0 - r - 1 + k, 0), a.W - 1), y = min(max(y0 - r - 1 + j, 0), a.H - 1);
    sI[j][k] = I[(size_t)y * a.W + x];
  }
  __syncthreads();
  // ---- B: sg[j][k] = (gx, gy)(x0 - r + k, y0 - r + j), k < cols: the neighbours of sI[j + 1][k + 1] -------------------------------
  for (int i = tid; i < rows * kCorCols; i += 256) {
    const int j = i / kCorCols, k = i - j * kCorCols;
    if (k >= cols) continue;
    const int x = x0 - r + k, y = y0 - r + j;
    const bool in = x >= 0 && x < a.W && y >= 0 && y < a.H;
    const int gx = (int)sI[j + 1][k + 2] - (int)sI[j + 1][k], gy = (int)sI[j + 2][k + 1] - (int)sI[j][k + 1];
    sg[j][k] = in ? make_short2((short)min(max(gx, -a.cap), a.cap), (short)min(max(gy, -a.cap), a.cap)) : make_short2(0, 0);
  }
  __syncthreads();
  // ---- C: the row sums of gx^2, gx gy, gy^2 over x0 + lane - r .. x0 + lane + r at row y0 - r + j ----------------------------------
  for (int j = wv; j < rows; j += 4) {
    int sa = 0, sb = 0, sc = 0;
    for (int i = 0; i <= 2 * r; i++) {
      const short2 g = sg[j][lane + i];
      sa += (int)g.x * g.x;
      sb += (int)g.x * g.y;
      sc += (int)g.y * g.y;
    }
    sA[j][lane] = sa;
    sB[j][lane] = sb;
    sC[j][lane] = sc;
  }
  __syncthreads();
  // ---- D: A, B, C of (x0 + lane, y0 + 4 wv + i) = rows 4 wv + i .. 4 wv + i + 2 r of the row sums --------------------------------
  const int x = x0 + lane, ly = wv * (kCorTileH / 4);
  int A = 0, B = 0, Cc = 0;
  for (int j = 0; j <= 2 * r; j++) {
    A += sA[ly + j][lane];
    B += sB[ly + j][lane];
    Cc += sC[ly + j][lane];
  }
#pragma unroll
  for (int i = 0; i < kCorTileH / 4; i++) {
    const int y = y0 + ly + i;
    if (x < a.W && y < a.H) {
      const size_t p = fN + (size_t)y * a.W + x;
      const long long S = (long long)A + Cc, d = (long long)A - Cc, D = d * d + 4ll * B * B;
      if constexpr (OUT == kCornerPlane) {
        a.strength[p] = (uint32_t)((S - ceil_sqrt(D)) >> 1);
      } else {
        const long long m = S - 2ll * a.threshold;
        if (!(m >= 0 && m * m >= D)) a.flow[p] = make_float2(__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u));
      }
    }
    if (i + 1 < kCorTileH / 4) {
      A += sA[ly + i + 1 + 2 * r][lane] - sA[ly + i][lane];
      B += sB[ly + i + 1 + 2 * r][lane] - sB[ly + i][lane];
      Cc += sC[ly + i + 1 + 2 * r][lane] - sC[ly + i][lane];
    }
  }
}

}  // namespace

void launch_corner(int W, int H, int frames, int window, int cap, int threshold, const uint8_t *grey, uint32_t *strength, float *flow,
                   hipStream_t s) {
  const CornerArgs a{W, H, (window - 1) / 2, cap, threshold, grey, strength, reinterpret_cast<float2 *>(flow)};
  const dim3 grid((W + kCorTileW - 1) / kCorTileW, (H + kCorTileH - 1) / kCorTileH, frames);
  if (strength) hipLaunchKernelGGL(k_corner<kCornerPlane>, grid, dim3(256), 0, s, a);
  else if (flow) hipLaunchKernelGGL(k_corner<kCornerReject>, grid, dim3(256), 0, s, a);
}
