// disparity_filter.hip — the speckle filter of the disparity estimator (mod_set_disparity_filters, mod_disparity_speckle_dev;
// DESIGN.md 3.4b): every 4-connected region of at most `size` pixels of a float disparity plane becomes `invalid`.
//
// What stereo_image_proc / StereoSGBM's filterSpeckles offers, stated so that the result does not depend on any order: a pixel
// takes part iff it is finite and >= lo; 4-neighbours that both take part are linked iff fabsf(a - b) <= range (pairwise, never
// against a seed); the regions are the connected components of that graph.  tests/models/sgm_filters_model.py restates it.
//
// Four launches over the planes of a group of frames (frames in grid.z), the union-find of cluster_common.h on planes of its own
// (SpkArgs.parent / size — NOT the cluster stage's, which carry invariants between calls):
//   k_spk_tile    one workgroup per 64 x 16 tile, values and parents in LDS: rows pre-linked into runs with ballots, one LDS union
//                 per pair of runs that touch vertically, the size of every tile-local component reduced in LDS (one add per run);
//                 parent[p] = tile-local root (-1 where p does not take part), size[p] = members at a tile-local root, else 0.
//   k_spk_seams   unions across the right and bottom tile borders (device-scope atomicMin hooks between tile roots).
//   k_spk_fold    every tile-local root that is not final adds its size to its final root: one atomic per tile-local component.
//   k_spk_apply   pixel -> final root -> size <= speckle_size -> store `invalid`.
// INVARIANT of every parent entry, in LDS and in memory, at every moment: parent[a] <= a, and parent[a] == a exactly at a root.
// A link only ever points to a SMALLER index, so every find loop below walks a strictly decreasing sequence and ends; no loop's
// exit depends on what another workgroup does.
#include "cluster_common.h"

#include <algorithm>

namespace {

struct SpkArgs {
  int W, H;
  float lo, range, invalid;
  int max_size;
  float *disp;               // [F][H][W], filtered in place
  int32_t *parent, *size;    // [F][H][W] scratch
  unsigned long long *dbg;   // the context's diagnostic counters (checked build: index assertion 17)
};

constexpr int kSpkTileW = 64, kSpkTileH = 16, kSpkRows = kSpkTileH / 4;   // 4 waves, kSpkRows rows each

__device__ __forceinline__ bool spk_takes_part(float v, float lo) { return fabsf(v) < __builtin_inff() && v >= lo; }   // finite (NaN fails both)

__global__ __launch_bounds__(256) void k_spk_tile(SpkArgs a) {
  __shared__ float sv[kSpkTileH][kSpkTileW];
  __shared__ int spar[kSpkTileH * kSpkTileW], scnt[kSpkTileH * kSpkTileW];
  __shared__ unsigned long long slink[kSpkTileH];      // per row: lanes linked to their left neighbour
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x0 = blockIdx.x * kSpkTileW, y0 = blockIdx.y * kSpkTileH, x = x0 + lane;
  const size_t fN = (size_t)blockIdx.z * a.W * a.H;
  const float *disp = a.disp + fN;
  float v[kSpkRows];
  bool take[kSpkRows], left[kSpkRows];
  unsigned long long L[kSpkRows];
  // ---- A: load; runs of every row by ballot: a run's pixels point at its first (smallest) pixel --------------------------------
#pragma unroll
  for (int i = 0; i < kSpkRows; i++) {
    const int r = wv * kSpkRows + i, y = y0 + r;
    const bool in = x < a.W && y < a.H;
    v[i] = in ? disp[(size_t)y * a.W + x] : -__builtin_inff();
    take[i] = in && spk_takes_part(v[i], a.lo);
    const float vl = wave_prev_f32(v[i]);                                   // all 64 lanes active
    const unsigned long long T = __ballot(take[i]);
    left[i] = take[i] && lane > 0 && ((T >> ((lane - 1) & 63)) & 1ull) && fabsf(v[i] - vl) <= a.range;
    L[i] = __ballot(left[i]);
    const unsigned long long starts = (T & ~L[i]) & (~0ull >> (63 - lane));   // run starts at or below this lane: one exists where take
    spar[r * kSpkTileW + lane] = take[i] ? r * kSpkTileW + (63 - __builtin_clzll(starts | 1ull)) : -1;   // (| 1: defined where !take)
    scnt[r * kSpkTileW + lane] = 0;
    sv[r][lane] = v[i];
    if (lane == 0) slink[r] = L[i];
  }
  __syncthreads();
  // ---- B: vertical links.  A link is skipped when the column to its left carries the same pair of runs already ----------------
#pragma unroll
  for (int i = 0; i < kSpkRows; i++) {
    const int r = wv * kSpkRows + i;
    if (r == 0) continue;                                                    // wave-uniform
    const int idx = r * kSpkTileW + lane, up = idx - kSpkTileW;
    const bool vlink = take[i] && spar[up] >= 0 && fabsf(v[i] - sv[r - 1][lane]) <= a.range;
    const unsigned long long V = __ballot(vlink);
    const bool repeated = left[i] && ((slink[r - 1] >> lane) & 1ull) && ((V >> ((lane - 1) & 63)) & 1ull);
    if (vlink && !repeated) uf_unite(spar, idx, up);                         // hooks the larger root under the smaller: parent <= self
  }
  __syncthreads();
  // ---- C: every pixel finds its tile-local root; every run adds its length to the root's count -------------------------------
  int root[kSpkRows];
#pragma unroll
  for (int i = 0; i < kSpkRows; i++) {
    const int idx = (wv * kSpkRows + i) * kSpkTileW + lane;
    root[i] = take[i] ? uf_find(spar, idx) : -1;
    if (take[i] && !left[i]) {                                               // first pixel of a run: the lanes above it that link left
      const int len = lane == 63 ? 1 : 1 + __builtin_ctzll(~(L[i] >> (lane + 1)));
      atomicAdd(&scnt[root[i]], len);
    }
  }
  __syncthreads();
  // ---- D: publish.  Local raster order is global raster order, so the tile-local root is the component's smallest pixel index ---
#pragma unroll
  for (int i = 0; i < kSpkRows; i++) {
    const int r = wv * kSpkRows + i, y = y0 + r, idx = r * kSpkTileW + lane;
    if (x >= a.W || y >= a.H) continue;
    const size_t p = fN + (size_t)y * a.W + x;
    a.parent[p] = take[i] ? (y0 + root[i] / kSpkTileW) * a.W + x0 + root[i] % kSpkTileW : -1;
    a.size[p] = root[i] == idx ? scnt[idx] : 0;
  }
}

// find on the parent plane in memory: the chain is strictly decreasing (see the invariant above)
__device__ __forceinline__ int spk_find(const SpkArgs &a, const int *parent, int p) {
  [[maybe_unused]] const int n = a.W * a.H;   // (checked build)
  int q = ld_relaxed(parent + p);
  while (q != p && MOD_CHECK(a, q >= 0 && q < p && q < n, 17)) { p = q; q = ld_relaxed(parent + p); }
  return p;
}

// blockIdx.y < hseams: the seam below tile row blockIdx.y, one thread per column; then the seam right of tile column
// blockIdx.y - hseams, one thread per image row
__global__ __launch_bounds__(256) void k_spk_seams(SpkArgs a, int hseams) {
  const size_t fN = (size_t)blockIdx.z * a.W * a.H;
  const float *disp = a.disp + fN;
  int *parent = a.parent + fN;
  const int t = blockIdx.x * 256 + threadIdx.x;
  int p, q;
  if ((int)blockIdx.y < hseams) {
    const int y = ((int)blockIdx.y + 1) * kSpkTileH - 1;                     // last row of the tile row; y + 1 < H by the grid
    if (t >= a.W) return;
    p = y * a.W + t; q = p + a.W;
  } else {
    const int x = ((int)blockIdx.y - hseams + 1) * kSpkTileW - 1;            // last column of the tile column; x + 1 < W by the grid
    if (t >= a.H) return;
    p = t * a.W + x; q = p + 1;
  }
  if (parent[p] < 0 || parent[q] < 0) return;                                // one of the two does not take part
  if (fabsf(disp[p] - disp[q]) <= a.range) uf_unite(parent, p, q);
}

__global__ __launch_bounds__(256) void k_spk_fold(SpkArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.W * a.H) return;
  const size_t fN = (size_t)blockIdx.z * a.W * a.H;
  const int *parent = a.parent + fN;
  int *size = a.size + fN;
  const int n = size[p];                                                     // > 0 exactly at the tile-local roots
  if (n <= 0 || parent[p] == p) return;                                      // final roots receive; nobody adds to a root that is not final
  atomicAdd(&size[spk_find(a, parent, p)], n);
}

__global__ __launch_bounds__(256) void k_spk_apply(SpkArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.W * a.H) return;
  const size_t fN = (size_t)blockIdx.z * a.W * a.H;
  const int *parent = a.parent + fN;
  if (parent[p] < 0) return;
  if (a.size[fN + spk_find(a, parent, p)] <= a.max_size) a.disp[fN + p] = a.invalid;
}

}  // namespace

void launch_speckle(int W, int H, int frames, float lo, float invalid, int speckle_size, int speckle_range, float *disparity,
                    int32_t *parent, int32_t *size, unsigned long long *dbg, hipStream_t s) {
  SpkArgs a{W, H, lo, (float)speckle_range, invalid, speckle_size, disparity, parent, size, dbg};
  const int tx = (W + kSpkTileW - 1) / kSpkTileW, ty = (H + kSpkTileH - 1) / kSpkTileH;
  const int hseams = (H - 1) / kSpkTileH, vseams = (W - 1) / kSpkTileW;      // seams with pixels on both sides
  const dim3 px((unsigned)(((size_t)W * H + 255) / 256), 1, frames);
  hipLaunchKernelGGL(k_spk_tile, dim3(tx, ty, frames), dim3(256), 0, s, a);
  if (hseams + vseams > 0)
    hipLaunchKernelGGL(k_spk_seams, dim3((std::max(W, H) + 255) / 256, hseams + vseams, frames), dim3(256), 0, s, a, hseams);
  hipLaunchKernelGGL(k_spk_fold, px, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_spk_apply, px, dim3(256), 0, s, a);
}
