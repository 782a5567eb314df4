// disparity_fill.hip — the occlusion hole fill of a finished disparity (mod_set_disparity_fill, mod_disparity_fill_dev; include/mod_sf.h
// states the rule, DESIGN.md §3.4e where it sits; tests/models/disparity_fill_model.py restates it):
//   a word d is VALID when it is finite and d >= lo
//   an invalid pixel p walks each of the first `directions` of (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,-1) (-1,+1) (+1,-1): it visits
//   p + s (dx, dy), s = 1 .. reach, inside the image of its own frame, and stops at the first valid word; n = the directions that found one
//   p valid or n < min_found: out = in, bit for bit
//   else out = the found word of rank 0 (MIN), min(1, n - 1) (SECOND) or (n - 1) >> 1 (MEDIAN) in ascending order of the key
//   k(b) = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000) of the words' bits
//
// k_disparity_fill: one workgroup (4 waves) per 64 x 8 tile, frames in grid.z; a wave owns two rows of the tile.
//   A  a wave reads the 64 words of a row, takes the ballot of "valid" and stores the valid lanes' words: the copy.  A tile without a hole
//      ends behind this step.  The two horizontal directions need no walk: a hole's nearest valid neighbour inside the chunk is a
//      count-trailing / count-leading-zeros on the ballot masked to the lanes right / left of it and one cross-lane read; the chunks
//      beyond are tested 64 pixels at a time, one load and one ballot each, while some hole of the row can still reach into them.
//   B  the tile's holes are compacted into an LDS list (ballot prefix inside a row, the rows' counts across the waves: no counter is contended), each
//      with its own word and the two words found in A.  A direction that found nothing holds kNone, a NaN no valid word equals.
//   C  the vertical and diagonal walks: one hole and one direction per lane, holes consecutive across lanes, so the waves are full of
//      walks whatever the tile's hole share is.  A walk loads one word per step (an L2 hit: a plane is a few MB) and tests the
//      image's bounds before the load: no load leaves the frame.
//   D  one hole per lane: the keys of its `directions` cells, a rank count in registers (for every found word i the number of found
//      words below and not above it; the one whose counts enclose the rank is the answer; equal keys are equal words), and ONE store
//      per hole: the selected word, or its own where n < min_found.
// Input and output are different planes (checked by the caller); every pixel of the output is stored once, plain vector stores.
#include "mod_launch.h"

namespace {

constexpr int kTileW = 64, kTileH = 8, kTileN = kTileW * kTileH, kRowsPerWave = kTileH / 4;
constexpr uint32_t kNone = 0x7FFFFFFFu;      // a NaN: never valid, and its key 0xFFFFFFFF is above every valid word's

struct DFillArgs {
  int W, H, reach, directions, mode, min_found;
  float lo;
  const uint32_t *in;       // [F][H][W]
  uint32_t *out;            // [F][H][W], not `in`
};

__device__ inline uint32_t fill_key(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ inline bool fill_valid(uint32_t b, float lo) { return (b & 0x7F800000u) != 0x7F800000u && __uint_as_float(b) >= lo; }

__global__ __launch_bounds__(256) void k_disparity_fill(DFillArgs a) {
  __shared__ uint32_t s_found[8][kTileN];     // per direction, per hole of the list: the found word or kNone
  __shared__ uint32_t s_own[kTileN];          // the hole's own word
  __shared__ uint16_t s_at[kTileN];           // the hole's place in the tile: 64 * row + column
  __shared__ int s_count[kTileH];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH, x = x0 + lane;
  const size_t fN = (size_t)blockIdx.z * a.W * a.H;
  const uint32_t *const in = a.in + fN;
  uint32_t *const out = a.out + fN;
  const uint64_t below = (1ull << lane) - 1, above = lane == 63 ? 0 : ~((2ull << lane) - 1);
  // ---- A: the copy and the horizontal directions --------------------------------------------------------------------------------------
  uint64_t holes[kRowsPerWave];
  uint32_t own[kRowsPerWave], right[kRowsPerWave], left[kRowsPerWave];
#pragma unroll
  for (int i = 0; i < kRowsPerWave; i++) {
    const int y = y0 + wv * kRowsPerWave + i;
    holes[i] = 0; own[i] = right[i] = left[i] = kNone;
    if (y >= a.H) continue;                                     // wave-uniform
    const uint32_t *const row = in + (size_t)y * a.W;
    const bool inside = x < a.W;
    const uint32_t w = inside ? row[x] : kNone;
    const bool valid = inside && fill_valid(w, a.lo);
    if (valid) out[(size_t)y * a.W + x] = w;
    const uint64_t vb = __ballot(valid);
    const bool hole = inside && !valid;
    holes[i] = __ballot(hole);
    own[i] = w;
    if (!holes[i]) continue;
    // (+1, 0): the valid lanes right of this one, then the chunks right of the tile
    {
      const uint64_t m = vb & above;
      const int pos = m ? __builtin_ctzll(m) : 0;
      const uint32_t v = __shfl(w, pos);
      bool searching = hole;
      if (m) { if (searching && pos - lane <= a.reach) right[i] = v; searching = false; }
      for (int c = 1;; c++) {
        const int cx0 = x0 + 64 * c;
        const bool want = searching && cx0 < a.W && 64 * c - lane <= a.reach;    // the chunk's first pixel is 64 c - lane steps away
        if (!__any(want)) break;
        const uint32_t w2 = cx0 + lane < a.W ? row[cx0 + lane] : kNone;
        const uint64_t b2 = __ballot(fill_valid(w2, a.lo));
        const int p2 = b2 ? __builtin_ctzll(b2) : 0;
        const uint32_t v2 = __shfl(w2, p2);
        if (want && b2) { if (64 * c + p2 - lane <= a.reach) right[i] = v2; searching = false; }
        if (!want) searching = false;
      }
    }
    // (-1, 0): the valid lanes left of this one, then the chunks left of the tile (all of them whole: x0 is a multiple of 64)
    {
      const uint64_t m = vb & below;
      const int pos = m ? 63 - __builtin_clzll(m) : 0;
      const uint32_t v = __shfl(w, pos);
      bool searching = hole;
      if (m) { if (searching && lane - pos <= a.reach) left[i] = v; searching = false; }
      for (int c = 1;; c++) {
        const int cx0 = x0 - 64 * c;
        const bool want = searching && cx0 >= 0 && lane + 64 * (c - 1) + 1 <= a.reach;   // the chunk's last pixel is that many steps away
        if (!__any(want)) break;
        const uint32_t w2 = row[cx0 + lane];
        const uint64_t b2 = __ballot(fill_valid(w2, a.lo));
        const int p2 = b2 ? 63 - __builtin_clzll(b2) : 0;
        const uint32_t v2 = __shfl(w2, p2);
        if (want && b2) { if (lane + 64 * c - p2 <= a.reach) left[i] = v2; searching = false; }
        if (!want) searching = false;
      }
    }
  }
  // ---- B: the tile's holes into one list -----------------------------------------------------------------------------------------------
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kRowsPerWave; i++) s_count[wv * kRowsPerWave + i] = __popcll(holes[i]);
  }
  __syncthreads();
  int total = 0, first = 0;
#pragma unroll
  for (int r = 0; r < kTileH; r++) {
    if (r == wv * kRowsPerWave) first = total;
    total += s_count[r];
  }
  if (total == 0) return;                                       // uniform over the workgroup
#pragma unroll
  for (int i = 0; i < kRowsPerWave; i++) {
    if ((holes[i] >> lane) & 1) {
      const int h = first + __popcll(holes[i] & below);
      s_at[h] = (uint16_t)((wv * kRowsPerWave + i) * kTileW + lane);
      s_own[h] = own[i];
      s_found[0][h] = right[i];
      s_found[1][h] = left[i];
    }
    first += __popcll(holes[i]);
  }
  __syncthreads();
  // ---- C: the walks, one hole and one direction per lane -----------------------------------------------------------------------------
  const int walks = a.directions - 2;
  for (int j = tid; j < total * walks; j += 256) {
    const int k = 2 + j / total, h = j - (k - 2) * total;
    // directions 2 .. 7: (0,+1) (0,-1) (+1,+1) (-1,-1) (-1,+1) (+1,-1)
    const int dx = k < 4 ? 0 : ((k == 4 || k == 7) ? 1 : -1), dy = (k == 2 || k == 4 || k == 6) ? 1 : -1;
    const int at = s_at[h];
    int px = x0 + (at & 63), py = y0 + (at >> 6);
    uint32_t found = kNone;
    for (int s = 1; s <= a.reach; s++) {
      px += dx; py += dy;
      if (px < 0 || px >= a.W || py < 0 || py >= a.H) break;
      const uint32_t w = in[(size_t)py * a.W + px];
      if (fill_valid(w, a.lo)) { found = w; break; }
    }
    s_found[k][h] = found;
  }
  __syncthreads();
  // ---- D: the selection, one hole per lane ----------------------------------------------------------------------------------------------
  for (int h = tid; h < total; h += 256) {
    uint32_t key[8];
    int n = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint32_t w = k < a.directions ? s_found[k][h] : kNone;
      key[k] = fill_key(w);                                     // kNone: 0xFFFFFFFF, above every found word's key
      n += w != kNone;
    }
    uint32_t o = s_own[h];
    if (n >= a.min_found) {                                     // min_found >= 1: n > 0 here
      const int rank = a.mode == MOD_DISPARITY_FILL_MIN ? 0 : a.mode == MOD_DISPARITY_FILL_SECOND ? (n > 1 ? 1 : 0) : (n - 1) >> 1;
      uint32_t sel = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        int less = 0, leq = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) { less += key[k] < key[i]; leq += key[k] <= key[i]; }
        if (less <= rank && rank < leq) sel = key[i];           // rank < n: a found word's key, never the sentinel's
      }
      o = sel ^ ((sel >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    }
    const int at = s_at[h];
    out[(size_t)(y0 + (at >> 6)) * a.W + x0 + (at & 63)] = o;
  }
}

}  // namespace

void launch_disparity_fill(int W, int H, int frames, float lo, int reach, int directions, int mode, int min_found, const float *in, float *out,
                           hipStream_t s) {
  const DFillArgs a{W, H, reach, directions, mode, min_found, lo, reinterpret_cast<const uint32_t *>(in), reinterpret_cast<uint32_t *>(out)};
  const dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, frames);
  hipLaunchKernelGGL(k_disparity_fill, grid, dim3(256), 0, s, a);
}
