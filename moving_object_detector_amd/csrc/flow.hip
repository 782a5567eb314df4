// flow.hip — on-GPU optical flow: coarse-to-fine census block matching.
//
// Stands in for the estimator the reference's constructor node calls every frame, pwc_net_.estimateOpticalFlow(previous_left,
// left) (scene_flow_constructor/src/scene_flow_constructor.cpp:279-290).  It is NOT a port of PWC-Net (a CNN whose weights the
// project does not have) and claims no parity with it: a classical, deterministic, integer estimator whose every step is fixed so
// that tests/models/flow_model.py reproduces it bit for bit.  Flow is indexed at the NOW pixel, prev = now - flow (32FC2, x then y).
// Kernels: image pyramid (2 x 2 rounded mean), per-level block matching over the SGM path's census words (k_sgm_census), and a
// finishing kernel (sub-pixel parabola, forward-backward check, f32 store).
#include "mod_launch.h"

namespace {

constexpr int kTW = 64, kTH = 4;          // output tile of the pyramid / match / finish kernels: 64 x 4 pixels, 256 threads
constexpr int kOutCost = 31;              // a prev sample outside the image
constexpr uint32_t kOutside = 0xffffffffu;   // marker of such a sample in registers (census words have 31 bits)

// Level l + 1 of both images: (a + b + c + d + 2) >> 2 over the 2 x 2 block at (2x, 2y) of level l.  grid.z = image * frames + frame.
__global__ __launch_bounds__(256) void k_flow_pyramid(int Ws, int Hs, int W, int H, int frames, const uint8_t *__restrict__ src0,
                                                      const uint8_t *__restrict__ src1, uint8_t *__restrict__ dst) {
  const int x = blockIdx.x * kTW + threadIdx.x, y = blockIdx.y * kTH + threadIdx.y;
  if (x >= W || y >= H) return;
  const int img = blockIdx.z / frames, f = blockIdx.z - img * frames;
  const uint8_t *s = (img ? src1 : src0) + (size_t)f * Ws * Hs + (size_t)(2 * y) * Ws + 2 * x;
  const uint32_t sum = (uint32_t)s[0] + s[1] + s[Ws] + s[Ws + 1];
  dst[(size_t)blockIdx.z * W * H + (size_t)y * W + x] = (uint8_t)((sum + 2) >> 2);
}

// popcount(now ^ prev), or 31 for a prev sample outside the image
__device__ __forceinline__ uint32_t flow_tap(uint32_t now, uint32_t prv) {
  return prv == kOutside ? (uint32_t)kOutCost : (uint32_t)__popc(now ^ prv);
}

// winner key: cost, then |dx - cx| + |dy - cy|, then the candidate's index in (dy, dx) raster order
__device__ __forceinline__ uint32_t flow_key(uint32_t cost, int ex, int ey, int idx) {
  return (cost << 20) | ((uint32_t)(abs(ex) + abs(ey)) << 10) | (uint32_t)idx;
}

// One pyramid level, both directions (blockIdx.z = dir * frames + frame; dir 0: now vs prev, dir 1: the roles swapped).
//   census [2][frames][W*H] (image 0 = prev, 1 = now); coarse [dirs][frames][W1*H1] (finer levels); out [dirs][frames][W*H];
//   sub [frames][W*H] (level 0, direction 0, when sub-pixel is on): per axis (c- - c+, c- - 2 c0 + c+), 0 where a neighbour of the
//   winner was not evaluated.
struct FlowMatchArgs {
  int W, H, W1, H1, frames, radius;
  const uint32_t *census;
  const short2 *coarse;
  short2 *out;
  short4 *sub;
};

// The now-census tile + its window halo sits in LDS; the prev samples are gathers through L1 / L2 (they move with the flow).
// COARSE: the coarsest level, candidates [-radius, radius]^2 around 0.  Otherwise: c + [-1, 1]^2 around twice the coarser winner,
// whose (WIN + 2)^2 prev samples are held in registers and shared by the 9 candidates (225 taps at WIN = 5 from 49 loads).
template <int WIN, bool COARSE>
__global__ __launch_bounds__(256) void k_flow_match(FlowMatchArgs a) {
  constexpr int R = WIN / 2, LW = kTW + 2 * R, LH = kTH + 2 * R;
  __shared__ uint32_t tile[LH][LW];
  const int W = a.W, H = a.H, dir = blockIdx.z / a.frames, f = blockIdx.z - dir * a.frames;
  const size_t N = (size_t)W * H;
  const uint32_t *cn = a.census + ((size_t)(1 - dir) * a.frames + f) * N;   // dir 0: now = image 1
  const uint32_t *cp = a.census + ((size_t)dir * a.frames + f) * N;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH, tid = threadIdx.y * kTW + threadIdx.x;
  for (int i = tid; i < LW * LH; i += 256) {
    const int ty = i / LW, tx = i - ty * LW, gx = x0 - R + tx, gy = y0 - R + ty;
    tile[ty][tx] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? cn[(size_t)gy * W + gx] : 0u;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x >= W || y >= H) return;
  // now taps and whether they lie inside the image (outside: they add 0)
  uint32_t nw[WIN * WIN];
  uint64_t nin = 0;
#pragma unroll
  for (int wy = 0; wy < WIN; wy++)
#pragma unroll
    for (int wx = 0; wx < WIN; wx++) {
      nw[wy * WIN + wx] = tile[threadIdx.y + wy][threadIdx.x + wx];
      const int qx = x + wx - R, qy = y + wy - R;
      if (qx >= 0 && qx < W && qy >= 0 && qy < H) nin |= 1ull << (wy * WIN + wx);
    }
  const uint64_t all_in = (WIN * WIN == 64) ? ~0ull : ((1ull << (WIN * WIN)) - 1);
  const size_t at = (size_t)f * N + (size_t)y * W + x;
  short2 *out = a.out + (size_t)dir * a.frames * N;
  const bool want_sub = a.sub && dir == 0;
  if (COARSE) {
    const int r = a.radius;
    auto cost_at = [&](int dx, int dy) -> uint32_t {
      uint32_t c = 0;
#pragma unroll
      for (int wy = 0; wy < WIN; wy++)
#pragma unroll
        for (int wx = 0; wx < WIN; wx++) {
          const int px = x + wx - R - dx, py = y + wy - R - dy;
          const uint32_t pv = (px >= 0 && px < W && py >= 0 && py < H) ? cp[(size_t)py * W + px] : kOutside;
          c += ((nin >> (wy * WIN + wx)) & 1) ? flow_tap(nw[wy * WIN + wx], pv) : 0u;
        }
      return c;
    };
    uint32_t best = 0xffffffffu;
    int idx = 0;
    for (int dy = -r; dy <= r; dy++)
      for (int dx = -r; dx <= r; dx++, idx++) best = min(best, flow_key(cost_at(dx, dy), dx, dy, idx));
    const int n = 2 * r + 1, b = (int)(best & 1023u), bx = b % n - r, by = b / n - r;
    out[at] = make_short2((short)bx, (short)by);
    if (want_sub) {
      const int c0 = (int)(best >> 20);
      short4 s = make_short4(0, 0, 0, 0);
      if (bx > -r && bx < r) { const int cm = (int)cost_at(bx - 1, by), cq = (int)cost_at(bx + 1, by); s.x = (short)(cm - cq); s.y = (short)(cm - 2 * c0 + cq); }
      if (by > -r && by < r) { const int cm = (int)cost_at(bx, by - 1), cq = (int)cost_at(bx, by + 1); s.z = (short)(cm - cq); s.w = (short)(cm - 2 * c0 + cq); }
      a.sub[at] = s;
    }
    return;
  } else {
    constexpr int P = WIN + 2;
    const short2 cc = a.coarse[((size_t)dir * a.frames + f) * a.W1 * a.H1 + (size_t)min(y >> 1, a.H1 - 1) * a.W1 + min(x >> 1, a.W1 - 1)];
    const int cx = 2 * cc.x, cy = 2 * cc.y;
    const int px0 = x - cx - R - 1, py0 = y - cy - R - 1;          // prev sample (0, 0) of the register block
    const bool inner = nin == all_in && px0 >= 0 && px0 + P <= W && py0 >= 0 && py0 + P <= H;
    uint32_t pv[P * P];
    if (__all(inner)) {
#pragma unroll
      for (int i = 0; i < P; i++)
#pragma unroll
        for (int j = 0; j < P; j++) pv[i * P + j] = cp[(size_t)(py0 + i) * W + px0 + j];
    } else {
#pragma unroll
      for (int i = 0; i < P; i++)
#pragma unroll
        for (int j = 0; j < P; j++) {
          const int px = px0 + j, py = py0 + i;
          pv[i * P + j] = (px >= 0 && px < W && py >= 0 && py < H) ? cp[(size_t)py * W + px] : kOutside;
        }
    }
    uint32_t cost[9];
#pragma unroll
    for (int k = 0; k < 9; k++) cost[k] = 0;
#pragma unroll
    for (int wy = 0; wy < WIN; wy++)
#pragma unroll
      for (int wx = 0; wx < WIN; wx++) {
        const bool on = (nin >> (wy * WIN + wx)) & 1;
#pragma unroll
        for (int ey = -1; ey <= 1; ey++)
#pragma unroll
          for (int ex = -1; ex <= 1; ex++) {
            // candidate c + e, tap q = p + w: prev sample q - c - e = register (wy - ey + 1, wx - ex + 1)
            const uint32_t h = flow_tap(nw[wy * WIN + wx], pv[(wy - ey + 1) * P + (wx - ex + 1)]);
            cost[(ey + 1) * 3 + ex + 1] += on ? h : 0u;
          }
      }
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < 9; k++) best = min(best, flow_key(cost[k], k % 3 - 1, k / 3 - 1, k));
    const int b = (int)(best & 1023u), bx = b % 3 - 1, by = b / 3 - 1;
    out[at] = make_short2((short)(cx + bx), (short)(cy + by));
    if (want_sub) {
      // both neighbours exist only along an axis on which the winner is the centre candidate
      const int c0 = (int)(best >> 20);
      short4 s = make_short4(0, 0, 0, 0);
      uint32_t xm = 0, xp = 0, ym = 0, yp = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (by == k - 1) { xm = cost[k * 3]; xp = cost[k * 3 + 2]; }
        if (bx == k - 1) { ym = cost[k]; yp = cost[6 + k]; }
      }
      if (bx == 0) { s.x = (short)((int)xm - (int)xp); s.y = (short)((int)xm - 2 * c0 + (int)xp); }
      if (by == 0) { s.z = (short)((int)ym - (int)yp); s.w = (short)((int)ym - 2 * c0 + (int)yp); }
      a.sub[at] = s;
    }
  }
}

// sub-pixel terms of the winner (bx, by) in [-1, 1]^2 with cost c0: both neighbours exist only along an axis on which the winner is
// the centre candidate
__device__ __forceinline__ short4 flow_sub9(const uint32_t *cost, int bx, int by, int c0) {
  short4 s = make_short4(0, 0, 0, 0);
  uint32_t xm = 0, xp = 0, ym = 0, yp = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (by == k - 1) { xm = cost[k * 3]; xp = cost[k * 3 + 2]; }
    if (bx == k - 1) { ym = cost[k]; yp = cost[6 + k]; }
  }
  if (bx == 0) { s.x = (short)((int)xm - (int)xp); s.y = (short)((int)xm - 2 * c0 + (int)xp); }
  if (by == 0) { s.z = (short)((int)ym - (int)yp); s.w = (short)((int)ym - 2 * c0 + (int)yp); }
  return s;
}

// A finer level with neighbour-seed propagation (mod_set_flow_propagation(5)): besides twice the parent's
// winner, twice the winners of the parent's four neighbours (clamped to the coarser level) seed a 3 x 3 search each; every seed picks
// its winner by flow_key, the pixel takes the seed winner of the smallest cost, ties to the lowest seed.  A seed whose centre equals
// that of a lower seed cannot win and is skipped, and a seed that no lane of the wave needs is skipped by the whole wave: away from
// motion boundaries all five centres coincide and the wave does k_flow_match's work plus four coarse loads.  Elsewhere the lanes
// that hold a distinct centre score it under their exec mask.  Same tile, same register block per seed; the body of a seed is
// k_flow_match's, statement for statement (shared helper functions were tried and cost both kernels registers: section 3.5a).
// The second launch bound keeps window 7 at two waves per SIMD and window 5 at four without spills.
constexpr int kFlowSeeds = 5;

template <int WIN>
__global__ __launch_bounds__(256, (WIN == 7 ? 2 : 4)) void k_flow_match_seeds(FlowMatchArgs a) {
  constexpr int R = WIN / 2, LW = kTW + 2 * R, LH = kTH + 2 * R, P = WIN + 2;
  __shared__ uint32_t tile[LH][LW];
  const int W = a.W, H = a.H, dir = blockIdx.z / a.frames, f = blockIdx.z - dir * a.frames;
  const size_t N = (size_t)W * H;
  const uint32_t *cn = a.census + ((size_t)(1 - dir) * a.frames + f) * N;   // dir 0: now = image 1
  const uint32_t *cp = a.census + ((size_t)dir * a.frames + f) * N;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH, tid = threadIdx.y * kTW + threadIdx.x;
  for (int i = tid; i < LW * LH; i += 256) {
    const int ty = i / LW, tx = i - ty * LW, gx = x0 - R + tx, gy = y0 - R + ty;
    tile[ty][tx] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? cn[(size_t)gy * W + gx] : 0u;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x >= W || y >= H) return;
  // now taps and whether they lie inside the image (outside: they add 0)
  uint32_t nw[WIN * WIN];
  uint64_t nin = 0;
#pragma unroll
  for (int wy = 0; wy < WIN; wy++)
#pragma unroll
    for (int wx = 0; wx < WIN; wx++) {
      nw[wy * WIN + wx] = tile[threadIdx.y + wy][threadIdx.x + wx];
      const int qx = x + wx - R, qy = y + wy - R;
      if (qx >= 0 && qx < W && qy >= 0 && qy < H) nin |= 1ull << (wy * WIN + wx);
    }
  const uint64_t all_in = (WIN * WIN == 64) ? ~0ull : ((1ull << (WIN * WIN)) - 1);
  // the five centres, packed (x in the low half): seed k's parent is the pixel's parent + (0,0) (-1,0) (+1,0) (0,-1) (0,+1), clamped
  const short2 *coarse = a.coarse + ((size_t)dir * a.frames + f) * a.W1 * a.H1;
  const int X = min(x >> 1, a.W1 - 1), Y = min(y >> 1, a.H1 - 1);
  uint32_t centre[kFlowSeeds];
  uint32_t distinct = 1;                                          // bit k: centre k differs from every lower one
#pragma unroll
  for (int k = 0; k < kFlowSeeds; k++) {
    const int ox = k == 1 ? -1 : k == 2 ? 1 : 0, oy = k == 3 ? -1 : k == 4 ? 1 : 0;
    const short2 cc = coarse[(size_t)min(max(Y + oy, 0), a.H1 - 1) * a.W1 + min(max(X + ox, 0), a.W1 - 1)];
    centre[k] = (uint32_t)(uint16_t)cc.x | ((uint32_t)(uint16_t)cc.y << 16);
    bool first = true;
#pragma unroll
    for (int j = 0; j < k; j++) first = first && centre[k] != centre[j];
    if (k && first) distinct |= 1u << k;
  }
  uint32_t win_cost = 0xffffffffu;
  short2 win = make_short2(0, 0);
  short4 win_sub = make_short4(0, 0, 0, 0);
  const bool want_sub = a.sub && dir == 0;
#pragma unroll 1
  for (int k = 0; k < kFlowSeeds; k++) {
    const bool mine = (distinct >> k) & 1;
    if (!__any(mine)) continue;                                   // wave-uniform: the common case runs seed 0 alone
    if (mine) {
      uint32_t c = centre[0];
#pragma unroll
      for (int j = 1; j < kFlowSeeds; j++) c = j == k ? centre[j] : c;
      const int cx = 2 * (int)(short)(c & 0xffffu), cy = 2 * (int)(short)(c >> 16);
      const int px0 = x - cx - R - 1, py0 = y - cy - R - 1;        // prev sample (0, 0) of the register block
      const bool inner = nin == all_in && px0 >= 0 && px0 + P <= W && py0 >= 0 && py0 + P <= H;
      uint32_t pv[P * P];
      if (__all(inner)) {
#pragma unroll
        for (int i = 0; i < P; i++)
#pragma unroll
          for (int j = 0; j < P; j++) pv[i * P + j] = cp[(size_t)(py0 + i) * W + px0 + j];
      } else {
#pragma unroll
        for (int i = 0; i < P; i++)
#pragma unroll
          for (int j = 0; j < P; j++) {
            const int px = px0 + j, py = py0 + i;
            pv[i * P + j] = (px >= 0 && px < W && py >= 0 && py < H) ? cp[(size_t)py * W + px] : kOutside;
          }
      }
      uint32_t cost[9];
#pragma unroll
      for (int q = 0; q < 9; q++) cost[q] = 0;
#pragma unroll
      for (int wy = 0; wy < WIN; wy++)
#pragma unroll
        for (int wx = 0; wx < WIN; wx++) {
          const bool on = (nin >> (wy * WIN + wx)) & 1;
#pragma unroll
          for (int ey = -1; ey <= 1; ey++)
#pragma unroll
            for (int ex = -1; ex <= 1; ex++) {
              const uint32_t h = flow_tap(nw[wy * WIN + wx], pv[(wy - ey + 1) * P + (wx - ex + 1)]);
              cost[(ey + 1) * 3 + ex + 1] += on ? h : 0u;
            }
        }
      uint32_t best = 0xffffffffu;
#pragma unroll
      for (int q = 0; q < 9; q++) best = min(best, flow_key(cost[q], q % 3 - 1, q / 3 - 1, q));
      if ((best >> 20) < win_cost) {                              // strictly: ties stay with the lower seed
        const int b = (int)(best & 1023u), bx = b % 3 - 1, by = b / 3 - 1;
        win_cost = best >> 20;
        win = make_short2((short)(cx + bx), (short)(cy + by));
        if (want_sub) win_sub = flow_sub9(cost, bx, by, (int)win_cost);
      }
    }
  }
  const size_t at = (size_t)f * N + (size_t)y * W + x;
  a.out[(size_t)dir * a.frames * N + at] = win;
  if (want_sub) a.sub[at] = win_sub;
}

__device__ __forceinline__ float flow_delta(int num, int den) {
  if (den <= 0) return 0.0f;
  const float d = (float)num / (float)(2 * den);                 // IEEE divide (-fhip-fp32-correctly-rounded-divide-sqrt)
  return fminf(fmaxf(d, -0.5f), 0.5f);
}

// Level-0 integer winners F (and the backward field G when fb >= 0) -> f32 flow: F + sub-pixel delta, NaN where the
// forward-backward check fails.
__global__ __launch_bounds__(256) void k_flow_finish(int W, int H, int frames, const short2 *__restrict__ F, const short2 *__restrict__ G,
                                                     const short4 *__restrict__ sub, int fb, float2 *__restrict__ flow) {
  const int x = blockIdx.x * kTW + threadIdx.x, y = blockIdx.y * kTH + threadIdx.y, f = blockIdx.z;
  if (x >= W || y >= H) return;
  const size_t base = (size_t)f * W * H, at = base + (size_t)y * W + x;
  const short2 d = F[at];
  float2 o = make_float2((float)d.x, (float)d.y);
  if (sub) {
    const short4 s = sub[at];
    o.x = o.x + flow_delta(s.x, s.y);
    o.y = o.y + flow_delta(s.z, s.w);
  }
  if (G) {
    const int px = x - d.x, py = y - d.y;
    bool ok = px >= 0 && px < W && py >= 0 && py < H;
    if (ok) {
      const short2 g = G[base + (size_t)py * W + px];
      ok = abs(d.x + g.x) <= fb && abs(d.y + g.y) <= fb;
    }
    if (!ok) o = make_float2(__builtin_nanf(""), __builtin_nanf(""));
  }
  flow[at] = o;
}

template <int WIN>
void launch_match_win(bool coarse, int seeds, const FlowMatchArgs &a, int dirs, hipStream_t s) {
  const dim3 grid((a.W + kTW - 1) / kTW, (a.H + kTH - 1) / kTH, a.frames * dirs), block(kTW, kTH);
  if (coarse) hipLaunchKernelGGL((k_flow_match<WIN, true>), grid, block, 0, s, a);
  else if (seeds == kFlowSeeds) hipLaunchKernelGGL((k_flow_match_seeds<WIN>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_flow_match<WIN, false>), grid, block, 0, s, a);
}

}  // namespace

void launch_flow_pyramid(int Ws, int Hs, int W, int H, int frames, const uint8_t *src0, const uint8_t *src1, uint8_t *dst, hipStream_t s) {
  const dim3 grid((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, 2 * frames), block(kTW, kTH);
  hipLaunchKernelGGL(k_flow_pyramid, grid, block, 0, s, Ws, Hs, W, H, frames, src0, src1, dst);
}

void launch_flow_match(int W, int H, int W1, int H1, int frames, int dirs, int window, int radius, int seeds, const uint32_t *census,
                       const short2 *coarse, short2 *out, short4 *sub, hipStream_t s) {
  FlowMatchArgs a{W, H, W1, H1, frames, radius, census, coarse, out, sub};
  const bool c = coarse == nullptr;
  if (window == 3) launch_match_win<3>(c, seeds, a, dirs, s);
  else if (window == 5) launch_match_win<5>(c, seeds, a, dirs, s);
  else launch_match_win<7>(c, seeds, a, dirs, s);
}

void launch_flow_finish(int W, int H, int frames, const short2 *F, const short2 *G, const short4 *sub, int fb, float *flow, hipStream_t s) {
  const dim3 grid((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, frames), block(kTW, kTH);
  hipLaunchKernelGGL(k_flow_finish, grid, block, 0, s, W, H, frames, F, G, sub, fb, reinterpret_cast<float2 *>(flow));
}
