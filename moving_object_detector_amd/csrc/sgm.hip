// sgm.hip — on-GPU disparity estimation, the complete estimator (BASELINE config 5).
//
// Replaces sgm_gpu::SgmGpu::computeDisparity, the un-vendored CUDA estimator the reference calls at
// scene_flow_constructor/src/scene_flow_constructor.cpp:35,267; its output contract is the stereo_msgs/DisparityImage consumed at
// disparity_image_proc/src/disparity_image_processor.cpp:25-27,41-42.  The algorithm (centre-symmetric 9 x 7 census, Hamming
// cost over D <= 128 disparities, 8-path semi-global aggregation with P1 / P2, winner-take-all, median, left-right check) and
// every choice the publication leaves open are stated in oracle/sgm_ref.cpp, which these kernels match bit for bit.
// Kernels: census transform, the eight aggregation paths (matching cost computed on the fly, never stored unless asked),
// winner-take-all over the summed paths (left and right disparity), 3 x 3 median, left-right check.
// Disparity offset `off` (mod_set_disparity_offset, 0 .. 128): index d of every volume and map stands for the disparity off + d.  The
// recurrences over d are untouched; the right census word of (x, d) is word x - off - d (the D == 128 kernels shift the right plane's
// base by `off` words, the one-line kernels the column), the border is x < off + d, the right map's column is x - off - d, and the
// left-right kernel adds `off` to what it stores.  off == 0 enqueues the same kernels and gives the same bytes as the estimator
// without the setting.
#include "mod_launch.h"
#include <cstdlib>
#include <string>
#include <type_traits>

namespace {

// Census: block 64 x 4 output pixels, the 72 x 10 input patch staged in LDS (each input byte is used by up to 62 windows).
__global__ __launch_bounds__(256) void k_sgm_census(int W, int H, const uint8_t *__restrict__ img, uint32_t *__restrict__ out) {
  constexpr int TW = 64, TH = 4, PW = TW + 8, PH = TH + 6;
  __shared__ uint8_t t[PH][PW];
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, f = blockIdx.z;
  const size_t fN = (size_t)f * W * H;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  for (int i = tid; i < PW * PH; i += 256) {
    const int py = i / PW, px = i - py * PW, gx = x0 - 4 + px, gy = y0 - 3 + py;
    t[py][px] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? img[fN + (size_t)gy * W + gx] : (uint8_t)0;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x >= W || y >= H) return;
  uint32_t c = 0;
  if (x >= 4 && x < W - 4 && y >= 3 && y < H - 3) {           // border choice of the oracle: windows that leave the image give 0
    const int cx = threadIdx.x + 4, cy = threadIdx.y + 3;
#pragma unroll
    for (int dy = -3; dy <= 0; dy++)
#pragma unroll
      for (int dx = -4; dx <= 4; dx++) {
        if (dy == 0 && dx >= 0) break;
        c = (c << 1) | (t[cy + dy][cx + dx] >= t[cy - dy][cx - dx] ? 1u : 0u);
      }
  }
  out[fN + (size_t)y * W + x] = c;
}

// One horizontal aggregation path over one image row: ONE wave, lane l owns disparities 2l and 2l + 1; the row's census words sit
// in LDS (the right word of disparity d at column x is word x - d: consecutive lanes read consecutive addresses), the previous
// column's path costs in registers: neighbours d +- 1 come through DPP wave shifts, the minimum over d through a DPP reduction.
//   L(x, d) = C(x, d) + min(L(xp, d), L(xp, d-1) + P1, L(xp, d+1) + P1, min_k L(xp, k) + P2) - min_k L(xp, k)
// One step of a path for the lane's two disparities, held as a PACKED pair of 16-bit numbers (low half: disparity 2 * lane, high
// half: disparity 2 * lane + 1; every quantity of the recurrence stays below 2^14): v_pk_min_u16 / v_pk_add_u16 do both at once,
// the neighbours d - 1 / d + 1 are one DPP wave shift + one v_alignbit each, and the pair leaves as ONE 2-byte store.
// `lp` previous path costs (kSgmNone where the disparity does not exist), `c` matching costs -> new path costs.  All 64 lanes active.
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
constexpr uint32_t kSgmNone = 0x3fffu;               // "no such disparity": larger than any cost + penalty, and twice it fits 16 bits
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2, a) + __builtin_bit_cast(us2, b)); }
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2, a) - __builtin_bit_cast(us2, b)); }
// minimum over the wave's 128 packed costs: the two halves, then a DPP butterfly inside each row of 16 lanes, then the rows through
// row_bcast (8 VALU instructions; the s_nop are the two wait states a DPP read of a just-written VGPR needs).  Wave-uniform (SGPR).
__device__ __forceinline__ uint32_t sgm_min128(uint32_t lp) {
  uint32_t v = min(lp & 0xffffu, lp >> 16);
  asm("s_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"
      : "+v"(v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// `prev` / `next` are the DPP shift registers, carried from step to step: a wave shift leaves the lane without a source (lane 0 /
// lane 63) untouched, so those lanes keep the kSgmNone they were initialised with and no constant is re-materialised per step.
struct SgmShift { uint32_t prev, next; };
__device__ __forceinline__ SgmShift sgm_shift_init() { return SgmShift{kSgmNone << 16, kSgmNone}; }
__device__ __forceinline__ uint32_t sgm_step(uint32_t lp, uint32_t c, uint32_t p1pk, uint32_t p2, SgmShift &sh) {
  const uint32_t m = sgm_min128(lp);                                  // min over all disparities
  const uint32_t mpk = m | (m << 16), mp2pk = (m + p2) | ((m + p2) << 16);   // scalar unit
  // d - 1: (high half of lane - 1, own low half); d + 1: (own high half, low half of lane + 1); the ends see kSgmNone
  sh.prev = (uint32_t)__builtin_amdgcn_update_dpp((int)sh.prev, (int)lp, 0x138, 0xF, 0xF, false);   // wave_shr:1
  sh.next = (uint32_t)__builtin_amdgcn_update_dpp((int)sh.next, (int)lp, 0x130, 0xF, 0xF, false);   // wave_shl:1
  const uint32_t a = __builtin_amdgcn_alignbit(lp, sh.prev, 16), b = __builtin_amdgcn_alignbit(sh.next, lp, 16);
  const uint32_t best = pk_min(pk_min(lp, mp2pk), pk_add(pk_min(a, b), p1pk));
  return pk_sub(pk_add(c, best), mpk);
}
// A wave-uniform GLOBAL pointer the compiler must keep in SGPRs, so that loads / stores take the "SGPR base + 32-bit lane offset"
// form instead of a 64-bit add per lane (the readfirstlane is a no-op on a value that is already scalar; it stops the optimiser
// from re-associating the lane offset into the base).
#define SGM_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ SGM_GLOBAL uint8_t *sgm_uniform(const void *p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (SGM_GLOBAL uint8_t *)(((uint64_t)hi << 32) | lo);
}

// where a path's costs go: the path's volume, and (stage tests) the matching cost
struct SgmOut {
  uint8_t *L, *C;       // [H][W][D]; C may be null
};
// lanes whose disparities do not exist (d >= D) keep kSgmNone in that half and store nothing
struct SgmLane {
  uint32_t keep, none;  // masks: halves that exist / kSgmNone in the halves that do not
  bool has0, has1;
};
__device__ __forceinline__ SgmLane sgm_lane(int lane, int D) {
  SgmLane s;
  s.has0 = 2 * lane < D; s.has1 = 2 * lane + 1 < D;
  s.keep = (s.has0 ? 0xffffu : 0u) | (s.has1 ? 0xffff0000u : 0u);
  s.none = (s.has0 ? 0u : kSgmNone) | (s.has1 ? 0u : (kSgmNone << 16));
  return s;
}
__device__ __forceinline__ void sgm_emit(const SgmOut &o, const SgmLane &ln, size_t at, uint32_t lane, uint32_t l, uint32_t c, bool even_d, uint32_t sel) {
  SGM_GLOBAL uint8_t *pl = sgm_uniform(o.L + at), *pc = o.C ? sgm_uniform(o.C + at) : nullptr;
  const uint32_t q = 2 * lane;
  if (ln.has1 && even_d) {                                          // both disparities exist and the pair is 2-byte aligned
    *(SGM_GLOBAL uint16_t *)(pl + q) = (uint16_t)__builtin_amdgcn_perm(0u, l, sel);
    if (pc) *(SGM_GLOBAL uint16_t *)(pc + q) = (uint16_t)__builtin_amdgcn_perm(0u, c, sel);
  } else {
    if (ln.has0) { pl[q] = (uint8_t)(l & 0xffu); if (pc) pc[q] = (uint8_t)(c & 0xffu); }
    if (ln.has1) { pl[q + 1] = (uint8_t)((l >> 16) & 0xffu); if (pc) pc[q + 1] = (uint8_t)((c >> 16) & 0xffu); }
  }
}

// The right census words of a lane's two disparities are neighbours in memory: word x - d1 (d1 = 2 lane + 1) and the one after it
// (x - d0).  They are read as ONE pair at max(x - d1, 0) — never left of the row (a saturating subtraction) — so near the left
// border (x < d1) the pair is (word 0, word 1) and the masked branch below picks word 0 for d0 == x.  Needs W >= 2.
struct SgmPair { uint32_t a, b; };
// matching costs of the lane's two disparities at column x (31 where the disparity leaves the right image); dlast = D - 1.
// With a disparity offset the caller passes x - off (the pair was read at max(x - off, 0)): a negative x takes the branch and
// gets 31 twice
__device__ __forceinline__ uint32_t sgm_cost_pk(uint32_t wl, SgmPair r, int x, int d0, int dlast) {
  uint32_t c = (uint32_t)__popc(wl ^ r.b) + ((uint32_t)__popc(wl ^ r.a) << 16);
  if (x <= dlast) {                                                   // wave-uniform: only the first off + D columns (x == D - 1: an odd D's last
                                                                      // lane owns d0 = x alone, its pair was read at word 0 as well)
    asm volatile("" ::: "memory");                                    // keep this a branch: the other columns skip it
    const uint32_t c0 = x > d0 ? (c & 0xffffu) : x == d0 ? (c >> 16) : 31u;
    const uint32_t c1 = x > d0 ? (c >> 16) : 31u;
    c = c0 | (c1 << 16);
  }
  return c;
}

template <bool RTL>
__global__ __launch_bounds__(64) void k_sgm_path_h(int W, int H, int D, int off, int P1, int P2, const uint32_t *__restrict__ cl,
                                                   const uint32_t *__restrict__ cr, SgmOut out) {
  extern __shared__ uint32_t srow[];                 // [W + 1] right census row, [W] left census row
  const int lane = threadIdx.x, y = blockIdx.x, f = blockIdx.y;
  const size_t row = ((size_t)f * H + y) * W;
  uint32_t *sr = srow, *sl = srow + W + 1;
  for (int i = lane; i < W; i += 64) { sl[i] = cl[row + i]; sr[i] = cr[row + i]; }
  if (lane == 0) sr[W] = 0;                          // W == 1: the pair read at x = 0
  __syncthreads();
  const int d0 = 2 * lane, d1 = 2 * lane + 1, dlast = D - 1;
  const bool even_d = !(D & 1);
  const SgmLane ln = sgm_lane(lane, D);
  const uint32_t p1pk = (uint32_t)P1 | ((uint32_t)P1 << 16);
  uint32_t sel = 0x0c0c0200u;                        // v_perm selector "bytes 0 and 2", pinned to an SGPR outside the loop
  asm volatile("" : "+s"(sel));
  const size_t vol = (size_t)f * H * W * D;
  out.L += vol;
  if (out.C) out.C += vol;
  uint32_t lp = kSgmNone | (kSgmNone << 16);
  // the census words of a step are read one step ahead, unconditionally: their LDS latency hides behind the recurrence of the
  // step before
  auto pair = [&](int xx) { const uint32_t i = __builtin_elementwise_sub_sat((uint32_t)max(xx - off, 0), (uint32_t)d1); SgmPair r; r.a = sr[i]; r.b = sr[i + 1]; return r; };
  SgmShift sh = sgm_shift_init();
  int x = RTL ? W - 1 : 0;
  uint32_t wl = sl[x];
  SgmPair r = pair(x);
  for (int step = 0; step < W; step++) {
    const int xn = min(max(RTL ? x - 1 : x + 1, 0), W - 1);
    const uint32_t wln = sl[xn];
    const SgmPair rn = pair(xn);
    const uint32_t c = sgm_cost_pk(wl, r, x - off, d0, dlast);
    uint32_t l = step > 0 ? sgm_step(lp, c, p1pk, (uint32_t)P2, sh) : c;
    l = (l & ln.keep) | ln.none;
    sgm_emit(out, ln, ((size_t)y * W + x) * D, lane, l, c, even_d, sel);
    lp = l;
    x = RTL ? x - 1 : x + 1;
    wl = wln; r = rn;
  }
}

// Vertical and diagonal paths: one wave per path LINE (direction (RX, RY), RY != 0).  Lines enter through the first row in path
// order (W of them) and, for the diagonals, through the first column in path order (H - 1 more).  Census words come straight from
// L2 / HBM (one 8-byte load per lane, see SgmPair), kPF steps ahead of their use: the recurrence is a dependent chain per step, a
// memory round trip per step would dominate it.
constexpr int kSgmPF = 4;
template <int RX, int RY>
__global__ __launch_bounds__(64) void k_sgm_path_line(int W, int H, int D, int off, int P1, int P2, const uint32_t *__restrict__ cl,
                                                      const uint32_t *__restrict__ cr, SgmOut out) {
  const int lane = threadIdx.x, line = blockIdx.x, f = blockIdx.y;
  int x, y;
  if (line < W) { x = RX < 0 ? W - 1 - line : line; y = RY > 0 ? 0 : H - 1; }   // long lines first (they enter at the far end when RX < 0)
  else { x = RX > 0 ? 0 : W - 1; y = RY > 0 ? line - W + 1 : H - 2 - (line - W); }   // the entry row's own pixel is a row line
  const size_t plane = (size_t)f * H * W, vol = plane * D;
  cl += plane; cr += plane;
  out.L += vol;
  if (out.C) out.C += vol;
  const int d0 = 2 * lane, d1 = 2 * lane + 1, dlast = D - 1;
  const bool even_d = !(D & 1);
  const SgmLane ln = sgm_lane(lane, D);
  const uint32_t p1pk = (uint32_t)P1 | ((uint32_t)P1 << 16);
  uint32_t sel = 0x0c0c0200u;                        // v_perm selector "bytes 0 and 2", pinned to an SGPR outside the loop
  asm volatile("" : "+s"(sel));
  // number of pixels on the line
  int len = RY > 0 ? H - y : y + 1;
  if (RX > 0) len = min(len, W - x);
  if (RX < 0) len = min(len, x + 1);
  auto fetch = [&](int i, uint32_t &wl, SgmPair &r) {                  // census words of the line's i-th pixel (clamped to the line)
    const int k = min(i, len - 1), xx = x + RX * k, yy = y + RY * k;
    const size_t rowp = (size_t)yy * W;
    wl = cl[rowp + xx];
    const SGM_GLOBAL uint32_t *q = (const SGM_GLOBAL uint32_t *)(sgm_uniform(cr + rowp) + 4u * __builtin_elementwise_sub_sat((uint32_t)max(xx - off, 0), (uint32_t)d1));
    r.a = q[0]; r.b = q[1];
  };
  uint32_t wl[kSgmPF];
  SgmPair r[kSgmPF];
#pragma unroll
  for (int i = 0; i < kSgmPF; i++) fetch(i, wl[i], r[i]);
  uint32_t lp = kSgmNone | (kSgmNone << 16);
  SgmShift sh = sgm_shift_init();
  for (int i0 = 0; i0 < len; i0 += kSgmPF) {         // wave-uniform
#pragma unroll
    for (int u = 0; u < kSgmPF; u++) {
      const int i = i0 + u;
      if (i >= len) break;                           // wave-uniform
      const int xx = x + RX * i, yy = y + RY * i;
      const uint32_t c = sgm_cost_pk(wl[u], r[u], xx - off, d0, dlast);
      fetch(i + kSgmPF, wl[u], r[u]);                // slot u is free again: the words of pixel i + kPF
      uint32_t l = i > 0 ? sgm_step(lp, c, p1pk, (uint32_t)P2, sh) : c;
      l = (l & ln.keep) | ln.none;
      sgm_emit(out, ln, ((size_t)yy * W + xx) * D, lane, l, c, even_d, sel);
      lp = l;
    }
  }
}

// FOUR path lines per wave (D == 128): lane = (line q of the wave's four, slot t of 16), slot t owns the EIGHT disparities
// 8t .. 8t + 7 as four packed pairs.  Against one line per wave (lane = two disparities, above):
//   * the minimum over the 128 disparities is 3 packed minima inside the lane + 4 DPP steps inside the 16-lane row (quad swaps, half
//     mirror, mirror) and stays in a vector register — no row_bcast steps, no v_readlane, no scalar round trip per step;
//   * six of the eight d - 1 / d + 1 neighbours are register moves (v_alignbit between the lane's own pairs); only the pair ends
//     cross a lane (one row_shr:1 and one row_shl:1 per step);
//   * one 8-byte store per lane and step; the lane's eight right census words are eight CONSECUTIVE words (two 16-byte loads).
// ~70 vector instructions per step of four lines (17 per line step, one-line kernels: ~30) and a shorter dependent chain.
// The four lines of a wave are neighbours (rows / columns / diagonals next to each other); they may differ in length by a few
// pixels: a line that has ended keeps computing on its last pixel and stores nothing.
constexpr int kSgmPrefetch = 2;   // census slots in flight per line (steps of prefetch; 1 .. 4 measured, no difference)
typedef uint32_t sgm_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t sgm_u2 __attribute__((ext_vector_type(2)));
// UNIFORM: the wave's four lines exist and have one length (rows / columns of an image whose height / width is a multiple of 4):
// every step stores unconditionally, so the compiler can count the memory operations in flight and the wait in front of a census
// slot leaves the younger slot's loads outstanding (a conditional store makes it wait for everything).  COST: also emit the
// matching cost (stage entry point only).
template <int RX, int RY, bool UNIFORM, bool COST>
__device__ __forceinline__ void sgm_path_q_body(int W, int H, int off, int P1, int P2, const uint32_t *__restrict__ cl, const uint32_t *__restrict__ cr,
                                                SgmOut out, int blk, int f) {
  constexpr int D = 128, kPF = kSgmPrefetch;
  const int lane = threadIdx.x, q = lane >> 4, t = lane & 15;
  const int nlines = RY == 0 ? H : (RX == 0 ? W : W + H - 1);
  const int line = blk * 4 + q;
  int x = 0, y = 0, len = 0;
  if (line < nlines) {
    if (RY == 0) { y = line; x = RX > 0 ? 0 : W - 1; len = W; }
    else {
      if (line < W) { x = RX < 0 ? W - 1 - line : line; y = RY > 0 ? 0 : H - 1; }
      else { x = RX > 0 ? 0 : W - 1; y = RY > 0 ? line - W + 1 : H - 2 - (line - W); }
      len = RY > 0 ? H - y : y + 1;
      if (RX > 0) len = min(len, W - x);
      if (RX < 0) len = min(len, x + 1);
    }
  }
  const int maxlen = max(max(__builtin_amdgcn_readlane(len, 0), __builtin_amdgcn_readlane(len, 16)),
                         max(__builtin_amdgcn_readlane(len, 32), __builtin_amdgcn_readlane(len, 48)));
  const size_t plane = (size_t)f * H * W, vol = plane * D;
  // the right plane's base `off` words early: word x - d of it is the plane's word x - off - d, and every load below stays as it is
  SGM_GLOBAL uint8_t *cl_b = sgm_uniform(cl + plane), *cr_b = sgm_uniform((cr + plane) - off);
  SGM_GLOBAL uint8_t *outL = sgm_uniform(out.L + vol), *outC = COST ? sgm_uniform(out.C + vol) : nullptr;
  const uint32_t p1pk = (uint32_t)P1 | ((uint32_t)P1 << 16), p2pk = (uint32_t)P2 | ((uint32_t)P2 << 16);
  const int dbase = 8 * t;
  // census words of the line's k-th pixel (clamped to the line): the left word, and the eight right words x - dbase - 7 .. x - dbase
  // of the shifted plane (word j of the window belongs to disparity index dbase + 7 - j).  Where a window starts left of the row
  // (x < off + 127 somewhere in the wave) the words in front of the row belong to disparities that do not exist: they get the border
  // cost below, whatever was read.
  struct Slot { uint32_t wl; uint32_t r[8]; };
  auto fetch = [&](int k, Slot &sl) {
    const int kk = max(min(k, len - 1), 0), xx = x + RX * kk, yy = y + RY * kk;
    const uint32_t rowo = (uint32_t)(yy * W) * 4u;
    sl.wl = *(const SGM_GLOBAL uint32_t *)(cl_b + (rowo + (uint32_t)xx * 4u));
    // ALWAYS the same three loads (the compiler can then count them: the wait before a slot's use leaves the younger slot's loads
    // in flight).  Near the left border the window starts left of the row — in the row above, or (first row of the plane) up to
    // off + 127 <= kSgmCensusLead - 1 words before the plane: the caller guarantees those bytes are readable; the words read there
    // belong to disparities that do not exist and are replaced by the border cost.
    const SGM_GLOBAL sgm_u4 *w = (const SGM_GLOBAL sgm_u4 *)(cr_b + (int32_t)(rowo + (uint32_t)(xx - dbase - 7) * 4u));
    const sgm_u4 a = w[0], b = w[1];
    sl.r[0] = a.x; sl.r[1] = a.y; sl.r[2] = a.z; sl.r[3] = a.w; sl.r[4] = b.x; sl.r[5] = b.y; sl.r[6] = b.z; sl.r[7] = b.w;
  };
  Slot slot[kPF];
#pragma unroll
  for (int u = 0; u < kPF; u++) fetch(u, slot[u]);
  uint32_t lp[4] = {0, 0, 0, 0};
  uint32_t shp = kSgmNone << 16, shn = kSgmNone;       // DPP shift registers: the row's end lanes keep "no such disparity"
  for (int i0 = 0; i0 < maxlen; i0 += kPF) {            // wave-uniform
#pragma unroll
    for (int u = 0; u < kPF; u++) {
      const int i = i0 + u;
      if (i >= maxlen) break;                           // wave-uniform
      const int kk = max(min(i, len - 1), 0), xx = x + RX * kk, yy = y + RY * kk;
      // matching costs of the lane's eight disparities (31 where the disparity leaves the right image)
      uint32_t c[4];
#pragma unroll
      for (int j = 0; j < 4; j++)
        c[j] = (uint32_t)__popc(slot[u].wl ^ slot[u].r[7 - 2 * j]) + ((uint32_t)__popc(slot[u].wl ^ slot[u].r[6 - 2 * j]) << 16);
      if (!__all(xx >= off + D - 1)) {                  // wave-uniform: only near the left border, the first off + D - 1 columns
        const int nvalid = xx - off - dbase + 1;        // indices dbase .. dbase + nvalid - 1 exist (off + d <= x)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t lo = 2 * j < nvalid ? (c[j] & 0xffffu) : 31u, hi = 2 * j + 1 < nvalid ? (c[j] >> 16) : 31u;
          c[j] = lo | (hi << 16);
        }
      }
      fetch(i + kPF, slot[u]);                          // the slot is free again
      uint32_t l[4];
      if (i > 0) {
        // minimum over the line's 128 path costs: inside the lane, then a butterfly over the row's 16 lanes
        uint32_t m = pk_min(pk_min(lp[0], lp[1]), pk_min(lp[2], lp[3]));
        m = min(m & 0xffffu, m >> 16);
        asm("s_nop 1\n\t"
            "v_min_u32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
            "v_min_u32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
            "v_min_u32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
            "v_min_u32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1"
            : "+v"(m));
        const uint32_t mpk = m | (m << 16), mp2pk = pk_add(mpk, p2pk);
        shp = (uint32_t)__builtin_amdgcn_update_dpp((int)shp, (int)lp[3], 0x111, 0xF, 0xF, false);   // row_shr:1: the slot below's last pair
        shn = (uint32_t)__builtin_amdgcn_update_dpp((int)shn, (int)lp[0], 0x101, 0xF, 0xF, false);   // row_shl:1: the slot above's first pair
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t below = j == 0 ? shp : lp[j - 1], above = j == 3 ? shn : lp[j + 1];
          const uint32_t a = __builtin_amdgcn_alignbit(lp[j], below, 16), b = __builtin_amdgcn_alignbit(above, lp[j], 16);   // d - 1, d + 1
          const uint32_t best = pk_min(pk_min(lp[j], mp2pk), pk_add(pk_min(a, b), p1pk));
          l[j] = pk_sub(pk_add(c[j], best), mpk);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) l[j] = c[j];
      }
      if (UNIFORM || i < len) {                         // lines that have ended store nothing
        const uint32_t at = (uint32_t)(yy * W + xx) * (uint32_t)D + (uint32_t)dbase;
        sgm_u2 v;
        v.x = __builtin_amdgcn_perm(l[1], l[0], 0x06040200u); v.y = __builtin_amdgcn_perm(l[3], l[2], 0x06040200u);
        __builtin_nontemporal_store(v, (SGM_GLOBAL sgm_u2 *)(outL + at));
        if (COST) {
          v.x = __builtin_amdgcn_perm(c[1], c[0], 0x06040200u); v.y = __builtin_amdgcn_perm(c[3], c[2], 0x06040200u);
          *(SGM_GLOBAL sgm_u2 *)(outC + at) = v;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) lp[j] = l[j];
    }
  }
}

template <int RX, int RY, bool UNIFORM, bool COST>
__global__ __launch_bounds__(64) void k_sgm_path_q(int W, int H, int off, int P1, int P2, const uint32_t *__restrict__ cl,
                                                   const uint32_t *__restrict__ cr, SgmOut out) {
  sgm_path_q_body<RX, RY, UNIFORM, COST>(W, H, off, P1, P2, cl, cr, out, (int)blockIdx.x, (int)blockIdx.y);
}

// All aggregation paths of a group of frames in ONE launch: blockIdx.x runs over the four-line blocks of direction 0, then 1, ...
// (the rows first: they are the longest lines, 1280 steps at 720p).  One grid instead of eight kernels on eight streams: the HIP
// runtime maps streams onto 4 hardware queues by default, so only four of the eight path kernels ever ran side by side (kernel
// trace of round 3) and the short ones queued behind the long ones; inside one grid the dispatcher fills every free wave slot
// with whatever block is next.  Path i writes its volume at out.L + i * path_stride.
template <bool UH, bool UV>
__global__ __launch_bounds__(64) void k_sgm_paths_all(int W, int H, int off, int P1, int P2, int paths, size_t path_stride, const uint32_t *__restrict__ cl,
                                                      const uint32_t *__restrict__ cr, uint8_t *__restrict__ L) {
  const int nh = (H + 3) / 4, nv = (W + 3) / 4, nd = (W + H - 1 + 3) / 4;
  int blk = (int)blockIdx.x;
  const int f = (int)blockIdx.y;
  SgmOut o{L, nullptr};
  // numbering of oracle/sgm_ref.cpp: 0 (+1,0) 1 (-1,0) 2 (0,+1) 3 (0,-1) 4 (+1,+1) 5 (-1,-1) 6 (-1,+1) 7 (+1,-1)
  if (blk < nh) { sgm_path_q_body<1, 0, UH, false>(W, H, off, P1, P2, cl, cr, o, blk, f); return; }
  blk -= nh; o.L += path_stride;
  if (blk < nh) { sgm_path_q_body<-1, 0, UH, false>(W, H, off, P1, P2, cl, cr, o, blk, f); return; }
  blk -= nh; o.L += path_stride;
  if (blk < nv) { sgm_path_q_body<0, 1, UV, false>(W, H, off, P1, P2, cl, cr, o, blk, f); return; }
  blk -= nv; o.L += path_stride;
  if (blk < nv) { sgm_path_q_body<0, -1, UV, false>(W, H, off, P1, P2, cl, cr, o, blk, f); return; }
  if (paths <= 4) return;
  blk -= nv; o.L += path_stride;
  if (blk < nd) { sgm_path_q_body<1, 1, false, false>(W, H, off, P1, P2, cl, cr, o, blk, f); return; }
  blk -= nd; o.L += path_stride;
  if (blk < nd) { sgm_path_q_body<-1, -1, false, false>(W, H, off, P1, P2, cl, cr, o, blk, f); return; }
  blk -= nd; o.L += path_stride;
  if (blk < nd) { sgm_path_q_body<-1, 1, false, false>(W, H, off, P1, P2, cl, cr, o, blk, f); return; }
  blk -= nd; o.L += path_stride;
  sgm_path_q_body<1, -1, false, false>(W, H, off, P1, P2, cl, cr, o, blk, f);
}

// Winner-take-all over the sum of the path volumes, one workgroup (4 waves) per image row.  A wave takes every fourth pixel:
// lane l owns disparities 2l and 2l + 1 (one 2-byte load per path volume), sums the paths, and
//   left  disparity of x : first minimum of S(x, .)              -> DPP minimum over keys (S << 8 | d): the smallest d wins ties
//   right disparity of x': first minimum of S(x' + d, d), x' + d < W -> the pixel x contributes its S(x, d) to x' = x - d with an LDS
//                          atomicMin on the same keys (one row of keys in LDS): the cost volume is read ONCE, coalesced, instead of
//                          gathering a diagonal per pixel.  With a disparity offset the column is x' = x - off - d, and a column no pixel
//                          contributes to (x' + off >= W) gets 0
//
// SUB (the sub-pixel mode, mod_set_disparity_subpixel): the left map holds v = 16 d + q, q the vertex of the parabola through
// S(x, d - 1), S(x, d), S(x, d + 1) in sixteenths (sgm_fraction).  The keys, the reduction and the right map are those of the
// integer kernel; the winner's neighbours may live in the adjacent lane, so every lane fetches its two outer neighbours with one DPP
// shift each way while all 64 lanes are active, and the ONE lane that owns the winner computes the fraction — one division per
// pixel, after the reduction — and stores the pixel.
//
// q = floor((16 num + den) / (2 den)), num = cm - cp, den = cm - 2 c0 + cp, for 1 <= d <= D - 2, else 0.  d is the FIRST minimum:
// cm > c0 <= cp, hence den >= 1 and |num| <= den: -8 <= q <= 8, and 16 num + 17 den >= 1 — the truncating unsigned division of
// that, minus 8, is the floor (the intermediate 16 * (cm - cp) may wrap; the sum does not).
__device__ __forceinline__ uint32_t sgm_fraction(uint32_t cm, uint32_t c0, uint32_t cp, uint32_t d, int D) {
  if (d < 1u || d + 2u > (uint32_t)D) return 16u * d;
  const uint32_t den = cm - 2u * c0 + cp;
  return 16u * d + (16u * (cm - cp) + 17u * den) / (2u * den) - 8u;
}

//
// UNIQ (the uniqueness test, mod_set_disparity_filters; StereoSGBM's rule, left map only): after the reduction that found the winner
// d with m = S(x, d), a second reduction of the same shape over the keys whose disparity is at least 2 away gives s2 = min S(x, d'),
// |d' - d| >= 2; the lane that stores the pixel rejects it iff such a d' exists and s2 * (100 - u) < m * 100 (S <= 8 * 255: no
// overflow) and stores the marker kSgmRejected<TL> instead — the largest value of the map's type (real values reach 127 / 2040), an
// ordinary value to the median, -1 behind the left-right kernels.  The right map is untouched.
template <class TL> constexpr uint32_t kSgmRejected = sizeof(TL) == 1 ? 255u : 65535u;
__device__ __forceinline__ uint32_t sgm_far_key(uint32_t key, uint32_t d) {   // the key, unless its disparity is the winner's or next to it
  const uint32_t kd = key & 255u;
  return kd + 1u >= d && kd <= d + 1u ? 0xffffffffu : key;
}
__device__ __forceinline__ bool sgm_ambiguous(uint32_t best, uint32_t second, int u) {
  return second != 0xffffffffu && (second >> 8) * (uint32_t)(100 - u) < (best >> 8) * 100u;
}

template <bool SUB, class TL, bool UNIQ>
__global__ __launch_bounds__(256) void k_sgm_wta(int W, int H, int D, int off, int paths, size_t path_stride, const uint8_t *__restrict__ Lv,
                                                 TL *__restrict__ dl, uint8_t *__restrict__ dr, int u) {
  extern __shared__ uint32_t rkey[];                 // [W]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, y = blockIdx.x, f = blockIdx.y;
  const size_t plane = (size_t)f * W * H;
  Lv += plane * D; dl += plane; dr += plane;
  for (int i = threadIdx.x; i < W; i += 256) rkey[i] = 0xffffffffu;
  __syncthreads();
  const int d0 = 2 * lane, d1 = d0 + 1;
  for (int x = wv; x < W; x += 4) {
    const size_t at = ((size_t)y * W + x) * D;
    uint32_t s0 = 0, s1 = 0;
    if (d0 < D) {
      for (int p = 0; p < paths; p++) {
        const uint8_t *q = Lv + (size_t)p * path_stride + at + d0;
        if (d1 < D && !(D & 1)) { const uint32_t v = *reinterpret_cast<const uint16_t *>(q); s0 += v & 255u; s1 += v >> 8; }   // even D: 2-byte aligned
        else { s0 += q[0]; if (d1 < D) s1 += q[1]; }
      }
    }
    const uint32_t k0 = d0 < D ? ((s0 << 8) | (uint32_t)d0) : 0xffffffffu, k1 = d1 < D ? ((s1 << 8) | (uint32_t)d1) : 0xffffffffu;
    const uint32_t kl = wave_min_u32(min(k0, k1));
    bool rejected = false;
    if constexpr (UNIQ) rejected = sgm_ambiguous(kl, wave_min_u32(min(sgm_far_key(k0, kl & 255u), sgm_far_key(k1, kl & 255u))), u);
    if constexpr (!SUB) {
      if (lane == 0) dl[(size_t)y * W + x] = (uint8_t)(rejected ? kSgmRejected<TL> : (kl & 255u));
    } else {
      // S(x, d0 - 1), S(x, d1 + 1): the neighbouring lanes' sums (all 64 lanes are active here)
      const uint32_t below = MOD_DPP(s1, 0x138), above = MOD_DPP(s0, 0x130);   // wave_shr:1, wave_shl:1
      const uint32_t d = kl & 255u;
      if ((uint32_t)lane == (d >> 1))                // the lane that owns the winner
        dl[(size_t)y * W + x] = (TL)(rejected ? kSgmRejected<TL> : (d & 1u) ? sgm_fraction(s0, kl >> 8, above, d, D) : sgm_fraction(below, kl >> 8, s1, d, D));
    }
    if (d0 < D && x - off - d0 >= 0) atomicMin(&rkey[x - off - d0], k0);
    if (d1 < D && x - off - d1 >= 0) atomicMin(&rkey[x - off - d1], k1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < W; i += 256) dr[(size_t)y * W + i] = (uint8_t)(rkey[i] == 0xffffffffu ? 0u : rkey[i] & 255u);
}

// The same for disparity counts that are multiples of 16 (the default 128 is): lane = (pixel of the wave's group of 8, 16 consecutive
// disparities) — one 16-byte load per path and lane, a wave reads 1 KB contiguous per path; the path costs are summed as packed pairs
// of 16-bit numbers (sums stay below 8 x 128), the minimum over a pixel's 8 lanes is three DPP steps.
// SUB: as above.  After the butterfly all 8 lanes of the pixel hold the winning key; lane d / 16 owns the winner and finds its two
// neighbours among its own 16 sums or, for the first / last of them, in the sum the adjacent lane passed over (row_shr:1 /
// row_shl:1 before the reduction; the lane across a pixel boundary is only ever asked for d = 0 or d = D - 1, which have no fraction).
// UNIQ: as above.  The second minimum runs over the lane's 16 keys again with those next to the winner masked, then through the same
// three DPP steps; every lane of the pixel holds it, so whichever lane stores the pixel does the one compare.
template <bool SUB, class TL, bool UNIQ>
__global__ __launch_bounds__(256) void k_sgm_wta16(int W, int H, int D, int off, int paths, size_t path_stride, const uint8_t *__restrict__ Lv,
                                                   TL *__restrict__ dl, uint8_t *__restrict__ dr, int u) {
  extern __shared__ uint32_t rkey[];                 // [W]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, y = blockIdx.x, f = blockIdx.y;
  const size_t plane = (size_t)f * W * H;
  Lv += plane * D; dl += plane; dr += plane;
  for (int i = threadIdx.x; i < W; i += 256) rkey[i] = 0xffffffffu;
  __syncthreads();
  const int sub = lane & 7, px = lane >> 3, dbase = sub * 16;
  const bool has = dbase < D;                        // D / 16 lanes of a pixel carry disparities
  for (int x0 = wv * 8; x0 < W; x0 += 32) {
    const int x = x0 + px;
    const bool live = has && x < W;
    uint32_t e[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};          // packed sums: e[j] = (byte 0 | byte 2 << 16) of word j, o[j] = (byte 1 | byte 3 << 16)
    if (live) {
      const uint8_t *q = Lv + ((size_t)y * W + x) * D + dbase;
      for (int p = 0; p < paths; p++) {
        typedef uint32_t wta_u4 __attribute__((ext_vector_type(4)));
        const wta_u4 wv_ = __builtin_nontemporal_load(reinterpret_cast<const wta_u4 *>(q + (size_t)p * path_stride));
        uint4 w; w.x = wv_.x; w.y = wv_.y; w.z = wv_.z; w.w = wv_.w;
        e[0] += w.x & 0x00ff00ffu; o[0] += (w.x >> 8) & 0x00ff00ffu;
        e[1] += w.y & 0x00ff00ffu; o[1] += (w.y >> 8) & 0x00ff00ffu;
        e[2] += w.z & 0x00ff00ffu; o[2] += (w.z >> 8) & 0x00ff00ffu;
        e[3] += w.w & 0x00ff00ffu; o[3] += (w.w >> 8) & 0x00ff00ffu;
      }
    }
    uint32_t edge_lo = 0, edge_hi = 0;               // S(x, dbase - 1), S(x, dbase + 16) (all 64 lanes active)
    if constexpr (SUB) { edge_lo = MOD_DPP(o[3], 0x111) >> 16; edge_hi = MOD_DPP(e[0], 0x101) & 0xffffu; }   // row_shr:1, row_shl:1
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t d = (uint32_t)(dbase + 4 * j);
      const uint32_t k0 = ((e[j] & 0xffffu) << 8) | d, k1 = ((o[j] & 0xffffu) << 8) | (d + 1), k2 = ((e[j] >> 16) << 8) | (d + 2), k3 = ((o[j] >> 16) << 8) | (d + 3);
      if (live) {
        best = min(best, min(min(k0, k1), min(k2, k3)));
        const int xr = x - off - (int)d;
        if (xr >= 0) atomicMin(&rkey[xr], k0);
        if (xr >= 1) atomicMin(&rkey[xr - 1], k1);
        if (xr >= 2) atomicMin(&rkey[xr - 2], k2);
        if (xr >= 3) atomicMin(&rkey[xr - 3], k3);
      }
    }
    // minimum over the 8 lanes of the pixel: quad swaps, then the mirror of the half row (lanes 0..7 <-> 7..0)
    uint32_t t;
    t = MOD_DPP(best, 0xB1); best = min(best, t);
    t = MOD_DPP(best, 0x4E); best = min(best, t);
    t = MOD_DPP(best, 0x141); best = min(best, t);
    bool rejected = false;
    if constexpr (UNIQ) {
      const uint32_t dw = best & 255u;
      uint32_t second = 0xffffffffu;
      if (live) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t d = (uint32_t)(dbase + 4 * j);
          const uint32_t k0 = ((e[j] & 0xffffu) << 8) | d, k1 = ((o[j] & 0xffffu) << 8) | (d + 1), k2 = ((e[j] >> 16) << 8) | (d + 2), k3 = ((o[j] >> 16) << 8) | (d + 3);
          second = min(second, min(min(sgm_far_key(k0, dw), sgm_far_key(k1, dw)), min(sgm_far_key(k2, dw), sgm_far_key(k3, dw))));
        }
      }
      t = MOD_DPP(second, 0xB1); second = min(second, t);
      t = MOD_DPP(second, 0x4E); second = min(second, t);
      t = MOD_DPP(second, 0x141); second = min(second, t);
      rejected = sgm_ambiguous(best, second, u);
    }
    if constexpr (!SUB) {
      if (sub == 0 && x < W) dl[(size_t)y * W + x] = (uint8_t)(rejected ? kSgmRejected<TL> : (best & 255u));
    } else {
      const uint32_t d = best & 255u;
      if ((d >> 4) == (uint32_t)sub && x < W) {      // the lane that owns the winner (a dead pixel's key names disparity 255: nobody)
        // sum i = d % 16 sits in word j = i / 4 at place k = i % 4: e[j] low, o[j] low, e[j] high, o[j] high
        const uint32_t j = (d >> 2) & 3u, k = d & 3u;
        const uint32_t ej = j == 0 ? e[0] : j == 1 ? e[1] : j == 2 ? e[2] : e[3], oj = j == 0 ? o[0] : j == 1 ? o[1] : j == 2 ? o[2] : o[3];
        const uint32_t before = j == 0 ? edge_lo : (j == 1 ? o[0] : j == 2 ? o[1] : o[2]) >> 16;         // the sum in front of word j
        const uint32_t after = j == 3 ? edge_hi : (j == 0 ? e[1] : j == 1 ? e[2] : e[3]) & 0xffffu;      // the sum behind it
        const uint32_t cm = k == 0 ? before : k == 1 ? (ej & 0xffffu) : k == 2 ? (oj & 0xffffu) : (ej >> 16);
        const uint32_t cp = k == 0 ? (oj & 0xffffu) : k == 1 ? (ej >> 16) : k == 2 ? (oj >> 16) : after;
        dl[(size_t)y * W + x] = (TL)(rejected ? kSgmRejected<TL> : sgm_fraction(cm, best >> 8, cp, d, D));
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < W; i += 256) dr[(size_t)y * W + i] = (uint8_t)(rkey[i] == 0xffffffffu ? 0u : rkey[i] & 255u);
}

// 3 x 3 median of a uint8 map, or of the sub-pixel mode's uint16 left map (border pixels keep their value): exact 9-element
// selection network
__device__ __forceinline__ void srt(int &a, int &b) { const int t = min(a, b); b = max(a, b); a = t; }
template <class T>
__global__ __launch_bounds__(256) void k_sgm_median3(int W, int H, const T *__restrict__ in, T *__restrict__ out) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  in += (size_t)blockIdx.z * W * H; out += (size_t)blockIdx.z * W * H;
  const size_t p = (size_t)y * W + x;
  if (x == 0 || y == 0 || x == W - 1 || y == H - 1) { out[p] = in[p]; return; }
  int v0 = in[p - W - 1], v1 = in[p - W], v2 = in[p - W + 1], v3 = in[p - 1], v4 = in[p], v5 = in[p + 1], v6 = in[p + W - 1], v7 = in[p + W], v8 = in[p + W + 1];
  srt(v1, v2); srt(v4, v5); srt(v7, v8); srt(v0, v1); srt(v3, v4); srt(v6, v7); srt(v1, v2); srt(v4, v5); srt(v7, v8);
  srt(v0, v3); srt(v5, v8); srt(v4, v7); srt(v3, v6); srt(v1, v4); srt(v2, v5); srt(v4, v7); srt(v4, v2); srt(v6, v4); srt(v4, v2);
  out[p] = (T)v4;
}

// left-right consistency check -> DisparityImage pixels (float, -1 = invalid).  A uint8 left map stores d itself; the sub-pixel mode's
// uint16 map stores v = 16 d + q: the check runs on the nearest integer, the pixel leaves as v / 16 (exact).  UNIQ: the marker of a
// pixel the uniqueness test (or the median of a rejected patch) left is -1 whatever the check says.  off: the disparity offset — the
// maps hold indices, the matching right column is x - off - d, the pixel leaves as off + its value (exact: at most 255.5)
template <class TL, bool UNIQ>
__global__ __launch_bounds__(256) void k_sgm_lr(int W, int H, int off, int lr_check, const TL *__restrict__ dl, const uint8_t *__restrict__ dr,
                                                float *__restrict__ disp) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  const size_t plane = (size_t)blockIdx.z * W * H;
  dl += plane; dr += plane; disp += plane;
  const size_t p = (size_t)y * W + x;
  const int v = dl[p], d = sizeof(TL) == 1 ? v : (v + 8) >> 4;
  bool ok = true;
  const int xs = x - off - d;
  if (lr_check) ok = xs >= 0 && abs((int)dr[(size_t)y * W + max(xs, 0)] - d) <= 1;
  if (UNIQ && v == (int)kSgmRejected<TL>) ok = false;
  disp[p] = ok ? (sizeof(TL) == 1 ? (float)(off + d) : (float)v * 0.0625f + (float)off) : -1.0f;
}

}  // namespace

void launch_sgm_census(int W, int H, int frames, const uint8_t *img, uint32_t *out, hipStream_t s) {
  hipLaunchKernelGGL(k_sgm_census, dim3((W + 63) / 64, (H + 3) / 4, frames), dim3(64, 4, 1), 0, s, W, H, img, out);
}

// The reference's numbering of the aggregation directions (oracle/sgm_ref.cpp): direction -> (RX, RY), the step along a path
constexpr int kSgmDir[kSgmPaths][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {-1, 1}, {1, -1}};

// f(std::integral_constant<int, direction>) (a number outside the table goes as the last direction), and f(std::bool_constant<flags>...):
// where run-time choices become template arguments
template <int I = 0, class F>
static void with_direction(int direction, F &&f) {
  if constexpr (I + 1 < kSgmPaths) { if (direction != I) return with_direction<I + 1>(direction, f); }
  f(std::integral_constant<int, I>{});
}
template <class F>
static void with_flags(F &&f) { f(); }
template <class F, class... B>
static void with_flags(F &&f, bool flag, B... rest) {
  if (flag) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

void launch_sgm_path(int W, int H, int frames, int D, int off, int P1, int P2, int direction, const uint32_t *cl, const uint32_t *cr,
                     uint8_t *L, uint8_t *cost, hipStream_t s) {
  SgmOut o{L, cost};
  with_direction(direction, [&](auto dir) {
    constexpr int RX = kSgmDir[dir.value][0], RY = kSgmDir[dir.value][1];
    const int lines = RY == 0 ? H : RX == 0 ? W : W + H - 1;     // rows, columns, diagonals
    // D == 128 (the published configuration): four lines per wave (UNIFORM: no partial quad of rows / columns); the one-line kernels
    // serve every other disparity count
    if (D == 128)
      with_flags([&](auto uniform, auto costs) {
        hipLaunchKernelGGL((k_sgm_path_q<RX, RY, uniform.value, costs.value>), dim3((lines + 3) / 4, frames), dim3(64), 0, s, W, H, off, P1, P2, cl, cr, o);
      }, (RX == 0 || RY == 0) && (lines & 3) == 0, cost != nullptr);
    else if constexpr (RY == 0)
      hipLaunchKernelGGL(k_sgm_path_h<(RX < 0)>, dim3(lines, frames), dim3(64), ((size_t)2 * W + 1) * sizeof(uint32_t), s, W, H, D, off, P1, P2, cl, cr, o);
    else
      hipLaunchKernelGGL((k_sgm_path_line<RX, RY>), dim3(lines, frames), dim3(64), 0, s, W, H, D, off, P1, P2, cl, cr, o);
  });
}

// every path of the published configuration (D == 128) in one grid; returns false when the combination is not covered (other D,
// other path counts): the caller then launches the paths one by one
bool launch_sgm_paths_all(int W, int H, int frames, int D, int off, int P1, int P2, int paths, size_t path_stride, const uint32_t *cl, const uint32_t *cr,
                          uint8_t *L, hipStream_t s) {
  if (D != 128 || (paths != 8 && paths != 4)) return false;
  const int nh = (H + 3) / 4, nv = (W + 3) / 4, nd = (W + H - 1 + 3) / 4;
  const dim3 g(2 * nh + 2 * nv + (paths == 8 ? 4 * nd : 0), frames), b(64);
  with_flags([&](auto uh, auto uv) {
    hipLaunchKernelGGL((k_sgm_paths_all<uh.value, uv.value>), g, b, 0, s, W, H, off, P1, P2, paths, path_stride, cl, cr, L);
  }, (H & 3) == 0, (W & 3) == 0);
  return true;
}

// uniqueness: 0 = off (the instantiations without the test), else the ratio u in percent
void launch_sgm_finish(int W, int H, int frames, int D, int off, int paths, size_t path_stride, int median, int lr_check, int uniqueness, const uint8_t *Lv,
                       const SgmMaps &m, float *disparity, hipStream_t s) {
  const dim3 g((W + 63) / 64, (H + 3) / 4, frames), b(64, 4), gw(H, frames), bw(256);
  const size_t lds = (size_t)W * sizeof(uint32_t);
  const int u = uniqueness;
  with_flags([&](auto sub, auto uniq, auto by16) {     // sub-pixel mode: 16-bit left maps, the right maps as ever
    using TL = std::conditional_t<sub.value, uint16_t, uint8_t>;
    TL *dl = static_cast<TL *>(m.left), *dlm = static_cast<TL *>(m.left_median);
    if constexpr (by16.value) hipLaunchKernelGGL((k_sgm_wta16<sub.value, TL, uniq.value>), gw, bw, lds, s, W, H, D, off, paths, path_stride, Lv, dl, m.right, u);
    else hipLaunchKernelGGL((k_sgm_wta<sub.value, TL, uniq.value>), gw, bw, lds, s, W, H, D, off, paths, path_stride, Lv, dl, m.right, u);
    if (median) {
      hipLaunchKernelGGL(k_sgm_median3<TL>, g, b, 0, s, W, H, dl, dlm);
      hipLaunchKernelGGL(k_sgm_median3<uint8_t>, g, b, 0, s, W, H, m.right, m.right_median);
    }
    hipLaunchKernelGGL((k_sgm_lr<TL, uniq.value>), g, b, 0, s, W, H, off, lr_check, median ? dlm : dl, median ? m.right_median : m.right, disparity);
  }, m.left_bytes == 2, u != 0, D % 16 == 0);
}
