// ccl_bits.hip — first half of MOD_STAGE_CCL_TILE: k_ccl_bits<n>, the tile stage on bit planes (overview: cluster_common.h)
#include "cluster_common.h"
#pragma clang fp contract(off)
namespace {

// ---------------------------------------------------------------------------------------------------------------
// k_ccl_bits<n> — the tile stage on BIT PLANES, for the tiles whose depth gates are decided by a few DEPTH CLASSES; one instance per
// neighbor_distance n = 1 .. 10 (Clusterer.cfg:11; the description uses the default n = 4).
//
// comparePoints links two dynamic pixels unless |z_p - z_q| > depth_diff (clusterer_nodelet.cpp:186-219).  When the dynamic cells
// of a tile and its halo, sorted by depth, fall into stretches that are each no wider than depth_diff and clear of each other by
// more than it (a tile inside one object: one stretch; at an object's rim: two — 99 % of the active tiles of the synthetic street
// scene need at most four), every gate inside a stretch passes and every gate between two fires: the tile's components are those of
// each stretch's MASK under the up-left 5 x 5 window.  They are found without touching a pixel: ONE wave per tile, lane = grid row
// (4 halo rows above + 16 tile rows), a row = 68 bits (4 halo columns + 64) in three registers, so that
//   * "has an up-left edge" (first_edge_key), "is somebody's up-left neighbour" and the closing of <= 3-cell gaps are a few
//     shifts / ORs per row, the rows above / below arrive by DPP wave shifts;
//   * the usual tile (every row one closed run, every row linked to a row above) is ONE component by inspection;
//   * anything else is flooded component by component from its first pixel in raster order (which is its root): per sweep the set
//     grows by the window in all rows at once and fills the closed runs it touches with a carry chain (c + s ripples through a
//     run of ones), 5-6 sweeps for a tile-high blob;
//   * publishing turns a component's row bits into lane predicates (v_readlane -> exec): parent[p] = root, one (size,
//     first_edge_key) record, root bits, one link request per connected group of halo cells — k_ccl_tile's contract.
// ~700 wave-instructions per such tile against ~17 000 of the union-find kernel.  Tiles that fail the depth test go to a list for
// k_ccl_tile_list.  Model of the bit algorithm against brute force: tests/models/ccl_bits_model.py.
namespace bits {
constexpr int TH = 16;

struct Row3 { uint32_t h, a, b; };   // the n halo columns x0-n .. x0-1 in the top n bits of h, x0 .. x0+31 in a, x0+32 .. x0+63 in b

__device__ __forceinline__ Row3 operator|(Row3 x, Row3 y) { return {x.h | y.h, x.a | y.a, x.b | y.b}; }
__device__ __forceinline__ Row3 operator&(Row3 x, Row3 y) { return {x.h & y.h, x.a & y.a, x.b & y.b}; }
__device__ __forceinline__ Row3 operator^(Row3 x, Row3 y) { return {x.h ^ y.h, x.a ^ y.a, x.b ^ y.b}; }
__device__ __forceinline__ Row3 andn(Row3 x, Row3 y) { return {x.h & ~y.h, x.a & ~y.a, x.b & ~y.b}; }
__device__ __forceinline__ bool any(Row3 x) { return (x.h | x.a | x.b) != 0u; }
// Shifts by K >= 1 columns.  NH = number of halo columns (= neighbor_distance): they sit in the top NH bits of h.
template <int K> __device__ __forceinline__ Row3 shl(Row3 v) {      // towards larger x
  return {v.h << K, __builtin_amdgcn_alignbit(v.a, v.h, 32 - K), __builtin_amdgcn_alignbit(v.b, v.a, 32 - K)};
}
template <int K, int NH> __device__ __forceinline__ Row3 shr(Row3 v) {      // towards smaller x; cells left of column x0 - NH do not exist
  return {__builtin_amdgcn_alignbit(v.a, v.h, K) & (~0u << (32 - NH)), __builtin_amdgcn_alignbit(v.b, v.a, K), v.b >> K};
}
// the row above / below arrives (zero into the first / last lane).  All 64 lanes must be active.
__device__ __forceinline__ uint32_t dn1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, false); }   // wave_shr:1
__device__ __forceinline__ uint32_t up1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, false); }   // wave_shl:1
__device__ __forceinline__ Row3 row_dn(Row3 v) { return {dn1(v.h), dn1(v.a), dn1(v.b)}; }
__device__ __forceinline__ Row3 row_up(Row3 v) { return {up1(v.h), up1(v.a), up1(v.b)}; }
template <int K, bool DN> __device__ __forceinline__ Row3 row_shift(Row3 v) {   // K rows
  if constexpr (K == 0) return v;
  else return row_shift<K - 1, DN>(DN ? row_dn(v) : row_up(v));
}
// OR of v shifted by 0 .. N - 1 (columns: DIR 0 right, 1 left; rows: DIR 2 down, 3 up) by doubling: a set that covers shifts
// 0 .. COV is ORed with itself shifted by min(COV + 1, rest).  N = 4: two steps (1, 2); N = 10: four (1, 2, 4, 2).
template <int COV, int N, int DIR> __device__ __forceinline__ Row3 grow(Row3 y) {
  if constexpr (COV >= N - 1) return y;
  else {
    constexpr int S = (COV + 1 < N - 1 - COV) ? COV + 1 : N - 1 - COV;
    Row3 t;
    if constexpr (DIR == 0) t = shl<S>(y);
    else if constexpr (DIR == 1) t = shr<S, N>(y);
    else t = row_shift<S, DIR == 2>(y);
    return grow<COV + S, N, DIR>(y | t);
  }
}
// v | v << 1 | .. | v << N; x: the same without v itself
template <int N> __device__ __forceinline__ void dil_r(Row3 v, Row3 &all, Row3 &x) { x = shl<1>(grow<0, N, 0>(v)); all = v | x; }
template <int N> __device__ __forceinline__ void dil_l(Row3 v, Row3 &all, Row3 &x) { x = shr<1, N>(grow<0, N, 1>(v)); all = v | x; }
// OR over dv = 1 .. N of the rows dv above (DN) / below
template <int N, bool DN> __device__ __forceinline__ Row3 vert(Row3 v) { return row_shift<1, DN>(grow<0, N, DN ? 2 : 3>(v)); }
// M with the gaps of <= N - 1 cells between two dynamic cells closed: a cell is in the result iff a dynamic cell lies i to its left
// and one j to its right with i + j <= N (cells of one run of the result are chained by same-row links)
template <int I, int N> __device__ __forceinline__ Row3 closed_rec(Row3 M, Row3 lprev) {   // term I: (dynamic within I to the left) & (dynamic N - I to the right)
  Row3 l, r;
  if constexpr (I == 0) l = M; else l = lprev | shl<I>(M);
  if constexpr (I == N) r = M; else r = shr<N - I, N>(M);
  const Row3 t = l & r;
  if constexpr (I == N) return t;
  else return t | closed_rec<I + 1, N>(M, l);
}
template <int N> __device__ __forceinline__ Row3 closed(Row3 M) { return closed_rec<0, N>(M, M); }
__device__ __forceinline__ Row3 rev(Row3 v) { return {__builtin_bitreverse32(v.b), __builtin_bitreverse32(v.a), __builtin_bitreverse32(v.h)}; }
// all bits of the runs of c that hold a bit of s (s subset of c), from the lowest such bit upwards: c + s ripples through a run
__device__ __forceinline__ Row3 fill_up(Row3 c, Row3 s) {
  uint32_t c1, c2, c3;
  Row3 t;
  t.h = __builtin_addc(c.h, s.h, 0u, &c1);
  t.a = __builtin_addc(c.a, s.a, c1, &c2);
  t.b = __builtin_addc(c.b, s.b, c2, &c3);
  return ((t ^ c) & c) | s;
}
__device__ __forceinline__ int popc3(Row3 v) { return __popc(v.h) + __popc(v.a) + __popc(v.b); }

// min / max of depths that are never signalling NaNs where it matters: a dynamic cell's depth is a number (checked for a caller's
// cloud, guaranteed by the fused kernel) and everything else has been replaced by a quiet NaN, which v_min / v_max pass over —
// the plain instructions, without the canonicalising v_max x, x that fminf / fmaxf put in front of every loaded value
__device__ __forceinline__ float zmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float zmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// the F32 of lane l (v_readlane moves bit patterns; the builtin is typed int)
__device__ __forceinline__ float lane_f32(float v, int l) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), l)); }
__device__ __forceinline__ float wave_fmin(float v) {
  v = fminf(v, __uint_as_float(MOD_DPP(__float_as_uint(v), 0xB1))); v = fminf(v, __uint_as_float(MOD_DPP(__float_as_uint(v), 0x4E)));
  v = fminf(v, __uint_as_float(MOD_DPP(__float_as_uint(v), 0x141))); v = fminf(v, __uint_as_float(MOD_DPP(__float_as_uint(v), 0x140)));
  const float a = lane_f32(v, 0), b = lane_f32(v, 16), c = lane_f32(v, 32), d = lane_f32(v, 48);
  return fminf(fminf(a, b), fminf(c, d));
}
__device__ __forceinline__ float wave_fmax(float v) {
  v = fmaxf(v, __uint_as_float(MOD_DPP(__float_as_uint(v), 0xB1))); v = fmaxf(v, __uint_as_float(MOD_DPP(__float_as_uint(v), 0x4E)));
  v = fmaxf(v, __uint_as_float(MOD_DPP(__float_as_uint(v), 0x141))); v = fmaxf(v, __uint_as_float(MOD_DPP(__float_as_uint(v), 0x140)));
  const float a = lane_f32(v, 0), b = lane_f32(v, 16), c = lane_f32(v, 32), d = lane_f32(v, 48);
  return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
// sum over lanes 0 .. 31 (the grid rows live in lanes 0 .. 15 + neighbor_distance)
__device__ __forceinline__ int wave_sum_lo32(int v) {
  v += (int)MOD_DPP(v, 0xB1); v += (int)MOD_DPP(v, 0x4E); v += (int)MOD_DPP(v, 0x141); v += (int)MOD_DPP(v, 0x140);
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16);
}
__device__ __forceinline__ uint64_t lane_bits(uint32_t lo, uint32_t hi, int l) {   // words of lane l as one scalar mask
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, l) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)lo, l);
}

// one tile (= one wave) per workgroup: 1 / 2 / 4 / 8 tiles per workgroup measured 0.451 / 0.455 / 0.521 / 0.642 ms per 512 pairs
// (in-process A/B): a workgroup's slot and LDS stay occupied until its slowest wave is done, and three quarters of the tiles are empty.
// (One wave walking a STRIP of 2 / 4 / 5 / 10 tiles, to save the empty tiles' launches — 0.17 ms per 512 pairs when no pixel is
// dynamic —: 0.495 / 0.495 / 0.510 / 0.515 against 0.435: active tiles sit next to each other and would queue behind one wave.)
constexpr int kTilesPerBlock = 1, kMaxClasses = 4, kMaxComps = 32;

// Global accesses of this kernel: ONE wave-uniform base per plane (frame's plane, in SGPRs) + a 32-bit byte offset per lane — the
// `global_load / global_store v, v_off, s[base]` form.  (A frame's planes span less than 2^29 bytes: mod_create caps W * H at 2^27.)
// Written as base + zext(offset) with the row's share folded into the OFFSET: left to itself the compiler adds the lane offset to
// the base first and then keeps one 64-bit VGPR address per row alive across the class loop (32 registers for the 16 parent rows).
template <class T> __device__ __forceinline__ T ldo(const void *base, uint32_t byte_off) { return *(const T *)((const char *)base + byte_off); }
template <class T> __device__ __forceinline__ void sto(void *base, uint32_t byte_off, T v) { *(T *)((char *)base + byte_off) = v; }

template <int HL>                                                     // HL = neighbor_distance = halo rows above = halo columns left
__global__ __launch_bounds__(64 * kTilesPerBlock) void k_ccl_bits(DevCam c, ClArgs a, int tiles_x, int tiles_y) {
  constexpr int PH = TH + HL;                                          // grid rows = lanes in use
  const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int wi = blockIdx.x * kTilesPerBlock + wv, ty = blockIdx.y, f = blockIdx.z;
  if (wi >= tiles_x) return;
  const size_t tix = (size_t)f * tiles_y * tiles_x + (size_t)ty * tiles_x + wi;
  int *hdr = a.tilehdr + tix * 2;
  if (__builtin_amdgcn_readfirstlane(hdr[0]) == 0) return;          // no dynamic pixel in the tile
  const int x0 = wi * 64, y0 = ty * TH, MW = c.mask_words, W = c.W, H = c.H;
  const size_t N = (size_t)W * H, fN = (size_t)f * N;
  // ---- the mask words of the 20 grid rows, lane = row -------------------------------------------------------------------------
  Row3 Mrem;                                                           // dynamic cells that no depth class holds yet
  {
    const int gy = y0 - HL + lane;
    const bool inrow = lane < PH && gy >= 0 && gy < H;
    const uint64_t *mr = a.mask + ((size_t)f * H + (inrow ? gy : 0)) * MW;
    const uint64_t q0 = mr[wi], qL = mr[max(wi - 1, 0)];              // unconditional loads, clamped addresses
    Mrem.h = (inrow && wi > 0) ? ((uint32_t)(qL >> 32) & (~0u << (32 - HL))) : 0u;
    Mrem.a = inrow ? (uint32_t)q0 : 0u;
    Mrem.b = inrow ? (uint32_t)(q0 >> 32) : 0u;
  }
  const bool il = lane >= HL && lane < PH;                             // a tile row
  const float th = c.depth_th, qnan = __uint_as_float(0x7fc00000u);
  // (uniform row base + 32-bit lane offset: the `global_load v, v_off, s[base]` form, no 64-bit address arithmetic per lane)
  const uint32_t oc = 4u * (uint32_t)min(x0 + lane, W - 1);
  uint32_t rootA = 0u, rootB = 0u;                                     // root bits of the tile rows (lane = row)
  int nreq = 0, ncomp = 0;
  uint2 *req = a.requests + tix * a.req_cap;
  float hi_prev = 0.0f;
  bool bail = false;
  // ---- depth classes.  comparePoints links two dynamic pixels unless |z_p - z_q| > depth_diff.  Sort the dynamic cells of the grid
  // by depth in thought: a CLASS is a stretch that spans at most depth_diff (every gate inside it passes: |z_p - z_q| <= max - min,
  // and F32 subtraction is monotone) and lies more than depth_diff from the next cell on either side (every gate that leaves it
  // fires).  Then the tile's components are those of each class's MASK, class by class.  Classes are peeled off from the
  // nearest: lo = smallest depth left, members = cells with !(z - lo > th); the tile goes to the union-find kernel when a class
  // is not clear of the next one, when more than kMaxClasses are needed, or when a dynamic cell has a NaN depth (NaN links with
  // everything).  One class — a tile inside one object — is the usual case; object rims have two. --------------------------------
  // The depths of the grid are read from HBM once: the first sweep (smallest / largest depth of the tile) works on them as they
  // arrive and parks the 64 tile columns in LDS (5 KB per wave) for the sweeps of a tile with more than one class.  The four halo
  // columns stay in registers in the ROW's lane (lane = row: four loads serve all 20 rows), next to the row's halo bits.
  const float *zplane = a.z + fN;
  __shared__ float zlds[kTilesPerBlock][PH][64];
  float(*zl)[64] = zlds[wv];
  float zh[HL];
  float lo = qnan, hi = qnan;
  // Round 5: the fused scene-flow kernel leaves, next to every non-zero mask word, the smallest and largest depth of the word's
  // dynamic pixels (ClArgs.zrange).  The union of the ranges of this tile's words (word wi of the grid rows; word wi - 1 of the rows
  // whose halo columns hold a dynamic cell — that word spans 64 columns, the halo HL of them, so the union can only be WIDER than the
  // grid's own range) no wider than depth_diff means ONE class (F32 subtraction is monotone: hi - lo of a subset cannot round
  // above that of its superset) and NO depth row is loaded at all; otherwise, and for a caller's cloud (zrange == null), the
  // depths are read as before.  A sufficient test only: the result is the same either way.
  bool need_z = true;
  if (a.zrange) {                                                      // wave-uniform
    const int gy = y0 - HL + lane;
    const bool inrow = lane < PH && gy >= 0 && gy < H;
    const float2 *zr = a.zrange + ((size_t)f * H + (inrow ? gy : 0)) * MW;
    const float2 r0 = zr[wi], rL = zr[max(wi - 1, 0)];                 // unconditional loads, clamped addresses (beside the mask words')
    const bool u0 = (Mrem.a | Mrem.b) != 0u, uL = Mrem.h != 0u;        // Mrem is zero outside the grid's rows
    lo = zmin(u0 ? r0.x : qnan, uL ? rL.x : qnan); hi = zmax(u0 ? r0.y : qnan, uL ? rL.y : qnan);
    lo = wave_fmin(lo); hi = wave_fmax(hi);
    need_z = hi - lo > th;                                             // (a NaN — impossible here — would take the row path's answer below)
  }
  if (need_z) {
    lo = qnan; hi = qnan;
    {
      const int gy = min(max(y0 - HL + lane, 0), H - 1);               // (lanes >= PH read the clamped last row: never used)
      // wi == 0 has no halo columns (Mrem.h == 0); an image narrower than HL still reads inside its rows (values unused)
      const int hx = max(x0 - HL, 0);
#pragma unroll
      for (int j = 0; j < HL; j++) zh[j] = ldo<float>(zplane, 4u * (uint32_t)(gy * W + min(hx + j, W - 1)));
    }
    uint64_t nanb = 0ull;
    constexpr int HB = (PH + 1) / 2;                                   // two batches of rows (10 + 10 at HL = 4)
#pragma unroll
    for (int g0 = 0; g0 < PH; g0 += HB) {
      float zr[HB];
#pragma unroll
      for (int i = 0; i < HB; i++) {
        const int gy = min(max(y0 - HL + g0 + i, 0), H - 1);
        zr[i] = ldo<float>(zplane, oc + 4u * (uint32_t)(gy * W));
      }
#pragma unroll
      for (int i = 0; i < HB; i++) {
        const int gr = g0 + i;
        if (gr >= PH) break;
        const bool dyn = __builtin_amdgcn_inverse_ballot_w64(lane_bits(Mrem.a, Mrem.b, gr));
        const float z1 = dyn ? zr[i] : qnan;
        lo = zmin(lo, z1); hi = zmax(hi, z1);
        zl[gr][lane] = zr[i];
        // the fused scene-flow kernel never marks a pixel without a finite depth as dynamic; a caller's cloud may
        if (!a.xy_from_z) nanb |= __ballot(dyn & (zr[i] != zr[i]));
      }
    }
#pragma unroll
    for (int j = 0; j < HL; j++) {
      const bool hd = (Mrem.h >> (32 - HL + j)) & 1u;
      const float z2 = hd ? zh[j] : qnan;
      lo = zmin(lo, z2); hi = zmax(hi, z2);
      if (!a.xy_from_z) nanb |= __ballot(hd & (zh[j] != zh[j]));
    }
    if (nanb != 0ull) {                                                // wave-uniform: NaN links with everything
      if (lane == 0) a.tilelist[atomicAdd(&a.counters[4], 1)] = (uint32_t)tix;
      return;
    }
  } else {
#pragma unroll
    for (int j = 0; j < HL; j++) zh[j] = qnan;                         // never read: one class ends the loop below after its first pass
  }
  for (int pass = 0;; pass++) {                                        // wave-uniform
    if (pass == kMaxClasses) { bail = true; break; }
    if (pass > 0) {                                                    // smallest / largest depth of what is left
      lo = qnan; hi = qnan;
#pragma unroll 4
      for (int gr = 0; gr < PH; gr++) {
        const bool dyn = __builtin_amdgcn_inverse_ballot_w64(lane_bits(Mrem.a, Mrem.b, gr));
        const float z1 = dyn ? zl[gr][lane] : qnan;
        lo = zmin(lo, z1); hi = zmax(hi, z1);
      }
#pragma unroll
      for (int j = 0; j < HL; j++) {
        const float z2 = ((Mrem.h >> (32 - HL + j)) & 1u) ? zh[j] : qnan;
        lo = zmin(lo, z2); hi = zmax(hi, z2);
      }
    }
    lo = wave_fmin(lo); hi = wave_fmax(hi);
    Row3 M;                                                            // the class
    if (!(hi - lo > th)) { M = Mrem; Mrem = {0u, 0u, 0u}; }            // everything that is left (wave-uniform)
    else {
      M = {0u, 0u, 0u};
      float chi = qnan;
#pragma unroll 4
      for (int gr = 0; gr < PH; gr++) {
        const bool dyn = __builtin_amdgcn_inverse_ballot_w64(lane_bits(Mrem.a, Mrem.b, gr));
        const float z1 = zl[gr][lane];
        const bool in1 = dyn & !(z1 - lo > th);
        const uint64_t b1 = __ballot(in1);
        const bool me = lane == gr;                                    // into the row's lane (two selects)
        M.a = me ? (uint32_t)b1 : M.a; M.b = me ? (uint32_t)(b1 >> 32) : M.b;
        chi = zmax(chi, in1 ? z1 : qnan);
      }
#pragma unroll
      for (int j = 0; j < HL; j++) {                                   // the halo columns, in the row's own lane
        const bool in2 = ((Mrem.h >> (32 - HL + j)) & 1u) & !(zh[j] - lo > th);
        M.h |= in2 ? (1u << (32 - HL + j)) : 0u;
        chi = zmax(chi, in2 ? zh[j] : qnan);
      }
      hi = wave_fmax(chi);
      Mrem = andn(Mrem, M);
    }
    if (pass > 0 && !(lo - hi_prev > th)) { bail = true; break; }      // the class before this one was not clear of it
    hi_prev = hi;
  // ---- per-row facts ---------------------------------------------------------------------------------------------------------------
  Row3 drA, drX, dlA, dlX;
  dil_r<HL>(M, drA, drX);
  dil_l<HL>(M, dlA, dlX);
  const Row3 above = vert<HL, true>(drA);                              // cells that have a dynamic cell up-left in one of the HL rows above
  const Row3 UL = M & (drX | above);                                   // has an up-left edge
  const Row3 E = UL | (M & (dlX | vert<HL, false>(dlA)));              // has any edge
  const Row3 C = closed<HL>(M);                                        // M with gaps of < HL cells closed: one run = one chain of same-row links
  const Row3 rC = rev(C);
  Row3 R = {0u, il ? (M.a & E.a) : 0u, il ? (M.b & E.b) : 0u};         // tile pixels with an edge that no component holds yet
  const uint32_t Za = il ? (M.a & ~E.a) : 0u, Zb = il ? (M.b & ~E.b) : 0u;   // tile pixels without any edge: roots of their own
  rootA |= Za; rootB |= Zb;
  // one component by inspection?  Every non-empty row is ONE closed run whose cells all have an edge, and every non-empty row
  // but the first has a link to a row above: by induction over the rows all dynamic cells of the grid are connected.
  bool single;
  {
    const uint64_t ne = __ballot(any(M));
    const int first = __builtin_ctzll(ne);                              // ne != 0: the tile has a dynamic pixel
    const Row3 starts = andn(C, shl<1>(C));
    const bool ok = !any(M) || (popc3(starts) == 1 && !any(E ^ M) && (lane == first || any(M & above)));
    single = __ballot(!ok) == 0ull && __ballot(any(R)) != 0ull;
  }
  for (;;) {                                                           // wave-uniform loop over the components with a tile pixel
    const uint64_t rrows = __ballot(any(R));
    if (rrows == 0ull) break;
    Row3 S;
    if (single) S = M;
    else {
      const int sr = __builtin_ctzll(rrows);                           // first pixel in raster order of what is left: the seed
      const uint32_t sa = (uint32_t)__builtin_amdgcn_readlane((int)R.a, sr), sb = (uint32_t)__builtin_amdgcn_readlane((int)R.b, sr);
      const uint32_t ba = sa & (0u - sa), bb = sa ? 0u : (sb & (0u - sb));
      S = {0u, lane == sr ? ba : 0u, lane == sr ? bb : 0u};
      for (;;) {                                                       // flood: S only grows, inside M
        Row3 rA, rX, lA, lX;
        dil_r<HL>(S, rA, rX);
        dil_l<HL>(S, lA, lX);
        const Row3 reach = M & (rA | lA | vert<HL, true>(rA) | vert<HL, false>(lA));
        const Row3 S2 = (fill_up(C, reach) | rev(fill_up(rC, rev(reach)))) & M;
        const bool grew = any(S2 ^ S);
        S = S2;
        if (__ballot(grew) == 0ull) break;
      }
    }
    // ---- publish the component ----
    const uint64_t irows = __ballot(il && (S.a | S.b) != 0u);
    const int rr = __builtin_ctzll(irows);                              // S holds a tile pixel (its seed, or R != 0)
    const uint32_t fa = (uint32_t)__builtin_amdgcn_readlane((int)S.a, rr), fb = (uint32_t)__builtin_amdgcn_readlane((int)S.b, rr);
    const int rcol = fa ? __builtin_ctz(fa) : 32 + __builtin_ctz(fb);
    const int rootg = (y0 + rr - HL) * W + x0 + rcol;                  // the component's first tile pixel in raster order
    if (lane == rr) { if (rcol < 32) rootA |= 1u << rcol; else rootB |= 1u << (rcol - 32); }
    int *pplane = a.parent + fN;
    uint32_t po = 4u * (uint32_t)(y0 * W + x0 + lane);                  // this lane's pixel in the tile's first row
    asm volatile("" : "+v"(po));                                       // (computed here, per component: not 16 row offsets held across the loop)
#pragma unroll
    for (int j = 0; j < TH; j++) {
      const uint64_t bitsj = lane_bits(S.a, S.b, HL + j);
      if (bitsj != 0ull && __builtin_amdgcn_inverse_ballot_w64(bitsj))
        sto<int>(pplane, po + 4u * (uint32_t)(j * W), rootg);
    }
    {
      const int cnt = il ? __popc(S.a) + __popc(S.b) : 0;
      const uint32_t ka = S.a & UL.a, kb = S.b & UL.b;
      uint32_t key = (uint32_t)kKeyNone;
      if (il && (ka | kb)) key = (uint32_t)((y0 + lane - HL) * W + x0 + (ka ? __builtin_ctz(ka) : 32 + __builtin_ctz(kb)));
      const int size = wave_sum_lo32(cnt);
      key = wave_min_u32(key);
      if (lane == 0) { sto<int>(a.rsize + fN, 4u * (uint32_t)rootg, size); sto<int>(a.rkey + fN, 4u * (uint32_t)rootg, (int)key); }
    }
    // halo cells of the component belong to other tiles: one link request (halo cell, root) per group of halo cells that are
    // direct neighbours (a cell whose left or upper neighbour is a halo cell of the set leaves it to that neighbour: the edge
    // between them is seen by the tile that owns the cell) — k_ccl_tile's rule
    {
      const Row3 HS = {S.h, lane < HL ? S.a : 0u, lane < HL ? S.b : 0u};
      const Row3 em = andn(HS, shl<1>(HS) | row_dn(HS));
      uint64_t todo = __ballot(any(em));
      while (todo) {                                                   // wave-uniform: the few grid rows that emit
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint64_t eb = lane_bits(em.a, em.b, l);
        const uint32_t eh = (uint32_t)__builtin_amdgcn_readlane((int)em.h, l) >> (32 - HL);
        const int hgrow = (y0 - HL + l) * W + x0;
        if (__builtin_amdgcn_inverse_ballot_w64((uint64_t)eh)) {       // left-halo columns x0 - HL + lane, lanes 0 .. HL - 1
          const int slot = nreq + __popc(eh & ((1u << lane) - 1u));
          if (MOD_CHECK(a, slot < a.req_cap, 12)) req[slot] = make_uint2((uint32_t)(hgrow - HL + lane), (uint32_t)rootg);
        }
        nreq += __popc(eh);
        if (eb != 0ull && __builtin_amdgcn_inverse_ballot_w64(eb)) {
          const int slot = nreq + __popcll((unsigned long long)(eb & ((1ull << lane) - 1ull)));
          if (MOD_CHECK(a, slot < a.req_cap, 12)) req[slot] = make_uint2((uint32_t)(hgrow + lane), (uint32_t)rootg);
        }
        nreq += __popcll((unsigned long long)eb);
      }
    }
    if (single) break;
    R = andn(R, S);
    // a tile in dozens of pieces (noise at a small window) is flooded piece by piece: beyond kMaxComps the union-find kernel,
    // which takes them all at once, is the cheaper one
    if (++ncomp >= kMaxComps && __ballot(any(R)) != 0ull) { bail = true; break; }
  }
  // ---- tile pixels without any edge: each its own root with an empty key (the reference never labels them) ----
  {
    uint64_t todo = __ballot((Za | Zb) != 0u);
    while (todo) {
      const int l = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      if (__builtin_amdgcn_inverse_ballot_w64(lane_bits(Za, Zb, l))) {
        const int p = (y0 + l - HL) * W + x0 + lane;
        sto<int>(a.parent + fN, 4u * (uint32_t)p, p); sto<int>(a.rsize + fN, 4u * (uint32_t)p, 1); sto<int>(a.rkey + fN, 4u * (uint32_t)p, kKeyNone);
      }
    }
  }
    if (bail || __ballot(any(Mrem)) == 0ull) break;                    // wave-uniform: every dynamic cell is in a class
  }
  if (bail) {                                                          // wave-uniform: leave the tile to the union-find kernel, which
    if (lane == 0) a.tilelist[atomicAdd(&a.counters[4], 1)] = (uint32_t)tix;   // rewrites whatever classes published before the bail
    return;
  }
  if (il && y0 + lane - HL < H) a.lroot[((size_t)f * H + (y0 + lane - HL)) * MW + wi] = ((uint64_t)rootB << 32) | rootA;
  if (lane == 0) { hdr[1] = nreq; hdr[0] = 2; }                       // 2: done here (k_ccl_tile_list never sees the tile)
}
}  // namespace bits
}  // namespace

void launch_ccl_bits(const DevCam &c, const ClArgs &a, int frames, hipStream_t s) {
  const dim3 tgrid = tile_grid(c, frames);
  const int tx = (int)tgrid.x, tyn = (int)tgrid.y;
  const dim3 bgrid((tgrid.x + bits::kTilesPerBlock - 1) / bits::kTilesPerBlock, tgrid.y, tgrid.z), bblock(64, bits::kTilesPerBlock, 1);
  switch (c.n) {
#define MOD_BITS_CASE(n) case n: hipLaunchKernelGGL(bits::k_ccl_bits<n>, bgrid, bblock, 0, s, c, a, tx, tyn); break;
    MOD_BITS_CASE(1) MOD_BITS_CASE(2) MOD_BITS_CASE(3) MOD_BITS_CASE(4) MOD_BITS_CASE(5)
    MOD_BITS_CASE(6) MOD_BITS_CASE(7) MOD_BITS_CASE(8) MOD_BITS_CASE(9) MOD_BITS_CASE(10)
#undef MOD_BITS_CASE
  }
}
