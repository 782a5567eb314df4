// ccl_tile.hip — MOD_STAGE_CCL_TILE: k_ccl_tile / k_ccl_tile_list, union-find over one tile and its halo (overview: cluster_common.h)
#include "cluster_common.h"
#include <algorithm>
#pragma clang fp contract(off)
namespace {

// Adds the members of one wave (grouped by the record they belong to) into the statistics records with one set of
// atomics per (wave, record).  `rec_idx` < 0 marks a lane without contribution.  Works on LDS slots and on the global planes.
__device__ __forceinline__ void wave_accumulate(int *sizes, int *keys, int stride, int rec_idx, uint32_t key, int lane) {
  uint64_t todo = __ballot(rec_idx >= 0);
  while (todo) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int lid = __builtin_amdgcn_readlane(rec_idx, leader);
    const bool mine = rec_idx == lid;
    const uint64_t grp = __ballot(mine);
    const uint32_t k = wave_min_u32(mine ? key : (uint32_t)kKeyNone);
    if (lane == leader) {
      atomicAdd(&sizes[(size_t)lid * stride], __popcll((unsigned long long)grp));
      if (k != (uint32_t)kKeyNone) atomicMin(&keys[(size_t)lid * stride], (int)k);
    }
    todo &= ~grp;
  }
}

// LDS union-find over node ids: interior cells use their grid index, halo cells carry bit 15 so that they compare
// larger than every interior cell — the root (minimum id) of any set that contains an interior pixel is interior.
constexpr int kHaloBit = 0x8000;
__device__ __forceinline__ int lds_find(int *L, int a) {
  // path halving with plain stores: only non-root cells are rewritten, and only with one of their ancestors, so a
  // racing atomicMin hook (which re-examines the value it displaced) never loses a link
  int p = ld_relaxed(L + (a & 0x7fff));
  while (p != a) {
    const int g = ld_relaxed(L + (p & 0x7fff));
    if (g != p) L[a & 0x7fff] = g;
    a = p; p = g;
  }
  return a;
}
__device__ __forceinline__ int lds_unite(int *L, int a, int b) {
  while (true) {
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return a;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a & 0x7fff], b);
    if (old == a) return b;
    a = old;
  }
}

// Unions of one window position for the whole wave.  Lanes of one run looking at one run above all hold the same
// (cur, other) pair, so only the first lane of each contiguous group of equal pairs performs the union; all such
// representatives run concurrently (LDS atomicMin hooks), then every lane that needed the union refreshes its root.
// `last` remembers the label a lane was united with most recently: the neighbours in one window row nearly always
// carry the same (possibly no longer root) label, and re-uniting them would cost a find each.
__device__ __forceinline__ int lds_find_compress(int *L, int a) {
  const int r = lds_find(L, a);
  if (r != a && ld_relaxed(L + (a & 0x7fff)) != r) L[a & 0x7fff] = r;   // benign race: r is an ancestor of a
  return r;
}
__device__ __forceinline__ void wave_unite_lds(int *L, bool need, int &cur, int &last, int other, int lane) {
  if (__ballot(need) == 0) return;
  const int pc = wave_prev_i32(cur), po = wave_prev_i32(other), pn = wave_prev_i32((int)need);
  const bool rep = need && !(lane > 0 && pn && pc == cur && po == other);
  if (rep) lds_unite(L, cur, other);
  if (need) { last = other; cur = lds_find_compress(L, cur); }
}

// Tile-local connected components INCLUDING the edges that leave the tile.
// Workgroup = 4 waves = one 64 x TH tile plus an n-pixel halo above and to the left (masked depth + parents in LDS).
//   A  cooperative load of the (TH+n) x (64+n) grid; rows pre-linked into runs with wave ballots (no atomics)
//   B  the rest of each pixel's up-left window: (n+1) batched LDS reads per window row, unions deduplicated per wave
//   C  publish: interior pixels hook onto their tile root, linked halo pixels are united with it in HBM (atomicMin
//      only), tile roots get an empty statistics record
//   D  partial statistics (size, first_edge_key, bbox) of the tile's components, one set of atomics per (wave, root)
// CCL_TPB consecutive tiles of a tile row share one workgroup, which walks the active ones one after the other: three quarters of
// the tiles of a street scene are empty, and 460 k workgroups that only read a header word and exit cost 0.3 ms per 512 pairs
// of workgroup launches (the kernel's time on a batch without any dynamic pixel).
#ifndef CCL_TPB
#define CCL_TPB 1
#endif
template <int TH, int NMAX, int NW, bool EXACT>
__device__ __forceinline__ void ccl_tile_body(const DevCam &c, const ClArgs &a, const int wi, const int ty, const int f, const int tiles_x, const int tiles_y);

template <int TH, int NMAX, int NW, bool EXACT>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_ccl_tile(DevCam c, ClArgs a, int tiles_x, int tiles_y) {
  const int ty = blockIdx.y, f = blockIdx.z;
#pragma unroll 1
  for (int t = 0; t < CCL_TPB; t++) {
    const int wi = blockIdx.x * CCL_TPB + t;
    if (wi >= tiles_x) break;
    // The tile's header says whether it holds a dynamic pixel at all (written with the mask words: by the scene-flow kernel's
    // epilogue, or by k_tile_flags).  Three quarters of the tiles of a street scene do not: they cost one scalar load.
    const int *hdr = a.tilehdr + ((size_t)f * tiles_y * tiles_x + (size_t)ty * tiles_x + wi) * 2;
    if (__builtin_amdgcn_readfirstlane(hdr[0]) == 0) continue;
    ccl_tile_body<TH, NMAX, NW, EXACT>(c, a, wi, ty, f, tiles_x, tiles_y);
    if (CCL_TPB > 1) __syncthreads();                // the next tile re-uses the LDS arrays
  }
}

template <int TH, int NMAX, int NW, bool EXACT>
__device__ __forceinline__ void ccl_tile_body(const DevCam &c, const ClArgs &a, const int wi, const int ty, const int f, const int tiles_x, const int tiles_y) {
  constexpr int RPW = TH / NW;                      // rows per wave (NW waves per tile)
  constexpr int PW = 64 + NMAX, PH = TH + NMAX, G = PW * PH;
  __shared__ float zt[G];
  __shared__ int Lt[G];
  __shared__ uint64_t m0[PH], mL[PH];
  __shared__ int s_uni[PH];                         // the one label every dynamic cell of the grid row carries after phase A3, or -1
  constexpr int kSlots = 32;
  __shared__ int s_nreq, s_nslots, s_anyhalo;
  __shared__ RootRec srec[kSlots];
  __shared__ int sroot[kSlots];
  // threadIdx.y is the wave index: the same in all 64 lanes, but it arrives in a vector register — as a scalar, every row
  // index derived from it stays on the scalar unit
  const int lane = threadIdx.x, w = __builtin_amdgcn_readfirstlane((int)threadIdx.y), tid = w * 64 + lane;
  const int x0 = wi * 64, y0 = ty * TH;
  // EXACT: neighbor_distance equals the instance's halo width (the default n = 4 does): the window loops get constant bounds
  const int MW = c.mask_words, n = EXACT ? NMAX : c.n;
  const size_t N = (size_t)c.W * c.H;
  const size_t fN = (size_t)f * N;
  int *hdr = a.tilehdr + ((size_t)f * tiles_y * tiles_x + (size_t)ty * tiles_x + wi) * 2;
  if (tid == 0) { s_nreq = 0; s_nslots = 0; }
  // ---- all HBM reads of the kernel, in ONE round trip: the mask words of the PH grid rows and the depth rows (unconditional,
  // clamped addresses; values of non-dynamic pixels are discarded: predicated loads would compile to one exec-masked branch +
  // wait each) ----
  {
    uint64_t q0 = 0ull, qL = 0ull;
    if (tid < PH) {
      const int gy = y0 - NMAX + tid;
      const bool inrow = gy >= 0 && gy < c.H && tid >= NMAX - n;
      const uint64_t *mr = a.mask + ((size_t)f * c.H + (inrow ? gy : 0)) * MW;
      q0 = inrow ? mr[wi] : 0ull;
      qL = (inrow && wi > 0) ? mr[wi - 1] : 0ull;
      m0[tid] = q0; mL[tid] = qL;
    }
    if (w == 0) {                                    // PH <= 64: all mask words sit in wave 0.  Any dynamic halo cell at all?
      const uint64_t hb = __ballot(tid < PH && (((tid < NMAX) ? q0 : 0ull) | (qL >> (64 - NMAX))) != 0ull);
      if (lane == 0) s_anyhalo = hb != 0ull;
    }
  }
  constexpr int AROWS = (PH + NW - 1) / NW;
  float zl[AROWS], zh[AROWS];
  const int xc = min(x0 + lane, c.W - 1), xhc = max(x0 - 1 - lane, 0);
#pragma unroll
  for (int i = 0; i < AROWS; i++) {
    const int gy = min(max(y0 - NMAX + w + NW * i, 0), c.H - 1);
    const size_t rowp = fN + (size_t)gy * c.W;
    zl[i] = a.z[rowp + xc];
    zh[i] = a.z[rowp + xhc];                          // left halo: column x0 - 1 - lane (lanes < n)
  }
  __syncthreads();
  // rows are dealt to the waves round-robin (wave w owns rows w, w + 4, ...): a blob's rows are contiguous, so contiguous
  // row blocks would leave most of a tile's work to one wave while the others wait at the barriers
  const float th = c.depth_th;
#ifdef MOD_PHASE_COUNTERS   // diagnostic build only (make PHASE_COUNTERS=1): per-phase cycle sums in ClArgs.dbg
  const bool prof = c.debug & 128;
  unsigned long long t0 = prof ? clock64() : 0, t1;
#define STAMP(i) if (prof) { t1 = clock64(); if (lane == 0) { atomicAdd(&a.dbg[i], t1 - t0); atomicMax(&a.dbg[16 + i], t1 - t0); } t0 = t1; }
#define COUNT(i, v) if (prof && lane == 0) atomicAdd(&a.dbg[i], (unsigned long long)(v));
#elif defined(MOD_PHASE_MARKERS)
#define STAMP(i) asm volatile("; PHASE_MARK " #i ::: "memory");
#define COUNT(i, v)
#else
#define STAMP(i)
#define COUNT(i, v)
#endif
  // ---- phase A: masked depth + identity parents; grid row gr = image row y0 - NMAX + gr, 4 rows per step -----------
#pragma unroll
  for (int i = 0; i < AROWS; i++) {
    const int gr = w + NW * i;
    if (gr < PH) {
      const uint64_t q0 = m0[gr], qL = mL[gr];        // zero for rows that are unused or outside the image
      const int cell = gr * PW + NMAX + lane;
      zt[cell] = ((q0 >> lane) & 1ull) ? zl[i] : 0.0f;
      Lt[cell] = (gr >= NMAX) ? cell : (cell | kHaloBit);
      if (lane < n) {
        const int hc = gr * PW + NMAX - 1 - lane;
        zt[hc] = ((qL >> (63 - lane)) & 1ull) ? zh[i] : 0.0f;
        Lt[hc] = hc | kHaloBit;
      }
    }
  }
  lds_barrier();
  STAMP(0)
  if (MOD_ABLATE(c, 1 << 14)) return;                // (ablation builds: kernel truncated after a phase, timing only — tools/ablate.sh)
  // ---- phase A1: horizontal runs of the wave's rows by ballot (no atomics) ---------------------------------------------
  // One row of the grid: runs of the 64 tile columns by ballot; the left-halo cells chained to lane 0 by horizontal links
  // (h0 - lane 0, h1 - h0, ...) join lane 0's run.  Returns "linked to the left neighbour" (an up-left edge).
  auto link_row = [&](int gr) -> bool {
    const bool halo_row = gr < NMAX;
    const int me = gr * PW + NMAX + lane;
    const uint64_t mw = m0[gr], ml = mL[gr];
    const bool dyn = (mw >> lane) & 1ull;
    const float z = zt[me];
    const float zl = wave_prev_f32(z);
    const bool cl = dyn && lane > 0 && ((mw >> (lane - 1)) & 1ull) && !(fabsf(z - zl) > th);   // linked to the left neighbour
    const uint64_t C = __ballot(cl);
    const uint64_t starts = mw & ~C;                // run starts: dynamic and not linked to the left
    // left-halo cells: lane j < n owns the cell in column x0-1-j; bit j of lk: it is linked to its right neighbour
    const int hc = gr * PW + NMAX - 1 - min(lane, NMAX - 1);
    int m = 0;                                      // cells h0 .. h(m-1) hang on lane 0 through an unbroken chain of links
    if ((ml >> 63) & mw & 1ull) {                   // wave-uniform: the chain starts with h0 - lane 0, both dynamic
      const bool hdyn = lane < n && ((ml >> (63 - lane)) & 1ull);
      const bool rdyn = lane == 0 ? (bool)(mw & 1ull) : (bool)((ml >> (64 - lane)) & 1ull);
      const bool hl = hdyn && rdyn && !(fabsf(zt[hc] - zt[hc + 1]) > th);
      const uint32_t lk = (uint32_t)__ballot(hl);
      m = __builtin_ctz(~lk);
    }
    // label of lane 0's run: its own cell — in a halo row the leftmost chained cell (parents must not be larger than children)
    const int id0 = halo_row ? ((gr * PW + NMAX - m) | kHaloBit) : (gr * PW + NMAX);
    if (dyn) {
      const int s = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));
      Lt[me] = s == 0 ? id0 : ((me - lane + s) | (halo_row ? kHaloBit : 0));
    }
    if (lane < m) Lt[hc] = id0;
    return cl || (lane == 0 && m > 0);
  };
  bool upr[RPW];
#pragma unroll
  for (int j = 0; j < RPW; j++) {
    const int rr = w + NW * j;
    upr[j] = link_row(rr + NMAX);
  }
  for (int hr = NMAX - 1 - w; hr >= NMAX - n; hr -= NW)   // the halo rows above the tile, dealt to the waves like the tile rows
    if (m0[hr] | mL[hr]) link_row(hr);                    // wave-uniform
  lds_barrier();
  if (MOD_ABLATE(c, 1 << 15)) return;
  // ---- phase A2: vertical pre-link (the pixel straight above), one union per distinct (run, run-above) pair -----------
  // The unions of all the wave's rows are first collected in a queue in LDS and then run ONE PER LANE: run in place they keep
  // about eight of a row's 64 lanes busy (the first lane of each run pair) — and a wave64 instruction costs its four cycles
  // however few lanes are active, which is what bounds this kernel.
  constexpr int kJobCap = 128;
  __shared__ int s_ja[NW][kJobCap], s_jb[NW][kJobCap];
  int njobs = 0;                                     // wave-uniform
  auto push_jobs = [&](bool rep, int ja, int jb) {
    const uint64_t m = __ballot(rep);
    if (m == 0) return;                              // wave-uniform
    const int cnt = __popcll((unsigned long long)m);
    if (njobs + cnt > kJobCap) { if (rep) lds_unite(Lt, ja, jb); return; }   // queue full (wave-uniform): unite in place
    if (rep) {
      const int slot = njobs + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      s_ja[w][slot] = ja; s_jb[w][slot] = jb;
    }
    njobs += cnt;
  };
  auto link_up = [&](int gr) -> bool {              // grid row gr with grid row gr - 1 (tile rows and halo rows alike)
    const int me = gr * PW + NMAX + lane;
    const uint64_t both = m0[gr] & m0[gr - 1], hboth = (mL[gr] & mL[gr - 1]) >> (64 - NMAX);
    bool link = false;
    if (both != 0 && !MOD_ABLATE(c, 2048)) {                                // wave-uniform
      link = ((both >> lane) & 1ull) && !(fabsf(zt[me] - zt[me - PW]) > th);
      // lanes of one run looking at one run above all hold the same (label, label above) pair: the first lane of each contiguous
      // group of equal pairs represents it.  (Labels are not refreshed afterwards: phase A3 flattens every cell.)
      const int cur = ld_relaxed(&Lt[me]), oth = ld_relaxed(&Lt[me - PW]);
      const int pc = wave_prev_i32(cur), po = wave_prev_i32(oth), pn = wave_prev_i32((int)link);
      push_jobs(link && !(lane > 0 && pn && pc == cur && po == oth), cur, oth);
    }
    if (hboth != 0) {                                                       // wave-uniform: the left-halo cells, column by column
      const int hc = gr * PW + NMAX - 1 - min(lane, NMAX - 1);
      const bool hlink = lane < n && ((hboth >> (NMAX - 1 - lane)) & 1ull) && !(fabsf(zt[hc] - zt[hc - PW]) > th);
      const int cur = ld_relaxed(&Lt[hc]), oth = ld_relaxed(&Lt[hc - PW]);
      const int pc = wave_prev_i32(cur), po = wave_prev_i32(oth), pn = wave_prev_i32((int)hlink);
      push_jobs(hlink && !(lane > 0 && pn && pc == cur && po == oth), cur, oth);
    }
    return link;
  };
#pragma unroll
  for (int j = 0; j < RPW; j++) {
    const int rr = w + NW * j;
    const bool link = link_up(rr + NMAX);
    upr[j] = upr[j] || link;
  }
  for (int hr = NMAX - 1 - w; hr > NMAX - n; hr -= NW) link_up(hr);
  auto run_jobs = [&]() {
    for (int j0 = 0; j0 < njobs; j0 += 64) {         // wave-uniform; the wave's own queue: its LDS writes are in order, no barrier
      const int j = j0 + lane;
      if (j < njobs) lds_unite(Lt, s_ja[w][j], s_jb[w][j]);
    }
    njobs = 0;
  };
  run_jobs();
  lds_barrier();
  if (MOD_ABLATE(c, 1 << 16)) return;
  // ---- phase A3: flatten, so that phase B can compare labels directly -------------------------------------------------
  auto flatten_row = [&](int gr) {
    const int me = gr * PW + NMAX + lane;
    const bool dyn = (m0[gr] >> lane) & 1ull, hdyn = lane < n && ((mL[gr] >> (63 - lane)) & 1ull);
    int lab = -1, hlab = -1;
    if (dyn) { lab = lds_find(Lt, ld_relaxed(&Lt[me])); if (ld_relaxed(&Lt[me]) != lab) Lt[me] = lab; }
    if (hdyn) {
      const int hc = gr * PW + NMAX - 1 - lane;
      hlab = lds_find(Lt, ld_relaxed(&Lt[hc]));
      if (ld_relaxed(&Lt[hc]) != hlab) Lt[hc] = hlab;
    }
    // row summary for phase B: when this row and a window row both carry one and the same label, no union can come of them
    const uint64_t db = __ballot(dyn), hb = __ballot(hdyn);
    int first = -1;
    if (db) first = __builtin_amdgcn_readlane(lab, __builtin_ctzll(db));
    else if (hb) first = __builtin_amdgcn_readlane(hlab, __builtin_ctzll(hb));
    const bool uni = __ballot((dyn && lab != first) || (hdyn && hlab != first)) == 0;
    if (lane == 0) s_uni[gr] = uni ? first : -1;
  };
#pragma unroll
  for (int j = 0; j < RPW; j++) flatten_row(w + NW * j + NMAX);
  for (int hr = NMAX - 1 - w; hr >= NMAX - n; hr -= NW) flatten_row(hr);
  lds_barrier();
  STAMP(1)
  if (MOD_ABLATE(c, 1 << 17)) return;
  // ---- phase B: the rest of the up-left window --------------------------------------------------------------------------
  const uint32_t kmask = (2u << n) - 1u;              // n + 1 low bits
#pragma unroll
  for (int j = 0; j < RPW; j++) {
    const int rr = w + NW * j;
    const uint64_t mw = m0[rr + NMAX];
    if (mw == 0 || MOD_ABLATE(c, 256)) continue;                           // wave-uniform
    const bool dyn = (mw >> lane) & 1ull;
    const int me = (rr + NMAX) * PW + NMAX + lane;
    const float zp = zt[me];
    int cur = dyn ? ld_relaxed(&Lt[me]) : -1, last = -1;
    bool up = upr[j];
    const int ul = s_uni[rr + NMAX];                 // wave-uniform
    bool rowup = __ballot(dyn & !up) == 0;           // every dynamic pixel of the row has an up-left edge (wave-uniform)
    COUNT(13, 1)
#pragma unroll
    for (int dv = 0; dv <= (EXACT ? NMAX : n); dv++) {   // unrolled in the EXACT instance
      const int qg = rr + NMAX - dv;                 // grid row of the window row
      const uint64_t q0 = m0[qg], qL = mL[qg];
      if ((q0 | qL) == 0) continue;                  // wave-uniform
      // both rows carry one label, the same (phase A3's summaries): nothing to unite; when every pixel of the row has its
      // up-left edge already, the window row is of no interest at all (wave-uniform, scalar)
      const bool same = ul >= 0 && s_uni[qg] == ul;
      if (same && rowup) continue;
      // bit i of nb = pixel (lane - n + i) of the window row is dynamic  (i = n - k)
      uint32_t nb;
      if (lane >= n) nb = (uint32_t)(q0 >> (lane - n));
      else nb = (uint32_t)((q0 << (n - lane)) | (qL >> (64 - (n - lane))));
      nb = dyn ? (nb & kmask) : 0u;
      if (dv == 0) nb &= ~(1u << n);                 // k == 0 is p itself
      if (__ballot(nb != 0) == 0) continue;          // wave-uniform
      COUNT(9, 1)
      if (MOD_ABLATE(c, 8192)) continue;             // (ablation builds: loop header only)
      const int base = qg * PW + NMAX + lane;
      if (same) {
        if (MOD_ABLATE(c, 4096)) continue;                                    // only pixels that still lack their first up-left edge look for it
        if (__ballot(!up & (nb != 0)) == 0) continue;
        uint32_t cand2 = __brev(nb) >> (31 - n);
        if (dv == 0) cand2 &= ~3u;
        if (dv == 1) cand2 &= ~1u;
        uint32_t g2 = 0;
#pragma unroll
        for (int k = 0; k <= NMAX; k++) g2 |= (fabsf(zp - zt[base - k]) > th) ? 0u : (1u << k);
        up = up || ((cand2 & g2) != 0);
        rowup = __ballot(dyn & !up) == 0;
        continue;
      }
      // pass 1, branch-free: labels first, one bit per window position (k = columns to the left)
      int lq[NMAX + 1];
#pragma unroll
      for (int k = 0; k <= NMAX; k++) lq[k] = ld_relaxed(&Lt[base - k]);
      uint32_t dmask = 0;                            // bit k: label differs from this pixel's
#pragma unroll
      for (int k = 0; k <= NMAX; k++) dmask |= (lq[k] != cur) ? (1u << k) : 0u;
      // nb holds pixel (lane - n + i) at bit i: reverse it so that bit k = pixel (lane - k)
      uint32_t cand = __brev(nb) >> (31 - n);
      // (0,0) is p itself; (0,-1) inside the wave is the run link of phase A1, (-1,0) the vertical link of phase A2
      if (dv == 0) cand &= ~3u;                      // (lane 0: its link to the halo cell left of it was made in phase A1 as well)
      if (dv == 1) cand &= ~1u;
      // Inside a blob that phases A1-A3 already merged, every candidate carries this pixel's label and the pixel has its
      // up-left edge: the depth gate cannot change anything, so its LDS reads and compares are skipped (wave-uniform).
      if (__ballot(((cand & dmask) != 0) | (!up & (cand != 0))) == 0) continue;
      COUNT(14, 1)
      COUNT(15, __popcll(__ballot((cand & dmask) != 0)) ? 1 : 0)
      float zq[NMAX + 1];
#pragma unroll
      for (int k = 0; k <= NMAX; k++) zq[k] = zt[base - k];
      uint32_t gmask = 0;                            // bit k: depth gate passes
#pragma unroll
      for (int k = 0; k <= NMAX; k++) gmask |= (fabsf(zp - zq[k]) > th) ? 0u : (1u << k);   // depthDiff gate (:194); NaN links
      const uint32_t vmask = cand & gmask;
      // halo cells are ordinary nodes of the union-find (their ids carry bit 15, so they never become the root of a set that has
      // a tile pixel); phases A1-A3 have linked them like tile pixels, so they mostly carry this pixel's label already
      const bool need_any = (vmask & dmask) != 0;
      up = up || (vmask != 0);
      // pass 2, rare after A1-A3: the unions go to the wave's job queue (run one per lane after the last row, like phase A2's);
      // `cur` is not refreshed meanwhile, so a pair may be queued again from a later window row — a void union, two finds
      if (!MOD_ABLATE(c, 1) && __ballot(need_any)) {
        COUNT(10, 1)
#pragma unroll
        for (int k = 0; k <= NMAX; k++) {
          if (k > n || (dv == 0 && k == 0)) continue;
          const int lab = lq[k];
          const bool need = ((vmask >> k) & 1u) && lab != cur && lab != last;
          if (__ballot(need)) {                        // wave-uniform
            COUNT(12, 1)
            const int pl = wave_prev_i32(lab), pc = wave_prev_i32(cur), pn = wave_prev_i32((int)need);
            push_jobs(need && !(lane > 0 && pn && pc == cur && pl == lab), cur, lab);
            if (need) last = lab;
          }
        }
      }
    }
    STAMP(3)
    upr[j] = up;
  }
  run_jobs();
  lds_barrier();
  STAMP(4)
  // ---- phase C: publish ----------------------------------------------------------------------------------------------
  // interior pixels point at their tile root (plain stores: nobody else writes these entries in this kernel), tile roots
  // get an empty statistics record and a bit in the root plane
  int rootg[RPW], rootc[RPW];
  uint64_t rootbits[RPW];
#pragma unroll
  for (int j = 0; j < RPW; j++) {
    const int rr = w + NW * j, gy = y0 + rr;
    const bool dyn = (m0[rr + NMAX] >> lane) & 1ull;
    int rg = -1, rc = -1;
    bool isroot = false;
    if (dyn) {
      const int me = (rr + NMAX) * PW + NMAX + lane;
      const int r = lds_find(Lt, me);                // interior by construction
      const int rgr = r / PW, rgc = r - rgr * PW;
      rg = (y0 + rgr - NMAX) * c.W + x0 + rgc - NMAX;
      rc = r;
      if (MOD_CHECK(a, rg >= 0 && (size_t)rg < N && rgr >= NMAX && rgc >= NMAX, 13)) a.parent[fN + (size_t)gy * c.W + x0 + lane] = rg;
      isroot = (r == me);
    }
    rootg[j] = rg; rootc[j] = rc;
    const uint64_t rb = __ballot(isroot);
    rootbits[j] = rb;
    if (lane == 0 && gy < c.H) a.lroot[((size_t)f * c.H + gy) * MW + wi] = rb;
  }
  STAMP(5)
  if (MOD_ABLATE(c, 1 << 18)) return;
  // halo pixels that ended up in a tile component belong to other tiles, whose roots are not known yet: leave one link
  // request (halo pixel, tile root) per connected group of them for k_ccl_link.  First every halo cell is flattened to its root
  // (no union runs any more), so that the neighbour tests below are plain LDS reads.
  {
    const int topcells = n * (64 + n);               // n rows x (n + 64) columns above the tile
    const int total = topcells + TH * n;             // + TH rows x n columns left of it
    auto cell_of = [&](int i, int &gr, int &gc) {
      if (i < topcells) { gr = NMAX - n + i / (64 + n); gc = NMAX - n + i % (64 + n); }
      else { const int t = i - topcells; gr = NMAX + t / n; gc = NMAX - n + t % n; }
    };
    auto halo_dyn = [&](int gr, int gc) {
      const int gx = x0 - NMAX + gc;
      const uint64_t mw = (gc >= NMAX) ? m0[gr] : mL[gr];
      return gx >= 0 && ((mw >> (gx & 63)) & 1ull);
    };
    const bool any_halo = !MOD_ABLATE(c, 1024) && s_anyhalo;   // workgroup-uniform
    for (int i0 = 0; i0 < total && any_halo; i0 += NW * 64) {
      const int i = i0 + tid;
      if (i < total) {
        int gr, gc;
        cell_of(i, gr, gc);
        if (halo_dyn(gr, gc)) { const int cell = gr * PW + gc; Lt[cell] = lds_find(Lt, cell | kHaloBit); }
      }
    }
    lds_barrier();
    uint2 *req = a.requests + ((size_t)f * tiles_y * tiles_x + (size_t)ty * tiles_x + wi) * a.req_cap;
    for (int i0 = 0; i0 < total && any_halo; i0 += NW * 64) {
      const int i = i0 + tid;
      bool linked = false;
      int hg = 0, rg = 0;
      if (i < total) {
        int gr, gc;
        cell_of(i, gr, gc);
        if (halo_dyn(gr, gc)) {
          const int r = Lt[gr * PW + gc];
          if (!(r & kHaloBit)) {                       // in a component that has a tile pixel (halo cells may also be linked among themselves)
            // A halo cell whose left or upper neighbour is a halo cell of the SAME set with a direct edge to it (dynamic, depth gate
            // passes) leaves the request to that neighbour: the edge between the two is an edge of the image graph that the tile
            // owning this cell sees itself, so one request per connected group of halo cells (its top-left-most cell) is enough.
            const float zme = zt[gr * PW + gc];
            auto covered = [&](int gr2, int gc2) {
              if (gr2 < NMAX - n || gc2 < NMAX - n || !halo_dyn(gr2, gc2)) return false;
              const int cell2 = gr2 * PW + gc2;
              return !(fabsf(zme - zt[cell2]) > th) && Lt[cell2] == r;
            };
            if (!(covered(gr, gc - 1) || covered(gr - 1, gc))) {
              const int rgr = r / PW, rgc = r - rgr * PW;
              rg = (y0 + rgr - NMAX) * c.W + x0 + rgc - NMAX;
              hg = (y0 - NMAX + gr) * c.W + x0 - NMAX + gc;
              linked = true;
            }
          }
        }
      }
      const uint64_t lb = __ballot(linked);
      if (lb) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_nreq, __popcll((unsigned long long)lb));
        base = __builtin_amdgcn_readfirstlane(base);
        if (linked) {
          const int slot = base + __popcll((unsigned long long)(lb & ((1ull << lane) - 1ull)));
          if (MOD_CHECK(a, slot >= 0 && slot < a.req_cap, 12) && MOD_CHECK(a, rg >= 0 && (size_t)rg < N && hg >= 0 && (size_t)hg < N, 13))
            req[slot] = make_uint2((uint32_t)hg, (uint32_t)rg);
        }
      }
    }
  }
  STAMP(6)
  lds_barrier();                                     // every find on Lt is done: root cells can be re-used as slot tags
  // ---- phase D: partial statistics of the tile's components --------------------------------------------------------
  // The tile owns its roots' records, so they are reduced in LDS slots and stored once — no global atomics.  Roots beyond
  // kSlots (very fragmented tiles) fall back to initialise-then-atomics on the global record.
#pragma unroll
  for (int j = 0; j < RPW; j++) {
    const bool isroot = (rootbits[j] >> lane) & 1ull;
    if (isroot) {
      const int slot = atomicAdd(&s_nslots, 1);
      RootRec rec;
      rec.size = 0; rec.key = kKeyNone;
      if (slot < kSlots) { srec[slot] = rec; sroot[slot] = rootg[j]; Lt[rootc[j]] = -(slot + 1); }
      else { a.rsize[fN + rootg[j]] = 0; a.rkey[fN + rootg[j]] = kKeyNone; }
    }
  }
  lds_barrier();     // slot tags visible
  if (s_nslots > kSlots) __syncthreads();   // overflow records must have reached L2 before any wave's atomics on them
  STAMP(7)
#pragma unroll
  for (int j = 0; j < RPW; j++) {
    const int rr = w + NW * j, gy = y0 + rr;
    if (m0[rr + NMAX] == 0 || MOD_ABLATE(c, 520)) continue;                // wave-uniform
    const int rg = rootg[j];
    uint32_t key = (uint32_t)kKeyNone;
    int slot = -1, over = -1;
    if (rg >= 0) {
      const size_t gp = (size_t)gy * c.W + x0 + lane;
      if (upr[j]) key = (uint32_t)gp;
      const int tag = Lt[rootc[j]];
      if (tag < 0) slot = -tag - 1; else over = rg;
    }
    wave_accumulate(&srec[0].size, &srec[0].key, 2, slot, key, lane);
    if (__ballot(over >= 0)) wave_accumulate(a.rsize + fN, a.rkey + fN, 1, over, key, lane);
  }
  lds_barrier();
  {
    const int ns = min(s_nslots, kSlots);
    if (tid < ns) { a.rsize[fN + sroot[tid]] = srec[tid].size; a.rkey[fN + sroot[tid]] = srec[tid].key; }
  }
  STAMP(8)
#undef STAMP
#undef COUNT
  if (tid == 0) hdr[1] = s_nreq;                   // s_nreq is final: the barrier after the request loop has passed (hdr[0] is 1 already)
}

// The same tile body for the tiles of a LIST (k_ccl_bits leaves the tiles it cannot decide there): a fixed number of workgroups,
// each pulling the next tile with one atomic — the list is a fifth of the active tiles, one workgroup per grid tile would spend
// the launch on 460 k header reads.  counters[4] = length of the list, counters[3] = cursor (both zeroed by the caller).
template <int TH, int NMAX, int NW, bool EXACT>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_ccl_tile_list(DevCam c, ClArgs a, int tiles_x, int tiles_y) {
  __shared__ int s_next;
  const int count = a.counters[4];
  // workgroup i starts with list entry i (a short list — the usual case — costs the other workgroups one scalar load), further
  // entries are pulled with the cursor, which starts behind the statically assigned ones
  int i = (int)blockIdx.x;
  const int per_frame = tiles_x * tiles_y;
  while (i < count) {
    const uint32_t t = a.tilelist[i];
    const int f = (int)(t / (uint32_t)per_frame), r = (int)(t - (uint32_t)f * (uint32_t)per_frame), ty = r / tiles_x, wi = r - ty * tiles_x;
    ccl_tile_body<TH, NMAX, NW, EXACT>(c, a, wi, ty, f, tiles_x, tiles_y);
    __syncthreads();                                 // the next tile re-uses the LDS arrays and s_next
    if (threadIdx.x == 0 && threadIdx.y == 0) s_next = (int)gridDim.x + atomicAdd(&a.counters[3], 1);
    __syncthreads();
    i = __builtin_amdgcn_readfirstlane(s_next);
  }
}
}  // namespace

void launch_ccl_tile(const DevCam &c, const ClArgs &a, int frames, hipStream_t s) {
  const dim3 block(64, kTileWaves, 1), tgrid = tile_grid(c, frames);
  const int tx = (int)tgrid.x, tyn = (int)tgrid.y;
  if (c.n >= 1 && c.n <= 10) {
    // the reference's parameter range (Clusterer.cfg:11): bit-plane kernel first (one wave per tile, one instance per window size),
    // then the union-find kernel over the tiles it listed — resident workgroups (8 per CU) that pull tiles with an atomic cursor
    launch_ccl_bits(c, a, frames, s);
    // (2048 workgroups = the 8 per CU that fit: 512 / 1024 / 4096 / 8192 measured slower or equal)
    const unsigned total = tgrid.x * tgrid.y * tgrid.z;
    const dim3 lgrid(std::min(2048u, total));
    if (c.n == 4) hipLaunchKernelGGL((k_ccl_tile_list<kTileH, 4, kTileWaves, true>), lgrid, block, 0, s, c, a, tx, tyn);
    else if (c.n < 4) hipLaunchKernelGGL((k_ccl_tile_list<kTileH, 4, kTileWaves, false>), lgrid, block, 0, s, c, a, tx, tyn);
    else if (c.n <= 8) hipLaunchKernelGGL((k_ccl_tile_list<kTileH, 8, kTileWaves, false>), lgrid, block, 0, s, c, a, tx, tyn);
    else hipLaunchKernelGGL((k_ccl_tile_list<kTileH, 16, kTileWaves, false>), lgrid, block, 0, s, c, a, tx, tyn);
    return;
  }
  const dim3 ggrid((tgrid.x + CCL_TPB - 1) / CCL_TPB, tgrid.y, tgrid.z);
  if (c.n < 4) hipLaunchKernelGGL((k_ccl_tile<kTileH, 4, kTileWaves, false>), ggrid, block, 0, s, c, a, tx, tyn);
  else if (c.n <= 8) hipLaunchKernelGGL((k_ccl_tile<kTileH, 8, kTileWaves, false>), ggrid, block, 0, s, c, a, tx, tyn);
  else hipLaunchKernelGGL((k_ccl_tile<kTileH, 16, kTileWaves, false>), ggrid, block, 0, s, c, a, tx, tyn);
}

int ccl_tile_rows() { return kTileH; }
int ccl_tiles(int mask_words, int H) { return mask_words * ((H + kTileH - 1) / kTileH); }
int ccl_request_capacity(int n) { return n * (64 + n) + kTileH * n; }
