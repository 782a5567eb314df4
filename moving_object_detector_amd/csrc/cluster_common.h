// cluster_common.h — moving-point clustering on gfx950 (MI355X): what the stages of the clusterer share.
//
// Replaces ClustererNodelet::clustering + publishMovingObjects
// (scene_flow_clusterer/src/clusterer_nodelet.cpp:85-95,324-343):
//   calculateInitialClusterMap + comparePoints + LookupTable   :56-83,186-219, include/lookup_table.h:10-33
//   integrateConnectedClusters                                  :253-267
//   removeSmallClusters                                         :354-393
//   clusterMap2IndicesCluster + cluster2MovingObject            :97-117,147-184
//
// The reference is a serial raster scan with a union-find; what it computes is order-independent (SURVEY.md
// Appendix A): the connected components of the graph whose edges join a dynamic pixel p to each dynamic pixel q in
// its up-left (n+1)x(n+1) window with !(|z_p - z_q| > depth_diff); components without an edge stay unlabelled;
// survivors of the size filter are numbered by ascending first_edge_key = the smallest raster index of a member that
// has an up-left edge (that is where the serial scan creates the component's first — hence smallest — label).
//
// GPU formulation (one launcher per stage, include/mod_sf.h MOD_STAGE_*; one source per stage: ccl_tile.hip + ccl_bits.hip, ccl_merge.hip,
//                  cluster_final.hip, cluster_median.hip)
//   k_ccl_tile     one workgroup per 64 x 16 tile + n-pixel halo (up / left): masked depth + parents live in LDS; rows are
//                  pre-linked into runs with wave ballots, vertically with one union per run pair, the remaining window edges
//                  are united with LDS atomicMin hooks; interior pixels publish parent[p] = tile root with plain stores, halo
//                  pixels that were reached leave link requests; one partial statistics record per tile root.
//   k_ccl_link     requests -> unions between tile roots (device-scope atomicMin hooks), one wave per tile.
//   k_ccl_merge    every tile root finds its final root, folds its record into it; final roots are listed; in a small batch the
//                  frame's last workgroup goes on to the size filter;
//   k_select       (large batches: a kernel of its own) size filter + ordering by first_edge_key (the reference's numbering), work list.
//   k_final        labels plane + per-cluster member lists (||v|| bits, pixel).
//   k_cluster_members  opt-in (mod_set_cluster_members): the member lists in the reference's column-major order, for the caller
//                  (cluster_final.hip; the layout it shares with k_median_ties is at the end of this header).
//   k_median       exact selection of the member at size/2 by ||v|| (norms held in registers, LDS histogram rounds);
//   k_median_ties  replay of libstdc++'s introsort for clusters whose median ties between different vectors; the launch's last
//                  workgroup assigns the object ids over the accepted clusters and zeroes the counters for the next call.
#pragma once
#include "mod_launch.h"

constexpr int kKeyNone = 0x7fffffff;

// Workgroup barrier for phases that only exchange data through LDS: waits for this wave's LDS operations, not for its
// outstanding global loads/stores (__syncthreads() drains vmcnt(0) and would serialise every HBM round trip).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------------------------------------------------------
// Union-find helpers.  parent[i] <= i always; roots satisfy parent[r] == r; a larger root is hooked under a smaller
// one with atomicMin, whose return value tells whether the node was still a root.  Reads are relaxed atomic loads so
// the compiler re-reads memory; values that are stale in a CU's L1 are harmless: every value ever stored in parent[a]
// is a member of a's set and smaller than a, so a stale chain still ends inside the same set.
__device__ __forceinline__ int ld_relaxed(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// device-scope store / load: to / from memory past the (per-XCD, mutually incoherent) L2s — how a workgroup reads, in the SAME kernel,
// what a workgroup on another XCD has written (k_ccl_merge's last workgroup per frame)
__device__ __forceinline__ void st_agent(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(const int *parent, int a) {
  int p = ld_relaxed(parent + a);
  while (p != a) { a = p; p = ld_relaxed(parent + a); }
  return a;
}

// unite the sets of a and b; returns the (current) root of the merged set
__device__ __forceinline__ int uf_unite(int *parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return a;
    if (a < b) { const int t = a; a = b; b = t; }   // hook the larger root a under the smaller b
    const int old = atomicMin(&parent[a], b);
    if (old == a) return b;                          // a was still a root
    a = old;                                         // a had been hooked meanwhile: unite its parent with b instead
  }
}

constexpr int kTileH = 16, kTileWaves = 4;   // tile = 64 x 16 px, 4 rows per wave (measured best of 8x4, 16x4, 16x8, 32x8)
static inline dim3 tile_grid(const DevCam &c, int frames) { return dim3(c.mask_words, ccl_tiles(1, c.H), frames); }   // (1 word: the tile rows)
void launch_ccl_bits(const DevCam &c, const ClArgs &a, int frames, hipStream_t s);   // k_ccl_bits<c.n>, c.n = 1 .. 10 (ccl_bits.hip)

// Block-level phase stamps of the diagnostic build (make PHASE_COUNTERS=1): PHASE_CLOCK starts the clock of a work item, PHASE_STAMP(i)
// adds the time since the previous stamp to a.dbg[i] (the whole workgroup meets at a barrier first; `a` and `tid` are the kernel's)
#ifdef MOD_PHASE_COUNTERS
#define PHASE_CLOCK unsigned long long pt0 = wall_clock64(), pt1;
#define PHASE_STAMP(i) { __syncthreads(); pt1 = wall_clock64(); if (tid == 0) atomicAdd(&a.dbg[i], pt1 - pt0); pt0 = pt1; }
#else
#define PHASE_CLOCK
#define PHASE_STAMP(i)
#endif

// ---------------------------------------------------------------------------------------------------------------
// Member layout — a cluster's member list put into the reference's order (column-major pixel order, clusterMap2IndicesCluster,
// clusterer_nodelet.cpp:97-117) without a sort.  Shared by k_median_ties (cluster_median.hip: the initial order of the replayed
// introsort) and k_cluster_members (cluster_final.hip: the lists a caller receives); tests/models/cluster_members_model.py restates
// it on Python integers.
//
// The members arrive as pixel indices in no particular order (k_final's compaction).  Their image-space bounding box is cut into
// cells of one column x 64 rows; pass A sets bit (row & 63) of a member's cell in a 64-bit LDS mask, a prefix over the cell
// populations in column-major cell order gives every cell its first slot, pass B puts member (column, row) at
// slot = start[cell] + popcount(mask[cell] below its bit).  Two coalesced passes over the list, no image reads.  Boxes with more
// cells than the LDS arrays hold take the two passes once per run of CELLS cells; `base` carries the members of the runs before.
//
// The group that lays a cluster out is NT threads: a whole workgroup (NT = its size, barriers) or one wave (NT = 64: the lanes
// run in lockstep and a wave's LDS operations complete in order, so the steps only wait for them).

// Row of pixel index p (the return value) and its column, by an integer divide.  (Images below 2^24 pixels used to take the row as
// (uint32_t)(((float)p + 0.5f) * (1.0f / W)).  That is NOT exact: the rounding of 1.0f / W and of the product outgrows the 0.5 / W
// margin from about p = 2^22 on.  At 3840 x 2160 the 834 last-column pixels from row 1326 down came out as row + 1 with column
// 0xffffffff, fell out of the column-major layout, and the replay sorted a list with stale entries.  tests/models/row_model.py keeps
// that formula and tests/test_row_model.py its failures.  Both passes that call this wait on memory, not on the divide.)
__device__ __forceinline__ uint32_t tie_row_col(uint32_t p, uint32_t W, uint32_t &x) {
  const uint32_t y = p / W;
  x = p - y * W;
  return y;
}

template <int NT> __device__ __forceinline__ void layout_sync() {
  if constexpr (NT == 64) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  else __syncthreads();
}

struct MemberBox { int xmin, ymin, ymax, ncols; };

// Image-space bounding box of the `size` (>= 1) members pix[0 .. size).  s_box: four LDS words of the group (unused by a wave).
// All NT threads must call it; a workgroup leaves it behind a barrier.
template <int NT> __device__ __forceinline__ MemberBox member_box(const uint32_t *pix, int size, uint32_t W, int *s_box, int tid) {
  const int lane = tid & 63;
  if constexpr (NT != 64) {
    if (tid == 0) { s_box[0] = 0x7fffffff; s_box[1] = 0; s_box[2] = 0x7fffffff; s_box[3] = 0; }
    __syncthreads();
  }
  uint32_t x0 = 0xffffffffu, x1 = 0, y0 = 0xffffffffu, y1 = 0;
  for (int i0 = tid; i0 < size; i0 += NT * 4) {
    uint32_t p4[4];
#pragma unroll
    for (int u = 0; u < 4; u++) p4[u] = pix[min(i0 + u * NT, size - 1)];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      uint32_t x;
      const uint32_t y = tie_row_col(p4[u], W, x);
      x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
    }
  }
  x0 = wave_min_u32(x0); x1 = wave_max_u32(x1); y0 = wave_min_u32(y0); y1 = wave_max_u32(y1);
  if constexpr (NT == 64) return MemberBox{(int)x0, (int)y0, (int)y1, (int)(x1 - x0) + 1};
  else {
    if (lane == 0 && x0 != 0xffffffffu) { atomicMin(&s_box[0], (int)x0); atomicMax(&s_box[1], (int)x1); atomicMin(&s_box[2], (int)y0); atomicMax(&s_box[3], (int)y1); }
    __syncthreads();
    return MemberBox{s_box[0], s_box[2], s_box[3], s_box[1] - s_box[0] + 1};
  }
}

// The two passes.  cmask / cstart: CELLS LDS entries each, the group's own; s_sum: NT / 64 + 1 LDS words (unused by a wave).
// load(i) fetches what else the caller keeps per list position (it leaves with pass B's pixel loads), emit(slot, p, extra, column,
// row) receives every member once, slot counting in column-major order from 0; stamp(0) / stamp(1) follow pass A / pass B of every
// run (phase stamps of the diagnostic build).  Returns the number of members placed (== size for a list of distinct pixels).
// All NT threads must call it; a workgroup leaves it behind a barrier.
template <int NT, int CELLS, class Load, class Emit, class Stamp>
__device__ __forceinline__ int member_layout(const uint32_t *pix, int size, uint32_t W, const MemberBox &bx, uint64_t *cmask, uint32_t *cstart,
                                             int *s_sum, int tid, Load load, Emit emit, Stamp stamp) {
  const int lane = tid & 63, wv = tid >> 6;
  const int xmin = bx.xmin, ymin = bx.ymin;
  const int nseg64 = (bx.ymax - ymin + 64) / 64;
  const int ncell = bx.ncols * nseg64;               // < 2^21 + W: W * H < 2^27
  auto cell_of = [&](uint32_t p, int &bit, uint32_t &x, uint32_t &y) {
    y = tie_row_col(p, W, x);
    const int ry = (int)y - ymin;
    bit = ry & 63;
    return ((int)x - xmin) * nseg64 + (ry >> 6);
  };
  int base = 0;
  for (int g0 = 0; g0 < ncell; g0 += CELLS) {        // group-uniform
    const int ncl = min(CELLS, ncell - g0);
    for (int i = tid; i < CELLS; i += NT) cmask[i] = 0ull;
    layout_sync<NT>();
    for (int i0 = tid; i0 < size; i0 += NT * 8) {
      uint32_t p8[8];
#pragma unroll
      for (int u = 0; u < 8; u++) p8[u] = pix[min(i0 + u * NT, size - 1)];
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (i0 + u * NT < size) {
          int bit;
          uint32_t x, y;
          const int cl = cell_of(p8[u], bit, x, y) - g0;
          if (cl >= 0 && cl < ncl) atomicOr((unsigned long long *)&cmask[cl], 1ull << bit);
        }
    }
    layout_sync<NT>();
    stamp(0);
    {   // exclusive prefix of the cell populations; thread t owns cells CPT t .. CPT t + CPT - 1
      constexpr int CPT = CELLS / NT;
      static_assert(CPT * NT == CELLS, "every thread owns the same number of cells");
      int cnt[CPT], tot = 0;
#pragma unroll
      for (int u = 0; u < CPT; u++) { const int ci2 = tid * CPT + u; cnt[u] = ci2 < ncl ? __popcll((unsigned long long)cmask[ci2]) : 0; tot += cnt[u]; }
      int incl = tot;
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
      int run;
      if constexpr (NT == 64) {
        run = base + incl - tot;
        base += __shfl(incl, 63);
      } else {
        if (lane == 63) s_sum[wv] = incl;
        __syncthreads();
        if (tid == 0) { int r = base; for (int t = 0; t < NT / 64; t++) { const int x = s_sum[t]; s_sum[t] = r; r += x; } s_sum[NT / 64] = r; }
        __syncthreads();
        run = s_sum[wv] + incl - tot;
        base = s_sum[NT / 64];
      }
#pragma unroll
      for (int u = 0; u < CPT; u++) { cstart[tid * CPT + u] = (uint32_t)run; run += cnt[u]; }
    }
    layout_sync<NT>();
    for (int i0 = tid; i0 < size; i0 += NT * 8) {
      uint32_t p8[8], k8[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { const int i = min(i0 + u * NT, size - 1); p8[u] = pix[i]; k8[u] = load(i); }
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (i0 + u * NT < size) {
          int bit;
          uint32_t x, y;
          const int cl = cell_of(p8[u], bit, x, y) - g0;
          if (cl >= 0 && cl < ncl) {
            const int slot = (int)cstart[cl] + __popcll((unsigned long long)(cmask[cl] & ((1ull << bit) - 1ull)));
            emit(slot, p8[u], k8[u], x, y);
          }
        }
    }
    layout_sync<NT>();
    stamp(1);
  }
  return base;
}
