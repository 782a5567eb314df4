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
