// ccl_merge.hip — MOD_STAGE_CCL_LINK, MOD_STAGE_CCL_MERGE: k_tile_flags, k_ccl_link, k_ccl_merge, k_select (overview: cluster_common.h)
#include "cluster_common.h"
#pragma clang fp contract(off)
namespace {

// Tile headers from a mask plane that did not come out of the fused scene-flow kernel (mod_cluster_dev): {1, 0} for tiles with a
// dynamic pixel, {0, 0} for the others.  One thread per tile.
template <int TH>
__global__ __launch_bounds__(256) void k_tile_flags(DevCam c, ClArgs a, int tiles_x, int tiles_per_frame, int total) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int f = t / tiles_per_frame, tt = t - f * tiles_per_frame, ty = tt / tiles_x, wi = tt - ty * tiles_x;
  const uint64_t *m = a.mask + ((size_t)f * c.H + (size_t)ty * TH) * c.mask_words + wi;
  const int rows = min(TH, c.H - ty * TH);
  uint64_t any = 0;
#pragma unroll 4
  for (int r = 0; r < rows; r++) any |= m[(size_t)r * c.mask_words];
  a.tilehdr[(size_t)t * 2] = any != 0 ? 1 : 0;
  a.tilehdr[(size_t)t * 2 + 1] = 0;
}

// Cross-tile links.  One workgroup per kLinkTiles consecutive tiles (most tiles have no dynamic pixel and no request: a
// workgroup each would spend the kernel on dispatch).  The tiles' request lists are walked as ONE index space by all 256
// threads — every request is a chain of dependent global accesses (request, parent of the halo pixel, two root searches, a
// hook), so what matters is how many are in flight, not which wave owns which tile.  A request is (halo pixel h, tile root r):
// h's own tile has published parent[h] = its tile root by now, so the union is between two tile roots — all parent writes
// here are atomicMin hooks on root entries.  Consecutive requests usually name the same pair; only the first lane of a run acts.
constexpr int kLinkTiles = 32;   // 4 / 8 / 16 / 32 / 64 tiles per workgroup: 0.138 / 0.108 / 0.093 / 0.083 / 0.093 ms per 512 pairs (in-process A/B)

__global__ __launch_bounds__(256) void k_ccl_link(DevCam c, ClArgs a, int tiles_per_frame) {
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int t0 = blockIdx.x * kLinkTiles;
  int cnt[kLinkTiles], total = 0;
#pragma unroll
  for (int u = 0; u < kLinkTiles; u++) {               // block-uniform scalar loads of the headers
    cnt[u] = 0;
    if (t0 + u < tiles_per_frame) {
      const int *hdr = a.tilehdr + ((size_t)f * tiles_per_frame + t0 + u) * 2;
      cnt[u] = hdr[0] ? hdr[1] : 0;
    }
    total += cnt[u];
  }
  if (total == 0) return;
  const size_t N = (size_t)c.W * c.H;
  int *parent = a.parent + (size_t)f * N;
  for (int i0 = 0; i0 < total; i0 += 256) {            // block-uniform
    int i = i0 + tid, u = 0;
#pragma unroll
    for (int v = 0; v < kLinkTiles - 1; v++) if (u == v && i >= cnt[v]) { i -= cnt[v]; u = v + 1; }
    int ra = -1, rb = -1;
    if (i0 + tid < total) {
      const uint2 q = a.requests[((size_t)f * tiles_per_frame + t0 + u) * a.req_cap + i];
      if (MOD_CHECK(a, (size_t)q.x < N && (size_t)q.y < N, 0)) { ra = parent[q.x]; rb = (int)q.y; }
      if (!MOD_CHECK(a, ra < 0 || ((size_t)ra < N && rb >= 0), 1)) ra = -1;
    }
    const int pa = wave_prev_i32(ra), pb = wave_prev_i32(rb);
    if (ra >= 0 && !(lane > 0 && pa == ra && pb == rb)) uf_unite(parent, ra, rb);
  }
}

// Root-level flatten: every tile root finds its final root, remembers it (path compression, so pixels are two hops from
// their final root), and folds its partial record into the final root's record; final roots list themselves for k_select.
// A wave takes 64 / TH tiles at once: lane = (tile, row of the tile) reads that row's root bits and walks them — the few roots
// of a row one after the other, all rows and tiles of the wave side by side (each root is a chain of dependent accesses).
__device__ void select_frame(const DevCam &c, const ClArgs &a, ClusterInfo *tmp, int f, int tid);

template <int TH, bool FILTER>
__global__ __launch_bounds__(256) void k_ccl_merge(DevCam c, ClArgs a, int tiles_per_frame, ClusterInfo *tmp) {
  static_assert(64 % TH == 0, "a wave covers whole tiles");
  constexpr int TPW = 64 / TH;                         // tiles per wave
  const int f = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int t = (blockIdx.x * 4 + wv) * TPW + lane / TH, j = lane % TH;
  const size_t N = (size_t)c.W * c.H;
  int *parent = a.parent + (size_t)f * N;
  int *rsize = a.rsize + (size_t)f * N, *rkey = a.rkey + (size_t)f * N;
  const int wi = t % c.mask_words, ty = t / c.mask_words, y = ty * TH + j;
  unsigned long long bits = 0ull;
  if (t < tiles_per_frame && y < c.H && a.tilehdr[((size_t)f * tiles_per_frame + t) * 2] != 0)   // (0: nothing dynamic in the tile)
    bits = a.lroot[((size_t)f * c.H + y) * c.mask_words + wi];
  while (bits) {
    const int b = __ffsll(bits) - 1;
    bits &= bits - 1ull;
    const int p = y * c.W + wi * 64 + b;
    const int r = uf_find(parent, p);
    if (!MOD_CHECK(a, r >= 0 && (size_t)r < N, 2)) continue;
    if (r == p) {
      const int slot = atomicAdd(&a.counters[f * 8 + 0], 1);
      if (MOD_CHECK(a, slot >= 0 && (size_t)slot < N, 3)) st_agent(&a.rootlist[(size_t)f * N + slot], p);   // read by the frame's last workgroup
    } else {
      parent[p] = r;   // r is final: no union runs after k_ccl_link
      const int sz = rsize[p], ky = rkey[p];
      // the running sum the add returns is this tile root's place among the component's members: [old, old + sz) of the component's
      // member segment (the final root's own tile pixels hold [0, its count): rsize[r] starts there).  Parked in the tile root's key
      // entry, which nobody reads again as a key — k_final takes it from there instead of reserving slots with an atomic of its own.
      rkey[p] = atomicAdd(&rsize[r], sz);
      if (ky != kKeyNone) atomicMin(&rkey[r], ky);
    }
  }
  // FILTER (small batches): the size filter needs every record of the frame folded — the frame's LAST workgroup to get here runs it
  // (one dependent launch less per call, which is what a small batch is made of; in a large batch the count below — an atomic and
  // two barriers in each of 30 k workgroups, most of which have nothing else to do — costs more than the launch: 0.080 -> 0.101 ms
  // per 512 pairs, so large batches keep the filter as a kernel of its own, k_select).  What it reads of the other
  // workgroups' work went to memory past the XCD's L2 — device-scope atomics (counts, sizes, keys) and device-scope stores (the root
  // list) — and has been acknowledged when the writer's waves pass the barrier below (it drains their memory counters); the last
  // workgroup reads it with device-scope loads.  No fence: a device-scope release is a write-back of the XCD's whole L2, and one per
  // workgroup made this kernel 20x slower (0.017 -> 0.36 ms per 64 pairs, measured).
  if (!FILTER) return;
  __shared__ int s_last;
  __syncthreads();
  if (threadIdx.x == 0) s_last = (atomicAdd(&a.counters[f * 8 + 2], 1) == (int)gridDim.x - 1) ? 1 : 0;
  __syncthreads();
  if (!s_last) return;                                 // block-uniform
  if (threadIdx.x == 0) a.counters[f * 8 + 2] = 0;     // (k_median_ties counts its workgroups in frame 0's slot)
  select_frame(c, a, tmp, f, (int)threadIdx.x);
}

// removeSmallClusters + the reference's numbering as a kernel of its own (large batches): one workgroup per frame
__global__ __launch_bounds__(256) void k_select(DevCam c, ClArgs a, ClusterInfo *tmp) { select_frame(c, a, tmp, (int)blockIdx.x, (int)threadIdx.x); }

// ---------------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per frame (the frame's last one in k_ccl_merge): size filter, ordering by first_edge_key, new labels,
// member-segment offsets, object shells.  What other workgroups of the same kernel wrote (root list, records) is read past the
// caches of this CU / XCD (ld_agent: device-scope loads).
__device__ void select_frame(const DevCam &c, const ClArgs &a, ClusterInfo *tmp, int f, int tid) {
  __shared__ int s_n;
  if (tid == 0) s_n = 0;
  __syncthreads();
  const size_t N = (size_t)c.W * c.H;
  const int nroots = ld_agent(&a.counters[f * 8 + 0]);
  int *rsize = a.rsize + (size_t)f * N, *rkey = a.rkey + (size_t)f * N;
  const int *roots = a.rootlist + (size_t)f * N;
  ClusterInfo *T = tmp + (size_t)f * a.max_objects;
  ClusterInfo *C = a.clusters + (size_t)f * a.max_objects;
  // removeSmallClusters: `cluster_size.at(i) < cluster_size_th_` drops the component (clusterer_nodelet.cpp:374);
  // a component without any edge never got a label in the reference (key == none)
  for (int i = tid; i < nroots; i += 256) {
    const int r = ld_agent(roots + i);
    if (!MOD_CHECK(a, r >= 0 && (size_t)r < N, 4)) continue;
    const int size = ld_agent(rsize + r), key = ld_agent(rkey + r);
    bool keep = (key != kKeyNone) && (size >= c.cluster_size);
    if (keep) {
      const int slot = atomicAdd(&s_n, 1);
      // capacity: mod_set_params admits a cluster_size only if max_width * max_height / cluster_size clusters fit max_objects,
      // so this cannot overflow (asserted in the checked build, code 15)
      if (MOD_CHECK(a, slot < a.max_objects, 15) && slot < a.max_objects) { T[slot].comp = r; T[slot].size = size; T[slot].offset = key; }
      else keep = false;
    }
    if (!keep) rkey[r] = -1;
  }
  __syncthreads();
  const int K = min(s_n, a.max_objects);
  // rank by key (distinct pixel indices) = the reference's increasing-root-id renumbering (:381)
  for (int s = tid; s < K; s += 256) {
    const int key = T[s].offset;
    int rank = 0;
    for (int t = 0; t < K; t++) rank += (T[t].offset < key) ? 1 : 0;
    ClusterInfo ci;
    ci.comp = T[s].comp; ci.size = T[s].size; ci.offset = 0; ci.med_pix = -1; ci.med_bits = 0; ci.ambiguous = 0;
    ci.pad[0] = ci.pad[1] = 0;
    C[rank] = ci;
    rkey[ci.comp] = rank;                               // k_final looks the new label up here
    ClusterBox bx;
    for (int d = 0; d < 8; d++) bx.w[d] = 0xffffffffu;
    a.cbox[(size_t)f * a.max_objects + rank] = bx;      // k_final folds the members' x, y, z into it
  }
  __syncthreads();
  if (tid == 0) {
    int off = 0;
    // the segment's start also goes to the final root's size entry (its size lives on in C[k].size): k_final's tile roots read
    // (new label, segment start) of their final root in one round trip
    for (int k = 0; k < K; k++) { C[k].offset = off; rsize[C[k].comp] = off; off += C[k].size; }
    a.counters[f * 8 + 1] = K;
    if (a.n_clusters) a.n_clusters[f] = K;
    // the launch's cluster list for k_median (order irrelevant): workgroups are then launched per cluster, not per frame
    const int base = K ? atomicAdd(&a.counters[6], K) : 0;
    for (int k = 0; k < K; k++) a.worklist[base + k] = (uint32_t)f * (uint32_t)a.max_objects + (uint32_t)k;
  }
  // object shells; bounding_box / center / velocity are filled by k_median once k_final has folded the members' coordinates
  ModObject *O = (ModObject *)a.objects + (size_t)f * a.max_objects;
  for (int k = tid; k < K; k += 256) {
    ModObject o;
    o.id = k; o.n_points = C[k].size;
    for (int d = 0; d < 3; d++) { o.bounding_box[d] = 0.0; o.center[d] = 0.0; o.velocity[d] = 0.0; }
    o.orientation[0] = 0.0; o.orientation[1] = 0.0; o.orientation[2] = 0.0; o.orientation[3] = 1.0;
    O[k] = o;
  }
}

constexpr int kFusedFilterFrames = 16;   // batches up to this size run the size filter inside k_ccl_merge (see there)
}  // namespace

void launch_tile_flags(const DevCam &c, const ClArgs &a, int frames, hipStream_t s) {
  const dim3 g = tile_grid(c, frames);
  const int tiles = (int)(g.x * g.y), total = tiles * frames;
  hipLaunchKernelGGL(k_tile_flags<kTileH>, dim3((total + 255) / 256), dim3(256), 0, s, c, a, (int)g.x, tiles, total);
}
void launch_ccl_link(const DevCam &c, const ClArgs &a, int frames, hipStream_t s) {
  const dim3 g = tile_grid(c, frames);
  const int tiles = (int)(g.x * g.y), per_block = kLinkTiles;
  hipLaunchKernelGGL(k_ccl_link, dim3((tiles + per_block - 1) / per_block, frames), dim3(256), 0, s, c, a, tiles);
}
void launch_ccl_merge(const DevCam &c, const ClArgs &a, int frames, ClusterInfo *rank_scratch, hipStream_t s) {
  const dim3 g = tile_grid(c, frames);
  const int tiles = (int)(g.x * g.y), per_block = 4 * (64 / kTileH);
  if (frames <= kFusedFilterFrames) hipLaunchKernelGGL((k_ccl_merge<kTileH, true>), dim3((tiles + per_block - 1) / per_block, frames), dim3(256), 0, s, c, a, tiles, rank_scratch);
  else {
    hipLaunchKernelGGL((k_ccl_merge<kTileH, false>), dim3((tiles + per_block - 1) / per_block, frames), dim3(256), 0, s, c, a, tiles, rank_scratch);
    hipLaunchKernelGGL(k_select, dim3(frames), dim3(256), 0, s, c, a, rank_scratch);
  }
}
