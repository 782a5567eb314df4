// cluster_final.hip — MOD_STAGE_FINAL: k_final, labels plane and member lists; k_cluster_members, the lists in the reference's order
// for the caller (overview: cluster_common.h)
#include "cluster_common.h"
#include <algorithm>
#pragma clang fp contract(off)
namespace {

// Final labels + member compaction, one workgroup per tile.  labels[p] = new label of p's component or -1 (the whole
// plane is written here, 4 B/px, when the caller asks for it: the reference renders its cluster image only for subscribers,
// clusterer_nodelet.cpp:235-236).  A pixel's parent entry names its tile root, so the few tile roots resolve their final
// root's new label once (into LDS) and every pixel just looks it up; members of surviving clusters are counted per tile
// root in LDS, one cursor atomic per (tile root) reserves their slots, then (||v|| bits, pixel) records are appended.
// XY_FROM_Z: the planes come from the fused scene-flow kernel of the same call (mod_process_dev), where every valid pixel has
// x = F32(ray_x(column) * (double)z), y = F32(ray_y(row) * (double)z) (sceneflow.hip sf_stage1, getPoint3D): the members' x, y are
// then recomputed from z and the ray tables — the same two operations, the same bits — instead of being read back (8 B/px of the
// active tiles less for this HBM-bound kernel).  Caller-supplied clouds (mod_cluster_dev) are read as they are.
#ifndef FINAL_PLAIN_LABELS   // streaming stores for the label plane: nobody on the GPU reads it (k_final 1.03 -> 0.97 ms per 512 pairs)
#define FINAL_ST(p, v) __builtin_nontemporal_store((int)(v), (p))
#else
#define FINAL_ST(p, v) (*(p) = (v))
#endif
constexpr int kFinalEarly = 32;   // dynamic pixels in a wave's rows from which its velocity / depth rows are fetched with the first round trip
template <int TH, int NW, bool XY_FROM_Z>
__global__ __launch_bounds__(NW * 64) void k_final(DevCam c, ClArgs a) {
  constexpr int RPW = TH / NW;
  __shared__ int nlmap[TH * 64];                     // per tile-root cell: new label of its component (or -1)
  __shared__ int lcount[TH * 64];                    // per tile-root cell: member count, then base slot of its members
  const int wi = blockIdx.x, f = blockIdx.z, lane = threadIdx.x, w = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const size_t tidx = (size_t)f * gridDim.y * gridDim.x + (size_t)blockIdx.y * gridDim.x + wi;
  const size_t N = (size_t)c.W * c.H;
  const size_t fN = (size_t)f * N;
  const int x0 = wi * 64, y0 = blockIdx.y * TH, r0 = w * RPW, x = x0 + lane;
  if (a.tilehdr[tidx * 2] == 0) {                    // nothing dynamic in the tile
    if (a.labels) {
#pragma unroll
      for (int j = 0; j < RPW; j++) { const int y = y0 + r0 + j; if (y < c.H && x < c.W) FINAL_ST(&a.labels[fN + (size_t)y * c.W + x], -1); }
    }
    return;
  }
  // ---- all row-independent HBM reads up front (clamped addresses, results of non-dynamic lanes are ignored) ----
  const int xc = min(x, c.W - 1);
  uint64_t mw[RPW], rw[RPW];
  int par[RPW];
#pragma unroll
  for (int j = 0; j < RPW; j++) {
    const int y = y0 + r0 + j, yc = min(y, c.H - 1);
    const size_t wo = ((size_t)f * c.H + yc) * c.mask_words + wi;
    mw[j] = (y < c.H) ? a.mask[wo] : 0ull;
    rw[j] = (y < c.H) ? a.lroot[wo] : 0ull;
    par[j] = a.parent[fN + (size_t)yc * c.W + xc];
  }
  // ---- tile roots: their parent entry names the final root (k_ccl_merge), whose entries hold the new label (rkey, k_select) and the
  // start of the cluster's member segment (rsize, k_select); the tile root's own key entry holds its place inside that segment
  // (k_ccl_merge).  ONE round trip, three independent gathers; the cell's counter starts at the first slot of its members, so that
  // the LDS atomics below hand out absolute slots — no global cursor atomic, no second barrier (round 4: four dependent round
  // trips and three barriers per tile) ----
#pragma unroll
  for (int j = 0; j < RPW; j++) {
    if ((rw[j] >> lane) & 1ull) {
      const int cell = (r0 + j) * 64 + lane;
      const int p = (y0 + r0 + j) * c.W + x;
      int lab = -1, first = 0;
      if (MOD_CHECK(a, par[j] >= 0 && (size_t)par[j] < N, 5)) {
        const int fr = par[j];
        lab = a.rkey[fN + fr];
        const int seg = a.rsize[fN + fr];
        const int own = a.rkey[fN + p];
        first = seg + (fr == p ? 0 : own);
      }
      nlmap[cell] = lab;
      lcount[cell] = first;
    }
  }
  // velocity (for the ||v|| bits) and depth (for the bounding box) of the wave's rows: tiles with this many dynamic pixels nearly
  // always hold members of a surviving cluster — their loads leave with the gathers above instead of after them
  float vx[RPW], vy[RPW], vz[RPW], px[RPW], py[RPW], pz[RPW];
  int ndyn = 0;
#pragma unroll
  for (int j = 0; j < RPW; j++) ndyn += __popcll((unsigned long long)mw[j]);
  const bool early = ndyn >= kFinalEarly;                            // wave-uniform
  auto load_members = [&]() {
#pragma unroll
    for (int j = 0; j < RPW; j++) {
      const size_t gp = fN + (size_t)min(y0 + r0 + j, c.H - 1) * c.W + xc;
      vx[j] = a.vx[gp]; vy[j] = a.vy[gp]; vz[j] = a.vz[gp];
      pz[j] = a.z[gp];
      if (!XY_FROM_Z) { px[j] = a.x[gp]; py[j] = a.y[gp]; }
    }
  };
  if (early) load_members();
  lds_barrier();
  // every wave of the tile has read the header: the tile stage's last reader leaves it zero for the next call (the scene-flow
  // epilogue / k_tile_flags only ever SET headers, so nobody has to clear 0.9 M of them per 512 pairs beforehand)
  if (w == 0 && lane == 0) a.tilehdr[tidx * 2] = 0;
  // ---- labels ----
  const float invW = 1.0f / (float)c.W;
  const int tile0 = y0 * c.W + x0;
  int nl[RPW], cell[RPW], slot[RPW];
  bool any_member = false;
#pragma unroll
  for (int j = 0; j < RPW; j++) {
    const int y = y0 + r0 + j;
    const bool dyn = (mw[j] >> lane) & 1ull;
    // tile-local coordinates of the tile root: d = ly * W + lx with lx < 64, ly < TH <= 16, i.e. d < 16 W + 64.  For such d the F32
    // product (d + 0.5) * (1 / W) truncates to ly exactly for every W an image can have: tests/test_row_model.py checks every W up to
    // 70000; the formula first fails near W = 4.19 M.  It is NOT exact for whole-image pixel indices (k_median_ties divides)
    const int d = par[j] - tile0;
    const int ly = (int)(((float)d + 0.5f) * invW);
    // a tile root's own entry was redirected to the final root (possibly in another tile) by k_ccl_merge: it is its own cell
    const bool isroot = (rw[j] >> lane) & 1ull;
    int cl = !dyn ? 0 : isroot ? ((r0 + j) * 64 + lane) : (ly * 64 + (d - ly * c.W));
    if (!MOD_CHECK(a, cl >= 0 && cl < TH * 64 && (!dyn || isroot || (d >= 0 && d - ly * c.W < 64)), 6)) cl = 0;
    int l = dyn ? nlmap[cl] : -1;
    if (!MOD_CHECK(a, l >= -1 && l < a.max_objects, 7)) l = -1;
    nl[j] = l; cell[j] = cl; slot[j] = 0;
    if (a.labels && y < c.H && x < c.W) FINAL_ST(&a.labels[fN + (size_t)y * c.W + x], l);
    any_member = any_member || (__ballot(l >= 0) != 0);
  }
  if (any_member) {                                  // wave-uniform
    if (!early) load_members();
    // ---- members: slots handed out per tile root in LDS ----
#pragma unroll
    for (int j = 0; j < RPW; j++) {
      const int l = nl[j], cl = cell[j];
      const uint64_t mb = __ballot(l >= 0);
      if (mb == 0) continue;                         // wave-uniform
      // lanes that share the first member's tile root reserve their slots with one LDS atomic; stragglers use their own
      const int lead = __ffsll((unsigned long long)mb) - 1;
      const int c0 = __builtin_amdgcn_readlane(cl, lead);
      const bool grp = l >= 0 && cl == c0;
      const uint64_t gb = __ballot(grp);
      int base = 0;
      if (lane == lead) base = atomicAdd(&lcount[c0], __popcll((unsigned long long)gb));
      base = __builtin_amdgcn_readlane(base, lead);
      if (grp) slot[j] = base + __popcll((unsigned long long)(gb & ((1ull << lane) - 1ull)));
      else if (l >= 0) slot[j] = atomicAdd(&lcount[cl], 1);
    }
    if (XY_FROM_Z) {
      const double rx = c.rayx[xc];
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        const double zd = (double)pz[j];
        px[j] = (float)(rx * zd);
        py[j] = (float)(c.rayy[min(y0 + r0 + j, c.H - 1)] * zd);
      }
    }
    uint32_t nb[RPW];                                // ||v|| bit patterns (norms are >= 0 and never NaN: the patterns order like the values)
#pragma unroll
    for (int j = 0; j < RPW; j++) nb[j] = __float_as_uint(norm3_f32(vx[j], vy[j], vz[j]));
#pragma unroll
    for (int j = 0; j < RPW; j++) {
      if (nl[j] >= 0) {
        if (MOD_CHECK(a, slot[j] >= 0 && (size_t)slot[j] < N, 8)) {
          a.mbits[fN + slot[j]] = nb[j];
          a.mpix[fN + slot[j]] = (uint32_t)((y0 + r0 + j) * c.W + x);
        }
      }
    }
    // bounding box of the cluster (pcl::getMinMax3D in cluster2MovingObject, clusterer_nodelet.cpp:151-152): the wave's members
    // are folded per cluster label with DPP reductions, one set of atomics per (wave, cluster) — nearly always one cluster
    int pend[RPW];
#pragma unroll
    for (int j = 0; j < RPW; j++) pend[j] = nl[j];
    for (;;) {
      int mine = -1;
#pragma unroll
      for (int j = 0; j < RPW; j++) mine = pend[j] >= 0 ? pend[j] : mine;
      const uint64_t b = __ballot(mine >= 0);
      if (b == 0) break;                               // wave-uniform
      const int L = __builtin_amdgcn_readlane(mine, __ffsll((unsigned long long)b) - 1);
      uint32_t mn0 = 0xffffffffu, mn1 = 0xffffffffu, mn2 = 0xffffffffu, mx0 = 0u, mx1 = 0u, mx2 = 0u, mn3 = 0xffffffffu, mx3 = 0u;
#pragma unroll
      for (int j = 0; j < RPW; j++) {
        if (pend[j] == L) {
          const uint32_t ox = f2ord(px[j]), oy = f2ord(py[j]), oz = f2ord(pz[j]);
          mn0 = min(mn0, ox); mx0 = max(mx0, ox); mn1 = min(mn1, oy); mx1 = max(mx1, oy); mn2 = min(mn2, oz); mx2 = max(mx2, oz);
          mn3 = min(mn3, nb[j]); mx3 = max(mx3, nb[j]);
          pend[j] = -1;
        }
      }
      mn0 = wave_min_u32(mn0); mn1 = wave_min_u32(mn1); mn2 = wave_min_u32(mn2); mn3 = wave_min_u32(mn3);
      mx0 = wave_max_u32(mx0); mx1 = wave_max_u32(mx1); mx2 = wave_max_u32(mx2); mx3 = wave_max_u32(mx3);
      // ONE atomic instruction per (wave, cluster): lanes 0..7 each fold one word (an atomic instruction costs the CU's memory
      // pipeline the same whether one lane or eight are active); the maxima are kept complemented so that all eight are minima.
      // Words 6, 7 (round 5): smallest / largest ||v|| of the members — k_median starts its selection from that range instead of
      // scanning the members for it
      uint32_t v = ~mx3;
      v = lane == 0 ? mn0 : v; v = lane == 1 ? mn1 : v; v = lane == 2 ? mn2 : v; v = lane == 3 ? ~mx0 : v; v = lane == 4 ? ~mx1 : v;
      v = lane == 5 ? ~mx2 : v; v = lane == 6 ? mn3 : v;
      if (lane < 8) atomicMin(&a.cbox[(size_t)f * a.max_objects + L].w[lane], v);
    }
  }
}

// ---- k_cluster_members, opt-in (mod_set_cluster_members): the clusters' member lists in the reference's order (pcl::IndicesClusters of
// clusterMap2IndicesCluster, clusterer_nodelet.cpp:97-117) ----
// k_final has compacted every surviving cluster's pixels into mpix[offset .. offset + size), in tile order; k_select laid the
// segments out in label order (ClusterInfo.offset is the exclusive prefix of the sizes), so offsets[k] IS ClusterInfo.offset and
// the ordered segment goes to indices + offset — same place, other array.  The kernel runs between k_final and k_median:
// k_median_ties turns mpix / mbits of a tied cluster into swap lists.
//
// Work: the launch's work list, static stride (all eight counter words of frame 0 are taken: no cursor).  A cluster is a chain of
// three passes over its list (box, pass A, pass B: cluster_common.h, member layout), each a memory round trip per NT * 8 members, with the LDS mask
// clear and the prefix in between.
//   * clusters of more than kMemWaveMax members: the whole workgroup, kMemCells cells per run — one round trip per pass up to
//     8192 members, ~10 workgroup barriers a cluster;
//   * the others: ONE WAVE each, sixteen clusters per workgroup side by side, kMemWaveCells = kMemCells / 16 cells of the same LDS
//     arrays per wave and no barrier at all.  A wave needs ceil(size / 512) round trips a pass where the workgroup needs one, so at
//     kMemWaveMax = 1024 members a wave's chain is at most twice as long as the workgroup's would be — and sixteen of them run in
//     the time, with none of the 1024-thread barriers that 15 idle waves would sit in.  Street-scene clusters are mostly a few
//     hundred members in a box of 20 - 60 columns x 1 - 2 row cells, far inside 512 cells; a sparse small cluster whose box has more
//     cells (a one-row stripe 600 px wide) takes further runs like any other box.  Reasoned from the code, not measured.
// The large clusters go first: theirs is the longest chain of the launch.
constexpr int kMemThreads = 1024, kMemCells = 8192, kMemWaveCells = kMemCells / (kMemThreads / 64), kMemWaveMax = 1024;

template <int NT, int CELLS, bool XY_FROM_Z, bool POINTS>
__device__ __forceinline__ void members_of(const DevCam &c, const ClArgs &a, const ClusterMemberOut &m, uint32_t item, int size, int off,
                                           uint64_t *cmask, uint32_t *cstart, int *s_box, int *s_sum, int tid) {
  const size_t N = (size_t)c.W * c.H;
  const int f = (int)(item / (uint32_t)a.max_objects);
  const size_t fN = (size_t)f * N;
  const uint32_t *pix = a.mpix + fN + off;
  int32_t *dst = m.indices + fN + off;
  float *pts = POINTS ? m.points + (fN + off) * 3 : nullptr;
  const float *px = XY_FROM_Z ? nullptr : a.x + fN, *py = XY_FROM_Z ? nullptr : a.y + fN, *pz = a.z + fN;   // (objects-only calls pass no x, y)
  const MemberBox bx = member_box<NT>(pix, size, (uint32_t)c.W, s_box, tid);
  [[maybe_unused]] const int placed = member_layout<NT, CELLS>(
      pix, size, (uint32_t)c.W, bx, cmask, cstart, s_sum, tid, [](int) { return 0u; },
      [&](int slot, uint32_t p, uint32_t, uint32_t x, uint32_t y) {
        if (!MOD_CHECK(a, slot >= 0 && slot < size && (size_t)p < N, 11)) return;
        dst[slot] = (int32_t)p;
        if (POINTS) {
          // x, y, z as the planes hold them; in a fused call x, y are the scene-flow kernel's two operations on z again (k_final)
          const float z = pz[p];
          float X, Y;
          if (XY_FROM_Z) { const double zd = (double)z; X = (float)(c.rayx[x] * zd); Y = (float)(c.rayy[y] * zd); }
          else { X = px[p]; Y = py[p]; }
          float *o = pts + (size_t)slot * 3;
          o[0] = X; o[1] = Y; o[2] = z;
        }
      },
      [](int) {});
  (void)MOD_CHECK(a, placed == size, 14);
}

template <bool XY_FROM_Z, bool POINTS>
__global__ __launch_bounds__(kMemThreads) void k_cluster_members(DevCam c, ClArgs a, ClusterMemberOut m, int frames) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t N = (size_t)c.W * c.H;
  const int nwork = a.counters[6];
  __shared__ uint64_t lraw[kMemCells + kMemCells / 2];               // 96 KB: the cell masks, then the cells' first slots
  uint64_t *cmask = &lraw[0];
  uint32_t *cstart = reinterpret_cast<uint32_t *>(&lraw[kMemCells]);
  __shared__ int s_box[4], s_sum[kMemThreads / 64 + 1];
  // ---- offsets: ClusterInfo.offset of the K clusters, the total from K on ----
  for (int f = blockIdx.x; f < frames; f += gridDim.x) {
    const ClusterInfo *C = a.clusters + (size_t)f * a.max_objects;
    const int K = min(a.counters[f * kClusterCounters + 1], a.max_objects);
    const int total = K > 0 ? C[K - 1].offset + C[K - 1].size : 0;
    int32_t *o = m.offsets + (size_t)f * (a.max_objects + 1);
    for (int k = tid; k <= a.max_objects; k += kMemThreads) o[k] = k < K ? C[k].offset : total;
  }
  // every segment is checked against the frame before anything is written through it
  auto segment = [&](uint32_t item, int &size, int &off) {
    const ClusterInfo *ci = a.clusters + item;       // item = frame * max_objects + cluster
    size = ci->size; off = ci->offset;
    return size >= 1 && off >= 0 && (size_t)off + (size_t)size <= N;
  };
  // ---- the large clusters: one per turn of the workgroup ----
  for (int wi = blockIdx.x; wi < nwork; wi += gridDim.x) {
    const uint32_t item = a.worklist[wi];
    int size, off;
    if (!segment(item, size, off) || size <= kMemWaveMax) continue;  // block-uniform
    members_of<kMemThreads, kMemCells, XY_FROM_Z, POINTS>(c, a, m, item, size, off, cmask, cstart, s_box, s_sum, tid);
  }
  __syncthreads();                                   // the LDS arrays change hands
  // ---- the small ones: one per turn of a wave, in the wave's sixteenth of the arrays ----
  for (int wi = blockIdx.x * (kMemThreads / 64) + wv; wi < nwork; wi += gridDim.x * (kMemThreads / 64)) {
    const uint32_t item = a.worklist[wi];
    int size, off;
    if (!segment(item, size, off) || size > kMemWaveMax) continue;   // wave-uniform
    members_of<64, kMemWaveCells, XY_FROM_Z, POINTS>(c, a, m, item, size, off, cmask + wv * kMemWaveCells, cstart + wv * kMemWaveCells, nullptr,
                                                     nullptr, lane);
  }
}
}  // namespace

void launch_final(const DevCam &c, const ClArgs &a, int frames, hipStream_t s) {
  // two waves per tile (8 rows each): 1 / 2 / 4 / 8 waves measured 1.419 (176 VGPRs: 2 waves per SIMD) / 0.965 / 1.001 / 1.460 ms per 512
  // pairs (in-process A/B)
  constexpr int kFinalWaves = 2;
  if (a.xy_from_z) hipLaunchKernelGGL((k_final<kTileH, kFinalWaves, true>), tile_grid(c, frames), dim3(64, kFinalWaves, 1), 0, s, c, a);
  else hipLaunchKernelGGL((k_final<kTileH, kFinalWaves, false>), tile_grid(c, frames), dim3(64, kFinalWaves, 1), 0, s, c, a);
}

void launch_cluster_members(const DevCam &c, const ClArgs &a, const ClusterMemberOut &m, int frames, hipStream_t s) {
  // a workgroup takes 96 KB of LDS: one per CU at most, fewer for small batches (a frame has tens of clusters, sixteen small ones
  // go side by side in a workgroup)
  const dim3 grid(std::min(256, frames * 4)), block(kMemThreads);
  const bool pts = m.points != nullptr;
  if (a.xy_from_z) {
    if (pts) hipLaunchKernelGGL((k_cluster_members<true, true>), grid, block, 0, s, c, a, m, frames);
    else hipLaunchKernelGGL((k_cluster_members<true, false>), grid, block, 0, s, c, a, m, frames);
  } else {
    if (pts) hipLaunchKernelGGL((k_cluster_members<false, true>), grid, block, 0, s, c, a, m, frames);
    else hipLaunchKernelGGL((k_cluster_members<false, false>), grid, block, 0, s, c, a, m, frames);
  }
}
