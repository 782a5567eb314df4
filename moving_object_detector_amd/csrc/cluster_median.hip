// cluster_median.hip — MOD_STAGE_MEDIAN: k_median, k_box_nan, k_median_ties, the objects (overview: cluster_common.h)
#include "cluster_common.h"
#include <algorithm>
#include <type_traits>
#include "introsort_emul.h"
#pragma clang fp contract(off)
namespace {

// Median-velocity member per cluster: the element at position size/2 of the members sorted by ||v|| descending
// (clusterer_nodelet.cpp:168-174).  All norms are >= 0 and never NaN, so their F32 bit patterns order like the values:
// a range-adaptive 2048-bin histogram over (bits - min) >> shift isolates the bin that holds rank size/2, its members
// (up to kMedDirect of them) are ranked exactly in LDS; degenerate distributions narrow the range and repeat.
// Round 5 — a cluster is a chain of barriers and memory round trips, so what counts is how many clusters are in flight; rounds 1-4
// held the norms in registers (32 per thread: 125 VGPRs with spills, ONE workgroup per CU, 25 us per cluster).  Now:
//   * the norms are STREAMED from L2 in every pass (eight loads in flight per thread; a cluster is some 90 KB that its own workgroup
//     read a few microseconds before): under 32 VGPRs, two 1024-thread workgroups per CU;
//   * the members' norm range comes with the cluster's box record (k_final folds it with the same atomic instruction): no pass
//     over the members for it;
//   * the bin that holds the rank is found by all 16 waves (two bins per thread, one wave scan + 16 wave totals), not by wave 0
//     walking 2048 bins; the bins are zeroed again as they are read;
//   * a bin with up to kMedDirect members ends the rounds: they are compacted with their list positions, ranked directly, and the
//     tie-break (smallest column-major index, differing vectors flagged) runs on that list — two passes over the norms for most
//     clusters;
//   * the rare paths left the kernel: NaN coordinates of a caller's cloud are k_box_nan's, the tie replay k_median_ties'.
constexpr int kMedThreads = 1024, kMedBins = 2048, kMedDirect = 256, kMedCand = kMedBins / 2;

// box of a cluster record -> bounding_box / center of the object (cluster2MovingObject, clusterer_nodelet.cpp:151-161): F32 max - min
// and (min + max) / 2, widened to F64 (getMinMax3D starts from +-FLT_MAX: members at +inf leave the minimum there, members at -inf the maximum)
__device__ __forceinline__ void box_to_object(const ClusterBox &rec, ModObject *o) {
  for (int d = 0; d < 3; d++) {
    const float mn = fminf(ord2f(rec.w[d]), 3.402823466e38f), mx = fmaxf(ord2f(~rec.w[3 + d]), -3.402823466e38f);
    o->bounding_box[d] = (double)(mx - mn);
    o->center[d] = (double)((mn + mx) / 2.0f);
  }
}

// f(bits, list position) for every member: kMedFlight coalesced loads in flight per thread — unconditional, at clamped positions
// (a predicated load is an exec-masked region of its own: the loads would leave one by one), 0xffffffff (not a norm) past the end
constexpr int kMedFlight = 10;   // (12: the first spills at 64 VGPRs)
template <class F> __device__ __forceinline__ void med_stream(const uint32_t *sbits, int size, int tid, F f) {
  for (int i0 = tid; i0 < size; i0 += kMedThreads * kMedFlight) {
    uint32_t b[kMedFlight];
#pragma unroll
    for (int u = 0; u < kMedFlight; u++) b[u] = *(const uint32_t *)((const char *)sbits + 4u * (uint32_t)min(i0 + u * kMedThreads, size - 1));
#pragma unroll
    for (int u = 0; u < kMedFlight; u++) { const int i = i0 + u * kMedThreads; f(i < size ? b[u] : 0xffffffffu, i); }
  }
}

__global__ __launch_bounds__(kMedThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_median(DevCam c, ClArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t N = (size_t)c.W * c.H;
  const int nwork = a.counters[6];
  __shared__ uint32_t hist[kMedBins];                // the bins; between the rounds and the tie-break: candidates (bits | list position)
  __shared__ uint32_t s_wsum[kMedThreads / 64];
  __shared__ uint32_t s_bin, s_rem, s_inbin, s_cnt, s_val, s_ties;
  __shared__ unsigned long long s_best;
  __shared__ int s_amb, s_item;
#ifdef MOD_PHASE_COUNTERS
  const unsigned long long bt0 = wall_clock64();
  if (tid == 0) atomicMin(&a.dbg[42], bt0);
  struct BlockEnd { unsigned long long *d; unsigned long long t0; int tid; bool busy;
    __device__ ~BlockEnd() { const unsigned long long t1 = wall_clock64(); if (tid == 0) { atomicMax(&d[43], t1); if (busy) { atomicAdd(&d[40], t1 - t0); atomicAdd(&d[41], 1ull); } } } };
  BlockEnd be{a.dbg, bt0, tid, (int)blockIdx.x < nwork};
#endif
  hist[tid] = 0u; hist[tid + kMedThreads] = 0u;      // every phase leaves the bins zeroed again
  for (;;) {
    // clusters differ 10x in size: workgroups take the next one when they are free (counters[5]) instead of a fixed share
    if (tid == 0) { s_item = atomicAdd(&a.counters[5], 1); s_cnt = 0u; s_best = ~0ull; s_amb = 0; }
    __syncthreads();
    // (the work item is the same in every lane, but arrives through LDS in a vector register: as a scalar, everything derived from
    // it — frame, cluster record, the list's base addresses — stays on the scalar unit and the member loads are `base + lane offset`)
    const int wi = __builtin_amdgcn_readfirstlane(s_item);
    if (wi >= nwork) break;                          // block-uniform; every workgroup gets here
    const uint32_t item = a.worklist[wi];
    const int f = (int)(item / (uint32_t)a.max_objects), k = (int)(item % (uint32_t)a.max_objects);
    ClusterInfo *ci = a.clusters + (size_t)f * a.max_objects + k;
    const int ci_size = __builtin_amdgcn_readfirstlane(ci->size), ci_off = __builtin_amdgcn_readfirstlane(ci->offset);
    const int size = MOD_CHECK(a, ci_size >= 1 && ci_off >= 0 && (size_t)ci_off + (size_t)ci_size <= N, 9) ? ci_size : 0;
    if (size == 0) continue;                                        // (checked build only; block-uniform)
    const uint32_t *sbits = a.mbits + (size_t)f * N + ci_off;       // ||v|| bits of the members ...
    const uint32_t *spix = a.mpix + (size_t)f * N + ci_off;         // ... and their pixel indices
    const ClusterBox *box = a.cbox + (size_t)f * a.max_objects + k; // complete: k_final has finished
    PHASE_CLOCK
    uint32_t lo = box->w[6], hi = ~box->w[7], rem = (uint32_t)(size / 2);   // the members' norm range (k_final)
    if (!MOD_CHECK(a, lo <= hi, 9)) { lo = 0u; hi = 0x7f800000u; }
    bool exact = false;                      // the live range is a single value: every member of it ties
    uint32_t val = 0, nties = 0;
    PHASE_STAMP(26)
    for (int round = 0; round < 8; round++) {        // one or two rounds in practice; the bound only guards against corrupt input
      const uint32_t range = hi - lo;
      const int shift = range < (uint32_t)kMedBins ? 0 : (32 - __clz((int)range) - 11);   // (range >> shift) < 2048
      // ---- histogram of the live range (the bins are zero: start of the kernel / the scan of the round before) ----
      med_stream(sbits, size, tid, [&](uint32_t b, int) { if (b >= lo && b <= hi) atomicAdd(&hist[(b - lo) >> shift], 1u); });
      __syncthreads();
      PHASE_STAMP(30 + (round > 0 ? 2 : 0))
      // ---- bin that holds descending rank `rem`: thread t owns bins 2047 - 2t and 2046 - 2t (walking down from the top) ----
      const int b0 = kMedBins - 1 - 2 * tid;
      const uint32_t h0 = hist[b0], h1 = hist[b0 - 1];
      hist[b0] = 0u; hist[b0 - 1] = 0u;
      uint32_t incl = h0 + h1;                       // inclusive prefix over the wave's lanes
      for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
      if (lane == 63) s_wsum[wv] = incl;
      __syncthreads();
      uint32_t before = 0;                           // members in the waves above this one
      for (int w2 = 0; w2 < kMedThreads / 64; w2++) before += (w2 < wv) ? s_wsum[w2] : 0u;
      const uint32_t upto = before + incl, excl = upto - (h0 + h1);
      if (rem >= excl && rem < upto) {               // exactly one thread
        const bool first = rem - excl < h0;
        s_bin = (uint32_t)(first ? b0 : b0 - 1); s_rem = first ? rem - excl : rem - excl - h0; s_inbin = first ? h0 : h1;
      }
      __syncthreads();
      const uint32_t bin = s_bin, inbin = s_inbin;
      rem = s_rem;
      const uint32_t nlo = lo + (bin << shift);
      const uint32_t nhi = shift ? (nlo + ((1u << shift) - 1u)) : nlo;
      lo = nlo; hi = nhi < hi ? nhi : hi;
      PHASE_STAMP(31 + (round > 0 ? 2 : 0))
      if (shift == 0) { exact = true; val = lo; nties = inbin; break; }
      if (inbin <= (uint32_t)kMedDirect) break;                     // rank the survivors directly
    }
    PHASE_STAMP(27)
    const float *pvx = a.vx + (size_t)f * N, *pvy = a.vy + (size_t)f * N, *pvz = a.vz + (size_t)f * N;
    uint32_t best, bvx, bvy, bvz;
    // canonical pick among the members of norm `val`: the smallest column-major index (the member list is in tile order)
    auto offer = [&](uint32_t p) {
      const uint32_t px = p % (uint32_t)c.W, py = p / (uint32_t)c.W;
      atomicMin(&s_best, ((unsigned long long)(px * (uint32_t)c.H + py) << 32) | p);
    };
    auto settle = [&]() {                            // after a barrier: the pick and its vector
      best = (uint32_t)(s_best & 0xffffffffull);
      if (s_best == ~0ull) best = spix[0];           // unreachable for consistent input; keeps every access in bounds
      if (!MOD_CHECK(a, s_best != ~0ull && (size_t)best < N, 10)) best = 0;
      bvx = __float_as_uint(pvx[best]); bvy = __float_as_uint(pvy[best]); bvz = __float_as_uint(pvz[best]);
    };
    auto differs = [&](uint32_t p) {
      return p != best && (__float_as_uint(pvx[p]) != bvx || __float_as_uint(pvy[p]) != bvy || __float_as_uint(pvz[p]) != bvz);
    };
    if (!exact) {
      // ---- the (<= kMedDirect) members left in [lo, hi], compacted with their list positions into the (zeroed) bins: exact rank,
      // then the tie-break on the same list ----
      med_stream(sbits, size, tid, [&](uint32_t b, int i) {
        if (b >= lo && b <= hi) { const uint32_t s0 = atomicAdd(&s_cnt, 1u); if (s0 < (uint32_t)kMedCand) { hist[s0] = b; hist[kMedCand + s0] = (uint32_t)i; } }
      });
      __syncthreads();
      PHASE_STAMP(34)
      const int fn = MOD_CHECK(a, s_cnt <= (uint32_t)kMedCand, 9) ? (int)s_cnt : kMedCand;
      uint32_t mine = 0, mypix = 0;
      if (tid < fn) {
        mine = hist[tid];
        uint32_t gt = 0, ge = 0;
        for (int j = 0; j < fn; j++) { const uint32_t o = hist[j]; gt += o > mine; ge += o >= mine; }
        if (gt <= rem && rem < ge) { s_val = mine; s_ties = ge - gt; }  // every member of that value writes the same
      }
      __syncthreads();
      val = s_val; nties = s_ties;
      const bool tied = tid < fn && mine == val;
      if (tied) { mypix = spix[hist[kMedCand + tid]]; offer(mypix); }
      __syncthreads();
      if (tid < fn) { hist[tid] = 0u; hist[kMedCand + tid] = 0u; }   // the bins are a histogram again
      settle();
      if (nties > 1u && tied && differs(mypix)) s_amb = 1;
    } else {
      // ---- a single value fills the bin (quantised inputs: possibly thousands of members): the tie-break streams the list ----
      med_stream(sbits, size, tid, [&](uint32_t b, int i) { if (b == val) offer(spix[i]); });
      __syncthreads();
      settle();
      if (nties > 1u) med_stream(sbits, size, tid, [&](uint32_t b, int i) { if (b == val && differs(spix[i])) s_amb = 1; });
    }
    __syncthreads();
    PHASE_STAMP(28)
    PHASE_STAMP(29)
    if (tid == 0) {
      ci->med_pix = (int)best; ci->med_bits = val; ci->ambiguous = s_amb;
      if (s_amb) a.tielist[atomicAdd(&a.counters[7], 1)] = item;
      ModObject *o = (ModObject *)a.objects + (size_t)f * a.max_objects + k;
      o->velocity[0] = (double)__uint_as_float(bvx); o->velocity[1] = (double)__uint_as_float(bvy); o->velocity[2] = (double)__uint_as_float(bvz);
      box_to_object(*box, o);
    }
    // (the next turn's first barrier orders tid 0's reads of s_amb / s_best with their re-initialisation)
    __syncthreads();
  }
}

// NaN coordinates among a cluster's members — only possible for caller-supplied clouds (mod_cluster_dev / mod_cluster_cloud_host: the
// scene-flow stage never marks a pixel dynamic without finite x, y, z), so the launcher starts this kernel for those calls only.
// pcl::getMinMax3D's dense path folds min_p = min_p.min(pt) in member order (column-major) with SSE semantics "(a < b) ? a : b": a NaN
// replaces the running value and the next point replaces the NaN, i.e. the result is the min / max over the members AFTER the
// last NaN, or NaN when the last member is NaN.  One workgroup walks the launch's clusters; those without a NaN cost three loads.
__global__ __launch_bounds__(kMedThreads) void k_box_nan(DevCam c, ClArgs a) {
  const int tid = threadIdx.x;
  const size_t N = (size_t)c.W * c.H;
  const int nwork = a.counters[6];
  __shared__ uint32_t s_last, s_mn, s_mx, s_n;
  for (int wi = blockIdx.x; wi < nwork; wi += gridDim.x) {
    const uint32_t item = a.worklist[wi];
    const int f = (int)(item / (uint32_t)a.max_objects), k = (int)(item % (uint32_t)a.max_objects);
    const ClusterInfo *ci = a.clusters + (size_t)f * a.max_objects + k;
    const ClusterBox rec = a.cbox[(size_t)f * a.max_objects + k];
    bool anynan = false;
    for (int d = 0; d < 3; d++) anynan = anynan || isnan(ord2f(rec.w[d])) || isnan(ord2f(~rec.w[3 + d]));
    if (!anynan) continue;                           // block-uniform
    const int size = ci->size;
    const uint32_t *spix = a.mpix + (size_t)f * N + ci->offset;
    const float *pl[3] = {a.x + (size_t)f * N, a.y + (size_t)f * N, a.z + (size_t)f * N};
    for (int d = 0; d < 3; d++) {
      __syncthreads();
      if (tid == 0) { s_last = 0u; s_mn = 0xffffffffu; s_mx = 0u; s_n = 0u; }   // last NaN key + 1, min, max, survivors
      __syncthreads();
      for (int i = tid; i < size; i += kMedThreads) {
        const uint32_t p = spix[i];
        if (isnan(pl[d][p])) atomicMax(&s_last, (p % (uint32_t)c.W) * (uint32_t)c.H + p / (uint32_t)c.W + 1u);
      }
      __syncthreads();
      const uint32_t lastnan = s_last;              // column-major key + 1 of the last NaN member, 0 if none
      for (int i = tid; i < size; i += kMedThreads) {
        const uint32_t p = spix[i];
        const uint32_t key1 = (p % (uint32_t)c.W) * (uint32_t)c.H + p / (uint32_t)c.W + 1u;
        if (key1 > lastnan) { const uint32_t o = f2ord(pl[d][p]); atomicMin(&s_mn, o); atomicMax(&s_mx, o); atomicAdd(&s_n, 1u); }
      }
      __syncthreads();
      if (tid == 0) {
        ModObject *o = (ModObject *)a.objects + (size_t)f * a.max_objects + k;
        const float nanv = __uint_as_float(0x7fc00000u);
        float mn = s_n ? ord2f(s_mn) : nanv, mx = s_n ? ord2f(s_mx) : nanv;
        if (lastnan == 0u) { mn = fminf(mn, 3.402823466e38f); mx = fmaxf(mx, -3.402823466e38f); }   // no NaN in this coordinate: the +-FLT_MAX start values hold
        o->bounding_box[d] = (double)(mx - mn);
        o->center[d] = (double)((mn + mx) / 2.0f);
      }
    }
  }
}

// Tied medians, exactly.  When k_median flagged a cluster (members tie on ||v|| with different vectors), the member that
// libstdc++'s std::sort leaves at size/2 is found by replaying introsort's moves on the sub-range that holds that position
// (introsort_emul.h): the members are laid out in the reference's initial order (column-major pixel order,
// clusterMap2IndicesCluster, clusterer_nodelet.cpp:97-117), each __unguarded_partition is done by the whole workgroup —
// its k-th swap exchanges the k-th element from the left that is not before the pivot with the k-th from the right that is
// not after it, so ranks from two prefix counts give every swap at once — and the finished (<= 16 element) range gets the
// stable insertion sort.  Rare path: one workgroup per flagged cluster, nothing to do for the others.
// Scratch (all dead by now): keys -> parent plane, pixels -> rsize plane, swap lists -> the member arrays.
constexpr int kTieThreads = 1024, kTieLds = 8192;   // (13 Ki elements = 156 KB, one partition level less in HBM: measured in round 5, no faster, and a
                                                     // workgroup that needs a whole CU's LDS waits for one beside the other chunk's kernels)

struct TieShared {           // control block of one workgroup of k_median_ties
  int cntA[kTieThreads / 64], cntB[kTieThreads / 64];
  int first, last, depth, m, totA, done;
  uint32_t answer, pivot;
#ifdef MOD_PHASE_COUNTERS
  unsigned long long sec[3][8];   // shader cycles per section of a partition step: [HBM arrays / LDS arrays, range > 2048 / LDS, range <= 2048][section]; [..][7] = steps
  int mode;
#endif
};
#ifdef MOD_PHASE_COUNTERS
#define TIE_SEC(i) { if (tid == 0) { const unsigned long long t_ = clock64(); sh.sec[grp][i] += t_ - tsec; tsec = t_; } }
#else
#define TIE_SEC(i)
#endif

// One __unguarded_partition_pivot step on [first, last) of (key, val), by the whole workgroup; updates sh.first / sh.last
// to the side that holds `want`.  Works on HBM or LDS arrays alike (KP is deduced per call site, so each instance keeps its
// address space).  All threads must call it; ends with a barrier.
template <class KP, class PP>
__device__ __forceinline__ void tie_partition_step(KP key, KP val, PP Apos, PP Bpos, int first, int last, int want, TieShared &sh,
                                                   int tid) {
  using namespace introsort_emul;
  const int lane = tid & 63, wv = tid >> 6;
  constexpr int NW = kTieThreads / 64;
  // elements a wave takes per loop trip, in units of 64: eight reads in flight on HBM arrays (a trip is a memory round trip); ONE on
  // LDS arrays — there a step is bound by the CU's vector issue (16 waves x the unrolled body: the position pass alone took 4-7 k
  // cycles whatever the range), and a wave whose slice is 128 elements must not execute the body of 512 (round 5, section clocks)
  constexpr int U = std::is_same<PP, uint16_t *>::value ? 1 : 8;
#ifdef MOD_PHASE_COUNTERS
  const int grp = sh.mode == 0 ? 0 : (last - first > 2048 ? 1 : 2);
  unsigned long long tsec = clock64();
  if (tid == 0) sh.sec[grp][7] += 1;
#endif
  if (tid == 0) {
    sh.depth--;
    // __move_median_to_first(first, first + 1, mid, last - 1): the three keys are fetched together (one memory round trip
    // instead of one per comparison), the comparison tree of introsort_emul::move_median_to_first picks the median's
    // position, and the pivot's key is handed to the workgroup through LDS
    const int ia = first + 1, ib = first + (last - first) / 2, ic = last - 1;
    const uint32_t ka = key[ia], kb = key[ib], kc = key[ic];
    int im;                                              // comp(x, y) = key[x] > key[y]
    if (ka > kb) im = (kb > kc) ? ib : (ka > kc) ? ic : ia;
    else im = (ka > kc) ? ia : (kb > kc) ? ic : ib;
    const uint32_t km = (im == ia) ? ka : (im == ib) ? kb : kc;
    const uint32_t kf = key[first], vf = val[first], vm = val[im];
    key[first] = km; val[first] = vm; key[im] = kf; val[im] = vf;
    sh.pivot = km;
  }
  __syncthreads();
  TIE_SEC(0)
  const uint32_t pk = sh.pivot;
  // A: elements NOT before the pivot (key <= pk), ranked from the left; B: elements NOT after it (key >= pk), ranked from the
  // right.  Wave w owns one contiguous slice and reads it 64 consecutive elements at a time (4 reads in flight).
  const int lo = first + 1, L = last - lo;
  const int slice = (((L + NW - 1) / NW) + 63) & ~63;          // a multiple of 64: a wave's 64-element reads never straddle slices
  const int w0 = min(lo + wv * slice, last), w1 = min(w0 + slice, last);
  int cntA = 0, cntB = 0;
  for (int j0 = w0; j0 < w1; j0 += 64 * U) {
    uint32_t k4[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int j = j0 + u * 64 + lane; k4[u] = (j < w1) ? key[j] : 0u; }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const bool in = j0 + u * 64 + lane < w1;
      cntA += __popcll((unsigned long long)__ballot(in && k4[u] <= pk));
      cntB += __popcll((unsigned long long)__ballot(in && k4[u] >= pk));
    }
  }
  if (lane == 0) { sh.cntA[wv] = cntA; sh.cntB[wv] = cntB; }
  __syncthreads();
  TIE_SEC(1)
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < NW; t++) { const int x = sh.cntA[t]; sh.cntA[t] = run; run += x; }
    sh.totA = run; run = 0;
    for (int t = NW - 1; t >= 0; t--) { const int x = sh.cntB[t]; sh.cntB[t] = run; run += x; }
    sh.m = 0;
  }
  __syncthreads();
  TIE_SEC(2)
  {
    int runA = sh.cntA[wv], seenB = 0, mloc = 0;
    const int sufB = sh.cntB[wv];
    const uint64_t lt = (1ull << lane) - 1ull, le_m = lt | (1ull << lane);
    for (int j0 = w0; j0 < w1; j0 += 64 * U) {
      uint32_t k4[U];
#pragma unroll
      for (int u = 0; u < U; u++) { const int j = j0 + u * 64 + lane; k4[u] = (j < w1) ? key[j] : 0u; }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int j = j0 + u * 64 + lane;
        const bool in = j < w1, le = in && k4[u] <= pk, ge = in && k4[u] >= pk;
        const uint64_t bl = __ballot(le), bg = __ballot(ge);
        const int iA = runA + __popcll((unsigned long long)(bl & lt));
        // elements of B strictly right of j: later waves' + this wave's not yet seen, minus those up to and including this lane
        const int geR = sufB + (cntB - seenB - __popcll((unsigned long long)(bg & le_m)));
        // the iA-th stop of the left pointer swaps iff the iA-th stop of the right pointer lies right of it
        if (le) Apos[iA] = j;
        mloc += __popcll((unsigned long long)__ballot(le && geR >= iA + 1));   // (wave-uniform: one LDS atomic per wave below, not one per lane — 1024 adds on one address serialise)
        if (ge) Bpos[geR] = j;
        runA += __popcll((unsigned long long)bl);
        seenB += __popcll((unsigned long long)bg);
      }
    }
    if (mloc && lane == 0) atomicAdd(&sh.m, mloc);
  }
  __syncthreads();
  TIE_SEC(3)
  const int m = sh.m;
  for (int i0 = tid; i0 < m; i0 += kTieThreads * 2) {           // the m swaps, two per thread in flight
    const int i1 = i0 + kTieThreads;
    const int a0 = (int)Apos[i0], b0 = (int)Bpos[i0];
    const int a1 = (i1 < m) ? (int)Apos[i1] : a0, b1 = (i1 < m) ? (int)Bpos[i1] : b0;
    const uint32_t ka0 = key[a0], va0 = val[a0], kb0 = key[b0], vb0 = val[b0];
    const uint32_t ka1 = key[a1], va1 = val[a1], kb1 = key[b1], vb1 = val[b1];
    key[a0] = kb0; val[a0] = vb0; key[b0] = ka0; val[b0] = va0;
    if (i1 < m) { key[a1] = kb1; val[a1] = vb1; key[b1] = ka1; val[b1] = va1; }
  }
  __syncthreads();
  TIE_SEC(4)
  if (tid == 0) {
    // the left pointer's final stop: the next untouched element of A, unless the right pointer's last swap partner comes first
    const int am = (m < sh.totA) ? (int)Apos[m] : 0x7fffffff, bm = (m > 0) ? (int)Bpos[m - 1] : 0x7fffffff;
    const int cut = am < bm ? am : bm;
    if (want >= cut) sh.first = cut; else sh.last = cut;
  }
  __syncthreads();
  TIE_SEC(5)
}

// Runs partition steps until the live range is at most `stop` elements long (or the depth limit turns it into a heap sort).
template <class KP, class PP>
__device__ __forceinline__ void tie_narrow(KP key, KP val, PP Apos, PP Bpos, int want, int stop, TieShared &sh, int tid) {
  using namespace introsort_emul;
  while (true) {
    const int first = sh.first, last = sh.last;
    if (last - first <= stop || sh.done) break;
    if (sh.depth == 0) {                             // depth limit hit: __partial_sort(first, last, last) = heap sort
      __syncthreads();
      if (tid == 0) { const View v{&key[0], &val[0]}; heap_sort(v, first, last); sh.answer = val[want]; sh.done = 1; }
      __syncthreads();
      break;
    }
    __syncthreads();
    tie_partition_step(key, val, Apos, Bpos, first, last, want, sh, tid);
  }
}

// publishMovingObjects (clusterer_nodelet.cpp:324-343): ids run over ACCEPTED clusters only; a cluster is rejected when
// (double)||median v|| < dynamic_speed (:176) — unreachable for members that are all dynamic, kept for exactness.
__device__ __forceinline__ void finalize_frame(const DevCam &c, const ClArgs &a, int f) {
  const int K = a.counters[f * 8 + 1];                 // (k_ccl_merge's, an earlier kernel)
  ModObject *O = (ModObject *)a.objects + (size_t)f * a.max_objects;
  const ClusterInfo *C = a.clusters + (size_t)f * a.max_objects;
  int n = 0;
  for (int k = 0; k < K; k++) {
    const float nrm = __uint_as_float(C[k].med_bits);
    if ((double)nrm < c.speed_th_d) continue;
    if (n != k) O[n] = O[k];
    O[n].id = n;
    n++;
  }
  a.n_objects[f] = n;
}

__global__ __launch_bounds__(kTieThreads) void k_median_ties(DevCam c, ClArgs a, int frames) {
  using namespace introsort_emul;
  const int tid = threadIdx.x;
  const size_t N = (size_t)c.W * c.H;
  const int nwork = a.counters[7];
  // 96 KB of LDS, used twice: while the members are laid out, as kTieLds 64-bit cell masks + kTieLds cell offsets; during the
  // LDS part of the sort, as keys, values and two 16-bit position lists (positions inside the resident range fit 16 bits)
  __shared__ uint64_t lraw[kTieLds + kTieLds / 2];
  uint32_t *lkey = reinterpret_cast<uint32_t *>(&lraw[0]), *lval = lkey + kTieLds;
  uint16_t *lA = reinterpret_cast<uint16_t *>(lval + kTieLds), *lB = lA + kTieLds;
  uint64_t *cmask = &lraw[0];
  uint32_t *cstart = reinterpret_cast<uint32_t *>(&lraw[kTieLds]);
  __shared__ int s_box[4], s_lay[kTieThreads / 64 + 1];
  __shared__ TieShared sh;
  for (int wi = blockIdx.x; wi < nwork; wi += gridDim.x) {
    const uint32_t item = a.tielist[wi];
    const int f = (int)(item / (uint32_t)a.max_objects), k = (int)(item % (uint32_t)a.max_objects);
    const size_t fN = (size_t)f * N;
    ClusterInfo *ci = a.clusters + (size_t)f * a.max_objects + k;
    if (ci->ambiguous != 1) continue;                // block-uniform (always 1 for a listed cluster)
    PHASE_CLOCK
    const int size = ci->size, off = ci->offset;
    uint32_t *key = (uint32_t *)(a.parent + fN) + off;
    uint32_t *val = (uint32_t *)(a.rsize + fN) + off;
    uint32_t *Apos = a.mbits + fN + off, *Bpos = a.mpix + fN + off;
    // ---- image-space bounding box of the cluster (from its member list, before that list becomes scratch) ----
    const MemberBox bx = member_box<kTieThreads>(Bpos, size, (uint32_t)c.W, s_box, tid);
    PHASE_STAMP(20)
    if (MOD_ABLATE(c, 1 << 20)) continue;
    // ---- members in column-major order (clusterMap2IndicesCluster's order, :97-117): cluster_common.h member_layout, kTieLds cells per run.
    // (Round 1 scanned the labels plane for boxes with more cells; the member list needs neither that plane nor the velocities again.)
    // The keys are the ||v|| bits as k_final computed them (norm3_f32) ----
    {
      [[maybe_unused]] const int placed = member_layout<kTieThreads, kTieLds>(
          Bpos, size, (uint32_t)c.W, bx, cmask, cstart, s_lay, tid, [&](int i) { return Apos[i]; },
          [&](int slot, uint32_t p, uint32_t k2, uint32_t, uint32_t) { if (MOD_CHECK(a, slot >= 0 && slot < size, 11)) { key[slot] = k2; val[slot] = p; } },
          [&](int i) { PHASE_STAMP(21 + i) });
      (void)MOD_CHECK(a, placed == size, 14);        // every member lies in exactly one cell
    }
    PHASE_STAMP(23)
    if (MOD_ABLATE(c, 1 << 22)) continue;
    if (tid == 0) { sh.first = 0; sh.last = size; sh.depth = 2 * floor_log2(size); sh.done = 0; }
    __syncthreads();
    // ---- introsort, only along the range that holds position size/2: in HBM while the range is long, then in LDS ----
    const int want = size / 2;
#ifdef MOD_PHASE_COUNTERS
    if (tid == 0) { sh.mode = 0; for (int g = 0; g < 3; g++) for (int i = 0; i < 8; i++) sh.sec[g][i] = 0; }
    __syncthreads();
#endif
    tie_narrow(key, val, Apos, Bpos, want, kTieLds, sh, tid);
    PHASE_STAMP(24)
    if (MOD_ABLATE(c, 1 << 23)) continue;
    __syncthreads();
    if (!sh.done) {
      const int first = sh.first, len = sh.last - first;
      for (int i = tid; i < len; i += kTieThreads) { lkey[i] = key[first + i]; lval[i] = val[first + i]; }
      __syncthreads();
      if (tid == 0) { sh.first = 0; sh.last = len; }
#ifdef MOD_PHASE_COUNTERS
      if (tid == 0) sh.mode = 1;
#endif
      __syncthreads();
      tie_narrow(lkey, lval, lA, lB, want - first, 16, sh, tid);
      __syncthreads();
      if (!sh.done && tid == 0) {
        const View v{lkey, lval};
        insertion_sort(v, sh.first, sh.last);
        sh.answer = lval[want - first];
      }
      __syncthreads();
    }
    PHASE_STAMP(25)
#ifdef MOD_PHASE_COUNTERS
    if (tid == 0) for (int g = 0; g < 3; g++) for (int i = 0; i < 8; i++) atomicAdd(&a.dbg[(g == 0 ? 0 : g == 1 ? 8 : 44) + i], sh.sec[g][i]);   // (slots 0-15 are k_ccl_tile's, unused with the bit-plane tile stage at n = 4)
#endif
    if (tid == 0) {
      const uint32_t best = sh.answer;
      ci->med_pix = (int)best; ci->ambiguous = 2;    // 2 = tie resolved by replaying the reference's sort
      ModObject *o = (ModObject *)a.objects + (size_t)f * a.max_objects + k;
      o->velocity[0] = (double)a.vx[fN + best]; o->velocity[1] = (double)a.vy[fN + best]; o->velocity[2] = (double)a.vz[fN + best];
      __threadfence();                               // device-wide before this workgroup's count below (rare path: once per tied cluster)
    }
    __syncthreads();
  }
  // ---- the launch's LAST workgroup to get here closes the call (round 5; k_finalize was a kernel of its own until then):
  // publishMovingObjects for every frame, and the counters go back to zero — every call finds them as mod_create left them,
  // no memset in front of the tile stage (mod_sf.hip: scratch_clean) ----
  __shared__ int s_last;
  __syncthreads();
  if (tid == 0) s_last = (atomicAdd(&a.counters[2], 1) == (int)gridDim.x - 1) ? 1 : 0;
  __syncthreads();
  if (!s_last) return;                                 // block-uniform
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the velocities other workgroups resolved (one invalidate per launch)
  for (int f = tid; f < frames; f += kTieThreads) finalize_frame(c, a, f);
  __syncthreads();                                     // (frame 0's thread has read its count before the words go)
  for (int i = tid; i < frames * 8; i += kTieThreads) a.counters[i] = 0;
}
}  // namespace

void launch_median(const DevCam &c, const ClArgs &a, int frames, hipStream_t s) {
  // one 1024-thread workgroup fills a CU and costs ~80 ns of wave dispatch whether it finds work or not: launch at most one
  // per CU (fewer for small batches) and let each walk the launch's cluster list (k_select) / tie list (k_median)
  // (round 5: two 64-VGPR workgroups fit a CU — 512 of them)
  hipLaunchKernelGGL(k_median, dim3(std::min(512, frames * 8)), dim3(kMedThreads), 0, s, c, a);
  if (!a.xy_from_z) hipLaunchKernelGGL(k_box_nan, dim3(std::min(64, frames * 2)), dim3(kMedThreads), 0, s, c, a);   // a caller's cloud may hold NaN coordinates
  hipLaunchKernelGGL(k_median_ties, dim3(std::min(64, frames * 2)), dim3(kTieThreads), 0, s, c, a, frames);   // + publishMovingObjects in its last workgroup
}
