// host_sgm.hip — the C ABI's on-GPU disparity estimator, host side (no kernel): its parameter check, the scratch of a group of frames,
// what a set holds (SgmSet) with the two halves of a group (sgm_start, sgm_finish), the entry points around them and the sub-pixel and
// offset settings.  The kernels live in sgm.hip; the texture and speckle stages, the smoother and the hole fill of sgm_finish are
// host_filters.hip's.
#include "host_options.h"

#include <algorithm>

int check_sgm_params(ModContext *c, const ModSgmParams *p) {
  if (!p) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null SGM parameters");
  if (p->disparities < 1 || p->disparities > MOD_SGM_MAX_DISPARITIES) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparities must be in 1..128");
  if (p->p1 < 0 || p->p2 < p->p1 || 31 + p->p2 > 255) return fail(c, MOD_ERR_INVALID_ARGUMENT, "need 0 <= P1 <= P2 <= 224 (path costs are uint8)");
  if (p->paths != 4 && p->paths != 8) return fail(c, MOD_ERR_INVALID_ARGUMENT, "paths must be 4 or 8");
  if (c->dc.W < 2) return fail(c, MOD_ERR_INVALID_ARGUMENT, "the disparity estimator needs images at least 2 pixels wide");
  if ((size_t)c->dc.W * 8 + 4 > 64 * 1024) return fail(c, MOD_ERR_CAPACITY, "image row does not fit the census row buffer in LDS");
  return MOD_OK;
}

// scratch of the complete estimator for a GROUP of frames (one wave walks a path line, so a single frame cannot fill the GPU; the
// frames of a group run side by side): per frame two census planes, one uint8 cost volume PER PATH (written once, never read
// back by the path kernels: a running sum would put its load latency into every step of a path), four disparity maps.  Census
// planes and volumes exist twice, as two sets: consecutive groups overlap (mod_sgm_compute_dev).
constexpr int kSgmGroup = 8;                             // frames per group (4 .. 16 measured in round 3: 8 is the knee)
constexpr size_t kSgmVolumeBudget = (size_t)24 << 30;    // bytes of cost volumes a context may hold

static int ensure_sgm_scratch(ModContext *c, int D, int frames, bool subpixel, int *group) {
  Buffers::Sgm &b = c->b.sgm;
  const size_t N = c->maxN;
  const int even = (frames + kSgmGroup - 1) / kSgmGroup;          // groups of equal size: 11 frames go as 6 + 5, not 8 + 3
  int g = (frames + even - 1) / even;
  while (g > 1 && 2 * (size_t)g * N * D * kSgmPaths > kSgmVolumeBudget) g--;
  *group = g;
  if (!b.fork[0]) {
    for (int k = 0; k < 2; k++) {
      HIP_TRY(c, hipEventCreateWithFlags(b.fork[k].put(), hipEventDisableTiming));
      for (int i = 0; i < kSgmPaths; i++) HIP_TRY(c, hipEventCreateWithFlags(b.join[k][i].put(), hipEventDisableTiming));
    }
    // (a CU-masked path stream that kept one CU in 8 / 4 / 3 free for the winner-take-all of the group before was measured in
    // round 3 and changed nothing: plain non-blocking side streams)
    for (int i = 0; i < kSgmPaths; i++) HIP_TRY(c, hipStreamCreateWithFlags(b.side[i].put(), hipStreamNonBlocking));
  }
  const bool volumes_fit = b.S && b.D >= D && b.G >= g;
  if (volumes_fit && (b.maps16 || !subpixel)) return MOD_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (volumes_fit) {                                   // the first sub-pixel call of a context that has its volumes: only the maps grow
    DevPtr<uint8_t> maps;                              // the old maps stay until the new ones exist: a failed allocation changes nothing
    HIP_TRY(c, dalloc(maps, sgm_maps_bytes(true) * N * b.G));
    b.maps = std::move(maps);                      // (swaps: the old buffer is released with `maps`)
    b.maps16 = true;
    return MOD_OK;
  }
  // grow-only in BOTH dimensions: calls that alternate between (few disparities, large group) and (many, small) settle on the
  // maxima after one reallocation each instead of freeing and allocating gigabytes on every call
  const int D2 = std::max(D, b.D), g2 = std::max(g, b.G);
  const bool maps16 = subpixel || b.maps16;         // ... and in the width of the left maps (sub-pixel mode: 16-bit)
  b.S.reset(); b.census.reset(); b.maps.reset(); b.D = 0; b.G = 0; b.maps16 = false;
  // two sets (sgm_set) behind the lead the D == 128 path kernels need (mod_launch.h) — inside the allocation even for tiny images
  HIP_TRY(c, dalloc(b.census, kSgmCensusLead + 2 * 2 * N * g2));
  HIP_TRY(c, dalloc(b.maps, sgm_maps_bytes(maps16) * N * g2));
  HIP_TRY(c, dalloc(b.S, 2 * N * (size_t)D2 * g2 * kSgmPaths));
  b.D = D2; b.G = g2; b.maps16 = maps16;
  return MOD_OK;
}

// What set k & 1 holds for group k of a call: `g` frames from frame `f0` on
struct SgmSet {
  int f0, g;
  uint32_t *cl, *cr;            // census planes [g][N]; cr follows cl inside the scratch allocation: it has its lead
  uint8_t *S;                   // one cost volume [g][H][W][D] per path, path_stride bytes apart
  size_t path_stride;
  hipEvent_t fork;              // recorded on the context's stream behind the census kernels
  const Event *join;            // [kSgmPaths], recorded on the side streams behind the path kernels
  bool all_in_one;              // the paths went as ONE grid on side stream 0 (sgm_start): only join[0] was recorded
};

static SgmSet sgm_set(const Buffers::Sgm &b, int k, int group, int frames, size_t N, int D) {
  const int f0 = k * group, g = std::min(group, frames - f0), s = k & 1;
  uint32_t *cl = b.census + kSgmCensusLead + s * (2 * N * group);
  return {f0, g, cl, cl + N * g, b.S + s * (N * D * group * kSgmPaths), N * D * g, b.fork[s], b.join[s], false};
}

// census of the group on the context's stream, then its aggregation paths on the side streams
static int sgm_start(ModContext *c, const ModSgmParams *p, int off, const uint8_t *left, const uint8_t *right, SgmSet &s) {
  const int W = c->dc.W, H = c->dc.H, D = p->disparities;
  const size_t N = (size_t)W * H;
  const Stream *side = c->b.sgm.side;
  launch_sgm_census(W, H, s.g, left + s.f0 * N, s.cl, c->stream);
  launch_sgm_census(W, H, s.g, right + s.f0 * N, s.cr, c->stream);
  HIP_TRY(c, hipEventRecord(s.fork, c->stream));
  // the published configuration: all paths in ONE grid on one side stream (sgm.hip k_sgm_paths_all)
  HIP_TRY(c, hipStreamWaitEvent(side[0], s.fork, 0));
  if ((s.all_in_one = launch_sgm_paths_all(W, H, s.g, D, off, p->p1, p->p2, p->paths, s.path_stride, s.cl, s.cr, s.S, side[0]))) {
    HIP_TRY(c, hipEventRecord(s.join[0], side[0]));
    return MOD_OK;
  }
  for (int i = 0; i < p->paths; i++) {   // 4 paths: directions 0 .. 3
    HIP_TRY(c, hipStreamWaitEvent(side[i], s.fork, 0));   // a failed wait would let a path read census planes in flight
    launch_sgm_path(W, H, s.g, D, off, p->p1, p->p2, i, s.cl, s.cr, s.S + i * s.path_stride, nullptr, side[i]);
    HIP_TRY(c, hipEventRecord(s.join[i], side[i]));
  }
  return MOD_OK;
}

// winner-take-all .. left-right check of the group (and the texture and speckle filters) on the context's stream, behind its paths
static int sgm_finish(ModContext *c, const ModSgmParams *p, const EstimatorOptions &opt, const uint8_t *left, const SgmSet &s, const SgmMaps &maps, float *disparity) {
  const int W = c->dc.W, H = c->dc.H;
  const ModDisparityFilters &filters = opt.disparity_filters;
  const ModTextureFilter &tex = opt.texture_filter;
  const ModDisparitySmooth &smooth = opt.disparity_smooth;
  const ModDisparityFill &fill = opt.disparity_fill;
  // with the hole fill on, the stages below work on the group's scratch plane (all of them are on the context's stream, so one plane serves
  // every group) and the fill, the last stage, writes the caller's; with the smoother on they work on its scratch plane and the smoother
  // writes the fill's, or the caller's where the fill is off: neither stage reads the plane it writes
  float *const filled = disparity + s.f0 * ((size_t)W * H);
  float *const smoothed = fill.reach ? c->b.sgm.unfilled.get() : filled;
  float *const out = smooth.window ? c->b.sgm.unsmoothed.get() : smoothed;
  // a failed wait would let the winner-take-all read volumes the path kernels are still writing: surface it
  for (int i = 0; i < (s.all_in_one ? 1 : p->paths); i++) HIP_TRY(c, hipStreamWaitEvent(c->stream, s.join[i], 0));
  launch_sgm_finish(W, H, s.g, p->disparities, opt.disparity_offset, p->paths, s.path_stride, p->median, p->lr_check, filters.uniqueness_ratio, s.S, maps, out, c->stream);
  // the texture rule on the group's left planes, BEFORE the speckle stage (StereoBM's order: a rejected pixel splits regions)
  if (texture_applies(tex, MOD_TEXTURE_DISPARITY))
    launch_texture(W, H, s.g, tex.window, tex.cap, tex.threshold, left + s.f0 * ((size_t)W * H), nullptr, out, -1.0f, nullptr, c->stream);
  // the last stage, behind the group's left-right kernel on the context's stream (the paths of the next group run beside it as ever);
  // invalid pixels are -1 whatever the disparity offset is, so ">= 0 takes part" holds with one
  if (filters.speckle_size > 0)
    launch_speckle(W, H, s.g, 0.0f, -1.0f, filters.speckle_size, filters.speckle_range, out, c->b.spk.parent, c->b.spk.size, c->b.dbg, c->stream);
  // invalid is "not finite or < 0" in both stages below too: the speckle stage's rule, whatever the offset is
  if (smooth.window) launch_disparity_smooth(W, H, s.g, 0.0f, smooth.window, smooth.tol, smooth.min_members, out, smoothed, c->stream);
  if (fill.reach) launch_disparity_fill(W, H, s.g, 0.0f, fill.reach, fill.directions, fill.mode, fill.min_found, smoothed, filled, c->stream);
  return MOD_OK;
}

static int check_disparity_subpixel(ModContext *c, const int32_t &fraction_bits) {
  if (fraction_bits != 0 && fraction_bits != MOD_SGM_FRACTION_BITS)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity fraction_bits must be 0 (off) or 4 (sixteenths of a pixel)");
  return MOD_OK;
}

static int check_disparity_offset(ModContext *c, const int32_t &min_disparity) {
  if (min_disparity < 0 || min_disparity > kSgmMaxOffset) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity offset must be in 0..128");
  return MOD_OK;
}

extern "C" {

// ---- first stages -----------------------------------------------------------------------------------
int mod_sgm_census_dev(ModContext *c, int32_t frames, const uint8_t *image, uint32_t *census) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!image || !census) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null image / census plane");
  launch_sgm_census(c->dc.W, c->dc.H, frames, image, census, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_sgm_path_dev(ModContext *c, int32_t frames, const uint32_t *census_left, const uint32_t *census_right, const ModSgmParams *p,
                     int32_t direction, uint8_t *path_cost, uint8_t *matching_cost) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!census_left || !census_right || !path_cost) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null plane");
  if ((rc = check_sgm_params(c, p))) return rc;
  if (direction < 0 || direction > 7) return fail(c, MOD_ERR_INVALID_ARGUMENT, "direction must be 0..7");
  // (stage entry point, tests and tracing) D == 128: the right plane behind the lead those kernels need (mod_launch.h), in a copy;
  // the lead is zeroed, not "border": the kernels replace what they read there by the border cost
  const int off = c->opt.disparity_offset;
  const size_t words = (size_t)frames * c->dc.W * c->dc.H;
  DevPtr<uint32_t> padded;
  hipError_t e = hipSuccess;
  if (p->disparities == 128) {
    e = dalloc(padded, words + kSgmCensusLead);
    if (e == hipSuccess) e = hipMemsetAsync(padded, 0, kSgmCensusLead * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(padded + kSgmCensusLead, census_right, words * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream);
  }
  if (e == hipSuccess) {
    launch_sgm_path(c->dc.W, c->dc.H, frames, p->disparities, off, p->p1, p->p2, direction, census_left, padded ? padded + kSgmCensusLead : census_right,
                    path_cost, matching_cost, c->stream);
    e = hipGetLastError();
  }
  if (padded) (void)hipStreamSynchronize(c->stream);   // before the copy is released: on every path, the failed ones included
  HIP_TRY(c, e);
  return MOD_OK;
}

// ---- the complete estimator ------------------------------------------------------------------------------------------------
int mod_sgm_compute_dev(ModContext *c, int32_t frames, const uint8_t *left, const uint8_t *right, const ModSgmParams *p, float *disparity) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!left || !right) return MOD_SKIP_NO_DISPARITY_NOW;     // no image pair: no disparity (estimateDisparity fails, :272-276)
  if (!disparity) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null disparity plane");
  if ((rc = check_sgm_params(c, p))) return rc;
  const EstimatorOptions opt = c->opt;                   // the options of THIS call: every kernel below is enqueued before it returns
  const bool subpixel = opt.disparity_subpixel != 0;
  int group = 1;
  if ((rc = ensure_sgm_scratch(c, p->disparities, frames, subpixel, &group))) return rc;
  if (opt.disparity_filters.speckle_size > 0 && (rc = ensure_speckle_scratch(c, group))) return rc;
  if (opt.disparity_smooth.window && (rc = ensure_disparity_smooth_scratch(c, group))) return rc;
  if (opt.disparity_fill.reach && (rc = ensure_disparity_fill_scratch(c, group))) return rc;
  const size_t N = (size_t)c->dc.W * c->dc.H;
  const Buffers::Sgm &b = c->b.sgm;
  // Groups of frames go through two sets of census planes and cost volumes: while the winner-take-all of group k streams its
  // volumes (HBM-bound, context stream), the aggregation paths of group k + 1 (instruction-bound, one side stream per path) already
  // run.  Order on the context stream: census(0) fork(0) | census(1) fork(1) join(0) finish(0) | census(2) fork(2) join(1) finish(1) ...
  // — set s is written again (census(k + 2), paths(k + 2) behind fork(k + 2)) only after finish(k) has been enqueued before it.
  const int ngroups = (frames + group - 1) / group;
  const SgmMaps maps = sgm_carve_maps(b.maps, N, group, subpixel);
  SgmSet set[2];
  const auto start = [&](int k) { return sgm_start(c, p, opt.disparity_offset, left, right, set[k & 1] = sgm_set(b, k, group, frames, N, p->disparities)); };
  if ((rc = start(0))) return rc;
  for (int k = 0; k < ngroups; k++) {
    if (k + 1 < ngroups && (rc = start(k + 1))) return rc;
    if ((rc = sgm_finish(c, p, opt, left, set[k & 1], maps, disparity))) return rc;
  }
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

// ---- its settings (EstimatorOptions; the rejection filters' pair is in host_filters.hip, beside their check) -----------------------
int mod_set_disparity_subpixel(ModContext *c, int32_t fraction_bits) { return set_option(c, &EstimatorOptions::disparity_subpixel, &fraction_bits, check_disparity_subpixel); }
int mod_get_disparity_subpixel(const ModContext *c, int32_t *fraction_bits) { return get_option(c, &EstimatorOptions::disparity_subpixel, fraction_bits); }
int mod_set_disparity_offset(ModContext *c, int32_t min_disparity) { return set_option(c, &EstimatorOptions::disparity_offset, &min_disparity, check_disparity_offset); }
int mod_get_disparity_offset(const ModContext *c, int32_t *min_disparity) { return get_option(c, &EstimatorOptions::disparity_offset, min_disparity); }

}  // extern "C"
