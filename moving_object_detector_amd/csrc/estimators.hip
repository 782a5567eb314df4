// estimators.hip — the C ABI's on-GPU estimators (SGM disparity, census optical flow, stereo ego-motion): their *_dev entry points
// and scratch, the texture threshold both image estimators share, the flow's min-eigenvalue threshold and its median filter.  Host-side
// only; the kernels live in sgm.hip, flow.hip, egomotion.hip, disparity_filter.hip, texture.hip, corner.hip and flow_median.hip.
#include "mod_context.h"

#include <algorithm>
#include <cmath>

// ---- on-GPU disparity (sgm.hip) --------------------------------------------------------------------------------------------
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

// ---- texture filter (texture.hip) ---------------------------------------------------------------------------------------------
constexpr int kTextureMax = 225 * 255;   // 57375: a 15 x 15 window of differences capped at 255

// window and cap: what the kernel needs; threshold and apply: what the rule and the estimators need
static int check_texture_kernel(ModContext *c, const ModTextureFilter &f) {
  if (f.window < 3 || f.window > 15 || f.window % 2 == 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "texture window must be odd and in 3..15");
  if (f.cap < 1 || f.cap > 255) return fail(c, MOD_ERR_INVALID_ARGUMENT, "texture cap must be in 1..255");
  return MOD_OK;
}

static int check_texture_filter(ModContext *c, const ModTextureFilter &f) {
  if (f.threshold < 0 || f.threshold > kTextureMax) return fail(c, MOD_ERR_INVALID_ARGUMENT, "texture threshold must be in 0..57375");
  if (int rc = check_texture_kernel(c, f)) return rc;
  if (f.apply < 1 || f.apply > (MOD_TEXTURE_DISPARITY | MOD_TEXTURE_FLOW))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "texture apply must be MOD_TEXTURE_DISPARITY, MOD_TEXTURE_FLOW or both");
  return MOD_OK;
}

static bool texture_applies(const ModTextureFilter &f, int to) { return f.threshold > 0 && (f.apply & to) != 0; }

// ---- min-eigenvalue filter of the flow (corner.hip) -----------------------------------------------------------------------------
// window and cap: what the kernel needs; threshold and reserved: what the rule and the setter need
static int check_corner_kernel(ModContext *c, const ModCornerFilter &f) {
  if (f.window < 3 || f.window > 15 || f.window % 2 == 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "corner window must be odd and in 3..15");
  if (f.cap < 1 || f.cap > 255) return fail(c, MOD_ERR_INVALID_ARGUMENT, "corner cap must be in 1..255");
  return MOD_OK;
}

static int check_corner_filter(ModContext *c, const ModCornerFilter &f) {
  if (f.threshold < 0 || f.threshold > MOD_CORNER_MAX) return fail(c, MOD_ERR_INVALID_ARGUMENT, "corner threshold must be in 0..14630625");
  if (int rc = check_corner_kernel(c, f)) return rc;
  if (f.reserved != 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "corner reserved must be 0");
  return MOD_OK;
}

// ---- median filter of the flow (flow_median.hip) ---------------------------------------------------------------------------------
static int check_flow_median(ModContext *c, const ModFlowMedian &f) {
  if (f.window != 0 && f.window != 3 && f.window != 5) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow median window must be 0, 3 or 5");
  if (f.min_valid < 0 || f.min_valid > f.window * f.window) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow median min_valid must be in 0..window^2");
  if (f.reserved[0] != 0 || f.reserved[1] != 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow median reserved must be 0");
  return MOD_OK;
}

// winner-take-all .. left-right check of the group (and the texture and speckle filters) on the context's stream, behind its paths
static int sgm_finish(ModContext *c, const ModSgmParams *p, int off, const ModDisparityFilters &filters, const ModTextureFilter &tex, const uint8_t *left,
                      const SgmSet &s, const SgmMaps &maps, float *disparity) {
  const int W = c->dc.W, H = c->dc.H;
  float *out = disparity + s.f0 * ((size_t)W * H);
  // a failed wait would let the winner-take-all read volumes the path kernels are still writing: surface it
  for (int i = 0; i < (s.all_in_one ? 1 : p->paths); i++) HIP_TRY(c, hipStreamWaitEvent(c->stream, s.join[i], 0));
  launch_sgm_finish(W, H, s.g, p->disparities, off, p->paths, s.path_stride, p->median, p->lr_check, filters.uniqueness_ratio, s.S, maps, out, c->stream);
  // the texture rule on the group's left planes, BEFORE the speckle stage (StereoBM's order: a rejected pixel splits regions)
  if (texture_applies(tex, MOD_TEXTURE_DISPARITY))
    launch_texture(W, H, s.g, tex.window, tex.cap, tex.threshold, left + s.f0 * ((size_t)W * H), nullptr, out, -1.0f, nullptr, c->stream);
  // the last stage, behind the group's left-right kernel on the context's stream (the paths of the next group run beside it as ever);
  // invalid pixels are -1 whatever the disparity offset is, so ">= 0 takes part" holds with one
  if (filters.speckle_size > 0)
    launch_speckle(W, H, s.g, 0.0f, -1.0f, filters.speckle_size, filters.speckle_range, out, c->b.spk.parent, c->b.spk.size, c->b.dbg, c->stream);
  return MOD_OK;
}

// ---- rejection filters of the disparity (sgm.hip: uniqueness; disparity_filter.hip: speckle) -------------------------------
int check_disparity_filters(ModContext *c, const ModDisparityFilters *f) {
  if (f->uniqueness_ratio < 0 || f->uniqueness_ratio > 99) return fail(c, MOD_ERR_INVALID_ARGUMENT, "uniqueness_ratio must be in 0..99");
  if (f->speckle_size < 0 || (size_t)f->speckle_size > (size_t)c->cfg.max_width * (size_t)c->cfg.max_height)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "speckle_size must be in 0..max_width * max_height");
  if (f->speckle_range < 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "speckle_range must be >= 0");
  if (f->reserved != 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ModDisparityFilters.reserved must be 0");
  return MOD_OK;
}

// parent and size planes for `frames` frames; grows, after a sync, when a larger count comes (the old planes stay if that fails)
static int ensure_speckle_scratch(ModContext *c, int frames) {
  Buffers::Speckle &b = c->b.spk;
  if (b.frames >= frames) return MOD_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  DevPtr<int32_t> parent, size;
  HIP_TRY(c, dalloc(parent, (size_t)frames * c->maxN));
  HIP_TRY(c, dalloc(size, (size_t)frames * c->maxN));
  b.parent = std::move(parent); b.size = std::move(size);   // (swaps: the old planes are released with the locals)
  b.frames = frames;
  return MOD_OK;
}

// ---- on-GPU optical flow (flow.hip) ---------------------------------------------------------------------------------------
constexpr int kFlowMaxLevels = 6;
constexpr int kFlowMinCoarse = 16;      // px on either side of the coarsest level

// The pyramid of a call: level l is W[l] x H[l] pixels (level 0: the camera's); its region [2][maxF][(max_width >> l) * (max_height >> l)] of the per-level
// scratch, sized for the capacity, starts img[l] / cen[l] elements into Buffers::Flow::img (l >= 1) / ::census; entry kFlowMaxLevels: the buffer's length
struct FlowPlan { int W[kFlowMaxLevels], H[kFlowMaxLevels]; size_t img[kFlowMaxLevels + 1], cen[kFlowMaxLevels + 1]; };

static FlowPlan flow_plan(const ModContext *c) {
  FlowPlan p{};
  for (int l = 0; l < kFlowMaxLevels; l++) {
    p.W[l] = c->dc.W >> l; p.H[l] = c->dc.H >> l;
    p.cen[l + 1] = p.cen[l] + (size_t)2 * c->cfg.max_frames * (size_t)(c->cfg.max_width >> l) * (size_t)(c->cfg.max_height >> l); p.img[l + 1] = p.cen[l + 1] - p.cen[1];
  }
  return p;
}

int check_flow_params(ModContext *c, const ModFlowParams *p, int frames) {
  if (!p) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow parameters");
  if (p->levels < 1 || p->levels > kFlowMaxLevels) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow levels must be in 1..6");
  if (p->radius < 1 || p->radius > 8) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow radius must be in 1..8");
  if (p->window != 3 && p->window != 5 && p->window != 7) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow window must be 3, 5 or 7");
  if (p->subpixel != 0 && p->subpixel != 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow subpixel must be 0 or 1");
  if ((c->dc.W >> (p->levels - 1)) < kFlowMinCoarse || (c->dc.H >> (p->levels - 1)) < kFlowMinCoarse)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "too many flow levels: the coarsest would be smaller than 16 px");
  if (2 * frames > 65535) return fail(c, MOD_ERR_CAPACITY, "flow takes at most 32767 frames per call");   // both images ride in grid.z
  return MOD_OK;
}

static int ensure_flow_scratch(ModContext *c, const FlowPlan &lv) {
  Buffers::Flow &b = c->b.flow;
  if (b.sub) return MOD_OK;                          // the last buffer of the set exists: all do
  HIP_TRY(c, dalloc(b.img, lv.img[kFlowMaxLevels]));
  HIP_TRY(c, dalloc(b.census, lv.cen[kFlowMaxLevels]));
  HIP_TRY(c, dalloc(b.winners, 2 * 2 * (size_t)c->cfg.max_frames * c->maxN));
  HIP_TRY(c, dalloc(b.sub, (size_t)c->cfg.max_frames * c->maxN));
  return MOD_OK;
}

// ---- on-GPU ego-motion (egomotion.hip) -------------------------------------------------------------------------------------
int check_ego_params(ModContext *c, const ModEgoParams *p) {
  if (!p) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null ego-motion parameters");
  if (p->stride < 1 || p->stride > 64) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion stride must be in 1..64");
  if (p->hypotheses < 1 || p->hypotheses > MOD_EGO_MAX_HYPOTHESES)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion hypotheses must be in 1..4096");
  if (p->iterations < 0 || p->iterations > 100) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion iterations must be in 0..100");
  if (p->min_inliers < 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion min_inliers must be >= 0");
  if (!(p->inlier_threshold > 0.0f) || !std::isfinite(p->inlier_threshold))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion inlier_threshold must be a positive number");
  if (!std::isfinite(p->min_disparity)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion min_disparity must be finite");
  return MOD_OK;
}

// Correspondence scratch for `stride` (max_width x max_height x max_frames / stride^2); grows, after a sync, when a smaller stride comes.
static int ensure_ego_scratch(ModContext *c, int stride) {
  Buffers::Ego &b = c->b.ego;
  const size_t F = (size_t)c->cfg.max_frames;
  const int gw = (c->cfg.max_width + stride - 1) / stride, gh = (c->cfg.max_height + stride - 1) / stride;
  const size_t cap = (size_t)gw * gh;
  if (cap > b.cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    b.corr.reset(); b.flag.reset(); b.blkcnt.reset(); b.cap = 0;
    HIP_TRY(c, dalloc(b.corr, F * 9 * cap));
    HIP_TRY(c, dalloc(b.flag, F * cap));
    HIP_TRY(c, dalloc(b.blkcnt, F * (size_t)ego_grid_blocks(gw, gh)));
    b.cap = cap;
  }
  if (!b.res) {
    HIP_TRY(c, dalloc(b.ncorr, F));
    HIP_TRY(c, dalloc(b.hyp, F * MOD_EGO_MAX_HYPOTHESES * 12));
    HIP_TRY(c, dalloc(b.hcnt, F * MOD_EGO_MAX_HYPOTHESES));
    HIP_TRY(c, dalloc(b.tf, F));
    HIP_TRY(c, dalloc(b.res, F));
  }
  return MOD_OK;
}

int run_egomotion(ModContext *c, int frames, const float *dprev, const float *dnow, const float *flow, const ModEgoParams *p,
                  ModTransform *tf, ModEgoResult *res, FrameConst *fc, double dt) {
  int rc = ensure_ego_scratch(c, p->stride);
  if (rc) return rc;
  Buffers::Ego &b = c->b.ego;
  EgoArgs a;
  a.W = c->dc.W; a.H = c->dc.H; a.frames = frames; a.stride = p->stride;
  a.gw = (a.W + p->stride - 1) / p->stride; a.gh = (a.H + p->stride - 1) / p->stride;
  a.cap = (int)b.cap;
  a.hyps = p->hypotheses; a.iterations = p->iterations; a.min_inliers = p->min_inliers; a.seed = p->seed;
  a.dlo = std::max(c->cam.min_disparity, p->min_disparity); a.dhi = c->cam.max_disparity;
  a.th = (double)p->inlier_threshold;
  a.fx = c->cam.fx; a.fy = c->cam.fy; a.cx = c->cam.cx; a.cy = c->cam.cy; a.Tx = c->cam.Tx; a.Ty = c->cam.Ty; a.fT = (double)c->dc.fT;
  a.dprev = dprev; a.dnow = dnow; a.flow = flow;
  a.corr = b.corr; a.blkcnt = b.blkcnt; a.ncorr = b.ncorr; a.hyp = b.hyp; a.hcnt = b.hcnt; a.flag = b.flag;
  a.tf = reinterpret_cast<double *>(tf ? tf : b.tf.get()); a.res = res ? res : b.res.get(); a.fc = fc; a.dt = dt;
  static_assert(sizeof(ModTransform) == 7 * sizeof(double), "ModTransform is 7 doubles");
  launch_egomotion(a, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

extern "C" {

// ---- on-GPU disparity, first stages ---------------------------------------------------------------
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
  const int off = c->sgm_offset;
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

int mod_sgm_compute_dev(ModContext *c, int32_t frames, const uint8_t *left, const uint8_t *right, const ModSgmParams *p, float *disparity) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!left || !right) return MOD_SKIP_NO_DISPARITY_NOW;     // no image pair: no disparity (estimateDisparity fails, :272-276)
  if (!disparity) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null disparity plane");
  if ((rc = check_sgm_params(c, p))) return rc;
  int group = 1;
  const bool subpixel = c->sgm_fraction_bits != 0;       // the setting of THIS call: every kernel below is enqueued before it returns
  const ModDisparityFilters filters = c->sgm_filters;   // ... and so are the filters
  const int off = c->sgm_offset;                         // ... and the disparity offset
  const ModTextureFilter tex = c->texture;               // ... and the texture filter
  if ((rc = ensure_sgm_scratch(c, p->disparities, frames, subpixel, &group))) return rc;
  if (filters.speckle_size > 0 && (rc = ensure_speckle_scratch(c, group))) return rc;
  const size_t N = (size_t)c->dc.W * c->dc.H;
  const Buffers::Sgm &b = c->b.sgm;
  // Groups of frames go through two sets of census planes and cost volumes: while the winner-take-all of group k streams its
  // volumes (HBM-bound, context stream), the aggregation paths of group k + 1 (instruction-bound, one side stream per path) already
  // run.  Order on the context stream: census(0) fork(0) | census(1) fork(1) join(0) finish(0) | census(2) fork(2) join(1) finish(1) ...
  // — set s is written again (census(k + 2), paths(k + 2) behind fork(k + 2)) only after finish(k) has been enqueued before it.
  const int ngroups = (frames + group - 1) / group;
  const SgmMaps maps = sgm_carve_maps(b.maps, N, group, subpixel);
  SgmSet set[2];
  const auto start = [&](int k) { return sgm_start(c, p, off, left, right, set[k & 1] = sgm_set(b, k, group, frames, N, p->disparities)); };
  if ((rc = start(0))) return rc;
  for (int k = 0; k < ngroups; k++) {
    if (k + 1 < ngroups && (rc = start(k + 1))) return rc;
    if ((rc = sgm_finish(c, p, off, filters, tex, left, set[k & 1], maps, disparity))) return rc;
  }
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_disparity_subpixel(ModContext *c, int32_t fraction_bits) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (fraction_bits != 0 && fraction_bits != MOD_SGM_FRACTION_BITS)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity fraction_bits must be 0 (off) or 4 (sixteenths of a pixel)");
  c->sgm_fraction_bits = fraction_bits;
  return MOD_OK;
}

int mod_get_disparity_subpixel(const ModContext *c, int32_t *fraction_bits) {
  if (!c || !fraction_bits) return MOD_ERR_INVALID_ARGUMENT;
  *fraction_bits = c->sgm_fraction_bits;
  return MOD_OK;
}

int mod_set_disparity_offset(ModContext *c, int32_t min_disparity) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (min_disparity < 0 || min_disparity > kSgmMaxOffset) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity offset must be in 0..128");
  c->sgm_offset = min_disparity;
  return MOD_OK;
}

int mod_get_disparity_offset(const ModContext *c, int32_t *min_disparity) {
  if (!c || !min_disparity) return MOD_ERR_INVALID_ARGUMENT;
  *min_disparity = c->sgm_offset;
  return MOD_OK;
}

int mod_set_disparity_filters(ModContext *c, const ModDisparityFilters *f) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!f) { c->sgm_filters = ModDisparityFilters{}; return MOD_OK; }
  if (int rc = check_disparity_filters(c, f)) return rc;
  c->sgm_filters = *f;
  return MOD_OK;
}

int mod_get_disparity_filters(const ModContext *c, ModDisparityFilters *f) {
  if (!c || !f) return MOD_ERR_INVALID_ARGUMENT;
  *f = c->sgm_filters;
  return MOD_OK;
}

int mod_set_flow_propagation(ModContext *c, int32_t seeds) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (seeds != 1 && seeds != MOD_FLOW_SEEDS) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow seeds must be 1 (off) or 5 (the parent and its four neighbours)");
  c->flow_seeds = seeds;
  return MOD_OK;
}

int mod_get_flow_propagation(const ModContext *c, int32_t *seeds) {
  if (!c || !seeds) return MOD_ERR_INVALID_ARGUMENT;
  *seeds = c->flow_seeds;
  return MOD_OK;
}

int mod_disparity_speckle_dev(ModContext *c, int32_t frames, float *disparity, int32_t speckle_size, int32_t speckle_range) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!disparity) return MOD_SKIP_NO_DISPARITY_NOW;
  const ModDisparityFilters f{0, speckle_size, speckle_range, 0};
  if ((rc = check_disparity_filters(c, &f))) return rc;
  if (speckle_size == 0) return MOD_OK;
  if ((rc = ensure_speckle_scratch(c, c->cfg.max_frames))) return rc;
  launch_speckle(c->dc.W, c->dc.H, frames, c->cam.min_disparity, c->cam.min_disparity - 1.0f, speckle_size, speckle_range, disparity,
                 c->b.spk.parent, c->b.spk.size, c->b.dbg, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_texture_filter(ModContext *c, const ModTextureFilter *f) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!f) { c->texture = ModContext{}.texture; return MOD_OK; }
  if (int rc = check_texture_filter(c, *f)) return rc;
  c->texture = *f;
  return MOD_OK;
}

int mod_get_texture_filter(const ModContext *c, ModTextureFilter *f) {
  if (!c || !f) return MOD_ERR_INVALID_ARGUMENT;
  *f = c->texture;
  return MOD_OK;
}

int mod_texture_dev(ModContext *c, int32_t frames, const uint8_t *grey, const ModTextureFilter *f, uint16_t *texture) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!grey || !texture) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null grey / texture plane");
  const ModTextureFilter t = f ? *f : c->texture;
  if ((rc = check_texture_kernel(c, t))) return rc;
  launch_texture(c->dc.W, c->dc.H, frames, t.window, t.cap, 0, grey, texture, nullptr, 0.0f, nullptr, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_texture_reject_dev(ModContext *c, int32_t frames, const uint8_t *grey, const ModTextureFilter *f, float *disparity, float *flow) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!grey || (!disparity && !flow)) return MOD_SKIP_NO_DISPARITY_NOW;
  const ModTextureFilter t = f ? *f : c->texture;
  if ((rc = check_texture_filter(c, t))) return rc;
  if (t.threshold == 0) return MOD_OK;
  launch_texture(c->dc.W, c->dc.H, frames, t.window, t.cap, t.threshold, grey, nullptr, disparity, c->cam.min_disparity - 1.0f, flow, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_flow_corner_filter(ModContext *c, const ModCornerFilter *f) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!f) { c->corner = ModContext{}.corner; return MOD_OK; }
  if (int rc = check_corner_filter(c, *f)) return rc;
  c->corner = *f;
  return MOD_OK;
}

int mod_get_flow_corner_filter(const ModContext *c, ModCornerFilter *f) {
  if (!c || !f) return MOD_ERR_INVALID_ARGUMENT;
  *f = c->corner;
  return MOD_OK;
}

int mod_flow_corner_dev(ModContext *c, int32_t frames, const uint8_t *grey, const ModCornerFilter *f, uint32_t *strength) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!grey || !strength) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null grey / corner strength plane");
  const ModCornerFilter t = f ? *f : c->corner;
  if ((rc = check_corner_kernel(c, t))) return rc;
  launch_corner(c->dc.W, c->dc.H, frames, t.window, t.cap, 0, grey, strength, nullptr, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_flow_corner_reject_dev(ModContext *c, int32_t frames, const uint8_t *grey, const ModCornerFilter *f, float *flow) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!grey || !flow) return MOD_SKIP_NO_FLOW;
  const ModCornerFilter t = f ? *f : c->corner;
  if ((rc = check_corner_filter(c, t))) return rc;
  if (t.threshold == 0) return MOD_OK;
  launch_corner(c->dc.W, c->dc.H, frames, t.window, t.cap, t.threshold, grey, nullptr, flow, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_flow_median(ModContext *c, const ModFlowMedian *f) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!f) { c->median = ModFlowMedian{}; return MOD_OK; }
  if (int rc = check_flow_median(c, *f)) return rc;
  c->median = *f;
  return MOD_OK;
}

int mod_get_flow_median(const ModContext *c, ModFlowMedian *f) {
  if (!c || !f) return MOD_ERR_INVALID_ARGUMENT;
  *f = c->median;
  return MOD_OK;
}

int mod_flow_median_dev(ModContext *c, int32_t frames, const float *flow_in, const ModFlowMedian *f, float *flow_out) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!flow_in || !flow_out) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow median plane");
  const ModFlowMedian m = f ? *f : c->median;
  if ((rc = check_flow_median(c, m))) return rc;
  if (m.window == 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow median window 0: nothing to do");
  const uintptr_t a = (uintptr_t)flow_in, b = (uintptr_t)flow_out, bytes = (uintptr_t)frames * c->dc.W * c->dc.H * 8;
  if (a < b + bytes && b < a + bytes) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow median planes overlap: a stencil cannot run in place");
  launch_flow_median(c->dc.W, c->dc.H, frames, m.window, m.min_valid, flow_in, flow_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_flow_compute_dev(ModContext *c, int32_t frames, const uint8_t *prev, const uint8_t *now, const ModFlowParams *p, float *flow) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!prev || !now) return MOD_SKIP_NO_FLOW;                  // no image pair: no flow (estimateOpticalFlow fails, :279-290)
  if (!flow) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow plane");
  if ((rc = check_flow_params(c, p, frames))) return rc;
  const FlowPlan lv = flow_plan(c);
  if ((rc = ensure_flow_scratch(c, lv))) return rc;
  const ModFlowMedian med = c->median;                   // the setting of THIS call, like the three below
  if (med.window) HIP_TRY(c, dalloc(c->b.flow.unfiltered, (size_t)c->cfg.max_frames * c->maxN));
  const Buffers::Flow &b = c->b.flow;
  // with the median filter on, the finishing step and the two rules write the scratch plane and the filter, last, the caller's
  float *const caller = flow;
  if (med.window) flow = reinterpret_cast<float *>(b.unfiltered.get());
  const int L = p->levels, F = frames, dirs = p->fb_check >= 0 ? 2 : 1;
  const int seeds = c->flow_seeds;                       // the setting of THIS call: every kernel below is enqueued before it returns
  const ModTextureFilter tex = c->texture;               // ... and the texture filter
  const ModCornerFilter cor = c->corner;                 // ... and the min-eigenvalue filter
  const int *const W = lv.W, *const H = lv.H; uint8_t *const img = b.img; uint32_t *const cen = b.census;   // level l >= 1 at img + lv.img[l], level l of the census planes at cen + lv.cen[l]: [2][F][H[l]][W[l]]
  const size_t N = (size_t)W[0] * H[0];
  for (int l = 1; l < L; l++) {
    uint8_t *const src = img + lv.img[l - 1];            // (level 0 is the caller's two images)
    launch_flow_pyramid(W[l - 1], H[l - 1], W[l], H[l], F, l == 1 ? prev : src, l == 1 ? now : src + F * ((size_t)W[l - 1] * H[l - 1]), img + lv.img[l], c->stream);
  }
  launch_sgm_census(W[0], H[0], F, prev, cen, c->stream);
  launch_sgm_census(W[0], H[0], F, now, cen + F * N, c->stream);
  for (int l = 1; l < L; l++) launch_sgm_census(W[l], H[l], 2 * F, img + lv.img[l], cen + lv.cen[l], c->stream);
  // coarse to fine; level l writes integer plane set (l & 1) and reads set ((l + 1) & 1)
  const size_t set = 2 * (size_t)c->cfg.max_frames * c->maxN;
  short4 *const sub = p->subpixel ? b.sub.get() : nullptr;
  for (int l = L - 1; l >= 0; l--) {
    const bool coarsest = l == L - 1;
    launch_flow_match(W[l], H[l], coarsest ? 0 : W[l + 1], coarsest ? 0 : H[l + 1], F, dirs, p->window, p->radius, seeds, cen + lv.cen[l],
                      coarsest ? nullptr : b.winners + ((l + 1) & 1) * set, b.winners + (l & 1) * set, l == 0 ? sub : nullptr, c->stream);
  }
  launch_flow_finish(W[0], H[0], F, b.winners, dirs == 2 ? b.winners + (size_t)F * N : nullptr, sub, p->fb_check, flow, c->stream);
  // the texture rule on the NOW image: the flow is indexed at the now pixel
  if (texture_applies(tex, MOD_TEXTURE_FLOW)) launch_texture(W[0], H[0], F, tex.window, tex.cap, tex.threshold, now, nullptr, nullptr, 0.0f, flow, c->stream);
  // the min-eigenvalue rule, on the NOW image as well; it stores only where it rejects and reads no flow, so its order against the
  // texture launch changes no byte
  if (cor.threshold > 0) launch_corner(W[0], H[0], F, cor.window, cor.cap, cor.threshold, now, nullptr, flow, c->stream);
  // the median filter, last: a vector the rules above rejected never votes
  if (med.window) launch_flow_median(W[0], H[0], F, med.window, med.min_valid, flow, caller, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_egomotion_dev(ModContext *c, int32_t frames, const float *disparity_prev, const float *disparity_now, const float *flow,
                      const ModEgoParams *p, ModTransform *transforms, ModEgoResult *results) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if ((rc = check_ego_params(c, p))) return rc;
  if (!transforms) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null transforms");
  if ((rc = construct_skip(flow, disparity_prev, true, disparity_now))) return rc;
  return run_egomotion(c, frames, disparity_prev, disparity_now, flow, p, transforms, results, nullptr, 0.0);
}

}  // extern "C"
