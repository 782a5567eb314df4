// host_flow.hip — the C ABI's on-GPU census optical flow, host side (no kernel): its parameter check, the pyramid's level sizes and
// scratch (FlowPlan), what one call works on (FlowCall) with the three steps of mod_flow_compute_dev, and the propagation setting.
// The kernels live in flow.hip (census: sgm.hip); the texture, min-eigenvalue and median stages of flow_finish are host_filters.hip's.
#include "host_options.h"

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

// every buffer of the set, and with the median filter on the plane in front of it (dalloc: a buffer that exists stays)
static int ensure_flow_scratch(ModContext *c, const FlowPlan &lv, bool median_on) {
  Buffers::Flow &b = c->b.flow;
  HIP_TRY(c, dalloc(b.img, lv.img[kFlowMaxLevels]));
  HIP_TRY(c, dalloc(b.census, lv.cen[kFlowMaxLevels]));
  HIP_TRY(c, dalloc(b.winners, 2 * 2 * (size_t)c->cfg.max_frames * c->maxN));
  HIP_TRY(c, dalloc(b.sub, (size_t)c->cfg.max_frames * c->maxN));
  if (median_on) HIP_TRY(c, dalloc(c->b.flow.unfiltered, (size_t)c->cfg.max_frames * c->maxN));
  return MOD_OK;
}

// What one call works on, gathered once the scratch exists: the pyramid, the parameters, the two images, and what the steps below share
struct FlowCall {
  FlowPlan lv;
  const ModFlowParams *p;
  const uint8_t *prev, *now;
  int F, dirs;                  // frames; directions matched (2: with the forward-backward check)
  size_t N, set;                // pixels of level 0; elements between the two integer plane sets of Buffers::Flow::winners
  short4 *sub;                  // the sub-pixel terms of level 0, or null
  float *out;                   // the plane the chain writes: the caller's, or with the median filter on Buffers::Flow::unfiltered ...
  float *caller;                // ... which the filter, last, reads on its way to the caller's
};

static FlowCall flow_call(const ModContext *c, const FlowPlan &lv, int frames, const uint8_t *prev, const uint8_t *now, const ModFlowParams *p, bool median_on, float *flow) {
  const Buffers::Flow &b = c->b.flow;
  return {lv, p, prev, now, frames, p->fb_check >= 0 ? 2 : 1, (size_t)lv.W[0] * lv.H[0], 2 * (size_t)c->cfg.max_frames * c->maxN,
          p->subpixel ? b.sub.get() : nullptr, median_on ? reinterpret_cast<float *>(b.unfiltered.get()) : flow, flow};
}

// the pyramid of both images, then the census planes of every level
static void flow_pyramid_census(ModContext *c, const FlowCall &k) {
  const FlowPlan &lv = k.lv;
  const int *const W = lv.W, *const H = lv.H, L = k.p->levels, F = k.F;
  uint8_t *const img = c->b.flow.img; uint32_t *const cen = c->b.flow.census;   // level l >= 1 at img + lv.img[l], level l of the census planes at cen + lv.cen[l]: [2][F][H[l]][W[l]]
  for (int l = 1; l < L; l++) {
    uint8_t *const src = img + lv.img[l - 1];            // (level 0 is the caller's two images)
    launch_flow_pyramid(W[l - 1], H[l - 1], W[l], H[l], F, l == 1 ? k.prev : src, l == 1 ? k.now : src + F * ((size_t)W[l - 1] * H[l - 1]), img + lv.img[l], c->stream);
  }
  launch_sgm_census(W[0], H[0], F, k.prev, cen, c->stream);
  launch_sgm_census(W[0], H[0], F, k.now, cen + F * k.N, c->stream);
  for (int l = 1; l < L; l++) launch_sgm_census(W[l], H[l], 2 * F, img + lv.img[l], cen + lv.cen[l], c->stream);
}

// coarse to fine; level l writes integer plane set (l & 1) and reads set ((l + 1) & 1)
static void flow_match(ModContext *c, const FlowCall &k, const EstimatorOptions &opt) {
  const Buffers::Flow &b = c->b.flow;
  const int *const W = k.lv.W, *const H = k.lv.H, L = k.p->levels;
  for (int l = L - 1; l >= 0; l--) {
    const bool coarsest = l == L - 1;
    launch_flow_match(W[l], H[l], coarsest ? 0 : W[l + 1], coarsest ? 0 : H[l + 1], k.F, k.dirs, k.p->window, k.p->radius, opt.flow_propagation, b.census + k.lv.cen[l],
                      coarsest ? nullptr : b.winners + ((l + 1) & 1) * k.set, b.winners + (l & 1) * k.set, l == 0 ? k.sub : nullptr, c->stream);
  }
}

// the finishing step into k.out, the two rejection rules on it and the median filter
static void flow_finish(ModContext *c, const FlowCall &k, const EstimatorOptions &opt) {
  const Buffers::Flow &b = c->b.flow;
  const int W = k.lv.W[0], H = k.lv.H[0], F = k.F;
  const ModTextureFilter &tex = opt.texture_filter;
  const ModCornerFilter &cor = opt.flow_corner_filter;
  const ModFlowMedian &med = opt.flow_median;
  launch_flow_finish(W, H, F, b.winners, k.dirs == 2 ? b.winners + (size_t)F * k.N : nullptr, k.sub, k.p->fb_check, k.out, c->stream);
  // the texture rule on the NOW image: the flow is indexed at the now pixel
  if (texture_applies(tex, MOD_TEXTURE_FLOW)) launch_texture(W, H, F, tex.window, tex.cap, tex.threshold, k.now, nullptr, nullptr, 0.0f, k.out, c->stream);
  // the min-eigenvalue rule, on the NOW image as well; it stores only where it rejects and reads no flow, so its order against the
  // texture launch changes no byte
  if (cor.threshold > 0) launch_corner(W, H, F, cor.window, cor.cap, cor.threshold, k.now, nullptr, k.out, c->stream);
  // the median filter, last: a vector the rules above rejected never votes
  if (med.window) launch_flow_median(W, H, F, med.window, med.min_valid, k.out, k.caller, c->stream);
}

static int check_flow_propagation(ModContext *c, const int32_t &seeds) {
  if (seeds != 1 && seeds != MOD_FLOW_SEEDS) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow seeds must be 1 (off) or 5 (the parent and its four neighbours)");
  return MOD_OK;
}

extern "C" {

int mod_flow_compute_dev(ModContext *c, int32_t frames, const uint8_t *prev, const uint8_t *now, const ModFlowParams *p, float *flow) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!prev || !now) return MOD_SKIP_NO_FLOW;                  // no image pair: no flow (estimateOpticalFlow fails, :279-290)
  if (!flow) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow plane");
  if ((rc = check_flow_params(c, p, frames))) return rc;
  const EstimatorOptions opt = c->opt;                   // the options of THIS call: every kernel below is enqueued before it returns
  const bool median_on = opt.flow_median.window != 0;
  const FlowPlan lv = flow_plan(c);
  if ((rc = ensure_flow_scratch(c, lv, median_on))) return rc;
  const FlowCall k = flow_call(c, lv, frames, prev, now, p, median_on, flow);
  flow_pyramid_census(c, k);
  flow_match(c, k, opt);
  flow_finish(c, k, opt);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_flow_propagation(ModContext *c, int32_t seeds) { return set_option(c, &EstimatorOptions::flow_propagation, &seeds, check_flow_propagation); }
int mod_get_flow_propagation(const ModContext *c, int32_t *seeds) { return get_option(c, &EstimatorOptions::flow_propagation, seeds); }

}  // extern "C"
