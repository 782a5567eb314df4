// host_filters.hip — the rules of the two image estimators that also exist as calls of their own, host side (no kernel): per filter its
// check, its setting's set / get pair (the defaults are EstimatorOptions') and its stand-alone entry points — the disparity's rejection
// filters with the speckle scratch, its smoother and its occlusion hole fill, the texture threshold both estimators share, the flow's min-eigenvalue threshold,
// its median and its hole fill.  host_sgm.hip and host_flow.hip enqueue the same launches inside their chains.  The kernels live in
// disparity_filter.hip (uniqueness: sgm.hip), disparity_smooth.hip, disparity_fill.hip, texture.hip, corner.hip, flow_median.hip and flow_fill.hip.
#include "host_options.h"

#include <cfloat>

// ---- rejection filters of the disparity (sgm.hip: uniqueness; disparity_filter.hip: speckle) -------------------------------
static int check_disparity_filters(ModContext *c, const ModDisparityFilters &f) {
  if (f.uniqueness_ratio < 0 || f.uniqueness_ratio > 99) return fail(c, MOD_ERR_INVALID_ARGUMENT, "uniqueness_ratio must be in 0..99");
  if (f.speckle_size < 0 || (size_t)f.speckle_size > (size_t)c->cfg.max_width * (size_t)c->cfg.max_height)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "speckle_size must be in 0..max_width * max_height");
  if (f.speckle_range < 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "speckle_range must be >= 0");
  if (f.reserved != 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ModDisparityFilters.reserved must be 0");
  return MOD_OK;
}

int ensure_speckle_scratch(ModContext *c, int frames) {
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

// ---- edge-preserving smoother of the disparity (disparity_smooth.hip) -----------------------------------------------------------------
static int check_disparity_smooth(ModContext *c, const ModDisparitySmooth &f) {
  if (f.window == 0 && f.min_members == 0 && f.tol == 0.0f && f.reserved == 0) return MOD_OK;   // all zero: off, what the getter returns for it
  if (f.window != 3 && f.window != 5 && f.window != 7) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity smooth window must be 3, 5 or 7");
  if (!(f.tol >= 0.0f) || f.tol > FLT_MAX) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity smooth tol must be finite and >= 0");
  if (f.min_members < 1 || f.min_members > f.window * f.window) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity smooth min_members must be in 1..window^2");
  if (f.reserved != 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity smooth reserved field must be 0");
  return MOD_OK;
}

// the estimator's plane in front of the smoother, for a group of `frames` frames (grow-only; host_sgm.hip)
int ensure_disparity_smooth_scratch(ModContext *c, int frames) {
  Buffers::Sgm &b = c->b.sgm;
  if (b.unsmoothed_frames >= frames) return MOD_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  DevPtr<float> plane;
  HIP_TRY(c, dalloc(plane, (size_t)frames * c->maxN));
  b.unsmoothed = std::move(plane);          // (swaps: the old plane is released with the local)
  b.unsmoothed_frames = frames;
  return MOD_OK;
}

// ---- occlusion hole fill of the disparity (disparity_fill.hip) -------------------------------------------------------------------------
static int check_disparity_fill(ModContext *c, const ModDisparityFill &f) {
  if (f.reach < 0 || f.reach > 256) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity fill reach must be in 0..256");
  if (f.reach == 0) return MOD_OK;          // off: the other fields have no range to lie in and are not looked at
  if (f.directions != 2 && f.directions != 4 && f.directions != 8) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity fill directions must be 2, 4 or 8");
  if (f.mode != MOD_DISPARITY_FILL_MIN && f.mode != MOD_DISPARITY_FILL_SECOND && f.mode != MOD_DISPARITY_FILL_MEDIAN)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity fill mode must be MOD_DISPARITY_FILL_MIN, _SECOND or _MEDIAN");
  if (f.min_found < 1 || f.min_found > f.directions) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity fill min_found must be in 1..directions");
  return MOD_OK;
}

// the estimator's plane in front of the fill, for a group of `frames` frames (grow-only; host_sgm.hip)
int ensure_disparity_fill_scratch(ModContext *c, int frames) {
  Buffers::Sgm &b = c->b.sgm;
  if (b.unfilled_frames >= frames) return MOD_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  DevPtr<float> plane;
  HIP_TRY(c, dalloc(plane, (size_t)frames * c->maxN));
  b.unfilled = std::move(plane);            // (swaps: the old plane is released with the local)
  b.unfilled_frames = frames;
  return MOD_OK;
}

// ---- what the texture and the min-eigenvalue kernel share ----------------------------------------------------------------------
// window and cap: what either kernel needs; threshold and apply / reserved: what the rule, the estimators and the setter need
static int check_window_cap(ModContext *c, const char *noun, int window, int cap) {
  if (window < 3 || window > 15 || window % 2 == 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, std::string(noun) + " window must be odd and in 3..15");
  if (cap < 1 || cap > 255) return fail(c, MOD_ERR_INVALID_ARGUMENT, std::string(noun) + " cap must be in 1..255");
  return MOD_OK;
}

// ---- texture filter (texture.hip) ---------------------------------------------------------------------------------------------
constexpr int kTextureMax = 225 * 255;   // 57375: a 15 x 15 window of differences capped at 255

static int check_texture_filter(ModContext *c, const ModTextureFilter &f) {
  if (f.threshold < 0 || f.threshold > kTextureMax) return fail(c, MOD_ERR_INVALID_ARGUMENT, "texture threshold must be in 0..57375");
  if (int rc = check_window_cap(c, "texture", f.window, f.cap)) return rc;
  if (f.apply < 1 || f.apply > (MOD_TEXTURE_DISPARITY | MOD_TEXTURE_FLOW))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "texture apply must be MOD_TEXTURE_DISPARITY, MOD_TEXTURE_FLOW or both");
  return MOD_OK;
}

// ---- min-eigenvalue filter of the flow (corner.hip) -----------------------------------------------------------------------------
static int check_corner_filter(ModContext *c, const ModCornerFilter &f) {
  if (f.threshold < 0 || f.threshold > MOD_CORNER_MAX) return fail(c, MOD_ERR_INVALID_ARGUMENT, "corner threshold must be in 0..14630625");
  if (int rc = check_window_cap(c, "corner", f.window, f.cap)) return rc;
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

// ---- disparity-gated hole fill of the flow (flow_fill.hip) -------------------------------------------------------------------------
static int check_flow_fill(ModContext *c, const ModFlowFill &f) {
  if (f.window != 0 && f.window != 3 && f.window != 5 && f.window != 7) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow fill window must be 0, 3, 5 or 7");
  if (f.window != 0 && (f.min_valid < 1 || f.min_valid > f.window * f.window - 1)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow fill min_valid must be in 1..window^2 - 1");
  // (window 0, off: min_valid has no range to lie in and is not looked at)
  if (!(f.tol_abs >= 0.0f && f.tol_abs <= FLT_MAX) || !(f.tol_rel >= 0.0f && f.tol_rel <= FLT_MAX))   // a NaN fails both comparisons
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow fill tolerances must be finite and >= 0");
  if (f.reserved[0] != 0 || f.reserved[1] != 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow fill reserved must be 0");
  return MOD_OK;
}

extern "C" {

// ---- the seven settings -----------------------------------------------------------------------------------------------------
int mod_set_disparity_filters(ModContext *c, const ModDisparityFilters *f) { return set_option(c, &EstimatorOptions::disparity_filters, f, check_disparity_filters); }
int mod_get_disparity_filters(const ModContext *c, ModDisparityFilters *f) { return get_option(c, &EstimatorOptions::disparity_filters, f); }
int mod_set_disparity_smooth(ModContext *c, const ModDisparitySmooth *f) { return set_option(c, &EstimatorOptions::disparity_smooth, f, check_disparity_smooth); }
int mod_get_disparity_smooth(const ModContext *c, ModDisparitySmooth *f) { return get_option(c, &EstimatorOptions::disparity_smooth, f); }
int mod_set_disparity_fill(ModContext *c, const ModDisparityFill *f) { return set_option(c, &EstimatorOptions::disparity_fill, f, check_disparity_fill); }
int mod_get_disparity_fill(const ModContext *c, ModDisparityFill *f) { return get_option(c, &EstimatorOptions::disparity_fill, f); }
int mod_set_texture_filter(ModContext *c, const ModTextureFilter *f) { return set_option(c, &EstimatorOptions::texture_filter, f, check_texture_filter); }
int mod_get_texture_filter(const ModContext *c, ModTextureFilter *f) { return get_option(c, &EstimatorOptions::texture_filter, f); }
int mod_set_flow_corner_filter(ModContext *c, const ModCornerFilter *f) { return set_option(c, &EstimatorOptions::flow_corner_filter, f, check_corner_filter); }
int mod_get_flow_corner_filter(const ModContext *c, ModCornerFilter *f) { return get_option(c, &EstimatorOptions::flow_corner_filter, f); }
int mod_set_flow_median(ModContext *c, const ModFlowMedian *f) { return set_option(c, &EstimatorOptions::flow_median, f, check_flow_median); }
int mod_get_flow_median(const ModContext *c, ModFlowMedian *f) { return get_option(c, &EstimatorOptions::flow_median, f); }
int mod_set_flow_fill(ModContext *c, const ModFlowFill *f) { return set_option(c, &EstimatorOptions::flow_fill, f, check_flow_fill); }
int mod_get_flow_fill(const ModContext *c, ModFlowFill *f) { return get_option(c, &EstimatorOptions::flow_fill, f); }

// ---- the stand-alone calls (f == null: the setting in force) -------------------------------------------------------------------
int mod_disparity_speckle_dev(ModContext *c, int32_t frames, float *disparity, int32_t speckle_size, int32_t speckle_range) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!disparity) return MOD_SKIP_NO_DISPARITY_NOW;
  if ((rc = check_disparity_filters(c, ModDisparityFilters{0, speckle_size, speckle_range, 0}))) return rc;
  if (speckle_size == 0) return MOD_OK;
  if ((rc = ensure_speckle_scratch(c, c->cfg.max_frames))) return rc;
  launch_speckle(c->dc.W, c->dc.H, frames, c->cam.min_disparity, c->cam.min_disparity - 1.0f, speckle_size, speckle_range, disparity,
                 c->b.spk.parent, c->b.spk.size, c->b.dbg, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_disparity_smooth_dev(ModContext *c, int32_t frames, const float *disparity_in, const ModDisparitySmooth *f, float *disparity_out) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!disparity_in || !disparity_out) return MOD_SKIP_NO_DISPARITY_NOW;
  const ModDisparitySmooth m = f ? *f : c->opt.disparity_smooth;
  if ((rc = check_disparity_smooth(c, m))) return rc;
  if (m.window == 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity smooth window must be 3, 5 or 7 (0: nothing to do)");
  const uintptr_t a = (uintptr_t)disparity_in, b = (uintptr_t)disparity_out, bytes = (uintptr_t)frames * c->dc.W * c->dc.H * 4;
  if (a < b + bytes && b < a + bytes) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity smooth planes overlap: the smoother cannot run in place");
  if ((a | b) & 3) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity smooth planes must be 4-byte aligned");
  launch_disparity_smooth(c->dc.W, c->dc.H, frames, c->cam.min_disparity, m.window, m.tol, m.min_members, disparity_in, disparity_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_disparity_fill_dev(ModContext *c, int32_t frames, const float *disparity_in, const ModDisparityFill *f, float *disparity_out) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!disparity_in || !disparity_out) return MOD_SKIP_NO_DISPARITY_NOW;
  const ModDisparityFill m = f ? *f : c->opt.disparity_fill;
  if ((rc = check_disparity_fill(c, m))) return rc;
  if (m.reach == 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity fill reach 0: nothing to do");
  const uintptr_t a = (uintptr_t)disparity_in, b = (uintptr_t)disparity_out, bytes = (uintptr_t)frames * c->dc.W * c->dc.H * 4;
  if (a < b + bytes && b < a + bytes) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity fill planes overlap: the fill cannot run in place");
  launch_disparity_fill(c->dc.W, c->dc.H, frames, c->cam.min_disparity, m.reach, m.directions, m.mode, m.min_found, disparity_in, disparity_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_texture_dev(ModContext *c, int32_t frames, const uint8_t *grey, const ModTextureFilter *f, uint16_t *texture) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!grey || !texture) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null grey / texture plane");
  const ModTextureFilter t = f ? *f : c->opt.texture_filter;
  if ((rc = check_window_cap(c, "texture", t.window, t.cap))) return rc;
  launch_texture(c->dc.W, c->dc.H, frames, t.window, t.cap, 0, grey, texture, nullptr, 0.0f, nullptr, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_texture_reject_dev(ModContext *c, int32_t frames, const uint8_t *grey, const ModTextureFilter *f, float *disparity, float *flow) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!grey || (!disparity && !flow)) return MOD_SKIP_NO_DISPARITY_NOW;
  const ModTextureFilter t = f ? *f : c->opt.texture_filter;
  if ((rc = check_texture_filter(c, t))) return rc;
  if (t.threshold == 0) return MOD_OK;
  launch_texture(c->dc.W, c->dc.H, frames, t.window, t.cap, t.threshold, grey, nullptr, disparity, c->cam.min_disparity - 1.0f, flow, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_flow_corner_dev(ModContext *c, int32_t frames, const uint8_t *grey, const ModCornerFilter *f, uint32_t *strength) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!grey || !strength) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null grey / corner strength plane");
  const ModCornerFilter t = f ? *f : c->opt.flow_corner_filter;
  if ((rc = check_window_cap(c, "corner", t.window, t.cap))) return rc;
  launch_corner(c->dc.W, c->dc.H, frames, t.window, t.cap, 0, grey, strength, nullptr, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_flow_corner_reject_dev(ModContext *c, int32_t frames, const uint8_t *grey, const ModCornerFilter *f, float *flow) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!grey || !flow) return MOD_SKIP_NO_FLOW;
  const ModCornerFilter t = f ? *f : c->opt.flow_corner_filter;
  if ((rc = check_corner_filter(c, t))) return rc;
  if (t.threshold == 0) return MOD_OK;
  launch_corner(c->dc.W, c->dc.H, frames, t.window, t.cap, t.threshold, grey, nullptr, flow, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_flow_median_dev(ModContext *c, int32_t frames, const float *flow_in, const ModFlowMedian *f, float *flow_out) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!flow_in || !flow_out) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow median plane");
  const ModFlowMedian m = f ? *f : c->opt.flow_median;
  if ((rc = check_flow_median(c, m))) return rc;
  if (m.window == 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow median window 0: nothing to do");
  const uintptr_t a = (uintptr_t)flow_in, b = (uintptr_t)flow_out, bytes = (uintptr_t)frames * c->dc.W * c->dc.H * 8;
  if (a < b + bytes && b < a + bytes) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow median planes overlap: a stencil cannot run in place");
  launch_flow_median(c->dc.W, c->dc.H, frames, m.window, m.min_valid, flow_in, flow_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_flow_fill_dev(ModContext *c, int32_t frames, const float *flow_in, const float *disparity, const ModFlowFill *f, float *flow_out) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!flow_in || !disparity || !flow_out) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow fill plane");
  const ModFlowFill m = f ? *f : c->opt.flow_fill;
  if ((rc = check_flow_fill(c, m))) return rc;
  if (m.window == 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow fill window 0: nothing to do");
  const uintptr_t a = (uintptr_t)flow_in, b = (uintptr_t)flow_out, bytes = (uintptr_t)frames * c->dc.W * c->dc.H * 8;
  if (a < b + bytes && b < a + bytes) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow fill planes overlap: a stencil cannot run in place");
  launch_flow_fill(c->dc.W, c->dc.H, frames, m.window, m.min_valid, m.tol_abs, m.tol_rel, flow_in, disparity, flow_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

}  // extern "C"
