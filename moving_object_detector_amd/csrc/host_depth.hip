// host_depth.hip — the C ABI's depth input, host side (no kernel): the settings (DepthOptions) and their set / get calls, the ray-table
// cache, the snapshot a call or submit takes of them (depth_plan), the one chain from device depth messages to disparity planes
// (run_depth_chain), what the stream stages of a host message (depth_stage), and the entry points around them.  The kernels live in
// depth.hip, depth_filter.hip, depth_spatial.hip, depth_temporal.hip, depth_decimate.hip.
#include "mod_context.h"

#include <algorithm>
#include <cmath>
#include <cstring>

static const char kLensNeedsRegistration[] = "a depth distortion needs a depth registration (aligned cameras: R = I, t = 0 and the depth intrinsics)";

// registered: a registration is in force (the whole message is scattered: no window, any message size)
static int check_depth_layout(ModContext *c, const ModDepthLayout &l, bool registered) {
  const int B = depth_bytes(l.encoding);
  if (!B) return fail(c, MOD_ERR_INVALID_ARGUMENT, "unknown depth encoding");
  if (l.width < 1 || l.height < 1 || l.width > MOD_MAX_WIDTH || l.height > MOD_MAX_WIDTH)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: width and height must be in 1..MOD_MAX_WIDTH");
  if ((int64_t)l.step < (int64_t)l.width * B || l.step % B) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: step must be a multiple of the sample size and >= width * sample size");
  if ((int64_t)l.step * l.height > INT32_MAX) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: step * height must be below 2^31");
  if (!std::isfinite(l.unit) || l.unit < 0.0f) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: unit must be 0 (the REP 118 default) or finite and positive");
  if (registered) {
    if (l.x0 || l.y0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: x0 and y0 must be 0 while a depth registration is set (the whole message is registered)");
  } else {
    const ModDepthDecimation &d = c->depth.decimation;   // the window taken from the message: (dx W) x (dy H)
    if (l.x0 < 0 || l.y0 < 0 || (int64_t)l.x0 + (int64_t)d.dx * c->dc.W > l.width || (int64_t)l.y0 + (int64_t)d.dy * c->dc.H > l.height)
      return fail(c, MOD_ERR_INVALID_ARGUMENT, d.dx * d.dy > 1 ? "the window of (dx W) x (dy H) samples that the depth decimation reads does not fit inside the depth image"
                                                               : "the camera-sized window does not fit inside the depth image");
  }
  return MOD_OK;
}

static ModDepthLayout default_depth_layout(const ModContext *c) {
  const int w = c->depth.decimation.dx * c->dc.W, h = c->depth.decimation.dy * c->dc.H;
  return ModDepthLayout{MOD_DEPTH_16UC1, w, h, 2 * w, 0, 0, 0.0f};
}
static ModDepthLayout layout_in_force(const ModContext *c) { return c->depth.has_layout ? c->depth.layout : default_depth_layout(c); }
static float depth_unit(const ModDepthLayout &l) { return l.unit != 0.0f ? l.unit : l.encoding == MOD_DEPTH_16UC1 ? 0.001f : 1.0f; }

int current_depth_layout(ModContext *c, ModDepthLayout *out) {
  *out = layout_in_force(c);
  return check_depth_layout(c, *out, c->depth.has_registration);   // the camera or the registration may have changed since the layout was set
}

// the layout a call works on: the given one, checked as `registered` says, or the context's
static int resolve_depth_layout(ModContext *c, const ModDepthLayout *given, bool registered, ModDepthLayout *l) {
  if (!given) return current_depth_layout(c, l);
  *l = *given;
  return check_depth_layout(c, *l, registered);
}

static depth_rays::Lens depth_lens_of(const ModContext *c) {
  depth_rays::Lens lens{};
  const ModDepthRegistration &r = c->depth.registration;
  for (int i = 0; i < 8; i++) lens.D[i] = c->depth.distortion.D[i];
  lens.fx = r.fx; lens.fy = r.fy; lens.cx = r.cx; lens.cy = r.cy;
  return lens;
}

// (callers have checked that a distortion and a registration are set and that lattice is one of the two)
static int ensure_depth_rays(ModContext *c, const ModDepthLayout &l, int lattice) {
  ModContext::DepthRayTable &t = c->depth_rays[lattice];
  const depth_rays::Lens lens = depth_lens_of(c);
  if (t.valid && t.width == l.width && t.height == l.height && !memcmp(&t.lens, &lens, sizeof lens)) return MOD_OK;
  if (t.valid && c->pipe.in_flight > 0)   // (a table never built has no reader)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the depth ray table must be rebuilt while frames are in flight: collect every ticket first");
  const int cols = l.width + lattice, rows = l.height + lattice;   // corners: one more per axis
  const size_t need = (size_t)cols * rows;
  t.valid = false;
  if (t.entries < need) {          // the old table's readers are on the context's stream
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    t.rays.reset(); t.entries = 0;
    HIP_TRY(c, dalloc(t.rays, need));
    t.entries = need;
  }
  // No wait: every reader of the old table (the registration kernels, mod_depth_rays_host's copy) and k_depth_rays are enqueued on
  // the context's stream, in program order.
  HIP_TRY(c, launch_depth_rays(lens, lattice == MOD_DEPTH_RAYS_CORNERS ? -0.5 : 0.0, cols, rows, t.rays, c->stream));
  t.lens = lens; t.width = l.width; t.height = l.height;
  t.valid = true;
  return MOD_OK;
}

static bool depth_decimation_on(const ModDepthDecimation &d) { return d.dx * d.dy > 1; }

int depth_plan(ModContext *c, const ModDepthLayout &l, bool own_input, DepthPlan *p) {
  const DepthOptions &o = c->depth;
  *p = DepthPlan{l, depth_unit(l), o.has_registration, DepthRegArgs{}, o.splat, DepthRayTables{nullptr, nullptr}, o.filter, o.spatial, o.temporal, o.decimation, 0, 0, own_input};
  if (p->registered && depth_decimation_on(o.decimation))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth decimation does not run under a depth registration (the scatter already lands the message in the camera's size): turn one of them off");
  if (p->registered) {
    const ModDepthRegistration &r = o.registration;
    DepthRegArgs &g = p->reg;
    g.fxd = r.fx; g.fyd = r.fy; g.cxd = r.cx; g.cyd = r.cy;
    for (int i = 0; i < 9; i++) g.R[i] = r.R[i];
    for (int i = 0; i < 3; i++) g.t[i] = r.t[i];
    g.fx = c->cam.fx; g.fy = c->cam.fy; g.cx = c->cam.cx; g.cy = c->cam.cy; g.Tx = c->cam.Tx; g.Ty = c->cam.Ty;
  }
  if (!o.has_distortion) return MOD_OK;
  if (!p->registered) return fail(c, MOD_ERR_INVALID_ARGUMENT, kLensNeedsRegistration);
  if (int rc = ensure_depth_rays(c, l, MOD_DEPTH_RAYS_CENTRES)) return rc;
  if (int rc = p->splat ? ensure_depth_rays(c, l, MOD_DEPTH_RAYS_CORNERS) : MOD_OK) return rc;
  p->rays.centres = c->depth_rays[MOD_DEPTH_RAYS_CENTRES].rays;
  p->rays.corners = p->splat ? c->depth_rays[MOD_DEPTH_RAYS_CORNERS].rays.get() : nullptr;
  return MOD_OK;
}

// a distortion is set, tickets are outstanding and a table in use was built for other intrinsics (r) / another message size (l)
static bool rebuilds_depth_rays(const ModContext *c, const ModDepthRegistration *r, const ModDepthLayout *l) {
  if (!c->depth.has_distortion || c->pipe.in_flight <= 0) return false;
  for (const ModContext::DepthRayTable &t : c->depth_rays) {
    if (!t.valid) continue;
    if (r && (t.lens.fx != r->fx || t.lens.fy != r->fy || t.lens.cx != r->cx || t.lens.cy != r->cy)) return true;
    if (l && (t.width != l->width || t.height != l->height)) return true;
  }
  return false;
}

static bool depth_filter_on(const ModDepthFilter &f) { return f.z_min != 0.0f || f.z_max != 0.0f || f.window != 0; }
static bool depth_temporal_on(const ModDepthTemporal &t) { return t.alpha != 0.0f; }
static bool depth_spatial_on(const ModDepthSpatial &s) { return s.window != 0; }

// null: valid, else what is wrong with it
static const char *check_depth_filter(const ModDepthFilter &f) {
  for (const float v : {f.z_min, f.z_max, f.tol_abs, f.tol_rel})
    if (!std::isfinite(v) || v < 0.0f) return "depth filter: z_min, z_max, tol_abs and tol_rel must be finite and >= 0";
  if (f.z_max != 0.0f && f.z_max < f.z_min) return "depth filter: z_max must be 0 (unbounded) or >= z_min";
  if (f.window != 0 && f.window != 3 && f.window != 5) return "depth filter: window must be 0 (off), 3 or 5";
  if (f.window != 0 && (f.min_support < 1 || f.min_support > f.window * f.window - 1)) return "depth filter: min_support must be in 1 .. window * window - 1";
  if (f.reserved[0] || f.reserved[1]) return "depth filter: reserved must be 0";
  return nullptr;
}

// null: valid, else what is wrong with it
static const char *check_depth_spatial(const ModDepthSpatial &s) {
  if (s.window != 0 && s.window != 3 && s.window != 5 && s.window != 7) return "depth spatial: window must be 0 (off), 3, 5 or 7";
  if (s.smooth != 0 && s.smooth != 1) return "depth spatial: smooth must be 0 or 1";
  if (s.fill_min < 0 || s.fill_min > std::max(s.window * s.window - 1, 0)) return "depth spatial: fill_min must be in 0 .. window * window - 1";
  if (s.window != 0 && !s.smooth && !s.fill_min) return "depth spatial: a window needs smooth or fill_min";
  for (const float v : {s.tol_abs, s.tol_rel})
    if (!std::isfinite(v) || v < 0.0f) return "depth spatial: tol_abs and tol_rel must be finite and >= 0";
  for (const int32_t v : s.reserved) if (v) return "depth spatial: reserved must be 0";
  return nullptr;
}

// null: valid, else what is wrong with it
static const char *check_depth_temporal(const ModDepthTemporal &t) {
  if (!(t.alpha >= 0.0f && t.alpha <= 1.0f)) return "depth temporal filter: alpha must be 0 (off) or in (0, 1]";
  for (const float v : {t.delta_abs, t.delta_rel})
    if (!std::isfinite(v) || v < 0.0f) return "depth temporal filter: delta_abs and delta_rel must be finite and >= 0";
  if (t.hold < 0 || t.hold > 254) return "depth temporal filter: hold must be in 0 .. 254";
  for (const int32_t v : t.reserved) if (v) return "depth temporal filter: reserved must be 0";
  return nullptr;
}

// null: valid, else what is wrong with it
static const char *check_depth_decimation(const ModDepthDecimation &d) {
  if (d.dx < 1 || d.dx > 4 || d.dy < 1 || d.dy > 4) return "depth decimation: dx and dy must be in 1..4";
  if (d.mode < MOD_DEPTH_DECIMATE_MEDIAN || d.mode > MOD_DEPTH_DECIMATE_NEAREST) return "depth decimation: mode must be one of MOD_DEPTH_DECIMATE_*";
  if (d.min_valid < 0 || d.min_valid > d.dx * d.dy) return "depth decimation: min_valid must be in 0 .. dx * dy";
  for (const float v : {d.tol_abs, d.tol_rel})
    if (!std::isfinite(v) || v < 0.0f) return "depth decimation: tol_abs and tol_rel must be finite and >= 0";
  for (const int32_t v : d.reserved) if (v) return "depth decimation: reserved must be 0";
  return nullptr;
}

// the context's state planes for messages of `l` whose origin in the camera's message is (ox, oy): grown where they are too small,
// and emptied where the geometry differs from the last launch's
static int context_temporal_state(ModContext *c, const ModDepthLayout &l, int ox, int oy) {
  ModContext::DepthTemporalState &st = c->depth_tstate;
  const float unit = depth_unit(l);
  const size_t n = (size_t)l.width * l.height;
  if (st.encoding != l.encoding || st.width != l.width || st.height != l.height || st.unit != unit || st.ox != ox || st.oy != oy ||
      st.s.bytes < 4 * n || st.age.bytes < n)   // (new planes hold nothing)
    forget_depth_history(c);
  st.encoding = l.encoding; st.width = l.width; st.height = l.height; st.unit = unit; st.ox = ox; st.oy = oy;
  if (int rc = ensure_stage_bytes(c, st.s, 4 * n)) return rc;
  return ensure_stage_bytes(c, st.age, n);
}

int run_depth_chain(ModContext *c, int frames, const void *depth, const DepthPlan &p, uint32_t *zbuf, float *disparity) {
  const ModDepthLayout &l = p.lay;
  const size_t bytes = (size_t)frames * l.step * l.height;
  bool own = p.own_input;             // `depth` is the library's: the slot's stage, or from the first stage that runs on the scratch
  if (depth_filter_on(p.filter)) {    // the whole messages: samples outside the window support
    if (int rc = ensure_stage_bytes(c, c->depth_filtered, bytes)) return rc;
    launch_depth_filter(l.encoding, l.width, l.height, frames, depth, l.step, p.unit, p.filter, c->depth_filtered.buf, c->stream);
    HIP_TRY(c, hipGetLastError());
    depth = c->depth_filtered.buf; own = true;
  }
  if (depth_spatial_on(p.spatial)) {  // the whole messages too, and never in place: it reads neighbours
    ModContext::RawStage &to = depth == c->depth_filtered.buf.get() ? c->depth_smoothed : c->depth_filtered;
    if (int rc = ensure_stage_bytes(c, to, bytes)) return rc;
    launch_depth_spatial(l.encoding, l.width, l.height, frames, depth, l.step, p.unit, p.spatial, to.buf, c->stream);
    HIP_TRY(c, hipGetLastError());
    depth = to.buf; own = true;
  }
  if (depth_temporal_on(p.temporal)) {
    if (int rc = own ? MOD_OK : ensure_stage_bytes(c, c->depth_filtered, bytes)) return rc;
    void *dst = own ? const_cast<void *>(depth) : c->depth_filtered.buf.get();   // in place, but never into a caller's input
    if (int rc = context_temporal_state(c, l, p.ox, p.oy)) return rc;
    ModContext::DepthTemporalState &st = c->depth_tstate;
    launch_depth_temporal(l.encoding, l.width, l.height, frames, depth, l.step, p.unit, p.temporal, st.fresh, reinterpret_cast<float *>(st.s.buf.get()),
                          st.age.buf, dst, c->stream);
    HIP_TRY(c, hipGetLastError());
    st.fresh = false;
    depth = dst;
  }
  const float invalid = c->dc.dmin - 1.0f;
  if (depth_decimation_on(p.decimation)) {   // (never registered: depth_plan) the window's blocks -> packed W x H messages, read at origin 0
    const int B = depth_bytes(l.encoding), W = c->dc.W, H = c->dc.H;
    if (int rc = ensure_stage_bytes(c, c->depth_decimated, (size_t)frames * W * H * B)) return rc;
    launch_depth_decimate(l.encoding, W, H, frames, depth, (size_t)l.step * l.height, l.step, l.x0, l.y0, p.unit, p.decimation, c->depth_decimated.buf, c->stream);
    HIP_TRY(c, hipGetLastError());
    launch_depth_to_disparity(l.encoding, W, H, frames, c->depth_decimated.buf, (size_t)W * B * H, W * B, 0, 0, p.unit, c->dc.fT, invalid, disparity, c->stream);
    HIP_TRY(c, hipGetLastError());
    return MOD_OK;
  }
  if (p.registered)
    HIP_TRY(c, launch_depth_register(l.encoding, c->dc.W, c->dc.H, frames, depth, l.width, l.height, l.step, p.unit, p.reg, p.splat, p.rays, c->dc.fT, invalid,
                                     zbuf, disparity, c->stream));
  else
    launch_depth_to_disparity(l.encoding, c->dc.W, c->dc.H, frames, depth, (size_t)l.step * l.height, l.step, l.x0, l.y0, p.unit, c->dc.fT, invalid,
                              disparity, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

DepthStage depth_stage(const ModContext *c, const DepthPlan &p) {
  const ModDepthLayout &l = p.lay;
  if (p.registered) return DepthStage{0, 0, 1, l.step, l.height, l};
  const int B = depth_bytes(l.encoding), W = p.decimation.dx * c->dc.W, H = p.decimation.dy * c->dc.H, R = p.filter.window / 2 + p.spatial.window / 2;
  const int ax = std::min(l.x0, R), ay = std::min(l.y0, R);                                     // the apron in front of the window ...
  const int bx = std::min(l.width - (l.x0 + W), R), by = std::min(l.height - (l.y0 + H), R);    // ... and behind it
  const int w = W + ax + bx, h = H + ay + by;
  return DepthStage{l.x0 - ax, l.y0 - ay, B, w, h, ModDepthLayout{l.encoding, w, h, w * B, ax, ay, l.unit}};
}

// The beginning of the three stand-alone stage calls: *l is the layout they work on, `layout` or the one in force, with the window dropped
// (the whole messages are filtered, whatever window a path reads of them)
static int stage_call_layout(ModContext *c, int32_t frames, const ModDepthLayout *layout, ModDepthLayout *l) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (frames < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "frames must be >= 1");
  if (frames > c->cfg.max_frames) return fail(c, MOD_ERR_CAPACITY, "frames exceeds ModConfig.max_frames");
  if (int rc = layout ? MOD_OK : need_camera(c)) return rc;
  *l = layout ? *layout : layout_in_force(c);
  l->x0 = l->y0 = 0;
  return check_depth_layout(c, *l, true);
}

extern "C" {

int mod_set_depth_temporal(ModContext *c, const ModDepthTemporal *t) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (const char *why = t ? check_depth_temporal(*t) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, why);
  c->depth.temporal = t && depth_temporal_on(*t) ? *t : ModDepthTemporal{};
  forget_depth_history(c);          // every successful call does
  return MOD_OK;
}

int mod_get_depth_temporal(const ModContext *c, ModDepthTemporal *t) {
  if (!c || !t) return MOD_ERR_INVALID_ARGUMENT;
  *t = c->depth.temporal;
  return MOD_OK;
}

int mod_reset_depth_temporal(ModContext *c) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  forget_depth_history(c);
  return MOD_OK;
}

int mod_depth_temporal_dev(ModContext *c, int32_t frames, const void *depth_in, const ModDepthLayout *layout, const ModDepthTemporal *filter,
                           float *state_s, uint8_t *state_age, void *depth_out) {
  ModDepthLayout l;
  if (int rc = stage_call_layout(c, frames, layout, &l)) return rc;
  if (const char *why = filter ? check_depth_temporal(*filter) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, why);
  if (!state_s != !state_age) return fail(c, MOD_ERR_INVALID_ARGUMENT, "state_s and state_age must both be given or both be NULL (the context's state)");
  if (!depth_in) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!depth_out) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null depth_out");
  if ((uintptr_t)depth_in % depth_bytes(l.encoding) || (uintptr_t)depth_out % depth_bytes(l.encoding) || (uintptr_t)state_s % 4)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth_in and depth_out must be aligned to the sample size and state_s to 4 bytes");
  const ModDepthTemporal t = filter ? *filter : c->depth.temporal;
  if (!depth_temporal_on(t)) {      // off: a copy; no state is touched
    if (depth_out != depth_in) HIP_TRY(c, hipMemcpyAsync(depth_out, depth_in, (size_t)frames * l.step * l.height, hipMemcpyDeviceToDevice, c->stream));
    return MOD_OK;
  }
  const bool own = !state_s;
  bool fresh = false;
  if (own) {
    if (int rc = context_temporal_state(c, l, 0, 0)) return rc;
    state_s = reinterpret_cast<float *>(c->depth_tstate.s.buf.get());
    state_age = c->depth_tstate.age.buf;
    fresh = c->depth_tstate.fresh;
  }
  launch_depth_temporal(l.encoding, l.width, l.height, frames, depth_in, l.step, depth_unit(l), t, fresh, state_s, state_age, depth_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  if (own) c->depth_tstate.fresh = false;
  return MOD_OK;
}

int mod_set_depth_spatial(ModContext *c, const ModDepthSpatial *s) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (const char *why = s ? check_depth_spatial(*s) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, why);
  c->depth.spatial = s && depth_spatial_on(*s) ? *s : ModDepthSpatial{};
  return MOD_OK;
}

int mod_get_depth_spatial(const ModContext *c, ModDepthSpatial *s) {
  if (!c || !s) return MOD_ERR_INVALID_ARGUMENT;
  *s = c->depth.spatial;
  return MOD_OK;
}

int mod_depth_spatial_dev(ModContext *c, int32_t frames, const void *depth_in, const ModDepthLayout *layout, const ModDepthSpatial *spatial, void *depth_out) {
  ModDepthLayout l;
  if (int rc = stage_call_layout(c, frames, layout, &l)) return rc;
  if (const char *why = spatial ? check_depth_spatial(*spatial) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, why);
  if (!depth_in) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!depth_out) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null depth_out");
  if (depth_out == depth_in) return fail(c, MOD_ERR_INVALID_ARGUMENT, "the depth spatial stage does not work in place");
  if ((uintptr_t)depth_in % depth_bytes(l.encoding) || (uintptr_t)depth_out % depth_bytes(l.encoding))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth_in and depth_out must be aligned to the sample size");
  const ModDepthSpatial s = spatial ? *spatial : c->depth.spatial;
  if (!depth_spatial_on(s)) {       // off: a copy
    HIP_TRY(c, hipMemcpyAsync(depth_out, depth_in, (size_t)frames * l.step * l.height, hipMemcpyDeviceToDevice, c->stream));
    return MOD_OK;
  }
  launch_depth_spatial(l.encoding, l.width, l.height, frames, depth_in, l.step, depth_unit(l), s, depth_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_depth_decimation(ModContext *c, const ModDepthDecimation *d) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (const char *why = d ? check_depth_decimation(*d) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, why);
  c->depth.decimation = d && depth_decimation_on(*d) ? *d : DepthOptions{}.decimation;
  return MOD_OK;
}

int mod_get_depth_decimation(const ModContext *c, ModDepthDecimation *d) {
  if (!c || !d) return MOD_ERR_INVALID_ARGUMENT;
  *d = c->depth.decimation;
  return MOD_OK;
}

int mod_depth_decimate_dev(ModContext *c, int32_t frames, const void *depth_in, const ModDepthLayout *layout, const ModDepthDecimation *decimation,
                           void *depth_out) {
  ModDepthLayout l;
  if (int rc = stage_call_layout(c, frames, layout, &l)) return rc;   // (drops the window's origin: the message itself is checked) ...
  l.x0 = layout ? layout->x0 : layout_in_force(c).x0;                  // ... but this stage honours it: the blocks start there
  l.y0 = layout ? layout->y0 : layout_in_force(c).y0;
  if (const char *why = decimation ? check_depth_decimation(*decimation) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, why);
  const ModDepthDecimation d = decimation ? *decimation : c->depth.decimation;
  if (l.x0 < 0 || l.y0 < 0 || l.x0 >= l.width || l.y0 >= l.height) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth decimation: x0, y0 must lie inside the depth image");
  const int out_w = (l.width - l.x0) / d.dx, out_h = (l.height - l.y0) / d.dy;
  if (out_w < 1 || out_h < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth decimation: the message holds no whole block behind (x0, y0)");
  if (!depth_in) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!depth_out) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null depth_out");
  if (depth_out == depth_in) return fail(c, MOD_ERR_INVALID_ARGUMENT, "the depth decimation does not work in place");
  if ((uintptr_t)depth_in % depth_bytes(l.encoding) || (uintptr_t)depth_out % depth_bytes(l.encoding))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth_in and depth_out must be aligned to the sample size");
  launch_depth_decimate(l.encoding, out_w, out_h, frames, depth_in, (size_t)l.step * l.height, l.step, l.x0, l.y0, depth_unit(l), d, depth_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_depth_filter(ModContext *c, const ModDepthFilter *f) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (const char *why = f ? check_depth_filter(*f) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, why);
  c->depth.filter = f ? *f : ModDepthFilter{};
  return MOD_OK;
}

int mod_get_depth_filter(const ModContext *c, ModDepthFilter *f) {
  if (!c || !f) return MOD_ERR_INVALID_ARGUMENT;
  *f = c->depth.filter;
  return MOD_OK;
}

int mod_depth_filter_dev(ModContext *c, int32_t frames, const void *depth_in, const ModDepthLayout *layout, const ModDepthFilter *filter, void *depth_out) {
  ModDepthLayout l;
  if (int rc = stage_call_layout(c, frames, layout, &l)) return rc;
  if (const char *why = filter ? check_depth_filter(*filter) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, why);
  if (!depth_in) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!depth_out) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null depth_out");
  if (depth_out == depth_in) return fail(c, MOD_ERR_INVALID_ARGUMENT, "the depth filter does not work in place");
  if ((uintptr_t)depth_in % depth_bytes(l.encoding) || (uintptr_t)depth_out % depth_bytes(l.encoding))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth_in and depth_out must be aligned to the sample size");
  launch_depth_filter(l.encoding, l.width, l.height, frames, depth_in, l.step, depth_unit(l), filter ? *filter : c->depth.filter, depth_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_depth_layout(ModContext *c, const ModDepthLayout *l) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (int rc = need_camera(c)) return rc;
  const ModDepthLayout nl = l ? *l : default_depth_layout(c);
  if (int rc = check_depth_layout(c, nl, c->depth.has_registration)) return rc;
  if (rebuilds_depth_rays(c, nullptr, &nl))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "a depth layout of another message size would rebuild the depth ray tables while frames are in flight: collect every ticket first");
  if (l) c->depth.layout = *l;
  c->depth.has_layout = l != nullptr;
  return MOD_OK;
}

int mod_get_depth_layout(const ModContext *c, ModDepthLayout *l) {
  if (!c || !l) return MOD_ERR_INVALID_ARGUMENT;
  if (!c->has_cam) return MOD_ERR_NOT_CONFIGURED;
  *l = layout_in_force(c);
  return MOD_OK;
}

int mod_set_depth_registration(ModContext *c, const ModDepthRegistration *r) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (r) {
    for (const double v : {r->fx, r->fy, r->cx, r->cy}) if (!std::isfinite(v)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: non-finite intrinsics");
    for (const double v : r->R) if (!std::isfinite(v)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: non-finite entry in R");
    for (const double v : r->t) if (!std::isfinite(v)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: non-finite entry in t");
    if (r->fx <= 0.0 || r->fy <= 0.0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: the focal lengths must be positive");
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const double d = r->R[3 * i] * r->R[3 * j] + r->R[3 * i + 1] * r->R[3 * j + 1] + r->R[3 * i + 2] * r->R[3 * j + 2];
        if (std::fabs(d - (i == j ? 1.0 : 0.0)) > 1e-6)
          return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: R is not a rotation (R R^T differs from I by more than 1e-6)");
      }
    if (rebuilds_depth_rays(c, r, nullptr))
      return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: other intrinsics would rebuild the depth ray tables while frames are in flight: collect every ticket first");
    c->depth.registration = *r;
  }
  c->depth.has_registration = r != nullptr;
  return MOD_OK;
}

int mod_get_depth_registration(const ModContext *c, ModDepthRegistration *r, int32_t *enabled) {
  if (!c || !enabled) return MOD_ERR_INVALID_ARGUMENT;
  *enabled = c->depth.has_registration;
  if (c->depth.has_registration && r) *r = c->depth.registration;
  return MOD_OK;
}

int mod_depth_to_disparity_dev(ModContext *c, int32_t frames, const void *depth, const ModDepthLayout *layout, float *disparity) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (int rc = need_camera(c)) return rc;
  if (frames < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "frames must be >= 1");
  if (frames > c->cfg.max_frames) return fail(c, MOD_ERR_CAPACITY, "frames exceeds ModConfig.max_frames");
  ModDepthLayout l;
  if (int rc = resolve_depth_layout(c, layout, c->depth.has_registration, &l)) return rc;
  if (!depth) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!disparity) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null disparity planes");
  if ((uintptr_t)depth % depth_bytes(l.encoding) || (uintptr_t)disparity % 4)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth must be aligned to its sample size and disparity to 4 bytes");
  DepthPlan p;
  if (int rc = depth_plan(c, l, false, &p)) return rc;   // the messages are the caller's
  if (p.registered) HIP_TRY(c, dalloc(c->depth_zbuf, (size_t)c->cfg.max_frames * c->maxN));
  return run_depth_chain(c, frames, depth, p, c->depth_zbuf, disparity);
}

int mod_set_depth_splat(ModContext *c, int32_t on) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (on != 0 && on != 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth splat: on must be 0 or 1");
  c->depth.splat = on != 0;
  return MOD_OK;
}

int mod_get_depth_splat(const ModContext *c, int32_t *on) {
  if (!c || !on) return MOD_ERR_INVALID_ARGUMENT;
  *on = c->depth.splat;
  return MOD_OK;
}

int mod_set_depth_distortion(ModContext *c, const ModDepthDistortion *d) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (d)
    for (const double v : d->D) if (!std::isfinite(v)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth distortion: non-finite coefficient");
  if (c->depth.has_distortion && c->pipe.in_flight > 0)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the depth distortion cannot change while frames are in flight: collect every ticket first");
  if (d) c->depth.distortion = *d;
  c->depth.has_distortion = d != nullptr;   // part of each table's key: rebuilt at the next use, behind the context's stream
  return MOD_OK;
}

int mod_get_depth_distortion(const ModContext *c, ModDepthDistortion *d, int32_t *enabled) {
  if (!c || !enabled) return MOD_ERR_INVALID_ARGUMENT;
  *enabled = c->depth.has_distortion;
  if (c->depth.has_distortion && d) *d = c->depth.distortion;
  return MOD_OK;
}

int mod_depth_rays_host(ModContext *c, const ModDepthLayout *layout, int32_t lattice, double *rays) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (int rc = need_camera(c)) return rc;
  if (lattice != MOD_DEPTH_RAYS_CENTRES && lattice != MOD_DEPTH_RAYS_CORNERS)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "lattice must be MOD_DEPTH_RAYS_CENTRES or MOD_DEPTH_RAYS_CORNERS");
  if (!rays) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null rays");
  if (!c->depth.has_distortion) return fail(c, MOD_ERR_NOT_CONFIGURED, "no depth distortion is set");
  if (!c->depth.has_registration) return fail(c, MOD_ERR_INVALID_ARGUMENT, kLensNeedsRegistration);
  ModDepthLayout l;
  if (int rc = resolve_depth_layout(c, layout, true, &l)) return rc;
  if (int rc = ensure_depth_rays(c, l, lattice)) return rc;
  const size_t entries = (size_t)(l.width + lattice) * (l.height + lattice);
  HIP_TRY(c, hipMemcpyAsync(rays, c->depth_rays[lattice].rays, sizeof(double2) * entries, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}

}  // extern "C"
