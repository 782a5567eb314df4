// host_images.hip — the C ABI's image input, host side (no kernel): image layouts, side by side, the binning, the rectification and
// its map cache, and the one path on which the host images of host_api.hip's calls become grey on the device (ImageIngest:
// ingest_copy, then ingest_to_grey).  The kernels live in ingest.hip, bayer.hip, rectify.hip, binning.hip.  Depth images: host_depth.hip.
#include "mod_context.h"
#include "bayer_region.h"

#include <cmath>
#include <cstring>

// the full window of binning b fits the context's capacity (the stages and maps sized by maxN then hold it)
static int check_binning_capacity(ModContext *c, const ModImageBinning &b) {
  const Window w = full_window(c, b);
  return w.w > c->cfg.max_width || w.h > c->cfg.max_height
             ? fail(c, MOD_ERR_CAPACITY, "image binning: bx * width / by * height of the camera exceed ModConfig.max_width / max_height") : MOD_OK;
}

// panes: the message holds both eyes side by side (width is a pane's, step the whole row's).  The window is the one of the binning in force.
static int check_layout(ModContext *c, const ModImageLayout &l, bool panes) {
  if (int rc = check_binning_capacity(c, c->binning)) return rc;
  const Window win = full_window(c, c->binning);
  const int C = image_channels(l.encoding);
  if (!C) return fail(c, MOD_ERR_INVALID_ARGUMENT, "unknown image encoding");
  if (l.width < 1 || l.height < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "image size must be positive");
  if (is_bayer(l.encoding) && (l.width < 3 || l.height < 3))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "a Bayer image must be at least 3 x 3 (a pixel of its frame copies an interior one)");
  if ((int64_t)l.step < (int64_t)l.width * C) return fail(c, MOD_ERR_INVALID_ARGUMENT, "step is smaller than width * channels");
  if (panes && (int64_t)l.step < 2 * (int64_t)l.width * C)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "side by side: step is smaller than 2 * width * channels (width is one eye's)");
  if (l.x0 < 0 || l.y0 < 0 || (int64_t)l.x0 + win.w > l.width || (int64_t)l.y0 + win.h > l.height)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the camera-sized window (with a binning: bx, by times the camera's size) does not fit inside the image");
  return MOD_OK;
}

static ModImageLayout default_layout(const ModContext *c) {
  const Window win = full_window(c, c->binning);
  return ModImageLayout{MOD_ENCODING_MONO8, win.w, win.h, win.w, 0, 0};
}

int current_layout(ModContext *c, ModImageLayout *out) {
  *out = c->has_layout ? c->layout : default_layout(c);
  if (!c->has_layout && !c->side_by_side) return binned(c->binning) ? check_binning_capacity(c, c->binning) : MOD_OK;
  return check_layout(c, *out, c->side_by_side);   // the camera may have changed since the layout was set
}

// the layout a call works on: the given one, or the context's
static int resolve_layout(ModContext *c, const ModImageLayout *given, ModImageLayout *l) {
  if (!given) return current_layout(c, l);
  *l = *given;
  return check_layout(c, *l, c->side_by_side);
}

// (callers have checked that a rectification is set and that eye is one of the two)
int ensure_rectify_map(ModContext *c, int eye, const ModImageLayout &l) {
  const ModRectifyCamera &cam = c->rect.cam[eye];
  if (l.width != cam.width || l.height != cam.height)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the image layout's width / height differ from the rectification's");
  ModContext::Rectify::Map &m = c->rect.map[eye];
  const Window win = full_window(c, c->binning);   // (the layout was checked against it: it fits maxN)
  const int W = win.w, H = win.h;
  const int32_t model = c->rect.model;
  if (m.valid && m.width == l.width && m.height == l.height && m.x0 == l.x0 && m.y0 == l.y0 && m.W == W && m.H == H && m.model == model) return MOD_OK;
  if (c->pipe.in_flight > 0)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the rectification map must be rebuilt while frames are in flight: collect every ticket first");
  HIP_TRY(c, dalloc(m.q, 2 * c->maxN));
  m.valid = false;
  // No wait: every reader of the old map (k_rectify, mod_rectify_map_host's copy) and k_rectify_map are enqueued on the context's
  // stream, in program order; kernels of calls and of frames that ended at a guard read the old map in front of this launch.
  HIP_TRY(c, launch_rectify_map(model, cam, l.x0, l.y0, W, H, m.q, c->stream));
  m.width = l.width; m.height = l.height; m.x0 = l.x0; m.y0 = l.y0; m.W = W; m.H = H; m.model = model;
  m.valid = true;
  return MOD_OK;
}

int ensure_stage_bytes(ModContext *c, ModContext::RawStage &r, size_t need) {
  if (r.bytes >= need) return MOD_OK;
  for (hipStream_t q : {c->stream, (hipStream_t)c->pipe.h2d}) if (q) HIP_TRY(c, hipStreamSynchronize(q));
  r.buf.reset(); r.bytes = 0;
  HIP_TRY(c, dalloc(r.buf, need));
  r.bytes = need;
  return MOD_OK;
}

int ensure_raw_stages(ModContext *c, const ImageIngest &in) {
  const ModImageLayout &l = in.lay;
  if (int rc = ensure_stage_bytes(c, *in.raw, 2 * (size_t)l.step * l.height)) return rc;
  return is_bayer(l.encoding) ? ensure_stage_bytes(c, *in.bayer_grey, 2 * (size_t)l.width * l.height) : MOD_OK;
}

int ensure_bin_stage(ModContext *c, const ImageIngest &in) {
  return binned(in.bin) ? ensure_stage_bytes(c, *in.bin_grey, 2 * full_window(c, in.bin).pixels()) : MOD_OK;
}

// Bayer under a rectification: `frames` whole messages at src (or their panes: src points at the pane, `pane` says which eye's) to
// the grey planes `grey` [frames][height][width], then k_rectify from those as mono8 through `map` (of window `win`) into mono; context's stream
static int rectify_bayer(ModContext *c, const ModImageLayout &l, Window win, int frames, const uint8_t *src, int pane, uint8_t *grey, const int32_t *map,
                  uint8_t *mono) {
  const size_t G = (size_t)l.width * l.height;
  launch_bayer_to_mono(l.width, l.height, frames, src, (size_t)l.step * l.height, l.step, l.width, l.height, 0, 0,
                       bayer_phase(l.encoding, pane == MOD_EYE_RIGHT ? l.width : 0, 0), grey, c->stream);
  launch_rectify(MOD_ENCODING_MONO8, win.w, win.h, frames, grey, G, G, l.width, l.width, l.height, map, mono, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

// ---- host images (mod_set_image_layout) --------------------------------------------------------------------------------
// (one copy when the window's rows are contiguous in the message, as in the default layout: the whole mono8 image; else a 2D copy)
hipError_t copy_window(const void *src, int32_t step, int32_t x0, int32_t y0, int bpp, int W, int H, void *dst, hipStream_t s) {
  const size_t row = (size_t)W * bpp;
  const uint8_t *o = static_cast<const uint8_t *>(src) + (size_t)y0 * step + (size_t)x0 * bpp;
  if ((size_t)step == row) return hipMemcpyAsync(dst, o, row * H, hipMemcpyHostToDevice, s);
  return hipMemcpy2DAsync(dst, row, o, (size_t)step, row, (size_t)H, hipMemcpyHostToDevice, s);
}

// bytes that hold two staged windows of any encoding: 4 bytes a pixel, or two Bayer regions (bayer_region.h: <= 6 N + 12 bytes while W H <= N)
size_t window_stage_bytes(const ModContext *c) { return 8 * c->maxN + 16; }
// the region of one host message (src: the message, or its pane) to dst on stream s, rows packed
static hipError_t copy_bayer_region(const ModImageLayout &l, const BayerRegion &g, const uint8_t *src, uint8_t *dst, hipStream_t s) {
  return hipMemcpy2DAsync(dst, (size_t)g.rw, src + (size_t)g.ay * l.step + g.ax, (size_t)l.step, (size_t)g.rw, (size_t)g.rh, hipMemcpyHostToDevice, s);
}
// ... and the grey of window `win` from it on the context's stream; right_pane: the message the region came from is a right pane
static void bayer_region_to_mono(ModContext *c, const ModImageLayout &l, Window win, const BayerRegion &g, bool right_pane, const uint8_t *staged,
                                 uint8_t *grey) {
  launch_bayer_to_mono(win.w, win.h, 1, staged, 0, g.rw, g.rw, g.rh, l.x0 - g.ax, l.y0 - g.ay,
                       bayer_phase(l.encoding, g.ax + (right_pane ? l.width : 0), g.ay), grey, c->stream);
}

int check_one_message(ModContext *c, const uint8_t *left, const uint8_t *right) {
  return right && right != left ? fail(c, MOD_ERR_INVALID_ARGUMENT, "side by side: right must be NULL or equal to left") : MOD_OK;
}

// k_rectify from the whole raw messages at `raw` on the context's stream, each message (or each pane of the one message) with the map of its eye.  A
// pane is a message of the pane's width that starts width * channels bytes into the row and ends with the message's last byte.
// Bayer messages are demosaiced whole into `bayer` first (room for two grey planes of the message's, or pane's, size).  grey1 null:
// the first message alone.  win: the window the maps were built for, and the size of grey0 / grey1.
static int rectify_messages(ModContext *c, const ModImageLayout &l, Window win, bool panes, const uint8_t *raw, int eye1, uint8_t *bayer,
                            uint8_t *grey0, uint8_t *grey1) {
  const size_t M = (size_t)l.step * l.height, at1 = panes ? pane_offset(l, MOD_EYE_RIGHT) : M;
  if (is_bayer(l.encoding)) {
    if (int rc = rectify_bayer(c, l, win, 1, raw, MOD_EYE_LEFT, bayer, c->rect.map[MOD_EYE_LEFT].q, grey0)) return rc;
    return !grey1 ? MOD_OK : rectify_bayer(c, l, win, 1, raw + at1, panes ? MOD_EYE_RIGHT : MOD_EYE_LEFT, bayer + (size_t)l.width * l.height, c->rect.map[eye1].q, grey1);
  }
  launch_rectify(l.encoding, win.w, win.h, 1, raw, M, M, l.step, l.width, l.height, c->rect.map[MOD_EYE_LEFT].q, grey0, c->stream);
  if (grey1) launch_rectify(l.encoding, win.w, win.h, 1, raw + at1, M, panes ? M - at1 : M, l.step, l.width, l.height, c->rect.map[eye1].q, grey1,
                            c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

// ---- the one ingest path (ImageIngest, mod_context.h) ----------------------------------------------------------------------
// What both halves know of `stage`: the window (the full one when binning), its bytes P (rows of P / win.h), for Bayer messages
// the region staged in the window's place, and where the second window / region starts
struct Staged { Window win; BayerRegion g; size_t P, at1; };
static Staged stage_plan(const ModContext *c, const ImageIngest &in) {
  const ModImageLayout &l = in.lay;
  const Window win = full_window(c, in.bin);
  const size_t P = win.pixels() * image_channels(l.encoding);
  if (!is_bayer(l.encoding)) return {win, BayerRegion{}, P, P};
  const BayerRegion g = bayer_region(l.width, l.height, l.x0, l.y0, win.w, win.h);
  return {win, g, P, (size_t)g.rw * g.rh};
}
// binning: the two full-window grey planes in in.bin_grey (the second null when the call has one image)
struct BinPlanes { uint8_t *g0, *g1; };
static BinPlanes bin_planes(const ImageIngest &in, Window win) { return {in.bin_grey->buf, in.grey1 ? in.bin_grey->buf + win.pixels() : nullptr}; }

int ingest_copy(ModContext *c, const ImageIngest &in, const uint8_t *img0, const uint8_t *img1, hipStream_t s) {
  const ModImageLayout &l = in.lay;
  if (in.rectify) {   // the whole raw messages, one after the other: a rectified window needs source pixels outside the window
    const size_t M = (size_t)l.step * l.height;
    HIP_TRY(c, hipMemcpyAsync(in.raw->buf, img0, M, hipMemcpyHostToDevice, s));
    // ONE message that holds both eyes side by side crosses once; img1 null (an RGB-D frame): one message, one eye
    if (!in.panes && img1) HIP_TRY(c, hipMemcpyAsync(in.raw->buf + M, img1, M, hipMemcpyHostToDevice, s));
    return MOD_OK;
  }
  if (in.panes) img1 = img0 + pane_offset(l, MOD_EYE_RIGHT);   // one window from each pane
  const Staged st = stage_plan(c, in);
  const uint8_t *const src[2] = {img0, img1};
  uint8_t *dst[2] = {in.grey0, in.grey1};
  if (in.windows_staged()) { dst[0] = in.stage; dst[1] = in.stage + st.at1; }
  else if (binned(in.bin)) { const BinPlanes b = bin_planes(in, st.win); dst[0] = b.g0; dst[1] = b.g1; }   // mono8: binned straight from the copy
  for (int k = 0; k < (in.grey1 ? 2 : 1); k++)
    HIP_TRY(c, is_bayer(l.encoding) ? copy_bayer_region(l, st.g, src[k], dst[k], s)
                                    : copy_window(src[k], l.step, l.x0, l.y0, image_channels(l.encoding), st.win.w, st.win.h, dst[k], s));
  return MOD_OK;
}

int ingest_to_grey(ModContext *c, const ImageIngest &in) {
  const ModImageLayout &l = in.lay;
  if (!in.staged()) return MOD_OK;
  const Staged st = stage_plan(c, in);
  // binning: the converters below write the full window into the bin stage's two planes, and k_bin_mono makes the grey images from those
  const BinPlanes full = binned(in.bin) ? bin_planes(in, st.win) : BinPlanes{in.grey0, in.grey1};
  if (in.rectify) {
    if (int rc = rectify_messages(c, l, st.win, in.panes, in.raw->buf, in.eye1, in.bayer_grey->buf, full.g0, full.g1)) return rc;
  } else if (is_bayer(l.encoding)) {      // image_proc's debayer and cv_bridge's conversion on the GPU
    bayer_region_to_mono(c, l, st.win, st.g, false, in.stage, full.g0);
    if (full.g1) bayer_region_to_mono(c, l, st.win, st.g, in.panes, in.stage + st.at1, full.g1);
  } else if (in.windows_staged()) {       // cv_bridge::toCvCopy(..., MONO8) (scene_flow_constructor.cpp:220-221) on the GPU
    const int W = st.win.w, H = st.win.h, step = (int)(st.P / H);
    const bool one = in.batch2 && full.g1 == full.g0 + (size_t)W * H;   // (else a launch each: nothing is written past grey0's image)
    launch_to_mono(l.encoding, W, H, one ? 2 : 1, in.stage, st.P, step, 0, 0, full.g0, c->stream);
    if (full.g1 && !one) launch_to_mono(l.encoding, W, H, 1, in.stage + st.at1, st.P, step, 0, 0, full.g1, c->stream);
  }                                       // (else mono8 windows on their way to k_bin_mono: ingest_copy has put them into the bin stage)
  if (binned(in.bin)) {                   // image_proc/crop_decimate on the GPU; the bin stage's planes are a full window apart
    const bool one = in.grey1 == in.grey0 + (size_t)c->dc.W * c->dc.H;
    launch_bin_mono(in.bin, c->dc.W, c->dc.H, one ? 2 : 1, full.g0, in.grey0, c->stream);
    if (in.grey1 && !one) launch_bin_mono(in.bin, c->dc.W, c->dc.H, 1, full.g1, in.grey1, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

extern "C" {

int mod_set_image_layout(ModContext *c, const ModImageLayout *l) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (int rc = need_camera(c)) return rc;
  if (int rc = check_layout(c, l ? *l : default_layout(c), c->side_by_side)) return rc;   // (the default holds no two panes: refused while side by side)
  if (l) c->layout = *l;
  c->has_layout = l != nullptr;
  return MOD_OK;
}

int mod_set_side_by_side(ModContext *c, int32_t on) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (on != 0 && on != 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "side by side must be 0 or 1");
  if (on && c->has_cam) {           // the layout in force must hold two panes (without a camera there is none yet: checked at call time)
    const ModImageLayout l = c->has_layout ? c->layout : default_layout(c);
    if (int rc = check_layout(c, l, true)) return rc;
  }
  c->side_by_side = on != 0;
  return MOD_OK;
}

int mod_get_side_by_side(const ModContext *c, int32_t *on) {
  if (!c || !on) return MOD_ERR_INVALID_ARGUMENT;
  *on = c->side_by_side;
  return MOD_OK;
}

int mod_get_image_layout(const ModContext *c, ModImageLayout *l) {
  if (!c || !l) return MOD_ERR_INVALID_ARGUMENT;
  if (!c->has_cam) return MOD_ERR_NOT_CONFIGURED;
  *l = c->has_layout ? c->layout : default_layout(c);
  return MOD_OK;
}

int mod_image_to_mono_dev(ModContext *c, int32_t frames, const uint8_t *src, const ModImageLayout *layout, uint8_t *mono) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (int rc = need_camera(c)) return rc;
  if (frames < 1 || frames > 65535) return fail(c, MOD_ERR_INVALID_ARGUMENT, "frames must be in 1..65535");
  if (!src) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!mono) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null grey planes");
  ModImageLayout l;
  if (int rc = resolve_layout(c, layout, &l)) return rc;
  const ModImageBinning bin = c->binning;
  const Window win = full_window(c, bin);
  uint8_t *full = mono;            // binning: the full window's grey planes in the context's bin stage, and k_bin_mono from those
  if (binned(bin)) {
    if (int rc = ensure_stage_bytes(c, c->bin_grey, (size_t)frames * win.pixels())) return rc;
    full = c->bin_grey.buf;
  }
  if (is_bayer(l.encoding))        // the region is the message (side by side: the pane src points at, with the pattern as it lies there)
    launch_bayer_to_mono(win.w, win.h, frames, src, (size_t)l.step * l.height, l.step, l.width, l.height, l.x0, l.y0,
                         bayer_phase(l.encoding, 0, 0), full, c->stream);
  else
    launch_to_mono(l.encoding, win.w, win.h, frames, src, (size_t)l.step * l.height, l.step, l.x0, l.y0, full, c->stream);
  if (binned(bin)) launch_bin_mono(bin, c->dc.W, c->dc.H, frames, full, mono, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_image_binning(ModContext *c, const ModImageBinning *b) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  const ModImageBinning off{1, 1, MOD_BIN_MEAN, 0};
  const ModImageBinning nb = b ? *b : off;
  if (nb.bx < 1 || nb.bx > 4 || nb.by < 1 || nb.by > 4) return fail(c, MOD_ERR_INVALID_ARGUMENT, "image binning: bx and by must be in 1..4");
  if (nb.mode != MOD_BIN_MEAN && nb.mode != MOD_BIN_NEAREST) return fail(c, MOD_ERR_INVALID_ARGUMENT, "image binning: mode must be MOD_BIN_MEAN or MOD_BIN_NEAREST");
  if (nb.reserved != 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "image binning: reserved must be 0");
  if (int rc = c->has_cam ? check_binning_capacity(c, nb) : MOD_OK) return rc;   // (without a camera: checked at call time)
  c->binning = nb;
  return MOD_OK;
}

int mod_get_image_binning(const ModContext *c, ModImageBinning *b) {
  if (!c || !b) return MOD_ERR_INVALID_ARGUMENT;
  *b = c->binning;
  return MOD_OK;
}

int mod_set_rectification(ModContext *c, const ModRectifyCamera *left, const ModRectifyCamera *right) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!left != !right) return fail(c, MOD_ERR_INVALID_ARGUMENT, "rectification: both eyes or neither");
  for (const ModRectifyCamera *cam : {left, right})
    if (const char *what = cam ? check_rectify_camera(*cam) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, what);
  for (const ModRectifyCamera *cam : {left, right})   // (the call that comes second checks the pair: model and coefficients)
    if (const char *what = cam ? check_distortion(c->rect.model, *cam) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, what);
  if (c->pipe.in_flight > 0)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the rectification cannot change while frames are in flight: collect every ticket first");
  c->rect.on = left != nullptr;
  if (left) { c->rect.cam[MOD_EYE_LEFT] = *left; c->rect.cam[MOD_EYE_RIGHT] = *right; }
  for (ModContext::Rectify::Map &m : c->rect.map) m.valid = false;   // rebuilt at the next use, behind the context's stream
  return MOD_OK;
}

int mod_get_rectification(const ModContext *c, ModRectifyCamera *left, ModRectifyCamera *right, int32_t *enabled) {
  if (!c || !enabled) return MOD_ERR_INVALID_ARGUMENT;
  *enabled = c->rect.on;
  if (c->rect.on && left) *left = c->rect.cam[MOD_EYE_LEFT];
  if (c->rect.on && right) *right = c->rect.cam[MOD_EYE_RIGHT];
  return MOD_OK;
}

int mod_set_distortion_model(ModContext *c, int32_t model) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (model != MOD_DISTORTION_RATIONAL && model != MOD_DISTORTION_EQUIDISTANT)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "distortion model must be MOD_DISTORTION_RATIONAL or MOD_DISTORTION_EQUIDISTANT");
  if (c->rect.on)
    for (const ModRectifyCamera &cam : c->rect.cam)
      if (const char *what = check_distortion(model, cam)) return fail(c, MOD_ERR_INVALID_ARGUMENT, what);
  if (c->pipe.in_flight > 0)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the distortion model cannot change while frames are in flight: collect every ticket first");
  c->rect.model = model;   // part of each map's key: both are rebuilt at the next use, behind the context's stream
  return MOD_OK;
}

int mod_get_distortion_model(const ModContext *c, int32_t *model) {
  if (!c || !model) return MOD_ERR_INVALID_ARGUMENT;
  *model = c->rect.model;
  return MOD_OK;
}

// the layout a rectifying call works on (the given one, or the context's) and the map of `eye` for its window
static int rectify_setup(ModContext *c, const ModImageLayout *layout, int32_t eye, ModImageLayout *l) {
  if (int rc = need_camera(c)) return rc;
  if (eye != MOD_EYE_LEFT && eye != MOD_EYE_RIGHT) return fail(c, MOD_ERR_INVALID_ARGUMENT, "eye must be MOD_EYE_LEFT or MOD_EYE_RIGHT");
  if (!c->rect.on) return fail(c, MOD_ERR_NOT_CONFIGURED, "no rectification is set");
  if (int rc = resolve_layout(c, layout, l)) return rc;
  return ensure_rectify_map(c, eye, *l);
}

int mod_rectify_dev(ModContext *c, int32_t frames, const uint8_t *src, const ModImageLayout *layout, int32_t eye, uint8_t *mono) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (frames < 1 || frames > 65535) return fail(c, MOD_ERR_INVALID_ARGUMENT, "frames must be in 1..65535");
  ModImageLayout l;
  if (int rc = rectify_setup(c, layout, eye, &l)) return rc;
  if (!src) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!mono) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null grey planes");
  const size_t M = (size_t)l.step * l.height, pane = c->side_by_side ? pane_offset(l, eye) : 0;   // side by side: eye selects the pane too
  const ModImageBinning bin = c->binning;
  const Window win = full_window(c, bin);   // (the map is this window's: rectify_setup)
  uint8_t *full = mono;            // binning: the full window's rectified planes in the context's bin stage, and k_bin_mono from those
  if (binned(bin)) {
    if (int rc = ensure_stage_bytes(c, c->bin_grey, (size_t)frames * win.pixels())) return rc;
    full = c->bin_grey.buf;
  }
  if (is_bayer(l.encoding)) {      // debayer, then rectify: the whole messages (or panes) to grey planes of the context's, k_rectify from those
    if (int rc = ensure_stage_bytes(c, c->bayer_grey, (size_t)frames * l.width * l.height)) return rc;
    if (int rc = rectify_bayer(c, l, win, frames, src + pane, c->side_by_side ? eye : MOD_EYE_LEFT, c->bayer_grey.buf, c->rect.map[eye].q, full)) return rc;
  } else {
    launch_rectify(l.encoding, win.w, win.h, frames, src + pane, M, M - pane, l.step, l.width, l.height, c->rect.map[eye].q, full, c->stream);
  }
  if (binned(bin)) launch_bin_mono(bin, c->dc.W, c->dc.H, frames, full, mono, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_rectify_map_host(ModContext *c, int32_t eye, const ModImageLayout *layout, int32_t *map_qxqy) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!map_qxqy) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null map");
  ModImageLayout l;
  if (int rc = rectify_setup(c, layout, eye, &l)) return rc;
  HIP_TRY(c, hipMemcpyAsync(map_qxqy, c->rect.map[eye].q, sizeof(int32_t) * 2 * full_window(c, c->binning).pixels(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}

}  // extern "C"
