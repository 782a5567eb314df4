// host_api.hip — the C ABI's host-pointer entry points: the single-frame *_host calls, which stage one frame through device buffers
// of the context, and the submit / collect stream with its pipe of slots, copy streams and ring of planes.  Host-side only; how a
// host image becomes grey on the device is host_images.hip's (ImageIngest), how a depth message becomes disparity host_depth.hip's (DepthPlan).
#include "mod_context.h"

#include <algorithm>
#include <cstring>

using Pipe = ModContext::Pipe;
static size_t pixels(const ModContext *c) { return (size_t)c->dc.W * c->dc.H; }

static int alloc_frame_buffers(ModContext *c, ModContext::FrameBuffers &b, int planes) {
  const size_t N = c->maxN;
  HIP_TRY(c, dalloc(b.dprev, N));
  // + 16 bytes: the synchronous calls stage their two windows in the staging's flow buffer, which must hold window_stage_bytes()
  // (two Bayer regions of a camera one pixel high outgrow 8 N); the pipe's slots share this allocator and do not need the extra
  HIP_TRY(c, dalloc(b.flow, 2 * N + 4));
  HIP_TRY(c, dalloc(b.planes, planes * N));
  if (!b.aos) HIP_TRY(c, hipMalloc(b.aos.put(), 32 * N));
  HIP_TRY(c, dalloc(b.labels, N));
  HIP_TRY(c, dalloc(b.nobj, 8));
  HIP_TRY(c, dalloc(b.objects, (size_t)c->max_objects));
  return MOD_OK;
}

static int ensure_host_staging(ModContext *c) {
  ModContext::HostStaging &h = c->staging;
  if (h.ready) return MOD_OK;
  HIP_TRY(c, dalloc(h.dnow, c->maxN));
  const int rc = alloc_frame_buffers(c, h, 6);   // x, y, z, vx, vy, vz: mod_cluster_cloud_host unpacks a caller's cloud into all six
  h.ready = rc == MOD_OK;
  return rc;
}

// z, vx, vy, vz from `z` on: the host entry points write no x and y planes (see scene_flow_staged)
static ModSceneFlowPlanes planes_at(float *z, size_t N, void *cloud_aos) {
  ModSceneFlowPlanes pl{};
  pl.z = z; pl.vx = z + N; pl.vy = z + 2 * N; pl.vz = z + 3 * N; pl.cloud_aos = cloud_aos;
  return pl;
}
static ModClusterOut cluster_out(const ModContext::FrameBuffers &s, bool labels) {
  ModClusterOut out{};
  out.labels = labels ? s.labels.get() : nullptr; out.objects = s.objects; out.n_objects = s.nobj; out.n_clusters = s.nobj + 1;
  return out;
}
static hipError_t plane_in(ModContext *c, float *dst, const float *src, int k, hipStream_t s) {
  return hipMemcpyAsync(dst, src, 4 * k * pixels(c), hipMemcpyHostToDevice, s);
}
// The end of a synchronous call: its result (when dst is not null) to the host on the context's stream, and wait for it.
static int download_sync(ModContext *c, void *dst, const void *src, size_t bytes) {
  if (dst) HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}

// The frame's cluster image (mod_set_cluster_image) from the buffers' own label plane and cluster count into b.image, on the context's stream
static int render_frame_image(ModContext *c, ModContext::FrameBuffers &b) {
  HIP_TRY(c, dalloc(b.image, 3 * c->maxN));
  return render_cluster_image(c, 1, b.labels, b.nobj + 1, c->image_table, b.image);
}
// ... of a synchronous call: rendered and on its way to host_image; the call's last download waits for it
static int image_sync(ModContext *c, uint8_t *host_image) {
  if (int rc = render_frame_image(c, c->staging)) return rc;
  HIP_TRY(c, hipMemcpyAsync(host_image, c->staging.image, 3 * pixels(c), hipMemcpyDeviceToHost, c->stream));
  return MOD_OK;
}

static int fetch_cluster_results(ModContext *c, int32_t *labels, ModObject *objects, int32_t max_objects, int32_t *n_objects) {
  const ModContext::HostStaging &h = c->staging;
  int32_t n = 0;
  HIP_TRY(c, hipMemcpyAsync(&n, h.nobj, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (int rc = download_sync(c, labels, h.labels, sizeof(int32_t) * pixels(c))) return rc;
  if (n_objects) *n_objects = n;
  const int32_t ncopy = std::min(n, std::min(max_objects, (int32_t)c->max_objects));
  return objects && ncopy > 0 ? download_sync(c, objects, h.objects, sizeof(ModObject) * ncopy) : MOD_OK;
}

// The two images of a synchronous *_host call, grey on the device behind the context's stream (ingest_copy, ingest_to_grey): mono8
// straight into the flow staging slot (its 8 N bytes hold both), else staged in that slot, or with a rectification set in the raw
// staging, and grey in the cloud staging (img0 with the left map, img1 with the map of eye1).  panes: img0 holds both eyes.
static int upload_pair(ModContext *c, const uint8_t *img0, const uint8_t *img1, int eye1, bool panes, uint8_t **grey) {
  ModContext::HostStaging &h = c->staging;
  ImageIngest in{};
  in.rectify = c->rect.on; in.panes = panes; in.eye1 = eye1; in.batch2 = true;
  in.stage = reinterpret_cast<uint8_t *>(h.flow.get()); in.raw = &h.raw; in.bayer_grey = &h.bayer_grey;
  in.bin = c->binning; in.bin_grey = &h.bin_grey;
  if (int rc = current_layout(c, &in.lay)) return rc;
  for (int eye : {(int)MOD_EYE_LEFT, eye1}) if (int rc = in.rectify ? ensure_rectify_map(c, eye, in.lay) : MOD_OK) return rc;
  if (int rc = in.rectify ? ensure_raw_stages(c, in) : MOD_OK) return rc;
  if (int rc = ensure_bin_stage(c, in)) return rc;
  in.grey0 = *grey = in.staged() ? static_cast<uint8_t *>(h.aos.get()) : in.stage;
  in.grey1 = in.grey0 + pixels(c);
  if (int rc = ingest_copy(c, in, img0, img1, c->stream)) return rc;
  return ingest_to_grey(c, in);
}

// ---- host streaming: the pipe ------------------------------------------------------------------------------------------
static int ensure_pipe(ModContext *c) {
  Pipe &p = c->pipe;
  if (p.ready) return MOD_OK;
  if (!p.h2d) HIP_TRY(c, hipStreamCreateWithFlags(p.h2d.put(), hipStreamNonBlocking));
  if (!p.d2h) HIP_TRY(c, hipStreamCreateWithFlags(p.d2h.put(), hipStreamNonBlocking));
  for (Pipe::RingPlane &r : p.ring) HIP_TRY(c, dalloc(r.disparity, c->maxN));
  for (Pipe::Slot &s : p.slot) {
    if (int rc = alloc_frame_buffers(c, s, 4)) return rc;
    if (!s.h_n) HIP_TRY(c, hipHostMalloc((void **)s.h_n.put(), 64, hipHostMallocDefault));
    if (!s.h_obj) HIP_TRY(c, hipHostMalloc((void **)s.h_obj.put(), sizeof(ModObject) * (size_t)c->max_objects, hipHostMallocDefault));
    for (Event *e : {&s.ev_in, &s.ev_done, &s.ev_out, &s.img_read.ev}) HIP_TRY(c, make_event(*e));
  }
  HIP_TRY(c, make_event(p.ring_written.ev));
  for (Pipe::RingPlane &r : p.ring) HIP_TRY(c, make_event(r.copied_out.ev));
  p.ready = true;
  return MOD_OK;
}

// Every submit's beginning.  guards(): the entry's own, placed where callers rely on them (after the ticket pointer, before the capacity)
template <class Guards>
static int open_frame(ModContext *c, int32_t *ticket, Pipe::Frame *f, Guards &&guards) {
  if (int rc = check_ready(c, 1)) return rc;
  if (!ticket) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null ticket");
  *ticket = -1;
  if (int rc = guards()) return rc;
  if (c->pipe.in_flight >= MOD_PIPELINE_DEPTH) return fail(c, MOD_ERR_CAPACITY, "MOD_PIPELINE_DEPTH frames are already in flight");
  if (int rc = ensure_pipe(c)) return rc;
  *f = c->pipe.frame(c->pipe.seq);
  return MOD_OK;
}

// Where a ticketed frame's results go on the host; each may be null.  The last two are the image entries'.
struct FrameOut { void *cloud_aos; int32_t *labels; ModObject *objects; int32_t max_objects; float *disparity, *flow; };

// The tail of every ticketed frame (mod_submit_frame_host, submit_stereo), from the frame's inputs on the device to its ticket: the
// slot's planes and cluster outputs, the scene-flow stage alone or with the clustering, the results on the result stream (the
// odometry estimate when s.odo) and the slot's bookkeeping.
static int finish_frame(ModContext *c, Pipe::Slot &s, Pipe::RingPlane &now, const ModFrameBatch &in, const FrameOut &o, int32_t *ticket) {
  Pipe &p = c->pipe;
  const size_t N = pixels(c);
  const ModSceneFlowPlanes pl = planes_at(s.planes, N, o.cloud_aos ? s.aos.get() : nullptr);
  uint8_t *const image = cluster_host_image(c);   // read now: the frame keeps the buffer (and, in its launch's arguments, the table) of its submit
  const ModClusterOut out = cluster_out(s, o.labels || image);
  const bool cluster = o.labels || o.objects || image;     // none asked for: the scene-flow stage alone (see mod_process_frame_host)
  int rc = cluster ? process_dev(c, &in, &pl, &out, nullptr) : scene_flow_staged(c, &in, &pl);   // (a ticketed frame never writes the member lists)
  if (rc) return rc;
  if (image && (rc = render_frame_image(c, s))) return rc;
  HIP_TRY(c, hipEventRecord(s.ev_done, c->stream));
  // results: their own stream
  HIP_TRY(c, hipStreamWaitEvent(p.d2h, s.ev_done, 0));
  if (s.odo) HIP_TRY(c, hipMemcpyAsync(s.h_ego, s.ego, sizeof(Pipe::EgoSlot), hipMemcpyDeviceToHost, p.d2h));
  if (cluster) HIP_TRY(c, hipMemcpyAsync(s.h_n, s.nobj, sizeof(int32_t), hipMemcpyDeviceToHost, p.d2h));
  else *s.h_n = 0;
  if (o.labels) HIP_TRY(c, hipMemcpyAsync(o.labels, s.labels, sizeof(int32_t) * N, hipMemcpyDeviceToHost, p.d2h));
  if (image) HIP_TRY(c, hipMemcpyAsync(image, s.image, 3 * N, hipMemcpyDeviceToHost, p.d2h));
  if (o.disparity) {
    HIP_TRY(c, hipMemcpyAsync(o.disparity, now.disparity, sizeof(float) * N, hipMemcpyDeviceToHost, p.d2h));
    HIP_TRY(c, now.copied_out.record(p.d2h));
  }
  // the slot's flow buffer is next written by the frame that takes this slot after this ticket has been collected
  if (o.flow) HIP_TRY(c, hipMemcpyAsync(o.flow, s.flow, 8 * N, hipMemcpyDeviceToHost, p.d2h));
  const int32_t ncopy = o.objects ? std::max(0, std::min(o.max_objects, (int32_t)c->max_objects)) : 0;   // into h_obj: see Slot
  if (ncopy > 0) HIP_TRY(c, hipMemcpyAsync(s.h_obj, s.objects, sizeof(ModObject) * ncopy, hipMemcpyDeviceToHost, p.d2h));
  s.user_obj = o.objects; s.user_cap = ncopy;
  if (o.cloud_aos) HIP_TRY(c, hipMemcpyAsync(o.cloud_aos, s.aos, 32 * N, hipMemcpyDeviceToHost, p.d2h));
  HIP_TRY(c, hipEventRecord(s.ev_out, p.d2h));
  *ticket = (int32_t)(p.seq & 0x7fffffff);
  p.seq++; p.in_flight++;
  return MOD_OK;
}

// ---- host streaming: the image entries ---------------------------------------------------------------------------------
// mod_submit_stereo_host: flow and transform from the caller; _images_host: flow from the previous left image; _odometry_host: both estimated;
// mod_submit_depth_host: EstimatedFlow or Odometry with `rgbd` set: no right image, the disparity converted from `depth` instead of estimated
enum class StereoKind { CallerFlow, EstimatedFlow, Odometry };
struct StereoRequest {
  StereoKind kind;
  const uint8_t *left, *right;
  const ModSgmParams *sgm;
  double dt;
  FrameOut out;
  const float *flow;                // CallerFlow, else ...
  const ModFlowParams *flow_prm;
  const ModTransform *transform;    // CallerFlow and EstimatedFlow, else ...
  const ModEgoParams *ego_prm;
  ModTransform *transform_out;      // Odometry; may be null, like ...
  ModEgoResult *ego_out;
  bool rgbd;                        // left is the image of an RGB-D camera (right and sgm are null), and ...
  const void *depth;                // ... its depth message
  bool estimates_flow() const { return kind != StereoKind::CallerFlow; }
  bool odometry() const { return kind == StereoKind::Odometry; }
};
struct StereoFrame {
  Pipe::Slot &s;
  Pipe::RingPlane &now, &prev;
  ImageIngest img;                   // layout, rectification and side by side as they are at this submit; the slot's stages; grow_for: the grey images
  DepthPlan depth;                   // RGB-D: the depth settings as they are at this submit; upload_depth: of the staged copy
  ModFlowFill fill;                  // the flow's hole fill as it is at this submit; window 0 (and every submit that estimates no flow): off
  bool fills() const { return fill.window != 0; }
};

// what an RGB-D submit cannot do, whatever its arguments: the state stays as it was
static int rgbd_checks(ModContext *c, DepthPlan *plan) {
  if (c->side_by_side) return fail(c, MOD_ERR_INVALID_ARGUMENT, "mod_submit_depth_host takes one image: side by side must be off");
  if (c->rect.on && !c->depth.has_registration)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "a depth image aligned to the raw image cannot be aligned to the rectified one: set a depth registration");
  ModDepthLayout l;
  if (int rc = current_depth_layout(c, &l)) return rc;
  return depth_plan(c, l, true, plan);   // the chain reads the slot's stage
}

static int stereo_checks(ModContext *c, const StereoRequest &rq, ModImageLayout *lay, DepthPlan *plan) {
  if (int rc = rq.rgbd ? rgbd_checks(c, plan) : MOD_OK) return rc;
  // estimateDisparity() has nothing to work on: disparity_now_.reset() (scene_flow_constructor.cpp:272-276); side by side, left holds both eyes
  if (!rq.left || (rq.rgbd ? !rq.depth : !rq.right && !c->side_by_side)) {
    c->pipe.have_prev = false;      // ... which becomes the next frame's (missing) previous disparity (:397-398)
    c->pipe.have_prev_img = false;  // ... and the next frame has no previous image to estimate the flow from
    if (rq.rgbd) forget_depth_history(c);   // ... and the temporal depth filter starts over with it
    return MOD_SKIP_NO_DISPARITY_NOW;
  }
  if (int rc = rq.rgbd ? MOD_OK : check_sgm_params(c, rq.sgm)) return rc;
  if (int rc = rq.estimates_flow() ? check_flow_params(c, rq.flow_prm, 1) : MOD_OK) return rc;
  if (int rc = rq.odometry() ? check_ego_params(c, rq.ego_prm) : MOD_OK) return rc;
  if (int rc = c->side_by_side ? check_one_message(c, rq.left, rq.right) : MOD_OK) return rc;
  if (int rc = current_layout(c, lay)) return rc;
  if (!c->rect.on) return MOD_OK;
  if (int rc = ensure_rectify_map(c, MOD_EYE_LEFT, *lay)) return rc;
  return rq.rgbd ? MOD_OK : ensure_rectify_map(c, MOD_EYE_RIGHT, *lay);
}

static int grow_for(ModContext *c, const StereoRequest &rq, StereoFrame &f) {
  if (!rq.rgbd) HIP_TRY(c, dalloc(f.s.img, 2 * c->maxN));
  if (rq.estimates_flow()) HIP_TRY(c, dalloc(f.now.left, c->maxN));
  if (f.fills()) HIP_TRY(c, dalloc(c->b.flow.unfilled, c->maxN));
  if (rq.rgbd) {
    if (int rc = ensure_stage_bytes(c, f.s.depth, depth_stage(c, f.depth).bytes())) return rc;
    if (f.depth.registered) HIP_TRY(c, dalloc(f.s.zbuf, c->maxN));
  }
  if (f.img.rectify) {
    if (int rc = ensure_raw_stages(c, f.img)) return rc;
  } else if (f.img.windows_staged()) HIP_TRY(c, dalloc(f.s.stage, window_stage_bytes(c)));
  if (int rc = ensure_bin_stage(c, f.img)) return rc;
  f.img.stage = f.s.stage;
  f.img.grey0 = rq.estimates_flow() ? f.now.left.get() : f.s.img.get();
  f.img.grey1 = rq.rgbd ? nullptr : f.s.img.get() + pixels(c);
  return MOD_OK;
}

// RGB-D: what depth_stage says of the depth message to the slot's stage on the copy stream; f.depth becomes the plan of the staged copy
static int upload_depth(ModContext *c, const StereoRequest &rq, StereoFrame &f) {
  const DepthStage st = depth_stage(c, f.depth);
  HIP_TRY(c, f.s.depth_read.wait(c->pipe.h2d));
  HIP_TRY(c, copy_window(rq.depth, f.depth.lay.step, st.x, st.y, st.bpp, st.w, st.h, f.s.depth.buf, c->pipe.h2d));
  f.depth.lay = st.lay; f.depth.ox = st.x; f.depth.oy = st.y;
  return MOD_OK;
}

// The frame's images, grey on the device: the shared copies on the copy stream behind the fences of what they overwrite, with the
// frame's other inputs; the shared kernels on the context's stream, which is behind every older reader of the grey images already
static int upload_images(ModContext *c, const StereoRequest &rq, StereoFrame &f) {
  Pipe &p = c->pipe;
  const ImageIngest &in = f.img;
  if (!in.rectify && !rq.rgbd) HIP_TRY(c, f.s.img_read.wait(p.h2d));
  if (!in.staged() && rq.estimates_flow()) HIP_TRY(c, f.now.left_read.wait(p.h2d));   // only a copy into the left image waits for its readers
  if (in.staged()) HIP_TRY(c, f.s.stage_read.wait(p.h2d));   // the copies land in the slot's stage (raw messages, windows, regions)
  if (int rc = ingest_copy(c, in, rq.left, rq.right, p.h2d)) return rc;
  if (rq.flow) HIP_TRY(c, hipMemcpyAsync(f.s.flow, rq.flow, 8 * pixels(c), hipMemcpyHostToDevice, p.h2d));
  if (int rc = rq.rgbd ? upload_depth(c, rq, f) : MOD_OK) return rc;
  HIP_TRY(c, hipEventRecord(f.s.ev_in, p.h2d));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, f.s.ev_in, 0));
  if (int rc = ingest_to_grey(c, in)) return rc;
  if (in.staged()) HIP_TRY(c, f.s.stage_read.record(c->stream));   // ... and kernels have read it
  return MOD_OK;
}

static int estimate(ModContext *c, const StereoRequest &rq, StereoFrame &f) {
  Pipe &p = c->pipe;
  // estimateDisparity (:258-279) on the GPU, straight into the ring: this plane is `now` here and `previous` of the next frame.
  // Kernels of older frames that read the plane being replaced are ahead of the estimator on the same stream.
  HIP_TRY(c, f.now.copied_out.wait_once(c->stream));
  if (rq.rgbd) {                    // the depth conversion (depth.hip) in the estimator's place
    if (int rc = run_depth_chain(c, 1, f.s.depth.buf, f.depth, f.s.zbuf, f.now.disparity)) return rc;
    HIP_TRY(c, f.s.depth_read.record(c->stream));
  } else {
    if (int rc = mod_sgm_compute_dev(c, 1, f.img.grey0, f.img.grey1, rq.sgm, f.now.disparity)) return rc;
    HIP_TRY(c, f.s.img_read.record(c->stream));
  }
  HIP_TRY(c, p.ring_written.record(c->stream));
  if (rq.estimates_flow()) HIP_TRY(c, f.now.left_read.record(c->stream));
  // an RGB-D image pairs with an RGB-D image only, a stereo head's left image with one of its own: the other is "a submit of another kind"
  const bool had_prev = p.have_prev, has_flow = rq.estimates_flow() ? p.have_prev_img && p.prev_img_rgbd == rq.rgbd : rq.flow != nullptr;
  p.advance_ring();                 // whatever construct() does with the frame: it keeps its plane when it ends at a guard below
  p.have_prev_img = rq.estimates_flow();   // previous_left = left (:279-290)
  p.prev_img_rgbd = rq.rgbd;
  // disparity_now exists by now
  if (int rc = construct_skip(has_flow, had_prev, rq.transform || rq.odometry(), true)) return rc;
  // with the hole fill on, the measured flow goes to the context's plane in front of the fill (all flow work is on the context's stream, so one
  // plane serves every frame in flight) and the fill, below, writes the frame's flow buffer: everything behind it reads that one as ever
  float *const measured = f.fills() ? reinterpret_cast<float *>(c->b.flow.unfilled.get()) : f.s.flow.get();
  if (rq.estimates_flow()) {        // estimateOpticalFlow (:279-290) on the GPU, straight into the frame's flow buffer
    if (int rc = mod_flow_compute_dev(c, 1, f.prev.left, f.now.left, rq.flow_prm, measured)) return rc;
    HIP_TRY(c, f.prev.left_read.record(c->stream));
    HIP_TRY(c, f.now.left_read.record(c->stream));
  }
  if (rq.odometry()) {
    // the odometry stream: libviso2's process + getMotion (:214-256) on the GPU; its last kernel writes the frame's constants into b.fc,
    // which the scene-flow launch reads (fc_resident).  It sees measured vectors only: a filled one is a copy of a measured one and would vote twice
    HIP_TRY(c, dalloc(p.ego, MOD_PIPELINE_DEPTH));
    f.s.ego = p.ego.get() + (&f.s - p.slot);
    if (!f.s.h_ego) HIP_TRY(c, hipHostMalloc((void **)f.s.h_ego.put(), sizeof(Pipe::EgoSlot), hipHostMallocDefault));
    if (int rc = run_egomotion(c, 1, f.prev.disparity, f.now.disparity, measured, rq.ego_prm, &f.s.ego->tf, &f.s.ego->res, c->b.fc, rq.dt)) return rc;
  }
  if (!f.fills()) return MOD_OK;
  // the hole fill, the last flow stage, gated by disparity_now: the flow is addressed at the NOW pixel (sceneflow.hip reads flow[i] beside dnow[i] to find the previous point)
  launch_flow_fill(c->dc.W, c->dc.H, 1, f.fill.window, f.fill.min_valid, f.fill.tol_abs, f.fill.tol_rel, measured, f.now.disparity, f.s.flow, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

static int submit_stereo(ModContext *c, int32_t *ticket, const StereoRequest &rq) {
  Pipe::Frame at;
  ModImageLayout lay;
  DepthPlan plan{};
  int rc = open_frame(c, ticket, &at, [&] { return stereo_checks(c, rq, &lay, &plan); });
  if (rc) return rc;
  StereoFrame f{*at.s, *at.now, *at.prev, ImageIngest{}, plan, rq.estimates_flow() ? c->opt.flow_fill : ModFlowFill{}};
  f.img.lay = lay; f.img.rectify = c->rect.on; f.img.panes = c->side_by_side; f.img.eye1 = MOD_EYE_RIGHT; f.img.batch2 = false;
  f.img.raw = &f.s.raw; f.img.bayer_grey = &f.s.bayer_grey;
  f.img.bin = c->binning; f.img.bin_grey = &f.s.bin_grey;
  if ((rc = grow_for(c, rq, f)) || (rc = upload_images(c, rq, f)) || (rc = estimate(c, rq, f))) return rc;
  static const ModTransform kUnused = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};   // stands for the transform in HBM (never read)
  const ModFrameBatch in{1, 0, f.now.disparity, f.prev.disparity, f.s.flow, rq.odometry() ? &kUnused : rq.transform, &rq.dt};
  f.s.odo = rq.odometry(); f.s.user_tf = rq.transform_out; f.s.user_ego = rq.ego_out;
  c->fc_resident = rq.odometry();
  rc = finish_frame(c, f.s, f.now, in, rq.out, ticket);
  c->fc_resident = false;
  return rc;
}

extern "C" {

int mod_flow_compute_host(ModContext *c, const uint8_t *prev, const uint8_t *now, const ModFlowParams *p, float *flow) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (!prev || !now) return MOD_SKIP_NO_FLOW;
  if (!flow) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow image");
  uint8_t *dimg = nullptr;
  if ((rc = check_flow_params(c, p, 1)) || (rc = ensure_host_staging(c)) || (rc = upload_pair(c, prev, now, MOD_EYE_LEFT, false, &dimg))) return rc;
  if ((rc = mod_flow_compute_dev(c, 1, dimg, dimg + pixels(c), p, c->staging.planes))) return rc;
  return download_sync(c, flow, c->staging.planes, 8 * pixels(c));
}

int mod_egomotion_host(ModContext *c, const float *disparity_prev, const float *disparity_now, const float *flow, const ModEgoParams *p,
                       ModTransform *transform, ModEgoResult *result) {
  int rc;
  if ((rc = check_ready(c, 1)) || (rc = check_ego_params(c, p))) return rc;
  if (!transform) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null transform");
  if ((rc = construct_skip(flow, disparity_prev, true, disparity_now))) return rc;
  if ((rc = ensure_host_staging(c))) return rc;
  ModContext::HostStaging &h = c->staging;
  HIP_TRY(c, plane_in(c, h.dprev, disparity_prev, 1, c->stream));
  HIP_TRY(c, plane_in(c, h.dnow, disparity_now, 1, c->stream));
  HIP_TRY(c, plane_in(c, h.flow, flow, 2, c->stream));
  if ((rc = run_egomotion(c, 1, h.dprev, h.dnow, h.flow, p, nullptr, nullptr, nullptr, 0.0))) return rc;   // into b.ego.tf, b.ego.res
  ModEgoResult r{};
  HIP_TRY(c, hipMemcpyAsync(transform, c->b.ego.tf, sizeof(ModTransform), hipMemcpyDeviceToHost, c->stream));
  if ((rc = download_sync(c, &r, c->b.ego.res, sizeof(ModEgoResult)))) return rc;
  if (result) *result = r;
  return r.status == MOD_EGO_OK ? MOD_OK : MOD_SKIP_NO_TRANSFORM;   // visual odometry failed: construct() publishes nothing (:251-255)
}

int mod_sgm_compute_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *p, float *disparity) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  const bool panes = c->side_by_side;   // one message holds both eyes
  if (!left || (!right && !panes)) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!disparity) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null disparity image");
  if ((rc = panes ? check_one_message(c, left, right) : MOD_OK)) return rc;
  uint8_t *dimg = nullptr;
  if ((rc = ensure_host_staging(c)) || (rc = upload_pair(c, left, right, MOD_EYE_RIGHT, panes, &dimg))) return rc;
  if ((rc = mod_sgm_compute_dev(c, 1, dimg, dimg + pixels(c), p, c->staging.dnow))) return rc;
  return download_sync(c, disparity, c->staging.dnow, 4 * pixels(c));
}

int mod_process_frame_host(ModContext *c, const float *disparity_now, const float *disparity_prev, const float *flow,
                           const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects,
                           int32_t max_objects, int32_t *n_objects) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (n_objects) *n_objects = 0;
  if ((rc = construct_skip(flow, disparity_prev, transform, disparity_now))) return rc;
  if ((rc = ensure_host_staging(c))) return rc;
  ModContext::HostStaging &h = c->staging;
  const size_t N = pixels(c);
  HIP_TRY(c, plane_in(c, h.dnow, disparity_now, 1, c->stream));
  HIP_TRY(c, plane_in(c, h.dprev, disparity_prev, 1, c->stream));
  HIP_TRY(c, plane_in(c, h.flow, flow, 2, c->stream));
  const ModFrameBatch in{1, 0, h.dnow, h.dprev, h.flow, transform, &dt};   // frames, reserved, now, previous, flow, transforms, dt
  const ModSceneFlowPlanes pl = planes_at(h.planes + 2 * N, N, cloud_aos ? h.aos.get() : nullptr);
  uint8_t *const image = cluster_host_image(c);
  const ModClusterOut out = cluster_out(h, labels || image);
  // no cluster output asked for (neither labels nor objects nor their count nor the cluster image): the scene-flow stage alone — a constructor whose
  // moving objects nobody takes does not cluster (the reference's constructor never does; its clusterer is a node of its own)
  const bool cluster = labels || objects || n_objects || image;
  rc = cluster ? process_dev(c, &in, &pl, &out, cluster_members(c)) : scene_flow_staged(c, &in, &pl);
  if (rc) return rc;
  if (image && (rc = image_sync(c, image))) return rc;
  if (cloud_aos) HIP_TRY(c, hipMemcpyAsync(cloud_aos, h.aos, 32 * N, hipMemcpyDeviceToHost, c->stream));
  return cluster ? fetch_cluster_results(c, labels, objects, max_objects, n_objects) : download_sync(c, nullptr, nullptr, 0);
}

int mod_depth_image_host(ModContext *c, const float *disparity_now, float *depth) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (!disparity_now) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!depth) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null depth image");
  if ((rc = ensure_host_staging(c))) return rc;
  ModContext::HostStaging &h = c->staging;
  HIP_TRY(c, plane_in(c, h.dnow, disparity_now, 1, c->stream));
  launch_depth(c->dc, 1, h.dnow, h.planes, c->stream);
  HIP_TRY(c, hipGetLastError());
  return download_sync(c, depth, h.planes, 4 * pixels(c));
}

int mod_static_flow_host(ModContext *c, const float *disparity_prev, const ModTransform *transform, float *static_flow) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (!disparity_prev) return MOD_SKIP_NO_DISPARITY_PREV;
  if (!transform) return MOD_SKIP_NO_TRANSFORM;
  if (!static_flow) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null static-flow image");
  if ((rc = ensure_host_staging(c))) return rc;
  ModContext::HostStaging &h = c->staging;
  const size_t N = pixels(c);
  HIP_TRY(c, plane_in(c, h.dprev, disparity_prev, 1, c->stream));
  // the static flow depends on the previous disparity and the transform only (sceneflow.hip sf_stage1): the kernel's other
  // inputs are fed the same plane / a zeroed flow, and its cloud goes to the staging planes nobody reads
  HIP_TRY(c, hipMemsetAsync(h.flow, 0, 8 * N, c->stream));
  const double dt = 1.0;
  const ModFrameBatch in{1, 0, h.dprev, h.dprev, h.flow, transform, &dt};
  ModSceneFlowPlanes pl = planes_at(h.planes + 2 * N, N, nullptr);
  pl.static_flow = static_cast<float *>(h.aos.get());   // 8 of the staging cloud's 32 bytes per pixel
  if ((rc = scene_flow_staged(c, &in, &pl))) return rc;
  return download_sync(c, static_flow, h.aos, 8 * N);
}

int mod_cluster_cloud_host(ModContext *c, const void *cloud, int32_t width, int32_t height, int32_t point_step,
                           int32_t row_step, int32_t *labels, ModObject *objects, int32_t max_objects, int32_t *n_objects) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  int rc;
  if (n_objects) *n_objects = 0;
  if (!c->has_cam) {
    // A clusterer-only context (the nodelet lives in its own process, clusterer_nodelet.cpp:221-242): the clusterer reads the
    // image size from the cloud it is handed and needs nothing else of the camera — the context takes the size from the call.
    if (!c->has_prm) return fail(c, MOD_ERR_NOT_CONFIGURED, "parameters must be set first");
    if (width < 1 || height < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cloud size must be positive");
    if (width > c->cfg.max_width || height > c->cfg.max_height || (size_t)width * height > c->maxN)
      return fail(c, MOD_ERR_CAPACITY, "cloud larger than ModConfig.max_width/max_height");
    if (c->dc.W != width || c->dc.H != height) {
      c->cam = ModCamera{};
      c->cam.width = width; c->cam.height = height; c->cam.fx = c->cam.fy = 1.0;
      refresh_devcam(c);
    }
  } else if ((rc = check_ready(c, 1))) return rc;
  if (!cloud) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null cloud");
  // an unorganized / mis-sized cloud is an error (the reference would throw from .at(), clusterer_nodelet.h:99-102)
  if (width != c->dc.W || height != c->dc.H) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cloud size differs from the configured camera");
  if (point_step != 32 || row_step < 32 * width) return fail(c, MOD_ERR_INVALID_ARGUMENT, "expected PointXYZVelocity records (point_step 32)");
  if ((rc = ensure_host_staging(c))) return rc;
  ModContext::HostStaging &h = c->staging;
  const size_t N = pixels(c);
  HIP_TRY(c, hipMemcpy2DAsync(h.aos, (size_t)32 * width, cloud, (size_t)row_step, (size_t)32 * width, (size_t)height,
                              hipMemcpyHostToDevice, c->stream));
  ModSceneFlowPlanes pl = planes_at(h.planes + 2 * N, N, nullptr);
  pl.x = h.planes; pl.y = h.planes + N;         // the caller's cloud unpacked for the clusterer: the x and y planes too
  launch_unpack(N, h.aos, pl.x, pl.y, pl.z, pl.vx, pl.vy, pl.vz, c->stream);
  HIP_TRY(c, hipGetLastError());
  uint8_t *const image = cluster_host_image(c);
  const ModClusterOut out = cluster_out(h, labels || image);
  if ((rc = begin_cluster_scratch(c)) || (rc = run_cluster(c, 1, &pl, c->b.cluster.mask, false, false, &out, cluster_members(c)))) return rc;
  c->scratch_clean = true;
  if (image && (rc = image_sync(c, image))) return rc;
  return fetch_cluster_results(c, labels, objects, max_objects, n_objects);
}

// ---- host streaming ----------------------------------------------------------------------------------------------------
int mod_submit_frame_host(ModContext *c, const float *disparity_now, const float *disparity_prev, const float *flow,
                          const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects,
                          int32_t max_objects, int32_t *ticket) {
  Pipe::Frame f;
  int rc = open_frame(c, ticket, &f, [&] {
    c->pipe.have_prev_img = false;  // mod_submit_images_host pairs only with a left image of its own previous submit
    return construct_skip(flow, disparity_prev || c->pipe.have_prev, transform, disparity_now);
  });
  if (rc) return rc;
  Pipe &p = c->pipe;
  Pipe::Slot &s = *f.s;
  Pipe::RingPlane &now = *f.now, &prev = *f.prev;
  // inputs: their own stream.  `now` was last read by the frame DEPTH planes ago (as its "previous"), which has been collected: at most
  // MOD_PIPELINE_DEPTH - 1 frames are in flight here.  For planes the image entries filled see Pipe::ring_written, RingPlane::copied_out.
  HIP_TRY(c, p.ring_written.wait_once(p.h2d));
  HIP_TRY(c, now.copied_out.wait_once(p.h2d));
  HIP_TRY(c, plane_in(c, now.disparity, disparity_now, 1, p.h2d));
  if (disparity_prev) HIP_TRY(c, plane_in(c, s.dprev, disparity_prev, 1, p.h2d));
  HIP_TRY(c, plane_in(c, s.flow, flow, 2, p.h2d));
  HIP_TRY(c, hipEventRecord(s.ev_in, p.h2d));
  // kernels: the context's stream
  HIP_TRY(c, hipStreamWaitEvent(c->stream, s.ev_in, 0));
  const ModFrameBatch in{1, 0, now.disparity, disparity_prev ? s.dprev : prev.disparity, s.flow, transform, &dt};
  s.odo = false;
  if ((rc = finish_frame(c, s, now, in, FrameOut{cloud_aos, labels, objects, max_objects, nullptr, nullptr}, ticket))) return rc;
  p.advance_ring();                 // only now: a disparity frame that fails or is skipped has taken no plane
  return MOD_OK;
}

int mod_submit_stereo_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm, const float *flow,
                           const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects,
                           int32_t max_objects, float *disparity, int32_t *ticket) {
  StereoRequest rq{StereoKind::CallerFlow, left, right, sgm, dt, {cloud_aos, labels, objects, max_objects, disparity, nullptr}};
  rq.flow = flow; rq.transform = transform;
  return submit_stereo(c, ticket, rq);
}

int mod_submit_images_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm, const ModFlowParams *flow_prm,
                           const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects,
                           int32_t max_objects, float *disparity, float *flow_out, int32_t *ticket) {
  if (c && !flow_prm) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow parameters");
  StereoRequest rq{StereoKind::EstimatedFlow, left, right, sgm, dt, {cloud_aos, labels, objects, max_objects, disparity, flow_out}};
  rq.flow_prm = flow_prm; rq.transform = transform;
  return submit_stereo(c, ticket, rq);
}

int mod_submit_odometry_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm, const ModFlowParams *flow_prm,
                             const ModEgoParams *ego_prm, double dt, void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects,
                             float *disparity, float *flow_out, ModTransform *transform_out, ModEgoResult *ego_out, int32_t *ticket) {
  if (c && !flow_prm) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow parameters");
  if (c && !ego_prm) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null ego-motion parameters");
  StereoRequest rq{StereoKind::Odometry, left, right, sgm, dt, {cloud_aos, labels, objects, max_objects, disparity, flow_out}};
  rq.flow_prm = flow_prm; rq.ego_prm = ego_prm; rq.transform_out = transform_out; rq.ego_out = ego_out;
  return submit_stereo(c, ticket, rq);
}

int mod_submit_depth_host(ModContext *c, const uint8_t *image, const void *depth, const ModFlowParams *flow_prm, const ModEgoParams *ego_prm,
                          const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects,
                          float *disparity, float *flow_out, ModTransform *transform_out, ModEgoResult *ego_out, int32_t *ticket) {
  if (c && !flow_prm) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow parameters");
  if (c && !transform && !ego_prm) return fail(c, MOD_ERR_INVALID_ARGUMENT, "a transform or ego-motion parameters: both are null");
  StereoRequest rq{transform ? StereoKind::EstimatedFlow : StereoKind::Odometry, image, nullptr, nullptr, dt,
                   {cloud_aos, labels, objects, max_objects, disparity, flow_out}};
  rq.flow_prm = flow_prm; rq.transform = transform; rq.rgbd = true; rq.depth = depth;
  if (rq.odometry()) { rq.ego_prm = ego_prm; rq.transform_out = transform_out; rq.ego_out = ego_out; }
  return submit_stereo(c, ticket, rq);
}

int mod_collect_frame_host(ModContext *c, int32_t ticket, int32_t *n_objects) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  Pipe &p = c->pipe;
  if (n_objects) *n_objects = 0;
  if (p.in_flight < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "no frame in flight");
  const int64_t oldest = p.seq - p.in_flight;
  if (ticket != (int32_t)(oldest & 0x7fffffff)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "tickets are collected in submission order");
  Pipe::Slot &s = *p.frame(oldest).s;
  HIP_TRY(c, hipEventSynchronize(s.ev_out));
  p.in_flight--;
  if (s.odo) {
    if (s.user_tf) *s.user_tf = s.h_ego.get()->tf;
    if (s.user_ego) *s.user_ego = s.h_ego.get()->res;
    // visual odometry failed: the reference publishes nothing (scene_flow_constructor.cpp:251-255)
    if (s.h_ego.get()->res.status != MOD_EGO_OK) return MOD_SKIP_NO_TRANSFORM;
  }
  const int32_t n = *s.h_n;
  if (n_objects) *n_objects = n;
  const int32_t ncopy = std::min(n, s.user_cap);
  if (s.user_obj && ncopy > 0) memcpy(s.user_obj, s.h_obj, sizeof(ModObject) * (size_t)ncopy);
  return MOD_OK;
}

int mod_forget_previous(ModContext *c) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  c->pipe.have_prev = false;
  c->pipe.have_prev_img = false;
  forget_depth_history(c);          // the temporal depth filter's state goes with the previous disparity
  return MOD_OK;
}

}  // extern "C"
