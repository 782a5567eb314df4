// host_api.hip — the C ABI's host-pointer entry points: the single-frame *_host calls, which stage one frame through device buffers
// of the context, and the submit / collect stream with its pipe of slots, copy streams and disparity ring.  Host-side only.
#include "mod_context.h"

#include <algorithm>
#include <cstring>

static int ensure_host_staging(ModContext *c) {
  Buffers &b = c->b;
  if (b.h_objects) return MOD_OK;                    // the last buffer of the set exists: all do
  const size_t N = c->maxN;
  HIP_TRY(c, dalloc(b.h_dnow, N));
  HIP_TRY(c, dalloc(b.h_dprev, N));
  HIP_TRY(c, dalloc(b.h_flow, 2 * N));
  HIP_TRY(c, dalloc(b.h_planes, 6 * N));
  if (!b.h_aos) HIP_TRY(c, hipMalloc(b.h_aos.put(), 32 * N));
  HIP_TRY(c, dalloc(b.h_labels, N));
  HIP_TRY(c, dalloc(b.h_nobj, 8));
  HIP_TRY(c, dalloc(b.h_objects, (size_t)c->max_objects));
  return MOD_OK;
}

// xy: the x and y planes too (a caller's cloud unpacked for the clusterer); the fused host paths leave them out (scene_flow_staged)
static void staged_planes(ModContext *c, ModSceneFlowPlanes *pl, bool xy) {
  const size_t N = (size_t)c->dc.W * c->dc.H;
  float *p = c->b.h_planes;
  memset(pl, 0, sizeof(*pl));
  if (xy) { pl->x = p; pl->y = p + N; }
  pl->z = p + 2 * N; pl->vx = p + 3 * N; pl->vy = p + 4 * N; pl->vz = p + 5 * N;
}

static int fetch_cluster_results(ModContext *c, int32_t *labels, ModObject *objects, int32_t max_objects, int32_t *n_objects) {
  const size_t N = (size_t)c->dc.W * c->dc.H;
  int32_t n = 0;
  HIP_TRY(c, hipMemcpyAsync(&n, c->b.h_nobj, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (labels) HIP_TRY(c, hipMemcpyAsync(labels, c->b.h_labels, sizeof(int32_t) * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_objects) *n_objects = n;
  const int32_t ncopy = std::min(n, std::min(max_objects, (int32_t)c->max_objects));
  if (objects && ncopy > 0) {
    HIP_TRY(c, hipMemcpyAsync(objects, c->b.h_objects, sizeof(ModObject) * ncopy, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return MOD_OK;
}

// ---- host images (mod_set_image_layout) --------------------------------------------------------------------------------
// The window of one host image to the device on stream s, as packed rows of W * channels bytes: one copy when the window's rows are
// contiguous in the message (the default layout: the whole mono8 image), else a 2D copy.  Only the window crosses PCIe.
static hipError_t copy_window(const ModImageLayout &l, int W, int H, const uint8_t *src, uint8_t *dst, hipStream_t s) {
  const int C = image_channels(l.encoding);
  const size_t row = (size_t)W * C;
  const uint8_t *o = src + (size_t)l.y0 * l.step + (size_t)l.x0 * C;
  if ((size_t)l.step == row) return hipMemcpyAsync(dst, o, row * H, hipMemcpyHostToDevice, s);
  return hipMemcpy2DAsync(dst, row, o, (size_t)l.step, row, (size_t)H, hipMemcpyHostToDevice, s);
}

// The two images of a synchronous *_host call, grey on the device behind the context's stream: mono8 straight into the flow
// staging slot (its 8 N bytes hold both), colour windows into that slot and k_to_mono from there into the cloud staging.
static int upload_pair(ModContext *c, const ModImageLayout &l, const uint8_t *img0, const uint8_t *img1, uint8_t **grey) {
  const int W = c->dc.W, H = c->dc.H;
  uint8_t *slot = reinterpret_cast<uint8_t *>(c->b.h_flow.get());
  const size_t P = (size_t)W * H * image_channels(l.encoding);
  HIP_TRY(c, copy_window(l, W, H, img0, slot, c->stream));
  HIP_TRY(c, copy_window(l, W, H, img1, slot + P, c->stream));
  if (l.encoding == MOD_ENCODING_MONO8) { *grey = slot; return MOD_OK; }
  *grey = static_cast<uint8_t *>(c->b.h_aos.get());
  launch_to_mono(l.encoding, W, H, 2, slot, P, (int)(P / H), 0, 0, *grey, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

// ---- host streaming: the pipe ------------------------------------------------------------------------------------------
static int ensure_pipe(ModContext *c) {
  ModContext::Pipe &p = c->pipe;
  if (p.ready) return MOD_OK;
  const size_t N = c->maxN;
  if (!p.h2d) HIP_TRY(c, hipStreamCreateWithFlags(p.h2d.put(), hipStreamNonBlocking));
  if (!p.d2h) HIP_TRY(c, hipStreamCreateWithFlags(p.d2h.put(), hipStreamNonBlocking));
  for (int i = 0; i <= MOD_PIPELINE_DEPTH; i++) HIP_TRY(c, dalloc(p.dnow[i], N));
  for (int i = 0; i < MOD_PIPELINE_DEPTH; i++) {
    HIP_TRY(c, dalloc(p.dprev[i], N));
    HIP_TRY(c, dalloc(p.flow[i], 2 * N));
    HIP_TRY(c, dalloc(p.planes[i], 4 * N));
    if (!p.aos[i]) HIP_TRY(c, hipMalloc(p.aos[i].put(), 32 * N));
    HIP_TRY(c, dalloc(p.labels[i], N));
    HIP_TRY(c, dalloc(p.nobj[i], 8));
    HIP_TRY(c, dalloc(p.objects[i], (size_t)c->max_objects));
    if (!p.h_n[i]) HIP_TRY(c, hipHostMalloc((void **)p.h_n[i].put(), 64, hipHostMallocDefault));
    if (!p.h_obj[i]) HIP_TRY(c, hipHostMalloc((void **)p.h_obj[i].put(), sizeof(ModObject) * (size_t)c->max_objects, hipHostMallocDefault));
    for (Event *e : {&p.ev_in[i], &p.ev_done[i], &p.ev_out[i], &p.ev_img[i]})
      if (!*e) HIP_TRY(c, hipEventCreateWithFlags(e->put(), hipEventDisableTiming));
  }
  if (!p.ev_ring) HIP_TRY(c, hipEventCreateWithFlags(p.ev_ring.put(), hipEventDisableTiming));
  for (Event &e : p.ev_plane_read) if (!e) HIP_TRY(c, hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
  p.ready = true;
  return MOD_OK;
}

// The tail of every ticketed frame (mod_submit_frame_host, submit_stereo), from the frame's inputs on the device to its ticket: the
// slot's planes and cluster outputs, the scene-flow stage alone or with the clustering, the results on the result stream (the
// odometry estimate when p.odo[slot]) and the slot's bookkeeping.  extra() enqueues the caller's own results behind the labels.
template <class Extra>
static int finish_frame(ModContext *c, int slot, const ModFrameBatch &in, void *cloud_aos, int32_t *labels, ModObject *objects,
                        int32_t max_objects, int32_t *ticket, Extra &&extra) {
  ModContext::Pipe &p = c->pipe;
  const size_t N = (size_t)c->dc.W * c->dc.H;
  ModSceneFlowPlanes pl;
  memset(&pl, 0, sizeof(pl));
  float *q = p.planes[slot];                 // z, vx, vy, vz for the cluster stage; no x, y planes (see scene_flow_staged)
  pl.z = q; pl.vx = q + N; pl.vy = q + 2 * N; pl.vz = q + 3 * N;
  pl.cloud_aos = cloud_aos ? p.aos[slot].get() : nullptr;
  ModClusterOut out{};
  out.labels = labels ? p.labels[slot].get() : nullptr; out.objects = p.objects[slot]; out.n_objects = p.nobj[slot]; out.n_clusters = p.nobj[slot] + 1;
  const bool cluster = labels || objects;     // neither asked for: the scene-flow stage alone (see mod_process_frame_host)
  int rc = cluster ? mod_process_dev(c, &in, &pl, &out) : scene_flow_staged(c, &in, &pl);
  if (rc) return rc;
  HIP_TRY(c, hipEventRecord(p.ev_done[slot], c->stream));
  // results: their own stream
  HIP_TRY(c, hipStreamWaitEvent(p.d2h, p.ev_done[slot], 0));
  if (p.odo[slot]) HIP_TRY(c, hipMemcpyAsync(p.h_ego[slot], &p.ego[slot], sizeof(ModContext::Pipe::EgoSlot), hipMemcpyDeviceToHost, p.d2h));
  if (cluster) HIP_TRY(c, hipMemcpyAsync(p.h_n[slot], p.nobj[slot], sizeof(int32_t), hipMemcpyDeviceToHost, p.d2h));
  else *p.h_n[slot] = 0;
  if (labels) HIP_TRY(c, hipMemcpyAsync(labels, p.labels[slot], sizeof(int32_t) * N, hipMemcpyDeviceToHost, p.d2h));
  if ((rc = extra())) return rc;
  // the count is not known yet: the caller's capacity goes to a pinned staging array (a pageable destination would make this
  // call wait for the kernels); mod_collect_frame_host hands the objects over
  const int32_t ncopy = objects ? std::max(0, std::min(max_objects, (int32_t)c->max_objects)) : 0;
  if (ncopy > 0) HIP_TRY(c, hipMemcpyAsync(p.h_obj[slot], p.objects[slot], sizeof(ModObject) * ncopy, hipMemcpyDeviceToHost, p.d2h));
  p.user_obj[slot] = objects; p.user_cap[slot] = ncopy;
  if (cloud_aos) HIP_TRY(c, hipMemcpyAsync(cloud_aos, p.aos[slot], 32 * N, hipMemcpyDeviceToHost, p.d2h));
  HIP_TRY(c, hipEventRecord(p.ev_out[slot], p.d2h));
  *ticket = (int32_t)(p.seq & 0x7fffffff);
  p.seq++; p.in_flight++;
  return MOD_OK;
}

// mod_submit_stereo_host (flow from the caller, fprm == nullptr), mod_submit_images_host (flow == nullptr, estimated on the GPU
// from the previous submit's left image with fprm) and mod_submit_odometry_host (eprm != nullptr: the transform estimated on the GPU too)
static int submit_stereo(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm, const float *flow,
                         const ModFlowParams *fprm, const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels,
                         ModObject *objects, int32_t max_objects, float *disparity, float *flow_out, int32_t *ticket,
                         const ModEgoParams *eprm = nullptr, ModTransform *transform_out = nullptr, ModEgoResult *ego_out = nullptr) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (!ticket) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null ticket");
  *ticket = -1;
  ModContext::Pipe &p = c->pipe;
  const bool images = fprm != nullptr, odo = eprm != nullptr;
  if (!left || !right) {            // estimateDisparity() has nothing to work on: disparity_now_.reset() (scene_flow_constructor.cpp:272-276)
    p.have_prev = false;            // ... which becomes the next frame's (missing) previous disparity (:397-398)
    p.have_prev_img = false;        // ... and the next frame has no previous image to estimate the flow from
    return MOD_SKIP_NO_DISPARITY_NOW;
  }
  if ((rc = check_sgm_params(c, sgm))) return rc;
  if (images && (rc = check_flow_params(c, fprm, 1))) return rc;
  if (odo && (rc = check_ego_params(c, eprm))) return rc;
  ModImageLayout lay;
  if ((rc = current_layout(c, &lay))) return rc;
  const bool colour = lay.encoding != MOD_ENCODING_MONO8;
  if (p.in_flight >= MOD_PIPELINE_DEPTH) return fail(c, MOD_ERR_CAPACITY, "MOD_PIPELINE_DEPTH frames are already in flight");
  if ((rc = ensure_pipe(c))) return rc;
  constexpr int R = MOD_PIPELINE_DEPTH + 1;
  const int slot = (int)(p.seq % MOD_PIPELINE_DEPTH), nowi = (int)(p.dring % R), previ = (int)((p.dring + R - 1) % R);
  const int W = c->dc.W, H = c->dc.H;
  const size_t N = (size_t)W * H;
  if (!p.img[slot]) HIP_TRY(c, dalloc(p.img[slot], 2 * c->maxN));
  if (images && !p.limg[nowi]) HIP_TRY(c, dalloc(p.limg[nowi], c->maxN));
  if (images && !p.ev_limg[nowi]) HIP_TRY(c, hipEventCreateWithFlags(p.ev_limg[nowi].put(), hipEventDisableTiming));
  if (colour && !p.stage[slot]) HIP_TRY(c, dalloc(p.stage[slot], 8 * c->maxN));
  if (colour && !p.ev_stage[slot]) HIP_TRY(c, hipEventCreateWithFlags(p.ev_stage[slot].put(), hipEventDisableTiming));
  // images (and flow) on the copy stream; the slot's image buffer may still be read by the estimator of a frame that ended at a
  // guard (it took no ticket, so nobody waited for it): the copy queues behind that estimator.  A resident left image is replaced
  // only after the last kernel that reads it (its own frame's and the next frame's estimators).  Colour windows go to the slot's
  // staging, which is replaced only after the kernels that read it; their grey is written on the context's stream, behind every
  // older reader of img[slot] / limg[nowi].
  if (p.img_used[slot]) HIP_TRY(c, hipStreamWaitEvent(p.h2d, p.ev_img[slot], 0));
  uint8_t *dleft = p.img[slot];
  if (images) {
    if (p.limg_used[nowi] && !colour) HIP_TRY(c, hipStreamWaitEvent(p.h2d, p.ev_limg[nowi], 0));
    dleft = p.limg[nowi];
  }
  const size_t P = N * image_channels(lay.encoding);
  if (colour) {
    if (p.stage_used[slot]) HIP_TRY(c, hipStreamWaitEvent(p.h2d, p.ev_stage[slot], 0));
    HIP_TRY(c, copy_window(lay, W, H, left, p.stage[slot], p.h2d));
    HIP_TRY(c, copy_window(lay, W, H, right, p.stage[slot] + P, p.h2d));
  } else {
    HIP_TRY(c, copy_window(lay, W, H, left, dleft, p.h2d));
    HIP_TRY(c, copy_window(lay, W, H, right, p.img[slot] + N, p.h2d));
  }
  if (flow) HIP_TRY(c, hipMemcpyAsync(p.flow[slot], flow, 8 * N, hipMemcpyHostToDevice, p.h2d));
  HIP_TRY(c, hipEventRecord(p.ev_in[slot], p.h2d));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, p.ev_in[slot], 0));
  if (colour) {                     // cv_bridge::toCvCopy(..., MONO8) (:220-221) on the GPU
    launch_to_mono(lay.encoding, W, H, 1, p.stage[slot], P, (int)(P / H), 0, 0, dleft, c->stream);
    launch_to_mono(lay.encoding, W, H, 1, p.stage[slot] + P, P, (int)(P / H), 0, 0, p.img[slot] + N, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(p.ev_stage[slot], c->stream));
    p.stage_used[slot] = true;
  }
  // estimateDisparity (:258-279) on the GPU, straight into the ring: this plane is `now` here and `previous` of the next frame.
  // Kernels of older frames that read the plane being replaced are ahead of the estimator on the same stream.
  if (p.plane_read_pending[nowi]) { HIP_TRY(c, hipStreamWaitEvent(c->stream, p.ev_plane_read[nowi], 0)); p.plane_read_pending[nowi] = false; }
  if ((rc = mod_sgm_compute_dev(c, 1, dleft, p.img[slot] + N, sgm, p.dnow[nowi]))) return rc;
  HIP_TRY(c, hipEventRecord(p.ev_img[slot], c->stream));
  HIP_TRY(c, hipEventRecord(p.ev_ring, c->stream));
  if (images) { HIP_TRY(c, hipEventRecord(p.ev_limg[nowi], c->stream)); p.limg_used[nowi] = true; }
  p.img_used[slot] = true; p.ring_by_kernels = true;
  const bool had_prev = p.have_prev, has_flow = images ? p.have_prev_img : flow != nullptr;
  p.dring++; p.have_prev = true;    // disparity_previous_ = disparity_now_, whatever construct() does with the frame (:397-398)
  p.have_prev_img = images;         // previous_left = left (:279-290), for the images stream only
  // disparity_now exists by now
  if ((rc = construct_skip(has_flow, had_prev, transform || odo, true))) return rc;
  if (images) {                     // estimateOpticalFlow (:279-290) on the GPU, straight into the frame's flow buffer
    if ((rc = mod_flow_compute_dev(c, 1, p.limg[previ], p.limg[nowi], fprm, p.flow[slot]))) return rc;
    HIP_TRY(c, hipEventRecord(p.ev_limg[previ], c->stream));
    HIP_TRY(c, hipEventRecord(p.ev_limg[nowi], c->stream));
  }
  // the odometry stream: libviso2's process + getMotion (:214-256) on the GPU; its last kernel writes the frame's constants into b.fc,
  // which the scene-flow launch below reads (fc_resident).  The slot's estimate was last copied out before its ticket was collected.
  static const ModTransform kUnused = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};   // stands for the transform in HBM (never read)
  if (odo) {
    if (!p.ego) HIP_TRY(c, dalloc(p.ego, MOD_PIPELINE_DEPTH));
    if (!p.h_ego[slot]) HIP_TRY(c, hipHostMalloc((void **)p.h_ego[slot].put(), sizeof(ModContext::Pipe::EgoSlot), hipHostMallocDefault));
    if ((rc = run_egomotion(c, 1, p.dnow[previ], p.dnow[nowi], p.flow[slot], eprm, &p.ego[slot].tf, &p.ego[slot].res, c->b.fc, dt))) return rc;
  }
  ModFrameBatch in{};
  in.frames = 1; in.disparity_now = p.dnow[nowi]; in.disparity_prev = p.dnow[previ];
  in.flow = p.flow[slot]; in.transforms = odo ? &kUnused : transform; in.dt = &dt;
  p.odo[slot] = odo; p.user_tf[slot] = transform_out; p.user_ego[slot] = ego_out;
  c->fc_resident = odo;
  rc = finish_frame(c, slot, in, cloud_aos, labels, objects, max_objects, ticket, [&]() -> int {
    if (disparity) {
      HIP_TRY(c, hipMemcpyAsync(disparity, p.dnow[nowi], sizeof(float) * N, hipMemcpyDeviceToHost, p.d2h));
      HIP_TRY(c, hipEventRecord(p.ev_plane_read[nowi], p.d2h));
      p.plane_read_pending[nowi] = true;
    }
    // the slot's flow buffer is next written by the frame that takes this slot after this ticket has been collected
    if (flow_out) HIP_TRY(c, hipMemcpyAsync(flow_out, p.flow[slot], 8 * N, hipMemcpyDeviceToHost, p.d2h));
    return MOD_OK;
  });
  c->fc_resident = false;
  return rc;
}

extern "C" {

int mod_flow_compute_host(ModContext *c, const uint8_t *prev, const uint8_t *now, const ModFlowParams *p, float *flow) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (!prev || !now) return MOD_SKIP_NO_FLOW;
  if (!flow) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow image");
  if ((rc = check_flow_params(c, p, 1))) return rc;
  if ((rc = ensure_host_staging(c))) return rc;
  const size_t N = (size_t)c->dc.W * c->dc.H;
  Buffers &b = c->b;
  ModImageLayout lay;
  uint8_t *dimg = nullptr;
  if ((rc = current_layout(c, &lay)) || (rc = upload_pair(c, lay, prev, now, &dimg))) return rc;
  if ((rc = mod_flow_compute_dev(c, 1, dimg, dimg + N, p, b.h_planes))) return rc;
  HIP_TRY(c, hipMemcpyAsync(flow, b.h_planes, 8 * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}

int mod_egomotion_host(ModContext *c, const float *disparity_prev, const float *disparity_now, const float *flow, const ModEgoParams *p,
                       ModTransform *transform, ModEgoResult *result) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if ((rc = check_ego_params(c, p))) return rc;
  if (!transform) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null transform");
  if ((rc = construct_skip(flow, disparity_prev, true, disparity_now))) return rc;
  if ((rc = ensure_host_staging(c))) return rc;
  const size_t N = (size_t)c->dc.W * c->dc.H;
  Buffers &b = c->b;
  HIP_TRY(c, hipMemcpyAsync(b.h_dprev, disparity_prev, 4 * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(b.h_dnow, disparity_now, 4 * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(b.h_flow, flow, 8 * N, hipMemcpyHostToDevice, c->stream));
  if ((rc = run_egomotion(c, 1, b.h_dprev, b.h_dnow, b.h_flow, p, nullptr, nullptr, nullptr, 0.0))) return rc;   // into b.ego_tf, b.ego_res
  ModEgoResult r{};
  HIP_TRY(c, hipMemcpyAsync(transform, b.ego_tf, sizeof(ModTransform), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&r, b.ego_res, sizeof(ModEgoResult), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (result) *result = r;
  return r.status == MOD_EGO_OK ? MOD_OK : MOD_SKIP_NO_TRANSFORM;   // visual odometry failed: construct() publishes nothing (:251-255)
}

int mod_sgm_compute_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *p, float *disparity) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (!left || !right) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!disparity) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null disparity image");
  if ((rc = ensure_host_staging(c))) return rc;
  const size_t N = (size_t)c->dc.W * c->dc.H;
  Buffers &b = c->b;
  ModImageLayout lay;
  uint8_t *dimg = nullptr;
  if ((rc = current_layout(c, &lay)) || (rc = upload_pair(c, lay, left, right, &dimg))) return rc;
  if ((rc = mod_sgm_compute_dev(c, 1, dimg, dimg + N, p, b.h_dnow))) return rc;
  HIP_TRY(c, hipMemcpyAsync(disparity, b.h_dnow, 4 * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}

int mod_process_frame_host(ModContext *c, const float *disparity_now, const float *disparity_prev, const float *flow,
                           const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects,
                           int32_t max_objects, int32_t *n_objects) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (n_objects) *n_objects = 0;
  if ((rc = construct_skip(flow, disparity_prev, transform, disparity_now))) return rc;
  rc = ensure_host_staging(c);
  if (rc) return rc;
  const size_t N = (size_t)c->dc.W * c->dc.H;
  Buffers &b = c->b;
  HIP_TRY(c, hipMemcpyAsync(b.h_dnow, disparity_now, 4 * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(b.h_dprev, disparity_prev, 4 * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(b.h_flow, flow, 8 * N, hipMemcpyHostToDevice, c->stream));
  ModFrameBatch in{};
  in.frames = 1; in.disparity_now = b.h_dnow; in.disparity_prev = b.h_dprev; in.flow = b.h_flow;
  in.transforms = transform; in.dt = &dt;
  ModSceneFlowPlanes pl;
  staged_planes(c, &pl, false);
  pl.cloud_aos = cloud_aos ? b.h_aos.get() : nullptr;
  ModClusterOut out{};
  out.labels = labels ? b.h_labels.get() : nullptr; out.objects = b.h_objects; out.n_objects = b.h_nobj; out.n_clusters = b.h_nobj + 1;
  // no cluster output asked for (neither labels nor objects nor their count): the scene-flow stage alone — a constructor whose
  // moving objects nobody takes does not cluster (the reference's constructor never does; its clusterer is a node of its own)
  const bool cluster = labels || objects || n_objects;
  rc = cluster ? mod_process_dev(c, &in, &pl, &out) : scene_flow_staged(c, &in, &pl);
  if (rc) return rc;
  if (cloud_aos) HIP_TRY(c, hipMemcpyAsync(cloud_aos, b.h_aos, 32 * N, hipMemcpyDeviceToHost, c->stream));
  if (!cluster) { HIP_TRY(c, hipStreamSynchronize(c->stream)); return MOD_OK; }
  return fetch_cluster_results(c, labels, objects, max_objects, n_objects);
}

int mod_depth_image_host(ModContext *c, const float *disparity_now, float *depth) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (!disparity_now) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!depth) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null depth image");
  if ((rc = ensure_host_staging(c))) return rc;
  const size_t N = (size_t)c->dc.W * c->dc.H;
  Buffers &b = c->b;
  HIP_TRY(c, hipMemcpyAsync(b.h_dnow, disparity_now, 4 * N, hipMemcpyHostToDevice, c->stream));
  launch_depth(c->dc, 1, b.h_dnow, b.h_planes, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(depth, b.h_planes, 4 * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}

int mod_static_flow_host(ModContext *c, const float *disparity_prev, const ModTransform *transform, float *static_flow) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (!disparity_prev) return MOD_SKIP_NO_DISPARITY_PREV;
  if (!transform) return MOD_SKIP_NO_TRANSFORM;
  if (!static_flow) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null static-flow image");
  if ((rc = ensure_host_staging(c))) return rc;
  const size_t N = (size_t)c->dc.W * c->dc.H;
  Buffers &b = c->b;
  HIP_TRY(c, hipMemcpyAsync(b.h_dprev, disparity_prev, 4 * N, hipMemcpyHostToDevice, c->stream));
  // the static flow depends on the previous disparity and the transform only (sceneflow.hip sf_stage1): the kernel's other
  // inputs are fed the same plane / a zeroed flow, and its cloud goes to the staging planes nobody reads
  HIP_TRY(c, hipMemsetAsync(b.h_flow, 0, 8 * N, c->stream));
  ModFrameBatch in{};
  const double dt = 1.0;
  in.frames = 1; in.disparity_now = b.h_dprev; in.disparity_prev = b.h_dprev; in.flow = b.h_flow; in.transforms = transform; in.dt = &dt;
  ModSceneFlowPlanes pl;
  staged_planes(c, &pl, false);
  pl.static_flow = static_cast<float *>(b.h_aos.get());   // 8 of the staging cloud's 32 bytes per pixel
  if ((rc = scene_flow_staged(c, &in, &pl))) return rc;
  HIP_TRY(c, hipMemcpyAsync(static_flow, b.h_aos, 8 * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
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
  rc = ensure_host_staging(c);
  if (rc) return rc;
  Buffers &b = c->b;
  HIP_TRY(c, hipMemcpy2DAsync(b.h_aos, (size_t)32 * width, cloud, (size_t)row_step, (size_t)32 * width, (size_t)height,
                              hipMemcpyHostToDevice, c->stream));
  ModSceneFlowPlanes pl;
  staged_planes(c, &pl, true);
  launch_unpack((size_t)width * height, b.h_aos, pl.x, pl.y, pl.z, pl.vx, pl.vy, pl.vz, c->stream);
  HIP_TRY(c, hipGetLastError());
  ModClusterOut out{};
  out.labels = labels ? b.h_labels.get() : nullptr; out.objects = b.h_objects; out.n_objects = b.h_nobj; out.n_clusters = b.h_nobj + 1;
  if ((rc = begin_cluster_scratch(c)) || (rc = run_cluster(c, 1, &pl, c->b.mask, false, false, &out))) return rc;
  c->scratch_clean = true;
  return fetch_cluster_results(c, labels, objects, max_objects, n_objects);
}

// ---- host streaming ----------------------------------------------------------------------------------------------------
int mod_submit_frame_host(ModContext *c, const float *disparity_now, const float *disparity_prev, const float *flow,
                          const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects,
                          int32_t max_objects, int32_t *ticket) {
  int rc = check_ready(c, 1);
  if (rc) return rc;
  if (!ticket) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null ticket");
  *ticket = -1;
  ModContext::Pipe &p = c->pipe;
  p.have_prev_img = false;          // mod_submit_images_host pairs only with a left image of its own previous submit
  if ((rc = construct_skip(flow, disparity_prev || p.have_prev, transform, disparity_now))) return rc;
  if (p.in_flight >= MOD_PIPELINE_DEPTH) return fail(c, MOD_ERR_CAPACITY, "MOD_PIPELINE_DEPTH frames are already in flight");
  if ((rc = ensure_pipe(c))) return rc;
  constexpr int R = MOD_PIPELINE_DEPTH + 1;
  const int slot = (int)(p.seq % MOD_PIPELINE_DEPTH), nowi = (int)(p.dring % R), previ = (int)((p.dring + R - 1) % R);
  const size_t N = (size_t)c->dc.W * c->dc.H;
  // inputs: their own stream.  dnow[nowi] was last read by the frame R - 1 planes ago (as its "previous"), which has been collected:
  // at most MOD_PIPELINE_DEPTH - 1 frames are in flight at this point.  (Planes the stereo entry filled were written by kernels,
  // and a frame it skipped took a plane without a ticket: the copy then also waits for the last of those kernels.)
  if (p.ring_by_kernels) { HIP_TRY(c, hipStreamWaitEvent(p.h2d, p.ev_ring, 0)); p.ring_by_kernels = false; }
  if (p.plane_read_pending[nowi]) { HIP_TRY(c, hipStreamWaitEvent(p.h2d, p.ev_plane_read[nowi], 0)); p.plane_read_pending[nowi] = false; }
  HIP_TRY(c, hipMemcpyAsync(p.dnow[nowi], disparity_now, 4 * N, hipMemcpyHostToDevice, p.h2d));
  if (disparity_prev) HIP_TRY(c, hipMemcpyAsync(p.dprev[slot], disparity_prev, 4 * N, hipMemcpyHostToDevice, p.h2d));
  HIP_TRY(c, hipMemcpyAsync(p.flow[slot], flow, 8 * N, hipMemcpyHostToDevice, p.h2d));
  HIP_TRY(c, hipEventRecord(p.ev_in[slot], p.h2d));
  // kernels: the context's stream
  HIP_TRY(c, hipStreamWaitEvent(c->stream, p.ev_in[slot], 0));
  ModFrameBatch in{};
  in.frames = 1; in.disparity_now = p.dnow[nowi]; in.disparity_prev = disparity_prev ? p.dprev[slot] : p.dnow[previ];
  in.flow = p.flow[slot]; in.transforms = transform; in.dt = &dt;
  p.odo[slot] = false;
  if ((rc = finish_frame(c, slot, in, cloud_aos, labels, objects, max_objects, ticket, [] { return MOD_OK; }))) return rc;
  p.dring++; p.have_prev = true;
  return MOD_OK;
}

int mod_submit_stereo_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm, const float *flow,
                           const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects,
                           int32_t max_objects, float *disparity, int32_t *ticket) {
  return submit_stereo(c, left, right, sgm, flow, nullptr, transform, dt, cloud_aos, labels, objects, max_objects, disparity, nullptr, ticket);
}

int mod_submit_images_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm, const ModFlowParams *flow_prm,
                           const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects,
                           int32_t max_objects, float *disparity, float *flow_out, int32_t *ticket) {
  if (c && !flow_prm) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow parameters");
  return submit_stereo(c, left, right, sgm, nullptr, flow_prm, transform, dt, cloud_aos, labels, objects, max_objects, disparity, flow_out, ticket);
}

int mod_submit_odometry_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm, const ModFlowParams *flow_prm,
                             const ModEgoParams *ego_prm, double dt, void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects,
                             float *disparity, float *flow_out, ModTransform *transform_out, ModEgoResult *ego_out, int32_t *ticket) {
  if (c && !flow_prm) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null flow parameters");
  if (c && !ego_prm) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null ego-motion parameters");
  return submit_stereo(c, left, right, sgm, nullptr, flow_prm, nullptr, dt, cloud_aos, labels, objects, max_objects, disparity, flow_out, ticket,
                       ego_prm, transform_out, ego_out);
}

int mod_collect_frame_host(ModContext *c, int32_t ticket, int32_t *n_objects) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  ModContext::Pipe &p = c->pipe;
  if (n_objects) *n_objects = 0;
  if (p.in_flight < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "no frame in flight");
  const int64_t oldest = p.seq - p.in_flight;
  if (ticket != (int32_t)(oldest & 0x7fffffff)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "tickets are collected in submission order");
  const int slot = (int)(oldest % MOD_PIPELINE_DEPTH);
  HIP_TRY(c, hipEventSynchronize(p.ev_out[slot]));
  if (p.odo[slot]) {
    const ModContext::Pipe::EgoSlot &e = *p.h_ego[slot];
    if (p.user_tf[slot]) *p.user_tf[slot] = e.tf;
    if (p.user_ego[slot]) *p.user_ego[slot] = e.res;
    if (e.res.status != MOD_EGO_OK) {   // visual odometry failed: the reference publishes nothing (scene_flow_constructor.cpp:251-255)
      p.in_flight--;
      return MOD_SKIP_NO_TRANSFORM;
    }
  }
  const int32_t n = *p.h_n[slot];
  if (n_objects) *n_objects = n;
  const int32_t ncopy = std::min(n, p.user_cap[slot]);
  if (p.user_obj[slot] && ncopy > 0) memcpy(p.user_obj[slot], p.h_obj[slot], sizeof(ModObject) * (size_t)ncopy);
  p.in_flight--;
  return MOD_OK;
}

int mod_forget_previous(ModContext *c) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  c->pipe.have_prev = false;
  c->pipe.have_prev_img = false;
  return MOD_OK;
}

}  // extern "C"
