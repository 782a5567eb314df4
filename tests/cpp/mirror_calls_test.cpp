// mirror_calls_test.cpp — what the host mirror (host/scene_flow_constructor.hpp, host/clusterer_nodelet.hpp) asks of the C ABI, call
// by call, without the library: ModContext is defined HERE as a call recorder and every mod_* function the two headers call is a stub
// that logs its name, its scalars (floating point with %a), its structs field by field and, for every pointer, WHICH buffer it is (a
// name the scenario registered, `null`, or `?`), returns a code the scenario queued and hands out tickets 0, 1, 2, ...  After each
// mirror call the scenario logs what the caller can see.  tests/test_mirror_calls.py compares the log with
// tests/golden/mirror_calls.txt byte for byte: the order of the calls, their arguments and the messages are pinned, on the CPU.
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#define private public   // the scenarios name the mirror's own buffers (pending_[i].objects, parked_, previous_pixels_)
#include "../../moving_object_detector_amd/host/scene_flow_constructor.hpp"
#include "../../moving_object_detector_amd/host/clusterer_nodelet.hpp"
#undef private

// ---- the recorder ----------------------------------------------------------------------------------------------------------
struct Submitted {   // what a submit handed over, for its collect
  ModObject *objects; int32_t max_objects; ModTransform *tf; ModEgoResult *ego;
};
struct ModContext {
  std::vector<std::pair<std::string, std::function<const void *()>>> names;   // evaluated at log time: vectors move when they grow
  std::map<std::string, std::deque<int>> codes;                                // return codes queued per function; default MOD_OK
  std::deque<int> counts;                                                      // object counts queued for collect / process / cluster
  std::deque<ModTransform> transforms;                                         // estimates queued for the collect of an odometry ticket
  std::deque<ModEgoResult> egos;
  std::map<int, Submitted> tickets;
  int next_ticket = 0;
  std::vector<void *> device;                                                  // mod_malloc'ed blocks, named dev0, dev1, ...
  ModClusterMembers members{};
  bool members_on = false;
  std::string error = "queued error text";

  void name(const std::string &n, std::function<const void *()> f) { names.emplace_back(n, std::move(f)); }
  std::string which(const void *p) const {
    if (!p) return "null";
    for (const auto &e : names) if (e.second() == p) return e.first;
    for (size_t i = 0; i < device.size(); i++) if (device[i] == p) return "dev" + std::to_string(i);
    return "?";
  }
  int code(const char *fn) {
    auto it = codes.find(fn);
    if (it == codes.end() || it->second.empty()) return MOD_OK;
    const int rc = it->second.front();
    it->second.pop_front();
    return rc;
  }
  int count() {
    if (counts.empty()) return 0;
    const int n = counts.front();
    counts.pop_front();
    return n;
  }
};

static void L(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vprintf(fmt, ap);
  va_end(ap);
  std::printf("\n");
}
static std::string tf_text(const ModTransform *t) {
  if (!t) return "null";
  char b[256];
  std::snprintf(b, sizeof b, "{t=%a,%a,%a q=%a,%a,%a,%a}", t->t[0], t->t[1], t->t[2], t->q[0], t->q[1], t->q[2], t->q[3]);
  return b;
}
static std::string sgm_text(const ModSgmParams *p) {
  if (!p) return "null";
  char b[128];
  std::snprintf(b, sizeof b, "{%d,%d,%d,%d,%d,%d}", p->disparities, p->p1, p->p2, p->paths, p->lr_check, p->median);
  return b;
}
static std::string flow_text(const ModFlowParams *p) {
  if (!p) return "null";
  char b[128];
  std::snprintf(b, sizeof b, "{%d,%d,%d,%d,%d}", p->levels, p->radius, p->window, p->subpixel, p->fb_check);
  return b;
}
static std::string ego_text(const ModEgoParams *p) {
  if (!p) return "null";
  char b[192];
  std::snprintf(b, sizeof b, "{%d,%d,%d,%d,%a,%a,%u,%d}", p->stride, p->hypotheses, p->iterations, p->min_inliers, p->inlier_threshold,
                p->min_disparity, p->seed, p->reserved);
  return b;
}
// the pattern an object array is filled with: recognisable by tag (ticket + 1; 80 and 90 for the synchronous calls) and index
static void pattern_objects(ModObject *objects, int32_t max_objects, int n, int tag) {
  for (int i = 0; objects && i < n && i < max_objects; i++) {
    ModObject o{};
    o.id = 100 * tag + i; o.n_points = 7 + i;
    for (int k = 0; k < 3; k++) { o.center[k] = tag + i / 16.0 + k; o.velocity[k] = -1.0 - k; o.bounding_box[k] = 0.5 * (k + 1); }
    o.orientation[3] = 1.0;
    objects[i] = o;
  }
}
// a ticket for a submit that returned MOD_OK
static void enqueue(ModContext *c, int rc, int32_t *ticket, ModObject *objects, int32_t max_objects, ModTransform *tf, ModEgoResult *ego) {
  if (rc != MOD_OK) return;
  *ticket = c->next_ticket++;
  c->tickets[*ticket] = Submitted{objects, max_objects, tf, ego};
}

// ---- the stubs: every mod_* function the two headers call ---------------------------------------------------------------------
extern "C" {
const char *mod_last_error(const ModContext *c) { L("  mod_last_error"); return c->error.c_str(); }
int mod_set_camera(ModContext *c, const ModCamera *m) {
  L("  mod_set_camera {%d,%d fx=%a fy=%a cx=%a cy=%a Tx=%a Ty=%a f=%a T=%a min=%a max=%a}", m->width, m->height, m->fx, m->fy, m->cx, m->cy,
    m->Tx, m->Ty, m->disp_f, m->disp_T, m->min_disparity, m->max_disparity);
  return c->code("mod_set_camera");
}
int mod_get_params(const ModContext *cc, ModParams *p) {
  ModContext *c = const_cast<ModContext *>(cc);
  const int rc = c->code("mod_get_params");
  L("  mod_get_params -> %d", rc);
  if (rc == MOD_OK) { p->dynamic_flow_diff = 7; p->cluster_size = 300; p->neighbor_distance = 2; p->reserved = 0; p->depth_diff = 0.25; p->dynamic_speed = 0.75; }
  return rc;
}
int mod_set_params(ModContext *c, const ModParams *p) {
  L("  mod_set_params {%d,%d,%d,%d,%a,%a}", p->dynamic_flow_diff, p->cluster_size, p->neighbor_distance, p->reserved, p->depth_diff, p->dynamic_speed);
  return c->code("mod_set_params");
}
int mod_set_disparity_subpixel(ModContext *c, int32_t bits) { L("  mod_set_disparity_subpixel %d", bits); return c->code("mod_set_disparity_subpixel"); }
int mod_set_disparity_filters(ModContext *c, const ModDisparityFilters *f) {
  L("  mod_set_disparity_filters {%d,%d,%d,%d}", f->uniqueness_ratio, f->speckle_size, f->speckle_range, f->reserved);
  return c->code("mod_set_disparity_filters");
}
int mod_set_flow_propagation(ModContext *c, int32_t seeds) { L("  mod_set_flow_propagation %d", seeds); return c->code("mod_set_flow_propagation"); }
int mod_set_image_binning(ModContext *c, const ModImageBinning *b) {
  L("  mod_set_image_binning {%d,%d,%d,%d}", b->bx, b->by, b->mode, b->reserved);
  return c->code("mod_set_image_binning");
}
int mod_set_side_by_side(ModContext *c, int32_t on) { L("  mod_set_side_by_side %d", on); return c->code("mod_set_side_by_side"); }
int mod_set_image_layout(ModContext *c, const ModImageLayout *l) {
  L("  mod_set_image_layout {enc=%d %dx%d step=%d x0=%d y0=%d}", l->encoding, l->width, l->height, l->step, l->x0, l->y0);
  return c->code("mod_set_image_layout");
}
int mod_set_depth_layout(ModContext *c, const ModDepthLayout *l) {
  L("  mod_set_depth_layout {enc=%d %dx%d step=%d x0=%d y0=%d unit=%a}", l->encoding, l->width, l->height, l->step, l->x0, l->y0, l->unit);
  return c->code("mod_set_depth_layout");
}
int mod_set_depth_registration(ModContext *c, const ModDepthRegistration *r) {
  if (!r) L("  mod_set_depth_registration null");
  else L("  mod_set_depth_registration {fx=%a fy=%a cx=%a cy=%a R=%a,%a,%a,%a,%a,%a,%a,%a,%a t=%a,%a,%a}", r->fx, r->fy, r->cx, r->cy, r->R[0], r->R[1],
         r->R[2], r->R[3], r->R[4], r->R[5], r->R[6], r->R[7], r->R[8], r->t[0], r->t[1], r->t[2]);
  return c->code("mod_set_depth_registration");
}
int mod_set_depth_splat(ModContext *c, int32_t on) { L("  mod_set_depth_splat %d", on); return c->code("mod_set_depth_splat"); }
int mod_forget_previous(ModContext *c) { L("  mod_forget_previous"); return c->code("mod_forget_previous"); }
int mod_depth_image_host(ModContext *c, const float *disparity_now, float *depth) {
  L("  mod_depth_image_host disparity_now=%s depth=%s", c->which(disparity_now).c_str(), c->which(depth).c_str());
  return c->code("mod_depth_image_host");
}
int mod_sgm_compute_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *params, float *disparity) {
  L("  mod_sgm_compute_host left=%s right=%s sgm=%s disparity=%s", c->which(left).c_str(), c->which(right).c_str(), sgm_text(params).c_str(),
    c->which(disparity).c_str());
  return c->code("mod_sgm_compute_host");
}
// `objects` of the two synchronous calls is an array local to the mirror's function: it cannot be registered, `local` says it is
// none of the registered buffers either; n_objects and ticket are locals too and are only said to be there
int mod_process_frame_host(ModContext *c, const float *disparity_now, const float *disparity_prev, const float *flow, const ModTransform *transform,
                           double dt, void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects, int32_t *n_objects) {
  const std::string o = c->which(objects);
  L("  mod_process_frame_host disparity_now=%s disparity_prev=%s flow=%s transform=%s dt=%a cloud=%s labels=%s objects=%s max_objects=%d n_objects=%s",
    c->which(disparity_now).c_str(), c->which(disparity_prev).c_str(), c->which(flow).c_str(), tf_text(transform).c_str(), dt, c->which(cloud_aos).c_str(),
    c->which(labels).c_str(), o == "?" ? "local" : o.c_str(), max_objects, n_objects ? "out" : "null");
  const int rc = c->code("mod_process_frame_host");
  if (rc == MOD_OK && n_objects) { *n_objects = c->count(); pattern_objects(objects, max_objects, *n_objects, 90); }
  return rc;
}
int mod_cluster_cloud_host(ModContext *c, const void *cloud, int32_t width, int32_t height, int32_t point_step, int32_t row_step, int32_t *labels,
                           ModObject *objects, int32_t max_objects, int32_t *n_objects) {
  const std::string o = c->which(objects);
  L("  mod_cluster_cloud_host cloud=%s %dx%d point_step=%d row_step=%d labels=%s objects=%s max_objects=%d n_objects=%s", c->which(cloud).c_str(), width,
    height, point_step, row_step, c->which(labels).c_str(), o == "?" ? "local" : o.c_str(), max_objects, n_objects ? "out" : "null");
  const int rc = c->code("mod_cluster_cloud_host");
  if (rc != MOD_OK) return rc;
  if (n_objects) { *n_objects = c->count(); pattern_objects(objects, max_objects, *n_objects, 80); }
  if (c->members_on) {   // two clusters of 3 and 2 members; the scenario's lists hold 5 offsets and 12 indices
    const int32_t offsets[5] = {0, 3, 5, 5, 5}, indices[5] = {1, 5, 9, 2, 6};
    std::memcpy(c->members.offsets, offsets, sizeof offsets);
    std::memcpy(c->members.indices, indices, sizeof indices);
    for (int i = 0; c->members.points && i < 15; i++) c->members.points[i] = 0.25f * i;
  }
  return rc;
}
int mod_set_cluster_members(ModContext *c, const ModClusterMembers *m) {
  if (!m) L("  mod_set_cluster_members null");
  else L("  mod_set_cluster_members {offsets=%s indices=%s points=%s reserved=%lld}", c->which(m->offsets).c_str(), c->which(m->indices).c_str(),
         c->which(m->points).c_str(), (long long)m->reserved);
  const int rc = c->code("mod_set_cluster_members");
  if (rc == MOD_OK) { c->members_on = m != nullptr; c->members = m ? *m : ModClusterMembers{}; }
  return rc;
}
int mod_malloc(ModContext *c, uint64_t bytes, void **dev_ptr) {
  const int rc = c->code("mod_malloc");
  if (rc == MOD_OK) { *dev_ptr = std::calloc(1, bytes); c->device.push_back(*dev_ptr); }
  L("  mod_malloc %llu -> %d %s", (unsigned long long)bytes, rc, rc == MOD_OK ? c->which(*dev_ptr).c_str() : "-");
  return rc;
}
int mod_free(ModContext *c, void *dev_ptr) {
  L("  mod_free %s", c->which(dev_ptr).c_str());
  for (void *&p : c->device) if (p == dev_ptr) { std::free(p); p = nullptr; }   // the name stays taken: dev<i> is never handed out twice
  return c->code("mod_free");
}
int mod_memcpy_d2h(ModContext *c, void *host_dst, const void *dev_src, uint64_t bytes) {
  L("  mod_memcpy_d2h dst=%s src=%s bytes=%llu", host_dst ? "host" : "null", c->which(dev_src).c_str(), (unsigned long long)bytes);
  const int rc = c->code("mod_memcpy_d2h");
  if (rc == MOD_OK) std::memcpy(host_dst, dev_src, bytes);
  return rc;
}
int mod_submit_frame_host(ModContext *c, const float *disparity_now, const float *disparity_prev, const float *flow, const ModTransform *transform, double dt,
                          void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects, int32_t *ticket) {
  L("  mod_submit_frame_host disparity_now=%s disparity_prev=%s flow=%s transform=%s dt=%a cloud=%s labels=%s objects=%s max_objects=%d ticket=%s",
    c->which(disparity_now).c_str(), c->which(disparity_prev).c_str(), c->which(flow).c_str(), tf_text(transform).c_str(), dt, c->which(cloud_aos).c_str(),
    c->which(labels).c_str(), c->which(objects).c_str(), max_objects, ticket ? "out" : "null");
  const int rc = c->code("mod_submit_frame_host");
  enqueue(c, rc, ticket, objects, max_objects, nullptr, nullptr);
  return rc;
}
int mod_submit_stereo_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm, const float *flow, const ModTransform *transform,
                           double dt, void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects, float *disparity, int32_t *ticket) {
  L("  mod_submit_stereo_host left=%s right=%s sgm=%s flow=%s transform=%s dt=%a cloud=%s labels=%s objects=%s max_objects=%d disparity=%s ticket=%s",
    c->which(left).c_str(), c->which(right).c_str(), sgm_text(sgm).c_str(), c->which(flow).c_str(), tf_text(transform).c_str(), dt,
    c->which(cloud_aos).c_str(), c->which(labels).c_str(), c->which(objects).c_str(), max_objects, c->which(disparity).c_str(), ticket ? "out" : "null");
  const int rc = c->code("mod_submit_stereo_host");
  enqueue(c, rc, ticket, objects, max_objects, nullptr, nullptr);
  return rc;
}
int mod_submit_odometry_host(ModContext *c, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm, const ModFlowParams *flow_prm,
                             const ModEgoParams *ego_prm, double dt, void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects,
                             float *disparity, float *flow_out, ModTransform *transform_out, ModEgoResult *ego_out, int32_t *ticket) {
  L("  mod_submit_odometry_host left=%s right=%s sgm=%s flow_prm=%s ego_prm=%s dt=%a cloud=%s labels=%s objects=%s max_objects=%d disparity=%s flow_out=%s "
    "transform_out=%s ego_out=%s ticket=%s",
    c->which(left).c_str(), c->which(right).c_str(), sgm_text(sgm).c_str(), flow_text(flow_prm).c_str(), ego_text(ego_prm).c_str(), dt,
    c->which(cloud_aos).c_str(), c->which(labels).c_str(), c->which(objects).c_str(), max_objects, c->which(disparity).c_str(), c->which(flow_out).c_str(),
    c->which(transform_out).c_str(), c->which(ego_out).c_str(), ticket ? "out" : "null");
  const int rc = c->code("mod_submit_odometry_host");
  enqueue(c, rc, ticket, objects, max_objects, transform_out, ego_out);
  return rc;
}
int mod_submit_depth_host(ModContext *c, const uint8_t *image, const void *depth, const ModFlowParams *flow_prm, const ModEgoParams *ego_prm,
                          const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects, float *disparity,
                          float *flow_out, ModTransform *transform_out, ModEgoResult *ego_out, int32_t *ticket) {
  L("  mod_submit_depth_host image=%s depth=%s flow_prm=%s ego_prm=%s transform=%s dt=%a cloud=%s labels=%s objects=%s max_objects=%d disparity=%s flow_out=%s "
    "transform_out=%s ego_out=%s ticket=%s",
    c->which(image).c_str(), c->which(depth).c_str(), flow_text(flow_prm).c_str(), ego_text(ego_prm).c_str(), tf_text(transform).c_str(), dt,
    c->which(cloud_aos).c_str(), c->which(labels).c_str(), c->which(objects).c_str(), max_objects, c->which(disparity).c_str(), c->which(flow_out).c_str(),
    c->which(transform_out).c_str(), c->which(ego_out).c_str(), ticket ? "out" : "null");
  const int rc = c->code("mod_submit_depth_host");
  enqueue(c, rc, ticket, objects, max_objects, transform_out, ego_out);
  return rc;
}
int mod_collect_frame_host(ModContext *c, int32_t ticket, int32_t *n_objects) {
  const int rc = c->code("mod_collect_frame_host");
  L("  mod_collect_frame_host ticket=%d n_objects=%s -> %d", ticket, n_objects ? "out" : "null", rc);
  auto it = c->tickets.find(ticket);
  if (it == c->tickets.end()) return MOD_ERR_INVALID_ARGUMENT;
  const Submitted s = it->second;
  c->tickets.erase(it);
  const int n = c->count();
  if (n_objects) *n_objects = n;
  pattern_objects(s.objects, s.max_objects, n, ticket + 1);
  if (s.tf) {          // an odometry ticket: the estimate arrives through the pointers its submit received
    ModTransform t{{0.125 * (ticket + 1), 0.25, -0.5}, {0.0, 0.0, 0.0, 1.0}};
    if (!c->transforms.empty()) { t = c->transforms.front(); c->transforms.pop_front(); }
    *s.tf = t;
  }
  if (s.ego) {
    ModEgoResult e{MOD_EGO_OK, 40, 30, 3, 0.5};
    if (!c->egos.empty()) { e = c->egos.front(); c->egos.pop_front(); }
    *s.ego = e;
  }
  return rc;
}
}   // extern "C"

// ---- what the caller can see ------------------------------------------------------------------------------------------------
using scene_flow_constructor::SceneFlowConstructor;
using scene_flow_clusterer::ClustererNodelet;
static const int W = 4, H = 3, N = W * H;   // the smallest camera that tells width from height

static std::string header_text(const mod_host::Header &h) {
  char b[160];
  std::snprintf(b, sizeof b, "{seq=%u stamp=%u.%09u frame=%s}", h.seq, h.stamp.sec, h.stamp.nsec, h.frame_id.c_str());
  return b;
}
static mod_host::Header header(uint32_t seq, uint32_t sec, uint32_t nsec, const char *frame) {
  mod_host::Header h;
  h.seq = seq; h.stamp = mod_host::Time(sec, nsec); h.frame_id = frame;
  return h;
}
static void show_objects(const char *what, const mod_host::MovingObjectArray &m) {
  std::string s;
  for (const auto &o : m.moving_object_array) { char b[64]; std::snprintf(b, sizeof b, " (%d %a)", o.id, o.center.position[0]); s += b; }
  L("    %s: header=%s n=%zu%s", what, header_text(m.header).c_str(), m.moving_object_array.size(), s.c_str());
}

// one constructor on one recorder, with the messages a caller hands in and gets back
struct Rig {
  ModContext ctx;
  SceneFlowConstructor sfc{&ctx};
  mod_host::PointCloud2 cloud;
  mod_host::MovingObjectArray objs;
  std::vector<float> flow_out, disparity_out, depth_image;
  std::vector<int32_t> labels;
  mod_host::Transform motion;
  // inputs: pixel buffers with fixed addresses
  std::vector<float> d[MOD_PIPELINE_DEPTH + 3], flow_pixels;
  std::vector<uint8_t> left_pixels, right_pixels, wide_pixels, other_wide_pixels, depth_pixels, colour_left, colour_right;
  mod_host::Transform tf;

  Rig() {
    for (int k = 0; k < MOD_PIPELINE_DEPTH + 3; k++) {
      d[k].assign(N, (float)k + 0.5f);
      ctx.name("d[" + std::to_string(k) + "].data", [this, k] { return (const void *)d[k].data(); });
    }
    flow_pixels.assign(2 * N, 0.25f);
    left_pixels.assign(N, 1); right_pixels.assign(N, 2); wide_pixels.assign(2 * N, 3); other_wide_pixels.assign(2 * N, 4); depth_pixels.assign(4 * N, 5);
    colour_left.assign(64 * 8, 6); colour_right.assign(64 * 8, 7);
    ctx.name("flow.data", [this] { return (const void *)flow_pixels.data(); });
    ctx.name("left.data", [this] { return (const void *)left_pixels.data(); });
    ctx.name("right.data", [this] { return (const void *)right_pixels.data(); });
    ctx.name("wide.data", [this] { return (const void *)wide_pixels.data(); });
    ctx.name("other_wide.data", [this] { return (const void *)other_wide_pixels.data(); });
    ctx.name("depth.data", [this] { return (const void *)depth_pixels.data(); });
    ctx.name("colour_left.data", [this] { return (const void *)colour_left.data(); });
    ctx.name("colour_right.data", [this] { return (const void *)colour_right.data(); });
    ctx.name("cloud.data", [this] { return (const void *)cloud.data.data(); });
    ctx.name("flow_out", [this] { return (const void *)flow_out.data(); });
    ctx.name("disparity_out", [this] { return (const void *)disparity_out.data(); });
    ctx.name("depth_image", [this] { return (const void *)depth_image.data(); });
    ctx.name("labels", [this] { return (const void *)labels.data(); });
    ctx.name("parked", [this] { return (const void *)sfc.parked_.data(); });
    ctx.name("previous_pixels", [this] { return (const void *)sfc.previous_pixels_.data(); });
    for (int i = 0; i < MOD_PIPELINE_DEPTH; i++) {
      const std::string p = "pending[" + std::to_string(i) + "].";
      ctx.name(p + "objects", [this, i] { return (const void *)sfc.pending_[i].objects.data(); });
      ctx.name(p + "tf", [this, i] { return (const void *)&sfc.pending_[i].tf; });
      ctx.name(p + "ego", [this, i] { return (const void *)&sfc.pending_[i].ego; });
    }
    tf.translation[0] = 0.5; tf.translation[1] = -0.25; tf.translation[2] = 2.0;
    tf.rotation[0] = 0.0; tf.rotation[1] = 0.6; tf.rotation[2] = 0.0; tf.rotation[3] = 0.8;
    sfc.setMaxObjects(3);
    // messages that carry something recognisable, so that "not touched" shows
    cloud.header = header(77, 7, 7, "untouched"); objs.header = header(88, 8, 8, "untouched");
    motion.translation[0] = -9.0;
  }
  void camera() {
    mod_host::CameraInfo info;
    info.width = W; info.height = H;
    for (int i = 0; i < 12; i++) info.P[i] = 10.0 + i;
    mod_host::DisparityImage disparity;
    disparity.f = 10.0f; disparity.T = 0.125f; disparity.min_disparity = 0.0f; disparity.max_disparity = 127.0f;
    L("setCameraInfo");
    sfc.setCameraInfo(info, disparity);
  }
  mod_host::DisparityImage disparity(int k, uint32_t sec, uint32_t nsec) {
    mod_host::DisparityImage m;
    m.header = header(10 + k, sec, nsec, "disparity"); m.width = W; m.height = H; m.data = d[k].data();
    return m;
  }
  mod_host::FlowImage flow(uint32_t seq, uint32_t sec, uint32_t nsec) {
    mod_host::FlowImage m;
    m.header = header(seq, sec, nsec, "flow"); m.width = W; m.height = H; m.data = flow_pixels.data();
    return m;
  }
  static mod_host::Image image(const std::vector<uint8_t> &pixels, int w, int h, uint32_t seq, uint32_t sec, uint32_t nsec, const char *frame) {
    mod_host::Image m;
    m.header = header(seq, sec, nsec, frame); m.width = w; m.height = h; m.data = pixels.data();
    return m;
  }
  void state() {
    L("    cloud: header=%s width=%u height=%u row_step=%u is_dense=%d data.size=%zu", header_text(cloud.header).c_str(), cloud.width, cloud.height,
      cloud.row_step, (int)cloud.is_dense, cloud.data.size());
    show_objects("objects", objs);
    L("    sizes: flow_out=%zu disparity_out=%zu labels=%zu depth_image=%zu", flow_out.size(), disparity_out.size(), labels.size(), depth_image.size());
    L("    motion: t=%a,%a,%a q=%a,%a,%a,%a", motion.translation[0], motion.translation[1], motion.translation[2], motion.rotation[0], motion.rotation[1],
      motion.rotation[2], motion.rotation[3]);
    const mod_host::Pose &p = sfc.integratedPose();
    L("    integratedPose: R=%a,%a,%a,%a,%a,%a,%a,%a,%a t=%a,%a,%a", p.R[0][0], p.R[0][1], p.R[0][2], p.R[1][0], p.R[1][1], p.R[1][2], p.R[2][0], p.R[2][1],
      p.R[2][2], p.t[0], p.t[1], p.t[2]);
  }
  // one mirror call: its name, the stubs' lines, the value returned or the exception, what the caller can see
  template <class F> void call(const char *what, F f) {
    L("%s", what);
    try { L("  returns: %d", (int)f()); }
    catch (const std::exception &e) { L("  throws: %s", e.what()); }
    state();
  }
};

// ---- scenarios -----------------------------------------------------------------------------------------------------------------
static void scenario_submit() {
  L("== submit");
  Rig r;
  r.camera();
  mod_host::DisparityImage d0 = r.disparity(0, 100, 900000000), d1 = r.disparity(1, 101, 100000000), d2 = r.disparity(2, 101, 350000000),
                           d3 = r.disparity(3, 102, 0), d4 = r.disparity(4, 102, 500000000), d5 = r.disparity(5, 103, 250000000);
  mod_host::FlowImage f1 = r.flow(21, 101, 100000001), f2 = r.flow(22, 101, 350000001);
  // the first frame has no flow: skipped, its disparity parked on the host
  r.ctx.codes["mod_submit_frame_host"] = {MOD_SKIP_NO_FLOW};
  int t0 = -2, t1 = -2, t2 = -2;
  r.call("submit(d0, no flow): skipped", [&] { return t0 = r.sfc.submit(&d0, nullptr, &r.tf, &r.cloud, &r.objs); });
  r.call("submit(d1): the parked copy is the previous disparity", [&] { return t1 = r.sfc.submit(&d1, &f1, &r.tf, &r.cloud, &r.objs); });
  r.call("submit(d2): the previous disparity is resident", [&] { return t2 = r.sfc.submit(&d2, &f2, nullptr, &r.cloud, nullptr); });
  r.ctx.counts = {5, 2};   // 5 > the capacity of 3
  r.call("collect(first ticket)", [&] { r.sfc.collect(t1); return 0; });
  r.call("collect(second ticket)", [&] { r.sfc.collect(t2); return 0; });
  r.call("collect(second ticket) again: unknown", [&] { r.sfc.collect(t2); return 0; });
  r.call("collectOdometry(99): unknown", [&] { return (int)r.sfc.collectOdometry(99, &r.motion); });
  // a null disparity forgets the previous frame, the stamp and the park
  r.call("submit(null)", [&] { return r.sfc.submit(nullptr, &f2, &r.tf, &r.cloud, &r.objs); });
  r.call("submit(d3) after null: dt is 0", [&] { return t0 = r.sfc.submit(&d3, &f2, &r.tf, &r.cloud, &r.objs); });
  r.call("collect", [&] { r.sfc.collect(t0); return 0; });
  // a skip, then a null disparity: the park is cleared
  r.ctx.codes["mod_submit_frame_host"] = {MOD_SKIP_NO_DISPARITY_PREV};
  r.call("submit(d4): skipped and parked", [&] { return r.sfc.submit(&d4, &f2, &r.tf, nullptr, &r.objs); });
  r.call("submit(null) clears the park", [&] { return r.sfc.submit(nullptr, nullptr, nullptr, nullptr, nullptr); });
  r.call("submit(d5): nothing parked", [&] { return t0 = r.sfc.submit(&d5, &f2, &r.tf, nullptr, &r.objs); });
  r.call("collect", [&] { r.sfc.collect(t0); return 0; });
  // a negative code throws and leaves the slot: the next submit uses the same one; dt comes from the stamp stored by the failed call
  r.ctx.codes["mod_submit_frame_host"] = {MOD_ERR_DEVICE};
  r.call("submit(d0): the library fails", [&] { return r.sfc.submit(&d0, &f1, &r.tf, &r.cloud, &r.objs); });
  r.call("submit(d1): the same slot", [&] { return t0 = r.sfc.submit(&d1, &f1, &r.tf, &r.cloud, &r.objs); });
  r.call("collect", [&] { r.sfc.collect(t0); return 0; });
  // the slot ring wraps
  for (int k = 0; k < MOD_PIPELINE_DEPTH + 2; k++) {
    mod_host::DisparityImage dk = r.disparity(k, 200 + k, 1000u * k);
    r.call("submit: ring", [&] { return t0 = r.sfc.submit(&dk, &f1, &r.tf, &r.cloud, &r.objs); });
    r.ctx.counts = {1};
    r.call("collect: ring", [&] { r.sfc.collect(t0); return 0; });
  }
  // collect() throws what the library reports
  mod_host::DisparityImage dk = r.disparity(0, 300, 0);
  r.call("submit", [&] { return t0 = r.sfc.submit(&dk, &f1, &r.tf, &r.cloud, &r.objs); });
  r.ctx.codes["mod_collect_frame_host"] = {MOD_ERR_DEVICE};
  r.call("collect: the library fails", [&] { r.sfc.collect(t0); return 0; });
}

static void scenario_submit_stereo() {
  L("== submitStereo");
  Rig r;
  r.camera();
  mod_host::Image l = Rig::image(r.left_pixels, W, H, 31, 50, 0, "left"), rt = Rig::image(r.right_pixels, W, H, 32, 50, 0, "right");
  mod_host::Image big = Rig::image(r.wide_pixels, W + 1, H, 33, 50, 500000000, "left_big");
  mod_host::FlowImage f = r.flow(41, 50, 1);
  int t = -2;
  r.call("submitStereo: usable images", [&] { return t = r.sfc.submitStereo(&l, &rt, &f, &r.tf, &r.cloud, &r.objs); });
  r.ctx.counts = {2};
  r.call("collect", [&] { r.sfc.collect(t); return 0; });
  l.header.stamp = mod_host::Time(50, 250000000);
  r.call("submitStereo: no cloud, no objects", [&] { return t = r.sfc.submitStereo(&l, &rt, &f, nullptr, nullptr, nullptr); });
  r.call("collect", [&] { r.sfc.collect(t); return 0; });
  // a left image of another size than the camera: null images, the stamp forgotten, the cloud not touched
  r.cloud.data.clear();
  r.ctx.codes["mod_submit_stereo_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitStereo: image of the wrong size", [&] { return r.sfc.submitStereo(&big, &rt, &f, &r.tf, &r.cloud, &r.objs); });
  l.header.stamp = mod_host::Time(51, 0);
  r.ctx.codes["mod_submit_stereo_host"] = {MOD_SKIP_NO_DISPARITY_PREV};
  r.call("submitStereo: the next frame has dt 0 and is skipped", [&] { return r.sfc.submitStereo(&l, &rt, &f, &r.tf, &r.cloud, &r.objs); });
  l.header.stamp = mod_host::Time(51, 500000000);
  r.call("submitStereo: the frame after", [&] { return t = r.sfc.submitStereo(&l, &rt, &f, &r.tf, &r.cloud, &r.objs); });
  r.call("collect", [&] { r.sfc.collect(t); return 0; });
  // the layout is refused: the images are unusable
  r.ctx.codes["mod_set_image_layout"] = {MOD_ERR_INVALID_ARGUMENT};
  r.ctx.codes["mod_submit_stereo_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitStereo: the library refuses the layout", [&] { return r.sfc.submitStereo(&l, &rt, &f, &r.tf, &r.cloud, &r.objs); });
  // a negative code
  r.ctx.codes["mod_submit_stereo_host"] = {MOD_ERR_CAPACITY};
  r.call("submitStereo: the library fails", [&] { return r.sfc.submitStereo(&l, &rt, &f, &r.tf, &r.cloud, &r.objs); });
  // side by side: one message of twice the width
  mod_host::Image wide = Rig::image(r.wide_pixels, 2 * W, H, 34, 52, 0, "wide"), other = Rig::image(r.other_wide_pixels, 2 * W, H, 35, 52, 0, "other_wide");
  r.sfc.setSideBySide(true);
  r.call("submitStereo: side by side, right == nullptr", [&] { return t = r.sfc.submitStereo(&wide, nullptr, &f, &r.tf, &r.cloud, &r.objs); });
  r.call("collect", [&] { r.sfc.collect(t); return 0; });
  wide.header.stamp = mod_host::Time(52, 125000000);
  r.call("submitStereo: side by side, right == left", [&] { return t = r.sfc.submitStereo(&wide, &wide, &f, &r.tf, &r.cloud, &r.objs); });
  r.call("collect", [&] { r.sfc.collect(t); return 0; });
  r.ctx.codes["mod_submit_stereo_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitStereo: side by side, two distinct images", [&] { return r.sfc.submitStereo(&wide, &other, &f, &r.tf, &r.cloud, &r.objs); });
  r.ctx.codes["mod_submit_stereo_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitStereo: side by side, camera-sized images", [&] { return r.sfc.submitStereo(&l, &rt, &f, &r.tf, &r.cloud, &r.objs); });
  r.sfc.setSideBySide(false);
  for (int k = 0; k < MOD_PIPELINE_DEPTH + 2; k++) {
    l.header.stamp = mod_host::Time(60 + k, 0);
    r.call("submitStereo: ring", [&] { return t = r.sfc.submitStereo(&l, &rt, &f, nullptr, &r.cloud, &r.objs); });
    r.ctx.counts = {1};
    r.call("collect: ring", [&] { r.sfc.collect(t); return 0; });
  }
  // estimateDisparity shares the layout path
  mod_host::CameraInfo li, ri;
  li.width = ri.width = W; li.height = ri.height = H;
  li.P[0] = ri.P[0] = 8.0; ri.P[3] = -2.0;
  mod_host::DisparityImage out;
  std::vector<float> pixels;
  r.ctx.name("pixels", [&pixels] { return (const void *)pixels.data(); });
  r.call("estimateDisparity", [&] { return (int)r.sfc.estimateDisparity(&l, &rt, li, ri, &out, &pixels); });
  L("    disparity: header=%s %dx%d data=%s f=%a T=%a min=%a max=%a pixels=%zu", header_text(out.header).c_str(), out.width, out.height,
    r.ctx.which(out.data).c_str(), out.f, out.T, out.min_disparity, out.max_disparity, pixels.size());
  r.ctx.codes["mod_sgm_compute_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("estimateDisparity: skipped", [&] { return (int)r.sfc.estimateDisparity(&l, &rt, li, ri, &out, &pixels); });
  r.sfc.setSideBySide(true);
  r.call("estimateDisparity: side by side, two distinct images", [&] { return (int)r.sfc.estimateDisparity(&l, &rt, li, ri, &out, &pixels); });
  r.ctx.names.pop_back();
}

static void scenario_submit_odometry() {
  L("== submitOdometry");
  Rig r;
  r.camera();
  // colour messages of 20 x 8 pixels with padded rows (64 > 20 * 3) and the camera-sized window at (5, 2)
  mod_host::Image l = Rig::image(r.colour_left, 20, 8, 51, 10, 0, "left"), rt = Rig::image(r.colour_right, 20, 8, 52, 10, 0, "right");
  l.encoding = rt.encoding = "bgr8"; l.step = rt.step = 64;
  int t = -2;
  r.ctx.codes["mod_submit_odometry_host"] = {MOD_SKIP_NO_FLOW};
  r.call("submitOdometry: first frame", [&] { return r.sfc.submitOdometry(&l, &rt, &r.objs, &r.flow_out, 5, 2, &r.disparity_out, &r.cloud); });
  l.header.stamp = rt.header.stamp = mod_host::Time(10, 40000000);
  r.call("submitOdometry: second frame", [&] { return t = r.sfc.submitOdometry(&l, &rt, &r.objs, &r.flow_out, 5, 2, &r.disparity_out, &r.cloud); });
  r.ctx.counts = {2};
  r.ctx.transforms = {ModTransform{{1.0, 2.0, 3.0}, {0.0, 0.0, 0.6, 0.8}}};
  r.call("collectOdometry: the estimate succeeded", [&] { return (int)r.sfc.collectOdometry(t, &r.motion); });
  // the estimate failed in the library: MOD_SKIP_NO_TRANSFORM
  l.header.stamp = mod_host::Time(10, 80000000);
  r.call("submitOdometry: objects only", [&] { return t = r.sfc.submitOdometry(&l, &rt, &r.objs); });
  r.ctx.codes["mod_collect_frame_host"] = {MOD_SKIP_NO_TRANSFORM};
  r.ctx.egos = {ModEgoResult{MOD_EGO_OK, 1, 1, 1, 0.0}};
  r.call("collectOdometry: MOD_SKIP_NO_TRANSFORM", [&] { return (int)r.sfc.collectOdometry(t, &r.motion); });
  l.header.stamp = mod_host::Time(10, 120000000);
  r.call("submitOdometry: nothing asked for", [&] { return t = r.sfc.submitOdometry(&l, &rt, nullptr); });
  r.ctx.egos = {ModEgoResult{MOD_EGO_FEW_INLIERS, 9, 2, 0, 0.0}};
  r.call("collectOdometry: MOD_EGO_FEW_INLIERS", [&] { return (int)r.sfc.collectOdometry(t, nullptr); });
  // missing images: the outputs are still resized, the stamp is forgotten
  r.flow_out.clear(); r.disparity_out.clear(); r.cloud.data.clear();
  r.ctx.codes["mod_submit_odometry_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitOdometry: missing images", [&] { return r.sfc.submitOdometry(nullptr, nullptr, &r.objs, &r.flow_out, 0, 0, &r.disparity_out, &r.cloud); });
  rt.step = 60;
  r.ctx.codes["mod_submit_odometry_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitOdometry: left and right disagree", [&] { return r.sfc.submitOdometry(&l, &rt, &r.objs, &r.flow_out, 5, 2); });
  rt.step = 64;
  l.encoding = rt.encoding = "16UC1";
  r.ctx.codes["mod_submit_odometry_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitOdometry: unknown encoding", [&] { return r.sfc.submitOdometry(&l, &rt, &r.objs); });
  l.encoding = rt.encoding = "bgr8";
  r.ctx.codes["mod_submit_odometry_host"] = {MOD_ERR_NOT_CONFIGURED};
  r.call("submitOdometry: the library fails", [&] { return r.sfc.submitOdometry(&l, &rt, &r.objs); });
  // estimator parameters and context settings are handed on
  r.sfc.setDisparityParams(ModSgmParams{64, 5, 80, 4, 0, 1});
  r.sfc.setEgoParams(ModEgoParams{2, 128, 5, 20, 1.5f, 0.5f, 11u, 0});
  L("setters");
  r.sfc.setDisparitySubpixel(true); r.sfc.setDisparitySubpixel(false); r.sfc.setDisparityFilters(10, 100, 2); r.sfc.setFlowPropagation(5);
  r.sfc.setImageBinning(2, 2); r.sfc.setImageBinning(1, 2, MOD_BIN_NEAREST); r.sfc.setDepthSplat(true); r.sfc.setDepthRegistration(nullptr);
  const ModDepthRegistration reg{1.0, 2.0, 3.0, 4.0, {1, 0, 0, 0, 1, 0, 0, 0, 1}, {0.5, 0.25, 0.125}};
  r.sfc.setDepthRegistration(&reg);
  r.ctx.codes["mod_set_flow_propagation"] = {MOD_ERR_INVALID_ARGUMENT};
  r.call("setFlowPropagation: refused", [&] { r.sfc.setFlowPropagation(3); return 0; });
  // side by side
  mod_host::Image wide = Rig::image(r.wide_pixels, 2 * W, H, 53, 11, 0, "wide");
  r.sfc.setSideBySide(true);
  r.call("submitOdometry: side by side, right == nullptr", [&] { return t = r.sfc.submitOdometry(&wide, nullptr, &r.objs); });
  r.call("collectOdometry", [&] { return (int)r.sfc.collectOdometry(t, &r.motion); });
  r.ctx.codes["mod_submit_odometry_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitOdometry: side by side, two distinct images", [&] { return r.sfc.submitOdometry(&l, &rt, &r.objs, nullptr, 5, 2); });
  r.sfc.setSideBySide(false);
  for (int k = 0; k < MOD_PIPELINE_DEPTH + 2; k++) {
    l.header.stamp = mod_host::Time(20 + k, 0);
    r.call("submitOdometry: ring", [&] { return t = r.sfc.submitOdometry(&l, &rt, &r.objs, &r.flow_out, 5, 2, &r.disparity_out, &r.cloud); });
    r.ctx.counts = {1};
    r.call("collectOdometry: ring", [&] { return (int)r.sfc.collectOdometry(t, &r.motion); });
  }
  // an odometry ticket joined by collect(): MOD_SKIP_NO_TRANSFORM does not throw
  r.call("submitOdometry", [&] { return t = r.sfc.submitOdometry(&l, &rt, &r.objs); });
  r.ctx.codes["mod_collect_frame_host"] = {MOD_SKIP_NO_TRANSFORM};
  r.call("collect of an odometry ticket", [&] { r.sfc.collect(t); return 0; });
  r.call("submitOdometry", [&] { return t = r.sfc.submitOdometry(&l, &rt, &r.objs); });
  r.ctx.codes["mod_collect_frame_host"] = {MOD_ERR_DEVICE};
  r.call("collectOdometry: the library fails", [&] { return (int)r.sfc.collectOdometry(t, &r.motion); });
  // the pose arithmetic on its own
  L("integrateEstimate");
  const ModTransform step{{0.5, 0.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
  L("  returns: %d", (int)r.sfc.integrateEstimate(step, MOD_EGO_DIVERGED));
  r.state();
  L("  returns: %d", (int)r.sfc.integrateEstimate(step, MOD_EGO_OK));
  r.state();
}

static void scenario_submit_depth() {
  L("== submitDepth");
  Rig r;
  r.camera();
  mod_host::Image im = Rig::image(r.left_pixels, W, H, 61, 30, 0, "image"), dm = Rig::image(r.depth_pixels, W, H, 62, 30, 0, "depth");
  dm.encoding = "16UC1";
  r.call("setDepthLayout: 16UC1, step 0", [&] { return (int)r.sfc.setDepthLayout(dm); });
  dm.encoding = "32FC1"; dm.step = 20;
  r.call("setDepthLayout: 32FC1, step, origin, unit", [&] { return (int)r.sfc.setDepthLayout(dm, 1, 2, 0.001f); });
  dm.encoding = "mono16";
  r.call("setDepthLayout: unknown encoding", [&] { return (int)r.sfc.setDepthLayout(dm); });
  dm.encoding = "16UC1"; dm.step = 0;
  r.ctx.codes["mod_set_depth_layout"] = {MOD_ERR_INVALID_ARGUMENT};
  r.call("setDepthLayout: refused", [&] { return (int)r.sfc.setDepthLayout(dm); });
  int t = -2;
  r.ctx.codes["mod_submit_depth_host"] = {MOD_SKIP_NO_FLOW};
  r.call("submitDepth: first frame, caller's transform", [&] { return r.sfc.submitDepth(&im, &dm, &r.objs, &r.tf, &r.flow_out, 0, 0, &r.disparity_out, &r.cloud); });
  im.header.stamp = mod_host::Time(30, 100000000);
  r.call("submitDepth: caller's transform", [&] { return t = r.sfc.submitDepth(&im, &dm, &r.objs, &r.tf, &r.flow_out, 0, 0, &r.disparity_out, &r.cloud); });
  r.ctx.counts = {1};
  r.call("collect", [&] { r.sfc.collect(t); return 0; });
  im.header.stamp = mod_host::Time(30, 200000000);
  r.call("submitDepth: no transform, the motion is estimated", [&] { return t = r.sfc.submitDepth(&im, &dm, &r.objs); });
  r.ctx.counts = {2};
  r.call("collectOdometry", [&] { return (int)r.sfc.collectOdometry(t, &r.motion); });
  // a missing depth image: the outputs are still resized
  r.flow_out.clear(); r.disparity_out.clear(); r.cloud.data.clear();
  r.ctx.codes["mod_submit_depth_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitDepth: no depth image", [&] { return r.sfc.submitDepth(&im, nullptr, &r.objs, nullptr, &r.flow_out, 0, 0, &r.disparity_out, &r.cloud); });
  im.header.stamp = mod_host::Time(31, 0);
  r.ctx.codes["mod_submit_depth_host"] = {MOD_SKIP_NO_DISPARITY_PREV};
  r.call("submitDepth: the next frame has dt 0", [&] { return r.sfc.submitDepth(&im, &dm, nullptr, &r.tf); });
  // side by side makes an RGB-D frame a missing image, without a layout call
  r.sfc.setSideBySide(true);
  r.ctx.codes["mod_submit_depth_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("submitDepth: side by side", [&] { return r.sfc.submitDepth(&im, &dm, &r.objs, &r.tf); });
  r.sfc.setSideBySide(false);
  r.ctx.codes["mod_submit_depth_host"] = {MOD_ERR_INVALID_ARGUMENT};
  r.call("submitDepth: the library fails", [&] { return r.sfc.submitDepth(&im, &dm, &r.objs, &r.tf); });
  for (int k = 0; k < MOD_PIPELINE_DEPTH + 2; k++) {
    im.header.stamp = mod_host::Time(40 + k, 0);
    r.call("submitDepth: ring", [&] { return t = r.sfc.submitDepth(&im, &dm, &r.objs, k % 2 ? &r.tf : nullptr, nullptr, 0, 0, nullptr, &r.cloud); });
    r.ctx.counts = {1};
    r.call("collectOdometry: ring", [&] { return (int)r.sfc.collectOdometry(t, &r.motion); });
  }
}

static void scenario_construct() {
  L("== construct / stereoCallback");
  Rig r;
  r.camera();
  mod_host::DisparityImage d0 = r.disparity(0, 70, 0), d1 = r.disparity(1, 70, 500000000), d2 = r.disparity(2, 71, 250000000);
  mod_host::FlowImage f = r.flow(71, 70, 500000001);
  r.ctx.counts = {5};   // 5 > the capacity of 3
  r.call("construct: everything asked for", [&] { return (int)r.sfc.construct(&d1, &d0, &f, &r.tf, &r.cloud, &r.labels, &r.objs, &r.depth_image); });
  r.ctx.codes["mod_depth_image_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.ctx.codes["mod_process_frame_host"] = {MOD_SKIP_NO_TRANSFORM};
  r.call("construct: the depth image is skipped, the frame too", [&] { return (int)r.sfc.construct(&d1, &d0, &f, nullptr, &r.cloud, &r.labels, &r.objs, &r.depth_image); });
  r.depth_image.assign(5, 1.0f);
  r.ctx.codes["mod_process_frame_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("construct: no disparity", [&] { return (int)r.sfc.construct(nullptr, &d0, &f, &r.tf, &r.cloud, nullptr, &r.objs, &r.depth_image); });
  r.ctx.codes["mod_process_frame_host"] = {MOD_SKIP_NO_DISPARITY_PREV};
  r.call("construct: no previous disparity, dt is 0", [&] { return (int)r.sfc.construct(&d1, nullptr, &f, &r.tf, nullptr, nullptr, nullptr, &r.depth_image); });
  r.call("construct: nothing asked for", [&] { return (int)r.sfc.construct(&d1, &d0, &f, &r.tf, nullptr); });
  r.ctx.codes["mod_depth_image_host"] = {MOD_ERR_DEVICE};
  r.call("construct: the depth image fails", [&] { return (int)r.sfc.construct(&d1, &d0, &f, &r.tf, &r.cloud, nullptr, nullptr, &r.depth_image); });
  r.ctx.codes["mod_process_frame_host"] = {MOD_ERR_DEVICE};
  r.call("construct: the library fails", [&] { return (int)r.sfc.construct(&d1, &d0, &f, &r.tf, &r.cloud); });
  // stereoCallback carries the previous disparity
  r.ctx.codes["mod_process_frame_host"] = {MOD_SKIP_NO_DISPARITY_PREV};
  r.call("stereoCallback: frame 0", [&] { return (int)r.sfc.stereoCallback(&d0, &f, &r.tf, &r.cloud, &r.objs); });
  r.ctx.counts = {1};
  r.call("stereoCallback: frame 1", [&] { return (int)r.sfc.stereoCallback(&d1, &f, &r.tf, &r.cloud, &r.objs); });
  L("    previous: header=%s pixel=%a", header_text(r.sfc.disparity_previous_.header).c_str(), r.sfc.previous_pixels_[0]);
  r.ctx.codes["mod_process_frame_host"] = {MOD_SKIP_NO_DISPARITY_NOW};
  r.call("stereoCallback: no disparity", [&] { return (int)r.sfc.stereoCallback(nullptr, &f, &r.tf, &r.cloud, &r.objs); });
  r.ctx.codes["mod_process_frame_host"] = {MOD_SKIP_NO_DISPARITY_PREV};
  r.call("stereoCallback: the frame after has no previous one", [&] { return (int)r.sfc.stereoCallback(&d2, &f, &r.tf, &r.cloud, &r.objs); });
  r.call("stereoCallback: the frame after that has", [&] { return (int)r.sfc.stereoCallback(&d1, &f, &r.tf, &r.cloud); });
}

static void scenario_reconfigure() {
  L("== reconfigureCB / reconfigureClusterer");
  Rig r;
  scene_flow_constructor::SceneFlowConstructorConfig config;
  config.dynamic_flow_diff = 9;
  r.call("reconfigureCB", [&] { r.sfc.reconfigureCB(config); return 0; });
  r.ctx.codes["mod_get_params"] = {MOD_ERR_NOT_CONFIGURED};
  r.call("reconfigureCB: no parameters yet, the reference defaults", [&] { r.sfc.reconfigureCB(config); return 0; });
  r.call("reconfigureClusterer", [&] { r.sfc.reconfigureClusterer(1000, 0.5, 1.5, 8); return 0; });
  r.ctx.codes["mod_get_params"] = {MOD_ERR_NOT_CONFIGURED};
  r.call("reconfigureClusterer: no parameters yet", [&] { r.sfc.reconfigureClusterer(1000, 0.5, 1.5, 8); return 0; });
  r.ctx.codes["mod_set_params"] = {MOD_ERR_INVALID_ARGUMENT};
  r.call("reconfigureCB: refused", [&] { r.sfc.reconfigureCB(config); return 0; });
  ClustererNodelet nodelet(&r.ctx);
  scene_flow_clusterer::ClustererConfig cc;
  cc.cluster_size = 400; cc.depth_diff = 0.125; cc.dynamic_speed = 0.625; cc.neighbor_distance = 3;
  r.call("ClustererNodelet::reconfigureCB", [&] { nodelet.reconfigureCB(cc); return 0; });
  r.ctx.codes["mod_get_params"] = {MOD_ERR_NOT_CONFIGURED};
  r.call("ClustererNodelet::reconfigureCB: no parameters yet", [&] { nodelet.reconfigureCB(cc); return 0; });
}

static void scenario_clusterer() {
  L("== ClustererNodelet::dataCB / clustering");
  Rig r;
  ClustererNodelet nodelet(&r.ctx);
  nodelet.setMaxObjects(2);
  mod_host::PointCloud2 input;
  input.header = header(91, 80, 5, "input"); input.width = W; input.height = H; input.row_step = 32 * W; input.data.assign(32 * N, 0);
  r.ctx.name("input.data", [&input] { return (const void *)input.data.data(); });
  r.ctx.counts = {3};   // 3 > the capacity of 2
  r.call("dataCB", [&] { nodelet.dataCB(input, &r.objs, &r.labels); return 0; });
  r.call("dataCB: no outputs", [&] { nodelet.dataCB(input, nullptr); return 0; });
  r.ctx.codes["mod_cluster_cloud_host"] = {MOD_ERR_INVALID_ARGUMENT};
  r.call("dataCB: the library fails", [&] { nodelet.dataCB(input, &r.objs, &r.labels); return 0; });
  ClustererNodelet::IndicesClusters clusters;
  ClustererNodelet::MarkerPoints points;
  auto lists = [&] {
    std::string s;
    for (const auto &c : clusters) { s += " ["; for (int i : c) s += " " + std::to_string(i); s += " ]"; }
    L("    clusters:%s", s.c_str());
    s.clear();
    for (const auto &c : points) { s += " ["; for (const auto &p : c) { char b[96]; std::snprintf(b, sizeof b, " (%a %a %a)", p[0], p[1], p[2]); s += b; } s += " ]"; }
    L("    marker_points:%s", s.c_str());
  };
  r.ctx.counts = {1};
  r.call("clustering: clusters and marker points", [&] { nodelet.clustering(input, 4, &clusters, &points, &r.objs, &r.labels); return 0; });
  lists();
  points.clear();
  r.call("clustering: clusters alone", [&] { nodelet.clustering(input, 4, &clusters, nullptr); return 0; });
  lists();
  r.ctx.codes["mod_cluster_cloud_host"] = {MOD_ERR_DEVICE};
  r.call("clustering: the library fails, the setting is switched off again", [&] { nodelet.clustering(input, 4, &clusters, &points); return 0; });
  r.ctx.codes["mod_malloc"] = {MOD_OK, MOD_ERR_DEVICE};
  r.call("clustering: no device memory", [&] { nodelet.clustering(input, 4, &clusters, &points); return 0; });
  r.ctx.codes["mod_set_cluster_members"] = {MOD_ERR_INVALID_ARGUMENT};
  r.call("clustering: the setting is refused", [&] { nodelet.clustering(input, 4, &clusters, &points); return 0; });
  r.ctx.names.pop_back();
  for (void *p : r.ctx.device) if (p) L("leaked device block");
}

int main() {
  scenario_submit();
  scenario_submit_stereo();
  scenario_submit_odometry();
  scenario_submit_depth();
  scenario_construct();
  scenario_reconfigure();
  scenario_clusterer();
  return 0;
}
