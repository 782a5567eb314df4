// side_by_side_mirror_test.cpp — the C++ host mirror's one-message paths on the GPU (tests/test_gpu_side_by_side_mirror.py):
// SceneFlowConstructor::setSideBySide with submitOdometry and submitStereo, against the same mirror fed the two messages cut out
// of the side-by-side one with the setting off.  The program compares for itself, byte for byte, and prints what differs.
//   side_by_side_mirror_test DIR
// DIR/setup.txt: "W H frames encoding step  P0 P2 P3 P5 P6 P7  f T min_d max_d" (W x H: ONE eye's image and its camera; the
// message is 2 W pixels wide and `step` bytes per row); DIR/both<k>.bin: the messages.  Exit 0 and "objects N" on stdout (the
// objects compared in all) when everything agrees.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../moving_object_detector_amd/host/scene_flow_constructor.hpp"

namespace {

using scene_flow_constructor::SceneFlowConstructor;

struct Setup {
  int W, H, F, step, C;
  std::string enc;
  mod_host::CameraInfo cam;
  mod_host::DisparityImage d;
  std::vector<std::vector<uint8_t>> both, left, right;   // the messages, and their panes as messages of their own (rows packed)
};

// how frame k is handed in
enum Mode { TWO = 0, ONE = 1, ONE_TWICE = 2 };   // two messages, off; one message, right null; one message in left and in right

struct Frames {
  std::vector<mod_host::MovingObjectArray> objs;
  std::vector<std::vector<float>> disp, flow;
  std::vector<mod_host::Transform> motion;
  std::vector<mod_host::PointCloud2> cloud;
  std::vector<int> ok, tickets;
  explicit Frames(int n) : objs(n), disp(n), flow(n), motion(n), cloud(n), ok(n, 0), tickets(n, -1) {}
};

std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

ModContext *context(const Setup &s) {
  ModConfig cfg{};
  cfg.max_width = s.W; cfg.max_height = s.H; cfg.max_frames = 1;
  ModContext *ctx = nullptr;
  return mod_create(&cfg, &ctx) == MOD_OK ? ctx : nullptr;
}

void configure(SceneFlowConstructor &sfc, const Setup &s) {
  sfc.setCameraInfo(s.cam, s.d);
  scene_flow_constructor::SceneFlowConstructorConfig c;
  sfc.reconfigureCB(c);
}

// the images of frame k in the form `mode` asks for; right is null for ONE
void images(const Setup &s, int k, int mode, mod_host::Image *l, mod_host::Image *r, const mod_host::Image **right) {
  l->header.stamp = r->header.stamp = mod_host::Time(100u, (uint32_t)(k * 66666667));
  l->encoding = r->encoding = s.enc;
  l->height = r->height = s.H;
  if (mode == TWO) {
    l->width = r->width = s.W; l->step = r->step = s.W * s.C;
    l->data = s.left[k].data(); r->data = s.right[k].data();
    *right = r;
  } else {
    l->width = r->width = 2 * s.W; l->step = r->step = s.step;
    l->data = r->data = s.both[k].data();
    *right = mode == ONE ? nullptr : r;
  }
}

// the odometry stream, the setting switched in front of every frame, up to MOD_PIPELINE_DEPTH frames in flight
bool odometry(const Setup &s, const std::vector<int> &mode, Frames *out) {
  ModContext *ctx = context(s);
  if (!ctx) return false;
  bool good = true;
  {
    SceneFlowConstructor sfc(ctx);
    configure(sfc, s);
    std::vector<int> order;
    auto collect = [&](int k) { out->ok[k] = sfc.collectOdometry(out->tickets[k], &out->motion[k]) ? 1 : 0; };
    for (int k = 0; k < s.F && good; k++) {
      mod_host::Image l, r;
      const mod_host::Image *right = nullptr;
      images(s, k, mode[k], &l, &r, &right);
      if (order.size() == MOD_PIPELINE_DEPTH) { collect(order.front()); order.erase(order.begin()); }
      sfc.setSideBySide(mode[k] != TWO);
      out->tickets[k] = sfc.submitOdometry(&l, right, &out->objs[k], &out->flow[k], 0, 0, &out->disp[k]);
      good = k == 0 ? out->tickets[k] == -1 : out->tickets[k] >= 0;
      if (k > 0 && good) order.push_back(k);
    }
    for (int k : order) collect(k);
  }
  mod_destroy(ctx);
  return good;
}

// submitStereo fed the flow and the motion an odometry run gave
bool stereo(const Setup &s, const std::vector<int> &mode, const Frames &from, Frames *out) {
  ModContext *ctx = context(s);
  if (!ctx) return false;
  bool good = true;
  {
    SceneFlowConstructor sfc(ctx);
    configure(sfc, s);
    std::vector<int> order;
    for (int k = 0; k < s.F && good; k++) {
      mod_host::Image l, r;
      const mod_host::Image *right = nullptr;
      images(s, k, mode[k], &l, &r, &right);
      mod_host::FlowImage fl;
      fl.header = l.header; fl.width = s.W; fl.height = s.H; fl.data = from.flow[k].data();
      if (order.size() == MOD_PIPELINE_DEPTH) { sfc.collect(order.front()); order.erase(order.begin()); }
      sfc.setSideBySide(mode[k] != TWO);
      // the first frame has no previous disparity: no flow and no motion go with it, and nothing is published
      const int t = sfc.submitStereo(&l, right, k ? &fl : nullptr, k ? &from.motion[k] : nullptr, &out->cloud[k], &out->objs[k]);
      good = k == 0 ? t == -1 : t >= 0;
      if (k > 0 && good) order.push_back(t);
    }
    for (int t : order) sfc.collect(t);
  }
  mod_destroy(ctx);
  return good;
}

int same_objects(const char *what, const Frames &a, const Frames &b, int F, int *seen) {
  for (int k = 1; k < F; k++) {
    const auto &x = a.objs[k].moving_object_array, &y = b.objs[k].moving_object_array;
    if (x.size() != y.size()) { std::fprintf(stderr, "%s: frame %d has %zu objects against %zu\n", what, k, x.size(), y.size()); return 1; }
    for (size_t i = 0; i < x.size(); i++)
      if (x[i].id != y[i].id || std::memcmp(x[i].center.position, y[i].center.position, 24) ||
          std::memcmp(x[i].center.orientation, y[i].center.orientation, 32) || std::memcmp(x[i].velocity, y[i].velocity, 24) ||
          std::memcmp(x[i].bounding_box, y[i].bounding_box, 24)) {
        std::fprintf(stderr, "%s: object %zu of frame %d differs\n", what, i, k);
        return 1;
      }
    *seen += (int)x.size();
  }
  return 0;
}

int same_odometry(const char *what, const Frames &a, const Frames &b, const Setup &s, int *seen) {
  const size_t n = (size_t)s.W * s.H;
  for (int k = 1; k < s.F; k++) {
    if (a.disp[k].size() != n || b.disp[k].size() != n || a.flow[k].size() != 2 * n || b.flow[k].size() != 2 * n) return 1;
    if (std::memcmp(a.disp[k].data(), b.disp[k].data(), 4 * n)) { std::fprintf(stderr, "%s: disparity of frame %d differs\n", what, k); return 1; }
    if (std::memcmp(a.flow[k].data(), b.flow[k].data(), 8 * n)) { std::fprintf(stderr, "%s: flow of frame %d differs\n", what, k); return 1; }
    if (a.ok[k] != b.ok[k] || std::memcmp(a.motion[k].translation, b.motion[k].translation, 24) ||
        std::memcmp(a.motion[k].rotation, b.motion[k].rotation, 32)) { std::fprintf(stderr, "%s: motion of frame %d differs\n", what, k); return 1; }
  }
  return same_objects(what, a, b, s.F, seen);
}

int same_stereo(const char *what, const Frames &a, const Frames &b, const Setup &s, int *seen) {
  for (int k = 1; k < s.F; k++)
    if (a.cloud[k].data.size() != (size_t)s.W * s.H * 32 || a.cloud[k].data != b.cloud[k].data) {
      std::fprintf(stderr, "%s: cloud of frame %d differs\n", what, k);
      return 1;
    }
  return same_objects(what, a, b, s.F, seen);
}

// while set, two distinct images are refused by every image entry point, and the mirror goes on with two messages once it is off
int refusals(const Setup &s) {
  ModContext *ctx = context(s);
  if (!ctx) return 1;
  int bad = 0;
  {
    SceneFlowConstructor sfc(ctx);
    configure(sfc, s);
    sfc.setSideBySide(true);
    mod_host::Image l, r;
    const mod_host::Image *right = nullptr;
    images(s, 0, TWO, &l, &r, &right);
    mod_host::DisparityImage d;
    std::vector<float> px;
    mod_host::MovingObjectArray objs;
    if (sfc.estimateDisparity(&l, &r, s.cam, s.cam, &d, &px)) { std::fprintf(stderr, "estimateDisparity took two images while set\n"); bad = 1; }
    if (sfc.submitOdometry(&l, &r, &objs) != -1) { std::fprintf(stderr, "submitOdometry took two images while set\n"); bad = 1; }
    images(s, 0, ONE_TWICE, &l, &r, &right);
    r.data = s.both[1].data();                     // a message of the right size that is not the left one
    if (sfc.submitOdometry(&l, &r, &objs) != -1) { std::fprintf(stderr, "submitOdometry took two side-by-side messages\n"); bad = 1; }
    sfc.setSideBySide(false);
    for (int k = 0; k < 2 && !bad; k++) {
      images(s, k, TWO, &l, &r, &right);
      const int t = sfc.submitOdometry(&l, right, &objs);
      if (k == 0 ? t != -1 : t < 0) { std::fprintf(stderr, "two messages after the setting went off: ticket %d at frame %d\n", t, k); bad = 1; }
      else if (k == 1) sfc.collectOdometry(t);
    }
  }
  mod_destroy(ctx);
  return bad;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 1;
  const std::string dir = argv[1];
  FILE *f = std::fopen((dir + "/setup.txt").c_str(), "r");
  if (!f) return 2;
  Setup s;
  char enc[16];
  double P0, P2, P3, P5, P6, P7;
  if (std::fscanf(f, "%d %d %d %15s %d %lf %lf %lf %lf %lf %lf %f %f %f %f", &s.W, &s.H, &s.F, enc, &s.step, &P0, &P2, &P3, &P5, &P6, &P7, &s.d.f,
                  &s.d.T, &s.d.min_disparity, &s.d.max_disparity) != 15) return 3;
  std::fclose(f);
  s.enc = enc;
  const int e = mod_host::image_encoding(s.enc);
  if (e < 0 || s.F < 4) return 3;
  s.C = mod_host::image_channels(e);
  s.cam.width = s.W; s.cam.height = s.H;
  s.cam.P[0] = P0; s.cam.P[2] = P2; s.cam.P[3] = P3; s.cam.P[5] = P5; s.cam.P[6] = P6; s.cam.P[7] = P7; s.cam.P[10] = 1.0;
  const size_t row = (size_t)s.W * s.C;
  for (int k = 0; k < s.F; k++) {
    s.both.push_back(slurp(dir + "/both" + std::to_string(k) + ".bin"));
    if (s.both[k].size() != (size_t)s.step * s.H || (size_t)s.step < 2 * row) return 5;
    s.left.emplace_back(row * s.H);
    s.right.emplace_back(row * s.H);
    for (int y = 0; y < s.H; y++) {
      std::memcpy(&s.left[k][y * row], &s.both[k][(size_t)y * s.step], row);
      std::memcpy(&s.right[k][y * row], &s.both[k][(size_t)y * s.step + row], row);
    }
  }
  try {
    std::vector<int> two(s.F, TWO), one(s.F, ONE), mixed(s.F);
    for (int k = 0; k < s.F; k++) mixed[k] = k % 4 == 0 ? ONE : k % 4 == 1 ? TWO : k % 4 == 2 ? ONE_TWICE : TWO;
    Frames o2(s.F), o1(s.F), om(s.F), s2(s.F), s1(s.F), sm(s.F);
    int seen = 0;
    if (!odometry(s, two, &o2) || !odometry(s, one, &o1) || !odometry(s, mixed, &om)) { std::fprintf(stderr, "an odometry submit was refused\n"); return 6; }
    if (same_odometry("odometry, one message", o1, o2, s, &seen) || same_odometry("odometry, switching", om, o2, s, &seen)) return 7;
    if (!stereo(s, two, o2, &s2) || !stereo(s, one, o2, &s1) || !stereo(s, mixed, o2, &sm)) { std::fprintf(stderr, "a stereo submit was refused\n"); return 8; }
    if (same_stereo("stereo, one message", s1, s2, s, &seen) || same_stereo("stereo, switching", sm, s2, s, &seen)) return 9;
    if (refusals(s)) return 10;
    std::printf("objects %d\n", seen);
  } catch (const std::exception &ex) {
    std::fprintf(stderr, "exception: %s\n", ex.what());
    return 11;
  }
  return 0;
}
