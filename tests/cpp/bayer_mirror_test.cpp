// bayer_mirror_test.cpp — the C++ host mirror fed 8-bit Bayer images on the GPU (tests/test_gpu_bayer_streams.py):
// SceneFlowConstructor::submitOdometry with bayer_* Images (rows padded, the camera-sized window at an origin inside the message)
// against the same mirror fed the grey the numpy model makes of those windows as mono8 Images.  The program compares for itself,
// byte for byte, and prints what differs.
//   bayer_mirror_test DIR
// DIR/setup.txt: "W H frames encoding width height step x0 y0  P0 P2 P3 P5 P6 P7  f T min_d max_d" (W x H: the camera; width x
// height, step: the messages); DIR/left<k>.bin, right<k>.bin: the messages; DIR/grey_left<k>.bin, grey_right<k>.bin: W x H grey.
// Exit 0 and "disparities N" on stdout (the valid disparities compared in all) when everything agrees.
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
  int W, H, F, width, height, step, x0, y0;
  std::string enc;
  mod_host::CameraInfo cam;
  mod_host::DisparityImage d;
  std::vector<std::vector<uint8_t>> msg[2], grey[2];
};

struct Frames {
  std::vector<mod_host::MovingObjectArray> objs;
  std::vector<std::vector<float>> disp, flow;
  std::vector<mod_host::Transform> motion;
  std::vector<int> ok, tickets;
  explicit Frames(int n) : objs(n), disp(n), flow(n), motion(n), ok(n, 0), tickets(n, -1) {}
};

std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// the odometry stream, Bayer messages (bayer[k]) or the model's grey, up to MOD_PIPELINE_DEPTH frames in flight
bool odometry(const Setup &s, const std::vector<int> &bayer, Frames *out) {
  ModConfig cfg{};
  cfg.max_width = s.W; cfg.max_height = s.H; cfg.max_frames = 1;
  ModContext *ctx = nullptr;
  if (mod_create(&cfg, &ctx) != MOD_OK) return false;
  bool good = true;
  {
    SceneFlowConstructor sfc(ctx);
    sfc.setCameraInfo(s.cam, s.d);
    scene_flow_constructor::SceneFlowConstructorConfig c;
    sfc.reconfigureCB(c);
    std::vector<int> order;
    auto collect = [&](int k) { out->ok[k] = sfc.collectOdometry(out->tickets[k], &out->motion[k]) ? 1 : 0; };
    for (int k = 0; k < s.F && good; k++) {
      mod_host::Image im[2];
      for (int e = 0; e < 2; e++) {
        im[e].header.stamp = mod_host::Time(100u, (uint32_t)(k * 66666667));
        if (bayer[k]) { im[e].encoding = s.enc; im[e].width = s.width; im[e].height = s.height; im[e].step = s.step; im[e].data = s.msg[e][k].data(); }
        else { im[e].encoding = "mono8"; im[e].width = s.W; im[e].height = s.H; im[e].step = s.W; im[e].data = s.grey[e][k].data(); }
      }
      if (order.size() == MOD_PIPELINE_DEPTH) { collect(order.front()); order.erase(order.begin()); }
      out->tickets[k] = sfc.submitOdometry(&im[0], &im[1], &out->objs[k], &out->flow[k], bayer[k] ? s.x0 : 0, bayer[k] ? s.y0 : 0, &out->disp[k]);
      good = k == 0 ? out->tickets[k] == -1 : out->tickets[k] >= 0;
      if (k > 0 && good) order.push_back(k);
    }
    for (int k : order) collect(k);
  }
  mod_destroy(ctx);
  return good;
}

int same(const char *what, const Frames &a, const Frames &b, const Setup &s, int *seen) {
  const size_t n = (size_t)s.W * s.H;
  for (int k = 1; k < s.F; k++) {
    if (a.disp[k].size() != n || b.disp[k].size() != n || a.flow[k].size() != 2 * n || b.flow[k].size() != 2 * n) return 1;
    if (std::memcmp(a.disp[k].data(), b.disp[k].data(), 4 * n)) { std::fprintf(stderr, "%s: disparity of frame %d differs\n", what, k); return 1; }
    if (std::memcmp(a.flow[k].data(), b.flow[k].data(), 8 * n)) { std::fprintf(stderr, "%s: flow of frame %d differs\n", what, k); return 1; }
    if (a.ok[k] != b.ok[k] || std::memcmp(a.motion[k].translation, b.motion[k].translation, 24) ||
        std::memcmp(a.motion[k].rotation, b.motion[k].rotation, 32)) { std::fprintf(stderr, "%s: motion of frame %d differs\n", what, k); return 1; }
    const auto &x = a.objs[k].moving_object_array, &y = b.objs[k].moving_object_array;
    if (x.size() != y.size()) { std::fprintf(stderr, "%s: frame %d has %zu objects against %zu\n", what, k, x.size(), y.size()); return 1; }
    for (size_t i = 0; i < x.size(); i++)
      if (x[i].id != y[i].id || std::memcmp(x[i].center.position, y[i].center.position, 24) || std::memcmp(x[i].velocity, y[i].velocity, 24) ||
          std::memcmp(x[i].bounding_box, y[i].bounding_box, 24)) { std::fprintf(stderr, "%s: object %zu of frame %d differs\n", what, i, k); return 1; }
    for (size_t i = 0; i < n; i++) *seen += a.disp[k][i] >= 0.0f;
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 1;
  const std::string dir = argv[1];
  FILE *f = std::fopen((dir + "/setup.txt").c_str(), "r");
  if (!f) return 2;
  Setup s;
  char enc[32];
  double P0, P2, P3, P5, P6, P7;
  if (std::fscanf(f, "%d %d %d %31s %d %d %d %d %d %lf %lf %lf %lf %lf %lf %f %f %f %f", &s.W, &s.H, &s.F, enc, &s.width, &s.height, &s.step, &s.x0,
                  &s.y0, &P0, &P2, &P3, &P5, &P6, &P7, &s.d.f, &s.d.T, &s.d.min_disparity, &s.d.max_disparity) != 19) return 3;
  std::fclose(f);
  s.enc = enc;
  // the mirror's names: a Bayer encoding is none of image_encoding()'s, and one byte per pixel
  const int e = mod_host::bayer_encoding(s.enc);
  if (e < 0 || mod_host::image_encoding(s.enc) != -1 || mod_host::image_channels(e) != 1 || s.F < 4) return 4;
  s.cam.width = s.W; s.cam.height = s.H;
  s.cam.P[0] = P0; s.cam.P[2] = P2; s.cam.P[3] = P3; s.cam.P[5] = P5; s.cam.P[6] = P6; s.cam.P[7] = P7; s.cam.P[10] = 1.0;
  const char *eye[2] = {"left", "right"};
  for (int k = 0; k < s.F; k++)
    for (int i = 0; i < 2; i++) {
      s.msg[i].push_back(slurp(dir + "/" + eye[i] + std::to_string(k) + ".bin"));
      s.grey[i].push_back(slurp(dir + "/grey_" + eye[i] + std::to_string(k) + ".bin"));
      if (s.msg[i][k].size() != (size_t)s.step * s.height || s.grey[i][k].size() != (size_t)s.W * s.H) return 5;
    }
  try {
    std::vector<int> bayer(s.F, 1), mono(s.F, 0), mixed(s.F);
    for (int k = 0; k < s.F; k++) mixed[k] = k % 2;          // the layout changes in front of every submit, frames in flight
    Frames ob(s.F), om(s.F), ox(s.F);
    int seen = 0;
    if (!odometry(s, bayer, &ob) || !odometry(s, mono, &om) || !odometry(s, mixed, &ox)) { std::fprintf(stderr, "an odometry submit was refused\n"); return 6; }
    if (same("bayer against mono8", ob, om, s, &seen) || same("switching against mono8", ox, om, s, &seen)) return 7;
    std::printf("disparities %d\n", seen);
  } catch (const std::exception &ex) {
    std::fprintf(stderr, "exception: %s\n", ex.what());
    return 11;
  }
  return 0;
}
