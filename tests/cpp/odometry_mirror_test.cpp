// odometry_mirror_test.cpp — the C++ host mirror's odometry path on the GPU (tests/test_gpu_odometry_mirror.py): SceneFlowConstructor
// fed colour messages through submitOdometry / collectOdometry, up to MOD_PIPELINE_DEPTH frames in flight.
//   odometry_mirror_test DIR
// DIR/setup.txt: "W H frames encoding msg_w msg_h step  P0 P2 P3 P5 P6 P7  f T min_d max_d" (P of the FULL message's camera: the
// mirror crops it with crop_camera_info and takes the centred window); DIR/left<k>.bin, DIR/right<k>.bin: the messages.
// DIR/out.bin, per frame k >= 1: int32 collected (1: the estimate succeeded), int32 n, n x (int32 id, 13 doubles: centre xyz,
// orientation xyzw, velocity xyz, box xyz), W*H float disparity, 7 doubles motion (t xyz, q xyzw), 12 doubles integrated pose.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../moving_object_detector_amd/host/scene_flow_constructor.hpp"

static std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
  if (argc != 2) return 1;
  const std::string dir = argv[1];
  FILE *s = std::fopen((dir + "/setup.txt").c_str(), "r");
  if (!s) return 2;
  int W, H, F, mw, mh, step;
  char enc[16];
  double P0, P2, P3, P5, P6, P7;
  float f, T, mind, maxd;
  if (std::fscanf(s, "%d %d %d %15s %d %d %d %lf %lf %lf %lf %lf %lf %f %f %f %f", &W, &H, &F, enc, &mw, &mh, &step, &P0, &P2, &P3, &P5, &P6, &P7,
                  &f, &T, &mind, &maxd) != 17) return 3;
  std::fclose(s);
  ModConfig cfg{};
  cfg.max_width = W; cfg.max_height = H; cfg.max_frames = 1;
  ModContext *ctx = nullptr;
  if (mod_create(&cfg, &ctx) != MOD_OK) return 4;
  {
    scene_flow_constructor::SceneFlowConstructor sfc(ctx);
    mod_host::CameraInfo full;
    full.width = mw; full.height = mh;
    full.P[0] = P0; full.P[2] = P2; full.P[3] = P3; full.P[5] = P5; full.P[6] = P6; full.P[7] = P7; full.P[10] = 1.0;
    mod_host::DisparityImage d;
    d.f = f; d.T = T; d.min_disparity = mind; d.max_disparity = maxd;
    sfc.setCameraInfo(mod_host::crop_camera_info(full, W, H), d);
    scene_flow_constructor::SceneFlowConstructorConfig c;
    sfc.reconfigureCB(c);
    int x0, y0;
    mod_host::centred_origin(mw, mh, W, H, &x0, &y0);
    std::vector<std::vector<uint8_t>> L(F), R(F);
    std::vector<mod_host::MovingObjectArray> objs(F);
    std::vector<std::vector<float>> disp(F);
    std::vector<int> tickets(F, -1), ok(F, 0);
    std::vector<mod_host::Transform> motion(F);
    std::vector<mod_host::Pose> pose(F);
    std::vector<int> order;
    auto collect = [&](int k) {
      ok[k] = sfc.collectOdometry(tickets[k], &motion[k]) ? 1 : 0;
      pose[k] = sfc.integratedPose();
    };
    for (int k = 0; k < F; k++) {
      L[k] = slurp(dir + "/left" + std::to_string(k) + ".bin");
      R[k] = slurp(dir + "/right" + std::to_string(k) + ".bin");
      if ((int)L[k].size() != step * mh || (int)R[k].size() != step * mh) return 5;
      mod_host::Image l, r;
      l.header.stamp = r.header.stamp = mod_host::Time(100u, (uint32_t)(k * 66666667));   // dt = 1e-9 * 66666667 s (15 Hz)
      l.width = r.width = mw; l.height = r.height = mh; l.encoding = r.encoding = enc; l.step = r.step = step;
      l.data = L[k].data(); r.data = R[k].data();
      if (order.size() == MOD_PIPELINE_DEPTH) { collect(order.front()); order.erase(order.begin()); }
      tickets[k] = sfc.submitOdometry(&l, &r, &objs[k], nullptr, x0, y0, &disp[k]);
      if (k == 0 ? tickets[k] != -1 : tickets[k] < 0) return 6;
      if (k > 0) order.push_back(k);
    }
    for (int k : order) collect(k);
    FILE *o = std::fopen((dir + "/out.bin").c_str(), "wb");
    for (int k = 1; k < F; k++) {
      const int32_t n = (int32_t)objs[k].moving_object_array.size();
      std::fwrite(&ok[k], 4, 1, o);
      std::fwrite(&n, 4, 1, o);
      for (const mod_host::MovingObject &m : objs[k].moving_object_array) {
        std::fwrite(&m.id, 4, 1, o);
        std::fwrite(m.center.position, 8, 3, o); std::fwrite(m.center.orientation, 8, 4, o);
        std::fwrite(m.velocity, 8, 3, o); std::fwrite(m.bounding_box, 8, 3, o);
      }
      std::fwrite(disp[k].data(), 4, disp[k].size(), o);
      std::fwrite(motion[k].translation, 8, 3, o); std::fwrite(motion[k].rotation, 8, 4, o);
      for (int i = 0; i < 3; i++) { std::fwrite(pose[k].R[i], 8, 3, o); std::fwrite(&pose[k].t[i], 8, 1, o); }
    }
    std::fclose(o);
  }
  mod_destroy(ctx);
  return 0;
}
