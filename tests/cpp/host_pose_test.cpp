// host_pose_test.cpp — the host mirror's crop and pose arithmetic without a device (tests/test_host_pose.py).
//   host_pose_test crop W H w h fx cx cy            -> "cx cy width height" of crop_camera_info
//   host_pose_test pose FILE                        FILE: the base -> camera transform (tx ty tz qx qy qz qw), then one line per
//                                                   estimate (status tx ty tz qx qy qz qw); prints, after every estimate, the
//                                                   integrated pose, odom -> base and camera -> odom (3 x 4 row-major each)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../moving_object_detector_amd/host/scene_flow_constructor.hpp"

static void print_pose(const mod_host::Pose &p) {
  for (int i = 0; i < 3; i++) std::printf(" %.17g %.17g %.17g %.17g", p.R[i][0], p.R[i][1], p.R[i][2], p.t[i]);
}

int main(int argc, char **argv) {
  if (argc == 9 && !std::strcmp(argv[1], "crop")) {
    mod_host::CameraInfo info;
    info.width = std::atoi(argv[2]); info.height = std::atoi(argv[3]);
    info.P[0] = info.P[5] = std::atof(argv[6]); info.P[2] = std::atof(argv[7]); info.P[6] = std::atof(argv[8]); info.P[10] = 1.0;
    const mod_host::CameraInfo c = mod_host::crop_camera_info(info, std::atoi(argv[4]), std::atoi(argv[5]));
    std::printf("%.17g %.17g %d %d\n", c.P[2], c.P[6], c.width, c.height);
    return 0;
  }
  if (argc == 3 && !std::strcmp(argv[1], "pose")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) return 2;
    mod_host::Transform base;
    if (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf", &base.translation[0], &base.translation[1], &base.translation[2], &base.rotation[0],
                    &base.rotation[1], &base.rotation[2], &base.rotation[3]) != 7) return 3;
    scene_flow_constructor::SceneFlowConstructor sfc(nullptr);
    sfc.setBaseToCamera(base);
    int status;
    ModTransform tf;
    while (std::fscanf(f, "%d %lf %lf %lf %lf %lf %lf %lf", &status, &tf.t[0], &tf.t[1], &tf.t[2], &tf.q[0], &tf.q[1], &tf.q[2], &tf.q[3]) == 8) {
      std::printf("%d", sfc.integrateEstimate(tf, status) ? 1 : 0);
      print_pose(sfc.integratedPose());
      print_pose(sfc.odomToBase());
      print_pose(sfc.cameraToOdom());
      std::printf("\n");
    }
    std::fclose(f);
    return 0;
  }
  return 1;
}
