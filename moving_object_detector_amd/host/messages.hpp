// messages.hpp — minimal stand-ins for the ROS message types on the hot path's boundary, so the host mirror compiles
// and runs without ROS.  Field names follow the ROS definitions; a ROS build maps the real messages onto these views
// (ros_adapter/) without copying pixels.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mod_sf.h"

namespace mod_host {

// ros::Time: seconds + nanoseconds.  The frame interval of the velocity (scene_flow_constructor.cpp:162-164,200-202) is
// `(stamp_now - stamp_previous).toSec()`: integer arithmetic on (sec, nsec), normalised to 0 <= nsec < 1e9, then
// `(double)sec + 1e-9 * (double)nsec` (roscpp_core: rostime/duration.h, impl/duration.h) — NOT the difference of two doubles,
// which would round differently; velocities are only bit-exact with the reference if dt is formed this way.
struct Time {
  uint32_t sec = 0, nsec = 0;
  Time() = default;
  Time(uint32_t s, uint32_t ns) : sec(s), nsec(ns) {}
  static Time fromSec(double t) {                       // ros::TimeBase::fromSec
    Time r;
    r.sec = (uint32_t)std::floor(t);
    r.nsec = (uint32_t)std::floor((t - (double)r.sec) * 1e9 + 0.5);   // boost::math::round for a non-negative value
    r.sec += r.nsec / 1000000000u; r.nsec %= 1000000000u;
    return r;
  }
  double toSec() const { return (double)sec + 1e-9 * (double)nsec; }
};
// (a - b).toSec() of two ros::Time values
inline double duration_sec(const Time &a, const Time &b) {
  int64_t sec = (int64_t)a.sec - (int64_t)b.sec, nsec = (int64_t)a.nsec - (int64_t)b.nsec;
  while (nsec >= 1000000000LL) { nsec -= 1000000000LL; ++sec; }     // normalizeSecNSecSigned
  while (nsec < 0) { nsec += 1000000000LL; --sec; }
  return (double)sec + 1e-9 * (double)nsec;
}

struct Header { uint32_t seq = 0; Time stamp; std::string frame_id; };

// stereo_msgs/DisparityImage: 32FC1 image + f, T, min/max_disparity (disparity_image_processor.cpp:5,25-27,41-42)
struct DisparityImage {
  Header header;
  int width = 0, height = 0;
  const float *data = nullptr;      // row-major, step == width * 4
  float f = 0.f, T = 0.f, min_disparity = 0.f, max_disparity = 0.f;
};

// sensor_msgs/CameraInfo: only the projection matrix P is used (image_geometry::PinholeCameraModel::fromCameraInfo)
struct CameraInfo { int width = 0, height = 0; double P[12] = {0}; };

// image_crop.cpp:24-40: the camera of the centred w x h window of an info.width x info.height image — the window starts at the
// integer ((W - w) / 2, (H - h) / 2) and the principal point moves by that offset (P[2], P[6]; K[2], K[5] alike in the reference)
inline void centred_origin(int W, int H, int w, int h, int *x0, int *y0) { *x0 = (W - w) / 2; *y0 = (H - h) / 2; }
inline CameraInfo crop_camera_info(const CameraInfo &info, int w, int h) {
  int x0 = 0, y0 = 0;
  centred_origin(info.width, info.height, w, h, &x0, &y0);
  CameraInfo c = info;
  c.P[2] = info.P[2] - x0;
  c.P[6] = info.P[6] - y0;
  c.width = w; c.height = h;
  return c;
}

// sensor_msgs/Image: row-major 8-bit pixels, `step` bytes per row (0: width * channels).  mono8 is what the disparity estimator
// consumes; bgr8 / rgb8 / bgra8 / rgba8 (image_rect_color) and packed yuv422 / yuv422_yuy2 (a UVC camera's own format) are
// converted on the GPU (mod_set_image_layout), and so are the 8-bit Bayer mosaics bayer_rggb8 / _bggr8 / _gbrg8 / _grbg8
struct Image {
  Header header; int width = 0, height = 0; const uint8_t *data = nullptr;
  std::string encoding = "mono8";
  int step = 0;
};

// An image the mirror produces (~clusters_image): the pixels live in `pixels`, view.data points at them
struct OwnedImage { Image view; std::vector<uint8_t> pixels; };

// visualization_msgs/Marker(Array) (melodic): every field of the .msg, with the defaults roscpp gives a fresh message (all zero,
// empty) — cluster2Marker (clusterer_nodelet.cpp:119-145) sets header, id, type, action, scale, color and points and leaves the rest
struct ColorRGBA { float r = 0.f, g = 0.f, b = 0.f, a = 0.f; };
struct Marker {
  enum : int32_t { POINTS = 8, ADD = 0, DELETEALL = 3 };
  Header header;
  std::string ns;
  int32_t id = 0, type = 0, action = 0;
  struct { double position[3] = {0, 0, 0}; double orientation[4] = {0, 0, 0, 0}; /* x y z w */ } pose;
  double scale[3] = {0, 0, 0};
  ColorRGBA color;
  struct { int32_t sec = 0, nsec = 0; } lifetime;
  bool frame_locked = false;
  std::vector<std::array<double, 3>> points;   // geometry_msgs/Point[]
  std::vector<ColorRGBA> colors;
  std::string text, mesh_resource;
  bool mesh_use_embedded_materials = false;
};
struct MarkerArray { std::vector<Marker> markers; };

// MOD_ENCODING_* of a sensor_msgs/Image encoding, -1 for one the library cannot take
inline int image_encoding(const std::string &e) {
  if (e == "mono8") return MOD_ENCODING_MONO8;
  if (e == "bgr8") return MOD_ENCODING_BGR8;
  if (e == "rgb8") return MOD_ENCODING_RGB8;
  if (e == "bgra8") return MOD_ENCODING_BGRA8;
  if (e == "rgba8") return MOD_ENCODING_RGBA8;
  if (e == "yuv422") return MOD_ENCODING_YUV422;             // UYVY
  if (e == "yuv422_yuy2") return MOD_ENCODING_YUV422_YUY2;   // YUYV
  return -1;
}
// MOD_ENCODING_BAYER_* of an 8-bit Bayer encoding ("bayer_rggb8", ...: demosaiced straight to grey on the GPU), -1 for any other
inline int bayer_encoding(const std::string &e) {
  if (e == "bayer_rggb8") return MOD_ENCODING_BAYER_RGGB8;
  if (e == "bayer_bggr8") return MOD_ENCODING_BAYER_BGGR8;
  if (e == "bayer_gbrg8") return MOD_ENCODING_BAYER_GBRG8;
  if (e == "bayer_grbg8") return MOD_ENCODING_BAYER_GRBG8;
  return -1;
}
// bytes per pixel of an encoding image_encoding() or bayer_encoding() returned
inline int image_channels(int encoding) {
  switch (encoding) {
    case MOD_ENCODING_MONO8: return 1;
    case MOD_ENCODING_BAYER_RGGB8: case MOD_ENCODING_BAYER_BGGR8: case MOD_ENCODING_BAYER_GBRG8: case MOD_ENCODING_BAYER_GRBG8: return 1;
    case MOD_ENCODING_YUV422: case MOD_ENCODING_YUV422_YUY2: return 2;
    case MOD_ENCODING_BGR8: case MOD_ENCODING_RGB8: return 3;
    default: return 4;
  }
}

// The layout of `image` with the camera-sized window at (x0, y0); false for an encoding the library cannot take.  side_by_side: the
// message holds both eyes, each in one half of every row (mod_set_side_by_side): the layout's width is a pane's, its step the row's
inline bool image_layout(const Image &image, int x0, int y0, ModImageLayout *layout, bool side_by_side = false) {
  const int known = image_encoding(image.encoding), enc = known >= 0 ? known : bayer_encoding(image.encoding);
  if (enc < 0 || (side_by_side && image.width % 2)) return false;
  layout->encoding = enc; layout->width = side_by_side ? image.width / 2 : image.width; layout->height = image.height;
  layout->step = image.step > 0 ? image.step : image.width * image_channels(enc);
  layout->x0 = x0; layout->y0 = y0;
  return true;
}

// cv_bridge::CvImage with encoding 32FC2: optical flow, x then y
struct FlowImage { Header header; int width = 0, height = 0; const float *data = nullptr; };

// geometry_msgs/Transform
struct Transform { double translation[3] = {0, 0, 0}; double rotation[4] = {0, 0, 0, 1}; /* x y z w */ };

// tf2::Transform in double: rotation matrix (row-major) and translation.  The pose arithmetic of integrateAndBroadcastTF
// (scene_flow_constructor.cpp:320-348): products, inverses, and the quaternion <-> matrix conversions of tf2::Matrix3x3.
struct Pose {
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  double t[3] = {0, 0, 0};
  static Pose fromTransform(const Transform &x) {          // tf2::Matrix3x3::setRotation
    const double qx = x.rotation[0], qy = x.rotation[1], qz = x.rotation[2], qw = x.rotation[3];
    const double d = qx * qx + qy * qy + qz * qz + qw * qw, s = 2.0 / d;
    const double xs = qx * s, ys = qy * s, zs = qz * s, wx = qw * xs, wy = qw * ys, wz = qw * zs;
    const double xx = qx * xs, xy = qx * ys, xz = qx * zs, yy = qy * ys, yz = qy * zs, zz = qz * zs;
    Pose p;
    const double m[3][3] = {{1.0 - (yy + zz), xy - wz, xz + wy}, {xy + wz, 1.0 - (xx + zz), yz - wx}, {xz - wy, yz + wx, 1.0 - (xx + yy)}};
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) p.R[i][j] = m[i][j]; p.t[i] = x.translation[i]; }
    return p;
  }
  Pose operator*(const Pose &o) const {
    Pose p;
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) p.R[i][j] = R[i][0] * o.R[0][j] + R[i][1] * o.R[1][j] + R[i][2] * o.R[2][j];
      p.t[i] = R[i][0] * o.t[0] + R[i][1] * o.t[1] + R[i][2] * o.t[2] + t[i];
    }
    return p;
  }
  Pose inverse() const {
    Pose p;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) p.R[i][j] = R[j][i];
    for (int i = 0; i < 3; i++) p.t[i] = -(p.R[i][0] * t[0] + p.R[i][1] * t[1] + p.R[i][2] * t[2]);
    return p;
  }
  Transform toTransform() const;
};

// The libviso2 hand-off (scene_flow_constructor.cpp:232-249): VisualOdometryStereo::getMotion() returns the 4x4 motion of the
// left camera from the previous to the current frame; the reference wraps it as tf2::Transform(Matrix3x3, Vector3) and stores
// tf2::toMsg() of it, i.e. the rotation goes through tf2::Matrix3x3::getRotation() (geometry2 0.6.x, LinearMath/Matrix3x3.h —
// not vendored by the reference; restated here, all in double) before construct() rebuilds a matrix from that quaternion.
// Feeding the kernels anything but this quaternion (e.g. the matrix itself) would differ from the reference in the last bits.
inline Transform transform_from_motion(const double m[4][4]) {
  Transform t;
  for (int i = 0; i < 3; i++) t.translation[i] = m[i][3];
  double q[4];
  const double trace = m[0][0] + m[1][1] + m[2][2];
  if (trace > 0.0) {
    double s = std::sqrt(trace + 1.0);
    q[3] = s * 0.5;
    s = 0.5 / s;
    q[0] = (m[2][1] - m[1][2]) * s;
    q[1] = (m[0][2] - m[2][0]) * s;
    q[2] = (m[1][0] - m[0][1]) * s;
  } else {
    const int i = m[0][0] < m[1][1] ? (m[1][1] < m[2][2] ? 2 : 1) : (m[0][0] < m[2][2] ? 2 : 0);
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    double s = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
    q[i] = s * 0.5;
    s = 0.5 / s;
    q[3] = (m[k][j] - m[j][k]) * s;
    q[j] = (m[j][i] + m[i][j]) * s;
    q[k] = (m[k][i] + m[i][k]) * s;
  }
  for (int i = 0; i < 4; i++) t.rotation[i] = q[i];     // x y z w
  return t;
}

inline Transform Pose::toTransform() const {   // tf2::Matrix3x3::getRotation, as transform_from_motion
  double m[4][4] = {};
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) m[i][j] = R[i][j]; m[i][3] = t[i]; }
  m[3][3] = 1.0;
  return transform_from_motion(m);
}

// sensor_msgs/PointCloud2 carrying pcl::PointXYZVelocity records (point_step 32; x@0 y@4 z@8 vx@16 vy@20 vz@24)
struct PointCloud2 {
  Header header;
  uint32_t width = 0, height = 0, point_step = 32, row_step = 0;
  bool is_dense = true;
  std::vector<uint8_t> data;
};

// moving_object_msgs/MovingObject(Array) (moving_object_msgs/msg/*.msg)
struct MovingObject {
  int32_t id = 0;
  struct { double position[3]; double orientation[4]; } center;
  double velocity[3];
  double bounding_box[3];
};
struct MovingObjectArray { Header header; std::vector<MovingObject> moving_object_array; };

inline MovingObject to_message(const ModObject &o) {
  MovingObject m;
  m.id = o.id;
  for (int i = 0; i < 3; i++) { m.center.position[i] = o.center[i]; m.velocity[i] = o.velocity[i]; m.bounding_box[i] = o.bounding_box[i]; }
  for (int i = 0; i < 4; i++) m.center.orientation[i] = o.orientation[i];
  return m;
}
// publishMovingObjects (clusterer_nodelet.cpp:324-343): the first n records the library reported, at most the `cap` the array holds
inline void fill_objects(MovingObjectArray &out, const Header &header, const ModObject *objects, int n, size_t cap) {
  out.header = header;
  out.moving_object_array.clear();
  for (int i = 0; i < n && i < (int)cap; i++) out.moving_object_array.push_back(to_message(objects[i]));
}
// publishPointcloud (scene_flow_constructor.cpp:351-362): the organized w x h cloud of 32-byte records around `data`
inline void describe_cloud(PointCloud2 &cloud, const Header &header, int w, int h) {
  cloud.header = header;
  cloud.width = w; cloud.height = h;
  cloud.point_step = 32; cloud.row_step = 32 * w;
  cloud.is_dense = true;   // PCL's (width, height, value) constructor leaves is_dense = true
}

// geometry_msgs/Transform <-> the C ABI's ModTransform
inline ModTransform to_mod(const Transform &x) {
  ModTransform m{};
  for (int i = 0; i < 3; i++) m.t[i] = x.translation[i];
  for (int i = 0; i < 4; i++) m.q[i] = x.rotation[i];
  return m;
}
inline Transform from_mod(const ModTransform &m) {
  Transform x;
  for (int i = 0; i < 3; i++) x.translation[i] = m.t[i];
  for (int i = 0; i < 4; i++) x.rotation[i] = m.q[i];
  return x;
}

}  // namespace mod_host
