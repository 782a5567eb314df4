// ros_wire_markers_test.cpp — the ROS-1 wire format of sensor_msgs/Image and visualization_msgs/MarkerArray (host/ros_wire.hpp)
// against buffers written out by hand from the .msg definitions: byte counts, field order, and the round trip through deserialize.
// No GPU, no library: headers only (tests/test_host_wire_markers.py compiles and runs it).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../moving_object_detector_amd/host/ros_wire.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static void put(std::vector<uint8_t> &b, std::initializer_list<int> v) { for (int x : v) b.push_back((uint8_t)x); }
static void zeros(std::vector<uint8_t> &b, int n) { b.insert(b.end(), n, 0); }

static bool same(const ros_wire::Bytes &got, const std::vector<uint8_t> &want, const char *what) {
  if (got.size() != want.size()) { fprintf(stderr, "%s: %zu bytes, expected %zu\n", what, got.size(), want.size()); return false; }
  for (size_t i = 0; i < got.size(); i++)
    if (got[i] != want[i]) { fprintf(stderr, "%s: byte %zu is %02x, expected %02x\n", what, i, got[i], want[i]); return false; }
  return true;
}

int main() {
  // ---- sensor_msgs/Image: 2 x 1 bgr8 ----
  const uint8_t px[6] = {10, 20, 30, 40, 50, 60};
  mod_host::Image im;
  im.header.stamp = mod_host::Time(5, 6); im.header.frame_id = "c";
  im.width = 2; im.height = 1; im.encoding = "bgr8"; im.step = 6; im.data = px;
  std::vector<uint8_t> e;
  put(e, {0, 0, 0, 0,  5, 0, 0, 0,  6, 0, 0, 0,  1, 0, 0, 0, 'c'});          // header: seq, stamp.sec, stamp.nsec, frame_id
  put(e, {1, 0, 0, 0,  2, 0, 0, 0});                                         // height, width
  put(e, {4, 0, 0, 0, 'b', 'g', 'r', '8'});                                  // encoding
  put(e, {0});                                                               // is_bigendian
  put(e, {6, 0, 0, 0});                                                      // step
  put(e, {6, 0, 0, 0, 10, 20, 30, 40, 50, 60});                              // data[]
  CHECK(e.size() == 48);
  const ros_wire::Bytes ib = ros_wire::serialize(im);
  CHECK(same(ib, e, "Image"));
  mod_host::OwnedImage back;
  ros_wire::deserialize(ib.data(), ib.size(), back);
  CHECK(back.view.header.seq == 0 && back.view.header.stamp.sec == 5 && back.view.header.stamp.nsec == 6 && back.view.header.frame_id == "c");
  CHECK(back.view.width == 2 && back.view.height == 1 && back.view.encoding == "bgr8" && back.view.step == 6);
  CHECK(back.pixels.size() == 6 && back.view.data == back.pixels.data() && memcmp(back.pixels.data(), px, 6) == 0);
  CHECK(ros_wire::serialize(back.view) == ib);
  im.step = 0;                                                               // packed rows: step = width * 3
  CHECK(ros_wire::serialize(im) == ib);
  bool threw = false;
  try { ros_wire::deserialize(ib.data(), ib.size() - 1, back); } catch (const std::runtime_error &) { threw = true; }
  CHECK(threw);

  // ---- visualization_msgs/MarkerArray: one marker with two points ----
  mod_host::MarkerArray arr;
  arr.markers.resize(1);
  mod_host::Marker &m = arr.markers[0];
  m.header.seq = 7; m.header.stamp = mod_host::Time(100, 200); m.header.frame_id = "cam";
  m.id = 3; m.type = mod_host::Marker::POINTS; m.action = mod_host::Marker::ADD;
  m.scale[0] = 0.05; m.scale[1] = 0.05; m.scale[2] = 0;
  m.color.r = 1.0f; m.color.g = 0.5f; m.color.b = 0.25f; m.color.a = 1.0f;
  m.points.push_back({1.0, 2.0, 3.0});
  m.points.push_back({-1.0, 0.5, 4.0});
  e.clear();
  put(e, {1, 0, 0, 0});                                                      // markers[] count
  put(e, {7, 0, 0, 0,  100, 0, 0, 0,  200, 0, 0, 0,  3, 0, 0, 0, 'c', 'a', 'm'});   // header
  put(e, {0, 0, 0, 0});                                                      // ns ""
  put(e, {3, 0, 0, 0,  8, 0, 0, 0,  0, 0, 0, 0});                            // id, type = POINTS, action = ADD
  zeros(e, 56);                                                              // pose: position 3 f64, orientation 4 f64, all 0
  put(e, {0x9a, 0x99, 0x99, 0x99, 0x99, 0x99, 0xa9, 0x3f});                  // scale.x = 0.05
  put(e, {0x9a, 0x99, 0x99, 0x99, 0x99, 0x99, 0xa9, 0x3f});                  // scale.y = 0.05
  zeros(e, 8);                                                               // scale.z = 0
  put(e, {0, 0, 0x80, 0x3f,  0, 0, 0, 0x3f,  0, 0, 0x80, 0x3e,  0, 0, 0x80, 0x3f});   // color r 1.0, g 0.5, b 0.25, a 1.0 (f32)
  zeros(e, 8);                                                               // lifetime sec, nsec
  put(e, {0});                                                               // frame_locked
  put(e, {2, 0, 0, 0});                                                      // points[] count
  put(e, {0, 0, 0, 0, 0, 0, 0xf0, 0x3f,  0, 0, 0, 0, 0, 0, 0x00, 0x40,  0, 0, 0, 0, 0, 0, 0x08, 0x40});   // (1, 2, 3)
  put(e, {0, 0, 0, 0, 0, 0, 0xf0, 0xbf,  0, 0, 0, 0, 0, 0, 0xe0, 0x3f,  0, 0, 0, 0, 0, 0, 0x10, 0x40});   // (-1, 0.5, 4)
  put(e, {0, 0, 0, 0});                                                      // colors[] count
  put(e, {0, 0, 0, 0,  0, 0, 0, 0});                                         // text "", mesh_resource ""
  put(e, {0});                                                               // mesh_use_embedded_materials
  CHECK(e.size() == 4 + 154 + 3 + 48);
  const ros_wire::Bytes mb = ros_wire::serialize(arr);
  CHECK(same(mb, e, "MarkerArray"));
  mod_host::MarkerArray got;
  ros_wire::deserialize(mb.data(), mb.size(), got);
  CHECK(got.markers.size() == 1);
  if (got.markers.size() == 1) {
    const mod_host::Marker &g = got.markers[0];
    CHECK(g.header.seq == 7 && g.header.stamp.sec == 100 && g.header.stamp.nsec == 200 && g.header.frame_id == "cam" && g.ns.empty());
    CHECK(g.id == 3 && g.type == 8 && g.action == 0 && g.scale[0] == 0.05 && g.scale[1] == 0.05 && g.scale[2] == 0.0);
    CHECK(g.color.r == 1.0f && g.color.g == 0.5f && g.color.b == 0.25f && g.color.a == 1.0f);
    CHECK(g.points.size() == 2 && g.points[1][0] == -1.0 && g.points[1][1] == 0.5 && g.points[1][2] == 4.0 && g.colors.empty());
    CHECK(g.pose.orientation[3] == 0.0 && !g.frame_locked && !g.mesh_use_embedded_materials && g.text.empty() && g.mesh_resource.empty());
  }
  CHECK(ros_wire::serialize(got) == mb);
  // what publishClusters puts first: a default marker whose action is DELETEALL is 154 bytes behind the array's count, action at byte 32
  mod_host::MarkerArray del;
  del.markers.resize(1);
  del.markers[0].action = mod_host::Marker::DELETEALL;
  const ros_wire::Bytes db = ros_wire::serialize(del);
  CHECK(db.size() == 4 + 154 && db[4 + 16 + 4 + 8] == 3);
  for (size_t i = 0; i < db.size(); i++) CHECK(db[i] == (i == 0 ? 1 : i == 32 ? 3 : 0));
  threw = false;
  try { ros_wire::deserialize(mb.data(), mb.size() - 5, got); } catch (const std::runtime_error &) { threw = true; }
  CHECK(threw);
  if (!fails) printf("ok: Image %zu bytes, MarkerArray %zu bytes\n", ib.size(), mb.size());
  return fails ? 1 : 0;
}
