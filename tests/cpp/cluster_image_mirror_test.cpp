// cluster_image_mirror_test.cpp — the host mirror's dataCB() asked for the ~clusters MarkerArray and the ~clusters_image message:
// both must follow from the mirror's OWN cluster map of the same call — the image is that map coloured with mod_cluster_color, the
// markers are DELETEALL, then cluster k as POINTS with colour k and the cloud's coordinates in clusterMap2IndicesCluster's order —
// and the objects and the map must equal those of a dataCB() that asks for neither.  Standalone process over the C ABI
// (tests/test_gpu_cluster_image_mirror.py hands it a golden cloud and compares the dumped image with the Python model).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../moving_object_detector_amd/host/clusterer_nodelet.hpp"
#include "../../moving_object_detector_amd/host/ros_wire.hpp"

template <class T>
static std::vector<T> read_all(const std::string &p) {
  FILE *f = fopen(p.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", p.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v(n / sizeof(T));
  if (fread(v.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return v;
}
static void write_all(const std::string &p, const void *d, size_t n) {
  FILE *f = fopen(p.c_str(), "wb");
  if (!f || fwrite(d, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", p.c_str()); exit(2); }
  fclose(f);
}

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: cluster_image_mirror_test <dir>\n"); return 1; }
  const std::string dir = argv[1];
  auto dims = read_all<double>(dir + "/dims.f64");   // W H
  auto prm = read_all<double>(dir + "/prm.f64");     // flow_diff cluster_size n depth_diff dynamic_speed
  auto cloud_f = read_all<float>(dir + "/cloud.f32"); // [H][W][8]: x y z _ vx vy vz _
  const int W = (int)dims[0], H = (int)dims[1];
  const size_t N = (size_t)W * H;
  if (cloud_f.size() != N * 8) { fprintf(stderr, "cloud size\n"); return 2; }

  ModConfig cfg{};
  cfg.device = 0; cfg.max_width = W; cfg.max_height = H; cfg.max_frames = 1;
  cfg.max_objects = W * H / (int)prm[1] + 1;
  ModContext *ctx = nullptr;
  if (mod_create(&cfg, &ctx) != MOD_OK) { fprintf(stderr, "mod_create failed\n"); return 4; }
  try {
    scene_flow_clusterer::ClustererNodelet clusterer(ctx);
    clusterer.setMaxObjects(cfg.max_objects);
    clusterer.setContextMaxObjects(cfg.max_objects);
    clusterer.reconfigureCB({(int)prm[1], prm[3], prm[4], (int)prm[2]});
    mod_host::PointCloud2 cloud;
    cloud.header.seq = 9; cloud.header.stamp = mod_host::Time(12, 34); cloud.header.frame_id = "left";
    cloud.width = W; cloud.height = H; cloud.row_step = 32 * W;
    cloud.data.resize(cloud_f.size() * 4);
    memcpy(cloud.data.data(), cloud_f.data(), cloud.data.size());

    mod_host::MovingObjectArray objs0, objs;
    std::vector<int32_t> map0, map;
    clusterer.dataCB(cloud, &objs0, &map0);                       // today's call
    mod_host::MarkerArray markers;
    mod_host::OwnedImage image;
    clusterer.dataCB(cloud, &objs, &map, &markers, &image);
    CHECK(map == map0 && ros_wire::serialize(objs) == ros_wire::serialize(objs0));
    int32_t on = -1;
    CHECK(mod_get_cluster_image(ctx, nullptr, &on) == MOD_OK && on == 0);
    CHECK(mod_get_cluster_members(ctx, nullptr, &on) == MOD_OK && on == 0);

    int K = 0;
    for (int32_t l : map) if (l + 1 > K) K = l + 1;
    CHECK(K >= 1);
    // ~clusters_image: header without seq, bgr8, packed; pixel i is black or colour map[i] of K
    const mod_host::Image &v = image.view;
    CHECK(v.header.seq == 0 && v.header.stamp.sec == 12 && v.header.stamp.nsec == 34 && v.header.frame_id == "left");
    CHECK(v.width == W && v.height == H && v.encoding == "bgr8" && v.step == 3 * W && v.data == image.pixels.data() && image.pixels.size() == 3 * N);
    size_t coloured = 0;
    for (size_t i = 0; i < N && image.pixels.size() == 3 * N; i++) {
      uint8_t want[3] = {0, 0, 0};
      if (map[i] >= 0) { CHECK(mod_cluster_color(map[i], K, nullptr, want) == MOD_OK); coloured++; }
      if (memcmp(want, &image.pixels[3 * i], 3) != 0) { fprintf(stderr, "pixel %zu (label %d) differs\n", i, map[i]); fails++; break; }
    }
    CHECK(ros_wire::serialize(v).size() == 12 + 4 + 4 + 8 + 8 + 1 + 4 + 4 + 3 * N);
    // ~clusters: DELETEALL, then marker k
    CHECK((int)markers.markers.size() == K + 1);
    if ((int)markers.markers.size() == K + 1) {
      mod_host::MarkerArray del;
      del.markers.resize(1);
      del.markers[0].action = mod_host::Marker::DELETEALL;
      mod_host::MarkerArray first;
      first.markers.push_back(markers.markers[0]);
      CHECK(ros_wire::serialize(first) == ros_wire::serialize(del));
      std::vector<std::vector<int>> want(K);                      // clusterMap2IndicesCluster: u outer, v inner
      for (int u = 0; u < W; u++)
        for (int vv = 0; vv < H; vv++) if (map[(size_t)vv * W + u] >= 0) want[map[(size_t)vv * W + u]].push_back(vv * W + u);
      FILE *mf = fopen((dir + "/markers.txt").c_str(), "w");
      for (int k = 0; k < K; k++) {
        const mod_host::Marker &m = markers.markers[k + 1];
        uint8_t bgr[3];
        CHECK(mod_cluster_color(k, K, nullptr, bgr) == MOD_OK);
        CHECK(m.header.seq == 9 && m.header.stamp.sec == 12 && m.header.stamp.nsec == 34 && m.header.frame_id == "left");
        CHECK(m.id == k && m.type == 8 && m.action == 0 && m.ns.empty() && m.colors.empty());
        CHECK(m.scale[0] == 0.05 && m.scale[1] == 0.05 && m.scale[2] == 0.0);
        CHECK(m.color.a == 1.0f && m.color.r == (float)(bgr[2] / 255.0) && m.color.g == (float)(bgr[1] / 255.0) && m.color.b == (float)(bgr[0] / 255.0));
        CHECK(m.points.size() == want[k].size());
        for (size_t i = 0; i < want[k].size() && m.points.size() == want[k].size(); i++) {
          const float *rec = &cloud_f[(size_t)want[k][i] * 8];
          const double e[3] = {(double)rec[0], (double)rec[1], (double)rec[2]};
          if (memcmp(e, m.points[i].data(), sizeof(e)) != 0) { fprintf(stderr, "marker %d point %zu differs\n", k, i); fails++; break; }
        }
        if (mf) fprintf(mf, "%d %.9g %.9g %.9g %zu\n", m.id, m.color.r, m.color.g, m.color.b, m.points.size());
      }
      if (mf) fclose(mf);
    }
    // each alone gives the same message
    mod_host::MarkerArray markers2;
    mod_host::OwnedImage image2;
    clusterer.dataCB(cloud, nullptr, nullptr, &markers2, nullptr);
    clusterer.dataCB(cloud, nullptr, nullptr, nullptr, &image2);
    CHECK(ros_wire::serialize(markers2) == ros_wire::serialize(markers));
    CHECK(image2.pixels == image.pixels && ros_wire::serialize(image2.view) == ros_wire::serialize(image.view));
    CHECK(mod_get_cluster_image(ctx, nullptr, &on) == MOD_OK && on == 0);
    write_all(dir + "/image.u8", image.pixels.data(), image.pixels.size());
    write_all(dir + "/labels.i32", map.data(), map.size() * sizeof(int32_t));
    if (!fails) printf("ok: %d clusters, %zu coloured pixels, %zu objects\n", K, coloured, objs.moving_object_array.size());
  } catch (const std::exception &e) {
    fprintf(stderr, "exception: %s\n", e.what());
    fails++;
  }
  mod_destroy(ctx);
  return fails ? 5 : 0;
}
