// cluster_members_test.cpp — the host mirror's clustering() asked for its clusters: the pcl::IndicesClusters content and the marker
// points must equal what the reference's double loop (clusterMap2IndicesCluster, clusterer_nodelet.cpp:104-116) makes of the
// mirror's OWN cluster map, and the coordinates of the cloud at those pixels.  Standalone process over the C ABI
// (tests/test_gpu_cluster_members_mirror.py hands it a golden cloud): no torch, no Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../moving_object_detector_amd/host/clusterer_nodelet.hpp"

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

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: cluster_members_test <dir>\n"); return 1; }
  const std::string dir = argv[1];
  auto dims = read_all<double>(dir + "/dims.f64");   // W H
  auto prm = read_all<double>(dir + "/prm.f64");     // flow_diff cluster_size n depth_diff dynamic_speed
  auto cloud_f = read_all<float>(dir + "/cloud.f32"); // [H][W][8]: x y z _ vx vy vz _
  const int W = (int)dims[0], H = (int)dims[1];
  if (cloud_f.size() != (size_t)W * H * 8) { fprintf(stderr, "cloud size\n"); return 2; }

  ModConfig cfg{};
  cfg.device = 0; cfg.max_width = W; cfg.max_height = H; cfg.max_frames = 1;
  cfg.max_objects = W * H / (int)prm[1] + 1;
  ModContext *ctx = nullptr;
  if (mod_create(&cfg, &ctx) != MOD_OK) { fprintf(stderr, "mod_create failed\n"); return 4; }
  int rc = 0;
  try {
    scene_flow_clusterer::ClustererNodelet clusterer(ctx);
    clusterer.setMaxObjects(cfg.max_objects);
    clusterer.reconfigureCB({(int)prm[1], prm[3], prm[4], (int)prm[2]});
    mod_host::PointCloud2 cloud;
    cloud.width = W; cloud.height = H; cloud.row_step = 32 * W;
    cloud.data.resize(cloud_f.size() * 4);
    memcpy(cloud.data.data(), cloud_f.data(), cloud.data.size());

    scene_flow_clusterer::ClustererNodelet::IndicesClusters clusters;
    scene_flow_clusterer::ClustererNodelet::MarkerPoints points;
    mod_host::MovingObjectArray objs;
    std::vector<int32_t> cluster_map;
    clusterer.clustering(cloud, cfg.max_objects, &clusters, &points, &objs, &cluster_map);

    // clusterMap2IndicesCluster on the mirror's own map: u outer, v inner, index v * W + u
    int K = 0;
    for (int32_t l : cluster_map) if (l + 1 > K) K = l + 1;
    std::vector<std::vector<int>> want(K);
    for (int u = 0; u < W; u++)
      for (int v = 0; v < H; v++) {
        const int32_t l = cluster_map[(size_t)v * W + u];
        if (l >= 0) want[l].push_back(v * W + u);
      }
    if ((int)clusters.size() != K || K == 0) { fprintf(stderr, "cluster count %zu, map holds %d\n", clusters.size(), K); rc = 5; }
    size_t members = 0;
    for (int k = 0; k < K && !rc; k++) {
      if (clusters[k] != want[k]) { fprintf(stderr, "cluster %d: list differs (%zu vs %zu members)\n", k, clusters[k].size(), want[k].size()); rc = 6; break; }
      if (points[k].size() != want[k].size()) { fprintf(stderr, "cluster %d: %zu marker points\n", k, points[k].size()); rc = 7; break; }
      for (size_t i = 0; i < want[k].size(); i++) {
        const float *rec = &cloud_f[(size_t)want[k][i] * 8];   // cluster2Marker: point.x = pc.at(index).x, ... (:137-141)
        const double e[3] = {(double)rec[0], (double)rec[1], (double)rec[2]};
        if (memcmp(e, points[k][i].data(), sizeof(e)) != 0) { fprintf(stderr, "cluster %d member %zu: marker point differs\n", k, i); rc = 8; break; }
      }
      members += want[k].size();
    }
    // the lists alone (no marker points asked for) are the same lists; the setting is off again afterwards
    scene_flow_clusterer::ClustererNodelet::IndicesClusters again;
    clusterer.clustering(cloud, cfg.max_objects, &again, nullptr);
    if (!rc && again != clusters) { fprintf(stderr, "lists differ without marker points\n"); rc = 9; }
    int32_t on = -1;
    if (!rc && (mod_get_cluster_members(ctx, nullptr, &on) != MOD_OK || on != 0)) { fprintf(stderr, "setting left on\n"); rc = 10; }
    if (!rc) printf("ok: %d clusters, %zu members, %zu objects\n", K, members, objs.moving_object_array.size());
  } catch (const std::exception &e) {
    fprintf(stderr, "exception: %s\n", e.what());
    rc = 11;
  }
  mod_destroy(ctx);
  return rc;
}
