// clusterer_nodelet.hpp — host-side mirror of scene_flow_clusterer::ClustererNodelet
// (scene_flow_clusterer/include/clusterer_nodelet.h:37-108): dataCB() on a PointCloud2 of pcl::PointXYZVelocity,
// reconfigureCB(), and the MovingObjectArray it publishes.  clustering() and cluster2MovingObject() run on the GPU
// through the C ABI (include/mod_sf.h).  clustering() also returns the pcl::IndicesClusters and the points cluster2Marker puts
// into the ~clusters markers (mod_set_cluster_members).  publishClusters() and publishClustersImage() fill the ~clusters MarkerArray
// and the ~clusters_image message; the markers' colours (ColorSet) and the image's pixels are the library's (mod_cluster_color,
// mod_set_cluster_image: the built-in table is the library's own, not OpenCV's COLORMAP_HSV).
#pragma once
#include <array>
#include <stdexcept>
#include <vector>

#include "messages.hpp"

namespace scene_flow_clusterer {

#ifndef MOD_HOST_ROS_CONFIG   // a ROS build includes the dynamic_reconfigure-generated scene_flow_clusterer/ClustererConfig.h first
struct ClustererConfig {   // cfg/Clusterer.cfg:8-11
  int cluster_size = 2500;
  double depth_diff = 0.15;
  double dynamic_speed = 0.3;
  int neighbor_distance = 4;
};
#endif

class ClustererNodelet {
 public:
  explicit ClustererNodelet(ModContext *ctx) : ctx_(ctx) {}
  typedef std::vector<std::vector<int>> IndicesClusters;                      // pcl::IndicesClusters' content
  typedef std::vector<std::vector<std::array<double, 3>>> MarkerPoints;       // per cluster, what cluster2Marker puts into marker.points

  // reconfigureCB (clusterer_nodelet.cpp:345-352); the constructor's dynamic_flow_diff in the shared block is preserved.
  void reconfigureCB(const ClustererConfig &config) {
    ModParams p{};
    if (mod_get_params(ctx_, &p) != MOD_OK) p.dynamic_flow_diff = 5;
    p.cluster_size = config.cluster_size; p.depth_diff = config.depth_diff;
    p.dynamic_speed = config.dynamic_speed; p.neighbor_distance = config.neighbor_distance;
    check(mod_set_params(ctx_, &p));
  }

  // dataCB (clusterer_nodelet.cpp:221-242): clustering() + publishMovingObjects().  `cluster_map` receives the final
  // cluster_map_ (-1 = NOT_BELONGED_).  An unorganized / wrongly sized cloud is an error, as .at() would throw there.
  void dataCB(const mod_host::PointCloud2 &input_pc_msg, mod_host::MovingObjectArray *moving_objects, std::vector<int32_t> *cluster_map = nullptr) {
    cluster(input_pc_msg, moving_objects, cluster_map);
  }

  // dataCB with clusters_msg / clusters_image (each may be null; with both null it is the call above): what
  // publishClusters (:269-290) and publishClustersImage (:292-322) would publish for this cloud — the reference makes each only
  // while its topic has subscribers (:233-236).  The image comes from ModClusterImage.host_image of the same
  // mod_cluster_cloud_host call that makes the objects; the markers need setContextMaxObjects().
  void dataCB(const mod_host::PointCloud2 &input_pc_msg, mod_host::MovingObjectArray *moving_objects,
              std::vector<int32_t> *cluster_map, mod_host::MarkerArray *clusters_msg, mod_host::OwnedImage *clusters_image) {
    if (!clusters_msg && !clusters_image) return cluster(input_pc_msg, moving_objects, cluster_map);
    const size_t n = (size_t)input_pc_msg.width * input_pc_msg.height;
    struct Off { ModContext *c; ~Off() { if (c) (void)mod_set_cluster_image(c, nullptr); } } off{clusters_image ? ctx_ : nullptr};   // the setting does not outlive the buffer
    if (clusters_image) {
      clusters_image->pixels.assign(3 * n, 0);
      ModClusterImage im{nullptr, clusters_image->pixels.data(), nullptr, 0};
      check(mod_set_cluster_image(ctx_, &im));
    }
    if (clusters_msg) {
      if (context_max_objects_ < 1) throw std::runtime_error("ClustererNodelet: setContextMaxObjects() must be called before the markers are asked for");
      IndicesClusters clusters;
      MarkerPoints points;
      clustering(input_pc_msg, context_max_objects_, &clusters, &points, moving_objects, cluster_map);
      publishClusters(input_pc_msg.header, points, clusters_msg);
    } else {
      cluster(input_pc_msg, moving_objects, cluster_map);
    }
    if (clusters_image) publishClustersImage(input_pc_msg.header, (int)input_pc_msg.width, (int)input_pc_msg.height, clusters_image);
  }

  // publishClusters (:269-290) with cluster2Marker (:119-145): one DELETEALL marker, then marker k = cluster k as POINTS with the
  // cluster's member points and colour k of ColorSet::resize(K) (mod_cluster_color; r, g, b = the bytes over 255.0, narrowed to F32)
  static void publishClusters(const mod_host::Header &input_header, const MarkerPoints &marker_points, mod_host::MarkerArray *clusters_msg) {
    clusters_msg->markers.assign(1, mod_host::Marker());
    clusters_msg->markers[0].action = mod_host::Marker::DELETEALL;
    const int32_t K = (int32_t)marker_points.size();
    for (int32_t k = 0; k < K; k++) {
      mod_host::Marker m;
      uint8_t bgr[3] = {0, 0, 0};
      if (mod_cluster_color(k, K, nullptr, bgr) != MOD_OK) throw std::runtime_error("libmod_sf: mod_cluster_color refused a cluster of its own frame");
      m.header = input_header;
      m.id = k; m.type = mod_host::Marker::POINTS; m.action = mod_host::Marker::ADD;
      m.scale[0] = 0.05; m.scale[1] = 0.05; m.scale[2] = 0;
      m.color.a = 1.0f;
      m.color.r = (float)(bgr[2] / 255.0); m.color.g = (float)(bgr[1] / 255.0); m.color.b = (float)(bgr[0] / 255.0);
      m.points = marker_points[k];
      clusters_msg->markers.push_back(std::move(m));
    }
  }

  // publishClustersImage (:292-322) around pixels the library has drawn into clusters_image->pixels: frame_id and stamp of the
  // input (seq is not copied, :317-319), bgr8, packed rows
  static void publishClustersImage(const mod_host::Header &input_header, int width, int height, mod_host::OwnedImage *clusters_image) {
    mod_host::Image &v = clusters_image->view;
    v.header = mod_host::Header();
    v.header.frame_id = input_header.frame_id; v.header.stamp = input_header.stamp;
    v.width = width; v.height = height;
    v.encoding = "bgr8"; v.step = 3 * width;
    v.data = clusters_image->pixels.data();
  }

  void setMaxObjects(int n) { max_objects_ = n; }
  // the capacity the context was created with (ModConfig.max_objects, or max_width * max_height / 100 when that was 0): the stride of
  // the member lists' offsets, which dataCB needs for the markers
  void setContextMaxObjects(int n) { context_max_objects_ = n; }

 private:
  // clustering() + publishMovingObjects(): one mod_cluster_cloud_host call
  void cluster(const mod_host::PointCloud2 &input_pc_msg, mod_host::MovingObjectArray *moving_objects, std::vector<int32_t> *cluster_map) {
    const size_t n = (size_t)input_pc_msg.width * input_pc_msg.height;
    if (cluster_map) cluster_map->resize(n);
    std::vector<ModObject> objs(max_objects_);
    int32_t n_obj = 0;
    check(mod_cluster_cloud_host(ctx_, input_pc_msg.data.data(), (int32_t)input_pc_msg.width, (int32_t)input_pc_msg.height,
                                 (int32_t)input_pc_msg.point_step, (int32_t)input_pc_msg.row_step,
                                 cluster_map ? cluster_map->data() : nullptr, objs.data(), (int32_t)objs.size(), &n_obj));
    // publishMovingObjects (:324-343): header = input header, ids over accepted clusters
    if (moving_objects) mod_host::fill_objects(*moving_objects, input_pc_msg.header, objs.data(), n_obj, objs.size());
  }

 public:
  // clustering() (clusterer_nodelet.cpp:85-95) asked for its result: dataCB, and with it `clusters` = the pcl::IndicesClusters
  // content (clusterMap2IndicesCluster, :97-117: per surviving cluster its pixel indices, column-major) and, when `marker_points`
  // is not null, per cluster the (x, y, z) cluster2Marker pushes into marker.points (:119-145; F32 coordinates widened to F64).
  // context_max_objects: the capacity the context was created with (ModConfig.max_objects, or max_width * max_height / 100 when
  // that was 0) — the stride of the offsets.  Only the offsets and the used prefix of the lists come back from the device.
  void clustering(const mod_host::PointCloud2 &input_pc_msg, int context_max_objects, IndicesClusters *clusters, MarkerPoints *marker_points,
                  mod_host::MovingObjectArray *moving_objects = nullptr, std::vector<int32_t> *cluster_map = nullptr) {
    const size_t n = (size_t)input_pc_msg.width * input_pc_msg.height;
    DeviceLists dev(ctx_, (size_t)context_max_objects + 1, n, marker_points != nullptr);
    ModClusterMembers m{dev.offsets, dev.indices, dev.points, 0};
    check(mod_set_cluster_members(ctx_, &m));
    struct Off { ModContext *c; ~Off() { (void)mod_set_cluster_members(c, nullptr); } } off{ctx_};   // the setting does not outlive the buffers
    dataCB(input_pc_msg, moving_objects, cluster_map);
    std::vector<int32_t> offsets((size_t)context_max_objects + 1);
    check(mod_memcpy_d2h(ctx_, offsets.data(), dev.offsets, sizeof(int32_t) * offsets.size()));
    size_t K = 0;                        // every surviving cluster has members: the offsets rise up to K, then stay
    while (K + 1 < offsets.size() && offsets[K + 1] > offsets[K]) K++;
    const size_t used = (size_t)offsets[K];
    std::vector<int32_t> idx(used);
    std::vector<float> pts(marker_points ? 3 * used : 0);
    if (used) check(mod_memcpy_d2h(ctx_, idx.data(), dev.indices, sizeof(int32_t) * used));
    if (used && marker_points) check(mod_memcpy_d2h(ctx_, pts.data(), dev.points, sizeof(float) * 3 * used));
    if (clusters) clusters->assign(K, std::vector<int>());
    if (marker_points) marker_points->assign(K, std::vector<std::array<double, 3>>());
    for (size_t k = 0; k < K; k++)
      for (int32_t i = offsets[k]; i < offsets[k + 1]; i++) {
        if (clusters) (*clusters)[k].push_back(idx[i]);
        if (marker_points) (*marker_points)[k].push_back({(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]});
      }
  }

 private:
  void check(int rc) { if (rc < 0) throw std::runtime_error(std::string("libmod_sf: ") + mod_last_error(ctx_)); }
  // the device buffers of one clustering() call
  struct DeviceLists {
    ModContext *c; int32_t *offsets = nullptr, *indices = nullptr; float *points = nullptr;
    DeviceLists(ModContext *ctx, size_t n_off, size_t n, bool pts) : c(ctx) {
      void *p = nullptr;
      bool ok = mod_malloc(c, sizeof(int32_t) * n_off, &p) == MOD_OK; offsets = (int32_t *)p; p = nullptr;
      ok = ok && mod_malloc(c, sizeof(int32_t) * n, &p) == MOD_OK; indices = (int32_t *)p; p = nullptr;
      if (pts) { ok = ok && mod_malloc(c, sizeof(float) * 3 * n, &p) == MOD_OK; points = (float *)p; }
      if (!ok) { release(); throw std::runtime_error("libmod_sf: no device memory for the cluster lists"); }
    }
    ~DeviceLists() { release(); }
    void release() { for (void *p : {(void *)offsets, (void *)indices, (void *)points}) if (p) (void)mod_free(c, p); offsets = indices = nullptr; points = nullptr; }
    DeviceLists(const DeviceLists &) = delete;
    DeviceLists &operator=(const DeviceLists &) = delete;
  };
  ModContext *ctx_;
  int max_objects_ = 1024;
  int context_max_objects_ = 0;
};

}  // namespace scene_flow_clusterer
