// scene_flow_constructor_node.cpp — the `scene_flow_constructor` executable of the reference (scene_flow_constructor/CMakeLists.txt:45-48,
// src/scene_flow_constructor_node.cpp:3-9) with the hot path on an MI355X.  Same node name, same subscriptions (left_image /
// right_image + their camera_info, exact-time synchronised, queue 1 — scene_flow_constructor.cpp:51-62), same four private topics
// (~depth, ~optical_flow, ~scene_flow, ~synthetic_optical_flow, :45-48), same dynamic_reconfigure server (:40-42), every publish
// gated on getNumSubscribers() (:99,114,141,144).
//
// What runs where:
//   disparity        on the GPU (libmod_sf's SGM), replacing sgm_gpu::SgmGpu::computeDisparity (:35,267)
//                    `~disparity_subpixel` (default false): disparities in sixteenths of a pixel (mod_set_disparity_subpixel)
//                    `~uniqueness_ratio`, `~speckle_size`, `~speckle_range` (stereo_image_proc's names; default 0 = off): the
//                    estimator's rejection filters (mod_set_disparity_filters)
//   scene flow       on the GPU, overlapped with the next frame's estimators like construct_thread_ (:389-392): submitStereo() /
//                    collect(); the disparity plane stays in HBM as the next frame's previous one (:397-398)
//   optical flow     on the GPU (libmod_sf's census flow, not PWC-Net) when `~gpu_estimators` is true (default); with it false, the
//                    CALL-OUT estimateOpticalFlow(): the reference asks pwc_net (:281-291); not part of this package
//                    `~flow_seeds` (default 1 = off; 5): neighbour-seed propagation of that flow (mod_set_flow_propagation)
//   camera motion    on the GPU (libmod_sf's stereo ego-motion, not libviso2) when `~gpu_estimators` is true: submitOdometry() /
//                    collectOdometry() take the images as they arrive (encoding and step from the message, mod_set_image_layout), the
//                    pose is integrated and odom -> base_link broadcast as integrateAndBroadcastTF does (:246,320-348; frame ids from
//                    `~visual_odometry/{base_link,odom}_frame_id`, base -> camera from TF, identity when it is not available); with it
//                    false, the CALL-OUT estimateCameraMotion(): the reference runs libviso2 and a TF lookup (:214-256)
//   crop             `~crop_width` / `~crop_height` (0 = off) take the centred window of the images on the GPU and the camera of
//                    crop_camera_info(), in place of the ZED launch's two image_crop nodes (image_crop.cpp:24-40)
//   clustering       on the GPU, IN THIS PROCESS, when `~publish_moving_objects` is true (default): the node then advertises
//                    `~moving_objects` itself (what the separate scene_flow_clusterer publishes, clusterer_nodelet.cpp:324-343) from the
//                    planes that are still in HBM — one clustering per frame, no 29.5 MB PointCloud2 hand-off between two processes
//                    (detect_moving_object.launch:19-33 wires constructor -> topic -> clusterer; INTEGRATION.md section 3 has the two
//                    launch-file lines that drop the separate clusterer).  The clusterer's four parameters are read from
//                    `~clusterer/{cluster_size, depth_diff, dynamic_speed, neighbor_distance}` (Clusterer.cfg's names, defaults and ranges) and served by a
//                    second dynamic_reconfigure server in that namespace from this package's own cfg/CollapsedClusterer.cfg — the
//                    reference's clusterer package build-depends on this one, so its generated header cannot be used here.  With the parameter false the node is the reference's
//                    constructor alone: no clustering runs here.
//   ~scene_flow      the 32-byte cloud is packed and copied to the host only while somebody subscribes (:141-142 gates exactly so)
// Not buildable in the image this was written in (no ROS): tests/test_ros_adapter_syntax.py compiles it against declaration-only
// stand-ins of the ROS headers; behaviour lives in the host mirror (moving_object_detector_amd/host/scene_flow_constructor.hpp) and the C ABI, which are tested.
#include <dynamic_reconfigure/server.h>
#include <geometry_msgs/Transform.h>
#include <image_transport/image_transport.h>
#include <image_transport/subscriber_filter.h>
#include <message_filters/subscriber.h>
#include <message_filters/time_synchronizer.h>
#include <moving_object_msgs/MovingObjectArray.h>
#include <ros/ros.h>
#include <scene_flow_constructor/CollapsedClustererConfig.h>   // this package's own cfg/CollapsedClusterer.cfg (no dependency on scene_flow_clusterer)
#include <scene_flow_constructor/SceneFlowConstructorConfig.h>
#include <sensor_msgs/CameraInfo.h>
#include <sensor_msgs/Image.h>
#include <sensor_msgs/PointCloud2.h>
#include <geometry_msgs/TransformStamped.h>
#include <tf2_ros/buffer.h>
#include <tf2_ros/transform_broadcaster.h>
#include <tf2_ros/transform_listener.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define MOD_HOST_ROS_CONFIG   // SceneFlowConstructorConfig is the generated one
#include "scene_flow_constructor.hpp"   // moving_object_detector_amd/host/ (an include directory of this package's CMakeLists.txt)

namespace scene_flow_constructor {

class SceneFlowConstructorNode {
 public:
  SceneFlowConstructorNode() : node_handle_(), private_node_handle_("~") {
    ModConfig cfg{};
    cfg.device = private_node_handle_.param("device", 0);
    cfg.max_width = private_node_handle_.param("max_width", 1920);
    cfg.max_height = private_node_handle_.param("max_height", 1080);
    cfg.max_frames = 1;
    if (mod_create(&cfg, &ctx_) != MOD_OK) { ROS_FATAL("mod_create failed: no MI355X visible or libmod_sf.so missing"); ros::shutdown(); return; }
    impl_.reset(new SceneFlowConstructor(ctx_));
    ModSgmParams sgm{};
    sgm.disparities = private_node_handle_.param("disparities", 128); sgm.p1 = private_node_handle_.param("p1", 6);
    sgm.p2 = private_node_handle_.param("p2", 96); sgm.paths = private_node_handle_.param("paths", 8); sgm.lr_check = 1; sgm.median = 1;
    impl_->setDisparityParams(sgm);
    impl_->setDisparitySubpixel(private_node_handle_.param("disparity_subpixel", false));   // sixteenths of a pixel; the fields of ~depth's source stay
    impl_->setDisparityFilters(private_node_handle_.param("uniqueness_ratio", 0), private_node_handle_.param("speckle_size", 0),
                               private_node_handle_.param("speckle_range", 0));   // stereo_image_proc's names; 0 = off
    impl_->setFlowPropagation(private_node_handle_.param("flow_seeds", 1));   // 1 = off; 5 = the parent's four neighbours seed the search too
    max_disparity_ = (float)(sgm.disparities - 1);

    // every estimator on the GPU (default), or the two CALL-OUTs below; optional centred crop of the incoming images
    gpu_estimators_ = private_node_handle_.param("gpu_estimators", true);
    crop_width_ = private_node_handle_.param("crop_width", 0);
    crop_height_ = private_node_handle_.param("crop_height", 0);
    ros::NodeHandle visual_odometry_nh(private_node_handle_, "visual_odometry");   // the reference's frame parameters (:28-30)
    base_link_frame_id_ = visual_odometry_nh.param("base_link_frame_id", std::string("base_link"));
    odom_frame_id_ = visual_odometry_nh.param("odom_frame_id", std::string("odom"));
    tf_listener_.reset(new tf2_ros::TransformListener(tf_buffer_));

    image_transport_.reset(new image_transport::ImageTransport(private_node_handle_));

    // dynamic reconfigure (scene_flow_constructor.cpp:40-42, :401-407)
    reconfigure_server_.reset(new dynamic_reconfigure::Server<SceneFlowConstructorConfig>(private_node_handle_));
    reconfigure_server_->setCallback([this](SceneFlowConstructorConfig &config, uint32_t) {
      ROS_INFO("Reconfigure Request: dynamic_flow_diff = %d, max_color_velocity = %f", config.dynamic_flow_diff, config.max_color_velocity);
      impl_->reconfigureCB(config);
    });

    // publishers (:45-48)
    depth_pub_ = private_node_handle_.advertise<sensor_msgs::Image>("depth", 1);
    optflow_pub_ = private_node_handle_.advertise<sensor_msgs::Image>("optical_flow", 1);
    pc_with_velocity_pub_ = private_node_handle_.advertise<sensor_msgs::PointCloud2>("scene_flow", 1);
    static_flow_pub_ = private_node_handle_.advertise<sensor_msgs::Image>("synthetic_optical_flow", 1);

    // collapsed mode: this process clusters too and publishes the moving objects (see the header comment)
    publish_moving_objects_ = private_node_handle_.param("publish_moving_objects", true);
    if (publish_moving_objects_) {
      clusterer_node_handle_ = ros::NodeHandle(private_node_handle_, "clusterer");
      clusterer_reconfigure_server_.reset(new dynamic_reconfigure::Server<CollapsedClustererConfig>(clusterer_node_handle_));
      clusterer_reconfigure_server_->setCallback([this](CollapsedClustererConfig &config, uint32_t) {
        impl_->reconfigureClusterer(config.cluster_size, config.depth_diff, config.dynamic_speed, config.neighbor_distance);
      });
      moving_objects_pub_ = private_node_handle_.advertise<moving_object_msgs::MovingObjectArray>("moving_objects", 1);
    }

    // subscribers + exact-time synchroniser, queue 1 (:51-62)
    const std::string left_image_topic = node_handle_.resolveName("left_image"), right_image_topic = node_handle_.resolveName("right_image");
    left_image_sub_.subscribe(*image_transport_, left_image_topic, 1);
    right_image_sub_.subscribe(*image_transport_, right_image_topic, 1);
    left_caminfo_sub_.subscribe(node_handle_, image_transport::getCameraInfoTopic(left_image_topic), 1);
    right_caminfo_sub_.subscribe(node_handle_, image_transport::getCameraInfoTopic(right_image_topic), 1);
    stereo_synchronizer_.reset(new StereoSynchronizer(left_image_sub_, right_image_sub_, left_caminfo_sub_, right_caminfo_sub_, 1));
    stereo_synchronizer_->registerCallback(&SceneFlowConstructorNode::stereoCallback, this);
  }
  ~SceneFlowConstructorNode() { impl_.reset(); if (ctx_) mod_destroy(ctx_); }

 private:
  using StereoSynchronizer = message_filters::TimeSynchronizer<sensor_msgs::Image, sensor_msgs::Image, sensor_msgs::CameraInfo, sensor_msgs::CameraInfo>;

  // ---- CALL-OUTS: the two estimators this package does not contain ------------------------------------------------------------
  // Optical flow previous -> now of the left image as 32FC2 (x then y, indexed at the NOW pixel), or null.  The reference calls
  // pwc_net_.estimateOpticalFlow(previous_left_image_, left_image, left_flow_) (:281-291).
  sensor_msgs::ImageConstPtr estimateOpticalFlow(const sensor_msgs::ImageConstPtr & /*previous_left*/, const sensor_msgs::ImageConstPtr & /*left*/) {
    return sensor_msgs::ImageConstPtr();
  }
  // Camera motion previous -> now in the left optical frame, or null when odometry failed (:251-255).  The reference feeds libviso2
  // and converts its 4 x 4 through tf2 (:214-249); mod_host::transform_from_motion() in the host mirror's messages.hpp restates that conversion.
  std::shared_ptr<geometry_msgs::Transform> estimateCameraMotion(const sensor_msgs::ImageConstPtr & /*left*/, const sensor_msgs::ImageConstPtr & /*right*/,
                                                                   const sensor_msgs::CameraInfoConstPtr & /*left_info*/, const sensor_msgs::CameraInfoConstPtr & /*right_info*/) {
    return std::shared_ptr<geometry_msgs::Transform>();
  }

  static mod_host::Header header_of(const std_msgs::Header &h) {
    mod_host::Header o;
    o.seq = h.seq; o.stamp = mod_host::Time(h.stamp.sec, h.stamp.nsec); o.frame_id = h.frame_id;
    return o;
  }
  static mod_host::Transform transform_of(const geometry_msgs::Transform &m) {
    mod_host::Transform t;
    t.translation[0] = m.translation.x; t.translation[1] = m.translation.y; t.translation[2] = m.translation.z;
    t.rotation[0] = m.rotation.x; t.rotation[1] = m.rotation.y; t.rotation[2] = m.rotation.z; t.rotation[3] = m.rotation.w;
    return t;
  }
  static geometry_msgs::Transform message_of(const mod_host::Transform &t) {
    geometry_msgs::Transform m;
    m.translation.x = t.translation[0]; m.translation.y = t.translation[1]; m.translation.z = t.translation[2];
    m.rotation.x = t.rotation[0]; m.rotation.y = t.rotation[1]; m.rotation.z = t.rotation[2]; m.rotation.w = t.rotation[3];
    return m;
  }
  // the first-frame block (:368-375): camera model from the left CameraInfo, of the centred crop window when `crop` is set
  // (image_crop.cpp:31-39); disparity fields as the estimator reports them
  void setCamera(const sensor_msgs::CameraInfo &left_camera_info, const sensor_msgs::CameraInfo &right_camera_info, bool crop) {
    mod_host::CameraInfo info;
    info.width = left_camera_info.width; info.height = left_camera_info.height;
    for (int i = 0; i < 12; i++) info.P[i] = left_camera_info.P[i];
    if (crop) info = mod_host::crop_camera_info(info, crop_width_, crop_height_);
    mod_host::DisparityImage d;
    d.f = (float)left_camera_info.P[0];
    d.T = (float)(-right_camera_info.P[3] / right_camera_info.P[0]);
    d.min_disparity = 0.0f; d.max_disparity = max_disparity_;
    impl_->setCameraInfo(info, d);
    camera_set_ = true;
  }

  // stereoCallback (:365-399)
  void stereoCallback(const sensor_msgs::ImageConstPtr &left_image, const sensor_msgs::ImageConstPtr &right_image,
                      const sensor_msgs::CameraInfoConstPtr &left_camera_info, const sensor_msgs::CameraInfoConstPtr &right_camera_info) {
    if (gpu_estimators_) { gpuCallback(left_image, right_image, left_camera_info, right_camera_info); return; }
    const ros::WallTime start_process = ros::WallTime::now();
    if (!camera_set_) setCamera(*left_camera_info, *right_camera_info, false);   // first frame (:368-375); the crop is the GPU path's
    // the estimators of THIS frame (the reference runs them on three threads, :378-388); the GPU is meanwhile busy with the
    // previous frame's scene flow
    sensor_msgs::ImageConstPtr left_flow = previous_left_image_ ? estimateOpticalFlow(previous_left_image_, left_image) : sensor_msgs::ImageConstPtr();
    std::shared_ptr<geometry_msgs::Transform> transform_prev2now = estimateCameraMotion(left_image, right_image, left_camera_info, right_camera_info);

    // the frame before has had a whole callback period: fetch it and publish (construct_thread_.join(), :389-390)
    publishPending();

    mod_host::Image l, r;
    l.header = header_of(left_image->header); l.width = left_image->width; l.height = left_image->height; l.data = left_image->data.data();
    r.header = header_of(right_image->header); r.width = right_image->width; r.height = right_image->height; r.data = right_image->data.data();
    mod_host::FlowImage f;
    if (left_flow) { f.header = header_of(left_flow->header); f.width = left_flow->width; f.height = left_flow->height;
                     f.data = reinterpret_cast<const float *>(left_flow->data.data()); }
    mod_host::Transform t;
    if (transform_prev2now) t = transform_of(*transform_prev2now);
    if (left_flow && optflow_pub_.getNumSubscribers() > 0) optflow_pub_.publish(left_flow);                 // (:99-100)
    // ~depth and ~synthetic_optical_flow are debugging views the reference renders only for subscribers (:114,141); they need the
    // disparity on the host, which the streaming path avoids: when somebody listens, this frame's disparity is fetched as well
    const bool want_views = depth_pub_.getNumSubscribers() > 0 || static_flow_pub_.getNumSubscribers() > 0;
    // outputs asked for THIS frame, gated like the reference's publishes: the cloud only while ~scene_flow has subscribers
    // (:141-142), the objects while the collapsed mode is on and ~moving_objects has subscribers (clusterer_nodelet.cpp:237-238);
    // with neither, the frame still goes through the scene-flow stage so that its disparity is the next frame's previous one
    pending_cloud_.reset(pc_with_velocity_pub_.getNumSubscribers() > 0 ? new mod_host::PointCloud2() : nullptr);
    pending_objects_.reset(publish_moving_objects_ && moving_objects_pub_.getNumSubscribers() > 0 ? new mod_host::MovingObjectArray() : nullptr);
    pending_ticket_ = impl_->submitStereo(&l, &r, left_flow ? &f : nullptr, transform_prev2now ? &t : nullptr, pending_cloud_.get(), pending_objects_.get());
    pending_header_ = left_flow ? left_flow->header : left_image->header;
    pending_keep_ = {left_image, right_image, left_flow};           // the buffers stay alive until the frame is collected
    if (want_views) publishViews(l, r, *left_camera_info, *right_camera_info, left_image->header, transform_prev2now ? &t : nullptr);

    ROS_INFO("process time: %f", (ros::WallTime::now() - start_process).toSec());
    previous_left_image_ = left_image;
  }

  static mod_host::Image image_of(const sensor_msgs::Image &m) {
    mod_host::Image o;
    o.header = header_of(m.header); o.width = m.width; o.height = m.height; o.data = m.data.data();
    o.encoding = m.encoding; o.step = (int)m.step;
    return o;
  }

  // stereoCallback with every estimator on the GPU: the images go in as they arrive (bgr8 / rgb8 / bgra8 / rgba8 / mono8 / yuv422 /
  // yuv422_yuy2 / the 8-bit Bayer mosaics, padded rows, the centred crop window), disparity, flow, camera motion, scene flow and clusters run there, the frame
  // before is collected, its objects published and the pose broadcast
  void gpuCallback(const sensor_msgs::ImageConstPtr &left_image, const sensor_msgs::ImageConstPtr &right_image,
                   const sensor_msgs::CameraInfoConstPtr &left_camera_info, const sensor_msgs::CameraInfoConstPtr &right_camera_info) {
    const ros::WallTime start_process = ros::WallTime::now();
    const bool crop = crop_width_ > 0 && crop_height_ > 0;
    if (!camera_set_) {               // first frame (:368-375); with the crop, the camera of the window (image_crop.cpp:31-39)
      setCamera(*left_camera_info, *right_camera_info, crop);
      camera_frame_id_ = left_image->header.frame_id;   // (:372)
    }
    publishPendingOdometry();
    int x0 = 0, y0 = 0;
    if (crop) mod_host::centred_origin((int)left_image->width, (int)left_image->height, crop_width_, crop_height_, &x0, &y0);
    mod_host::Image l = image_of(*left_image), r = image_of(*right_image);
    const bool usable = mod_host::image_encoding(left_image->encoding) >= 0 || mod_host::bayer_encoding(left_image->encoding) >= 0;
    if (!usable)                      // dropped like a failed estimateDisparity (:272-276): the next frame has no previous one
      ROS_ERROR("image encoding '%s' is not one of mono8, bgr8, rgb8, bgra8, rgba8, yuv422, yuv422_yuy2, bayer_{rggb,bggr,gbrg,grbg}8: frame dropped",
                left_image->encoding.c_str());
    pending_objects_.reset(publish_moving_objects_ && moving_objects_pub_.getNumSubscribers() > 0 ? new mod_host::MovingObjectArray() : nullptr);
    const bool want_flow = optflow_pub_.getNumSubscribers() > 0, want_depth = depth_pub_.getNumSubscribers() > 0;
    pending_flow_.clear(); pending_disparity_.clear();
    pending_cloud_.reset(pc_with_velocity_pub_.getNumSubscribers() > 0 ? new mod_host::PointCloud2() : nullptr);   // (:141-142)
    pending_ticket_ = impl_->submitOdometry(usable ? &l : nullptr, usable ? &r : nullptr, pending_objects_.get(), want_flow ? &pending_flow_ : nullptr,
                                            x0, y0, want_depth ? &pending_disparity_ : nullptr, pending_cloud_.get());
    pending_header_ = left_image->header;
    pending_keep_ = {left_image, right_image};        // the buffers stay alive until the frame is collected
    ROS_INFO("process time: %f", (ros::WallTime::now() - start_process).toSec());
  }

  // the frame before: objects, ~optical_flow, ~depth, and integrateAndBroadcastTF (:320-348) when its estimate succeeded
  void publishPendingOdometry() {
    if (pending_ticket_ < 0) return;
    const bool moved = impl_->collectOdometry(pending_ticket_);
    pending_ticket_ = -1;
    const size_t n = (size_t)impl_->imageWidth() * impl_->imageHeight();
    if (moved) {
      std::string error_msg;
      mod_host::Transform base_to_camera;            // identity unless TF knows better
      if (tf_buffer_.canTransform(base_link_frame_id_, camera_frame_id_, pending_header_.stamp, &error_msg)) {
        base_to_camera = transform_of(tf_buffer_.lookupTransform(base_link_frame_id_, camera_frame_id_, pending_header_.stamp).transform);
      } else {
        ROS_ERROR("The tf from '%s' to '%s' does not seem to be available, will assume it as identity! (%s)", base_link_frame_id_.c_str(),
                  camera_frame_id_.c_str(), error_msg.c_str());
      }
      impl_->setBaseToCamera(base_to_camera);
      geometry_msgs::TransformStamped msg;
      msg.header.stamp = pending_header_.stamp; msg.header.frame_id = odom_frame_id_;
      msg.child_frame_id = base_link_frame_id_;
      msg.transform = message_of(impl_->odomToBase().toTransform());
      tf_broadcaster_.sendTransform(msg);
    }
    if (!pending_flow_.empty() && optflow_pub_.getNumSubscribers() > 0) {      // (:99-100)
      sensor_msgs::Image m;
      m.header = pending_header_; m.width = impl_->imageWidth(); m.height = impl_->imageHeight(); m.encoding = "32FC2";
      m.step = 8 * m.width; m.data.resize(8 * n);
      std::memcpy(m.data.data(), pending_flow_.data(), 8 * n);
      optflow_pub_.publish(m);
    }
    if (!pending_disparity_.empty() && depth_pub_.getNumSubscribers() > 0) {   // ~depth (toDepthImage, :114-121)
      sensor_msgs::Image m;
      m.header = pending_header_; m.width = impl_->imageWidth(); m.height = impl_->imageHeight(); m.encoding = "32FC1";
      m.step = 4 * m.width; m.data.resize(4 * n);
      if (mod_depth_image_host(ctx_, pending_disparity_.data(), reinterpret_cast<float *>(m.data.data())) == MOD_OK) depth_pub_.publish(m);
    }
    if (moved && pending_objects_) publishObjects();
    if (moved && pending_cloud_) publishCloud();
    pending_objects_.reset();
    pending_cloud_.reset();
    pending_keep_.clear();
  }

  void publishObjects() {                                             // publishMovingObjects (clusterer_nodelet.cpp:324-343)
    moving_object_msgs::MovingObjectArray m;
    m.header = pending_header_;
    for (const auto &o : pending_objects_->moving_object_array) {
      moving_object_msgs::MovingObject mo;
      mo.id = o.id;
      mo.center.position.x = o.center.position[0]; mo.center.position.y = o.center.position[1]; mo.center.position.z = o.center.position[2];
      mo.center.orientation.x = 0; mo.center.orientation.y = 0; mo.center.orientation.z = 0; mo.center.orientation.w = 1;
      mo.velocity.x = o.velocity[0]; mo.velocity.y = o.velocity[1]; mo.velocity.z = o.velocity[2];
      mo.bounding_box.x = o.bounding_box[0]; mo.bounding_box.y = o.bounding_box[1]; mo.bounding_box.z = o.bounding_box[2];
      m.moving_object_array.push_back(mo);
    }
    moving_objects_pub_.publish(m);
  }

  void publishPending() {
    if (pending_ticket_ < 0) return;
    impl_->collect(pending_ticket_);
    pending_ticket_ = -1;
    if (pending_objects_) {
      publishObjects();
      pending_objects_.reset();
    }
    if (pending_cloud_) publishCloud();   // asked for because somebody subscribed (:144)
    pending_keep_.clear();
  }

  void publishCloud() {                   // publishPointcloud (:351-362)
    sensor_msgs::PointCloud2 msg;         // fields x, y, z, vx, vy, vz float32 at 0, 4, 8, 16, 20, 24 (pcl_point_xyz_velocity.h:27-34)
    msg.header = pending_header_; msg.width = pending_cloud_->width; msg.height = pending_cloud_->height;
    msg.point_step = 32; msg.row_step = pending_cloud_->row_step; msg.is_dense = true; msg.is_bigendian = false;
    msg.data = std::move(pending_cloud_->data);
    const char *names[6] = {"x", "y", "z", "vx", "vy", "vz"};
    const uint32_t offs[6] = {0, 4, 8, 16, 20, 24};
    for (int i = 0; i < 6; i++) { sensor_msgs::PointField pf; pf.name = names[i]; pf.offset = offs[i]; pf.datatype = sensor_msgs::PointField::FLOAT32; pf.count = 1; msg.fields.push_back(pf); }
    pc_with_velocity_pub_.publish(msg);
  }

  // ~depth (toDepthImage, :114-121) and ~synthetic_optical_flow (:136-145): synchronous side path, only while somebody subscribes
  void publishViews(const mod_host::Image &l, const mod_host::Image &r, const sensor_msgs::CameraInfo &li, const sensor_msgs::CameraInfo &ri,
                    const std_msgs::Header &header, const mod_host::Transform *t) {
    mod_host::CameraInfo a, b;
    a.width = li.width; a.height = li.height; b.width = ri.width; b.height = ri.height;
    for (int i = 0; i < 12; i++) { a.P[i] = li.P[i]; b.P[i] = ri.P[i]; }
    mod_host::DisparityImage d;
    std::vector<float> pixels;
    if (!impl_->estimateDisparity(&l, &r, a, b, &d, &pixels)) return;
    const size_t n = (size_t)l.width * l.height;
    if (depth_pub_.getNumSubscribers() > 0) {
      sensor_msgs::Image m;
      m.header = header; m.width = l.width; m.height = l.height; m.encoding = "32FC1"; m.step = 4 * l.width; m.data.resize(4 * n);
      if (mod_depth_image_host(ctx_, pixels.data(), reinterpret_cast<float *>(m.data.data())) == MOD_OK) depth_pub_.publish(m);
    }
    if (static_flow_pub_.getNumSubscribers() > 0 && t && !view_prev_disparity_.empty()) {
      const ModTransform tf = mod_host::to_mod(*t);
      sensor_msgs::Image m;
      m.header = header; m.width = l.width; m.height = l.height; m.encoding = "32FC2"; m.step = 8 * l.width; m.data.resize(8 * n);
      if (mod_static_flow_host(ctx_, view_prev_disparity_.data(), &tf, reinterpret_cast<float *>(m.data.data())) == MOD_OK) static_flow_pub_.publish(m);
    }
    view_prev_disparity_.swap(pixels);
  }

  ros::NodeHandle node_handle_, private_node_handle_;
  ModContext *ctx_ = nullptr;
  std::unique_ptr<SceneFlowConstructor> impl_;
  std::unique_ptr<image_transport::ImageTransport> image_transport_;
  std::unique_ptr<dynamic_reconfigure::Server<SceneFlowConstructorConfig>> reconfigure_server_;
  image_transport::SubscriberFilter left_image_sub_, right_image_sub_;
  message_filters::Subscriber<sensor_msgs::CameraInfo> left_caminfo_sub_, right_caminfo_sub_;
  std::unique_ptr<StereoSynchronizer> stereo_synchronizer_;
  ros::Publisher depth_pub_, optflow_pub_, pc_with_velocity_pub_, static_flow_pub_, moving_objects_pub_;
  bool publish_moving_objects_ = true;
  ros::NodeHandle clusterer_node_handle_;
  std::unique_ptr<dynamic_reconfigure::Server<CollapsedClustererConfig>> clusterer_reconfigure_server_;
  std::unique_ptr<mod_host::MovingObjectArray> pending_objects_;
  bool camera_set_ = false;
  float max_disparity_ = 127.0f;
  sensor_msgs::ImageConstPtr previous_left_image_;
  int pending_ticket_ = -1;
  std::unique_ptr<mod_host::PointCloud2> pending_cloud_;
  std_msgs::Header pending_header_;
  std::vector<sensor_msgs::ImageConstPtr> pending_keep_;
  std::vector<float> view_prev_disparity_;
  // ~gpu_estimators
  bool gpu_estimators_ = true;
  int crop_width_ = 0, crop_height_ = 0;
  std::vector<float> pending_flow_, pending_disparity_;
  std::string camera_frame_id_, base_link_frame_id_, odom_frame_id_;
  tf2_ros::Buffer tf_buffer_;
  std::unique_ptr<tf2_ros::TransformListener> tf_listener_;
  tf2_ros::TransformBroadcaster tf_broadcaster_;
};

}  // namespace scene_flow_constructor

int main(int argc, char **argv) {
  ros::init(argc, argv, "scene_flow_constructor");
  scene_flow_constructor::SceneFlowConstructorNode node;
  ros::spin();
  return 0;
}
