// scene_flow_constructor.hpp — host-side mirror of scene_flow_constructor::SceneFlowConstructor
// (scene_flow_constructor/include/scene_flow_constructor.h:33-275) for the part of the class that is on the hot path:
// construct(), the previous-frame state of stereoCallback() and reconfigureCB().  Same member names, same argument
// meaning, same "publish nothing when an input is missing" behaviour — the per-pixel work goes through the C ABI
// (include/mod_sf.h) to the HIP kernels.  estimateDisparity() is here as well (the on-GPU SGM of SURVEY.md section 8(f) row 3), and
// submitOdometry() runs every estimator on the GPU (colour images in, camera motion and moving objects out) with the pose
// integration of integrateAndBroadcastTF; the ROS wiring itself is in ros_adapter/.
#pragma once
#include <functional>
#include <stdexcept>

#include "messages.hpp"

namespace scene_flow_constructor {

#ifndef MOD_HOST_ROS_CONFIG   // a ROS build includes the dynamic_reconfigure-generated scene_flow_constructor/SceneFlowConstructorConfig.h first
struct SceneFlowConstructorConfig {   // cfg/SceneFlowConstructor.cfg:8-9
  int dynamic_flow_diff = 5;
  double max_color_velocity = 1.0;    // unused by live code in the reference as well
};
#endif

class SceneFlowConstructor {
 public:
  using CloudCallback = std::function<void(const mod_host::PointCloud2 &)>;

  // One context per constructor, like one node per camera.  `ctx` may be shared with a ClustererNodelet so that the
  // cloud never leaves the GPU between the two stages.
  explicit SceneFlowConstructor(ModContext *ctx) : ctx_(ctx) {}

  // stereoCallback()'s first-frame block (scene_flow_constructor.cpp:368-375): camera model from the left CameraInfo.
  void setCameraInfo(const mod_host::CameraInfo &left, const mod_host::DisparityImage &disparity) {
    ModCamera cam{};
    cam.width = left.width; cam.height = left.height;
    cam.fx = left.P[0]; cam.fy = left.P[5]; cam.cx = left.P[2]; cam.cy = left.P[6]; cam.Tx = left.P[3]; cam.Ty = left.P[7];
    cam.disp_f = disparity.f; cam.disp_T = disparity.T;
    cam.min_disparity = disparity.min_disparity; cam.max_disparity = disparity.max_disparity;
    check(mod_set_camera(ctx_, &cam));
    image_width_ = left.width; image_height_ = left.height;
  }

  // reconfigureCB (scene_flow_constructor.cpp:401-407).  The clusterer's parameters live in the same ModParams block;
  // they are preserved.
  void reconfigureCB(const SceneFlowConstructorConfig &config) {
    ModParams p = currentParams();
    p.dynamic_flow_diff = config.dynamic_flow_diff;
    check(mod_set_params(ctx_, &p));
  }

  // The clusterer's reconfigureCB (clusterer_nodelet.cpp:345-352) for a process that runs both stages on one context (the collapsed
  // node: `~publish_moving_objects`): the four Clusterer.cfg values go into the shared ModParams block, dynamic_flow_diff is preserved.
  void reconfigureClusterer(int cluster_size, double depth_diff, double dynamic_speed, int neighbor_distance) {
    ModParams p = currentParams();
    p.cluster_size = cluster_size; p.depth_diff = depth_diff; p.dynamic_speed = dynamic_speed; p.neighbor_distance = neighbor_distance;
    check(mod_set_params(ctx_, &p));
  }

  // estimateDisparity() (scene_flow_constructor.cpp:258-279): sgm_gpu_->computeDisparity(left, right, infos, disparity).  Fills
  // `disparity` as that call does for its caller — the stereo_msgs/DisparityImage contract DisparityImageProcessor reads
  // (disparity_image_processor.cpp:25-27,41-45): 32FC1 pixels with -1 = min_disparity - 1 where no match was found, f from the
  // left projection matrix, T = the baseline -P_right[3] / P_right[0], min_disparity 0, max_disparity D - 1 — into `pixels`, which
  // the message then points at.  Returns false (and leaves `disparity` alone) when an image is missing or of the wrong size: the
  // reference then resets disparity_now_, i.e. the caller passes a null disparity on.
  void setDisparityParams(const ModSgmParams &p) { sgm_ = p; }
  // sub-pixel disparity (mod_set_disparity_subpixel: sixteenths of a pixel); off unless asked for.  Frames already submitted keep
  // the setting of their submit.
  void setDisparitySubpixel(bool on) { check(mod_set_disparity_subpixel(ctx_, on ? MOD_SGM_FRACTION_BITS : 0)); }
  // minimum disparity of the estimator (mod_set_disparity_offset; stereo_image_proc's min_disparity): the search window becomes
  // [d0, d0 + disparities), 0 <= d0 <= 128; 0 = off, the default.  estimateDisparity() fills the DisparityImage's min_disparity /
  // max_disparity accordingly; invalid pixels stay -1.  Throws where the library refuses the value; frames already submitted keep
  // the offset of their submit.
  void setDisparityOffset(int d0) { check(mod_set_disparity_offset(ctx_, d0)); disparity_offset_ = d0; }
  // texture threshold of the disparity and flow estimators (mod_set_texture_filter; stereo_image_proc's texture_threshold in idea):
  // pixels whose window x window sum of capped horizontal differences is below `threshold` become invalid in the estimators named by
  // `apply` (MOD_TEXTURE_DISPARITY | MOD_TEXTURE_FLOW); threshold 0 = off, the default.  Throws where the library refuses a value;
  // frames already submitted keep the setting of their submit.
  void setTextureFilter(int threshold, int window = 9, int cap = 31, int apply = MOD_TEXTURE_DISPARITY | MOD_TEXTURE_FLOW) {
    const ModTextureFilter f{threshold, window, cap, apply};
    check(mod_set_texture_filter(ctx_, &f));
  }
  // min-eigenvalue (aperture) threshold of the flow estimator (mod_set_flow_corner_filter; calcOpticalFlowPyrLK's minEigThreshold in
  // idea): flow pixels whose window x window gradient structure tensor of the now image has a smaller eigenvalue below `threshold`
  // become (NaN, NaN); threshold 0 = off, the default.  Throws where the library refuses a value; frames already submitted keep the
  // setting of their submit.
  void setFlowCornerFilter(int threshold, int window = 9, int cap = 31) {
    const ModCornerFilter f{threshold, window, cap, 0};
    check(mod_set_flow_corner_filter(ctx_, &f));
  }
  // NaN-aware median filter of the flow estimator (mod_set_flow_median; cv::medianBlur on the two channels in idea): behind every other
  // step each valid flow pixel becomes the per-component lower median of the valid pixels of its window x window square (window 3 or
  // 5), or (NaN, NaN) where fewer than min_valid of them are valid; invalid pixels stay.  window 0 = off, the default.  Throws where the
  // library refuses a value; frames already submitted keep the setting of their submit.
  void setFlowMedian(int window, int min_valid = 0) {
    const ModFlowMedian f{window, min_valid, {0, 0}};
    check(mod_set_flow_median(ctx_, &f));
  }
  // disparity-gated hole fill of the flow (mod_set_flow_fill): the last flow stage of the submits that estimate the flow, behind the
  // median and the ego-motion estimate, in front of the scene flow.  An invalid flow pixel with a valid disparity d becomes the
  // per-component lower median of the valid flow pixels of its window x window square (window 3, 5 or 7) whose disparity lies within
  // tol_abs + tol_rel * d of d, where at least min_valid of them do; every other pixel stays.  window 0 = off, the default.  Throws
  // where the library refuses a value; frames already submitted keep the setting of their submit.  No node parameter sets it.
  void setFlowFill(int window, int min_valid, float tol_abs, float tol_rel) {
    const ModFlowFill f{window, min_valid, tol_abs, tol_rel, {0, 0}};
    check(mod_set_flow_fill(ctx_, &f));
  }
  // rejection filters of the disparity (mod_set_disparity_filters; stereo_image_proc's names): uniqueness ratio in percent, regions of at
  // most speckle_size pixels whose neighbours differ by at most speckle_range disparities are invalidated; all 0 = off, the default.
  // Frames already submitted keep the settings of their submit.
  void setDisparityFilters(int uniqueness_ratio, int speckle_size, int speckle_range) {
    const ModDisparityFilters f{uniqueness_ratio, speckle_size, speckle_range, 0};
    check(mod_set_disparity_filters(ctx_, &f));
  }
  // edge-preserving smoother of the disparity (mod_set_disparity_smooth): the estimator's stage behind the speckle stage and in front of
  // the hole fill.  A valid disparity d becomes the mean of the valid disparities of its window x window square (3, 5 or 7) within tol
  // px of d, where at least min_members (1..window^2) lie there; every other pixel stays.  window 0 = off, the default.  Throws where the
  // library refuses a value; frames already submitted keep the setting of their submit.  No node parameter sets it.
  void setDisparitySmooth(int window, float tol, int min_members) {
    const ModDisparitySmooth f{window, min_members, tol, 0};
    if (window == 0) check(mod_set_disparity_smooth(ctx_, nullptr));
    else check(mod_set_disparity_smooth(ctx_, &f));
  }
  // occlusion hole fill of the disparity (mod_set_disparity_fill): the estimator's last stage, behind the speckle stage.  An invalid
  // disparity walks the first `directions` (2, 4 or 8) path directions for up to `reach` (1..256) steps each to the first valid word and
  // becomes the lowest (MOD_DISPARITY_FILL_MIN), second lowest (_SECOND) or lower median (_MEDIAN) of the found words where at least
  // min_found directions found one; every other pixel stays.  reach 0 = off, the default.  Throws where the library refuses a value;
  // frames already submitted keep the setting of their submit.  No node parameter sets it.
  void setDisparityFill(int reach, int directions, int mode, int min_found) {
    const ModDisparityFill f{reach, directions, mode, min_found};
    check(mod_set_disparity_fill(ctx_, &f));
  }
  // neighbour-seed propagation of the optical flow (mod_set_flow_propagation): 1 = off, the default; 5 = every finer level also tries the
  // winners of the parent's four neighbours.  Frames already submitted keep the setting of their submit.
  void setFlowPropagation(int seeds) { check(mod_set_flow_propagation(ctx_, seeds)); }
  // side-by-side stereo messages (mod_set_side_by_side; what a stereo head used as a plain UVC camera delivers): while set,
  // submitStereo() and submitOdometry() take ONE message of twice the camera's width in left_image, its left half the left eye's
  // image, and right_image must be null or that message.  Off by default.  The layout is set with the next message: until then the
  // library refuses a layout that cannot hold two panes, so the setting is kept here and handed on with the layout.
  // While set, NO entry point takes two distinct images: estimateDisparity() returns false for them (it has no one-message form:
  // use submitStereo() or submitOdometry()), and the two submits treat them as missing images and return -1.  Switch it off before
  // handing two messages in again; frames already submitted keep the setting of their submit.
  void setSideBySide(bool on) { side_by_side_ = on; }
  // image binning (mod_set_image_binning; image_proc/crop_decimate's step on the GPU): while set, submitOdometry() and submitDepth()
  // take messages whose window at (x0, y0) is (bx W) x (by H) and reduce it to the camera's W x H; mode MOD_BIN_MEAN or
  // MOD_BIN_NEAREST; bx = by = 1: off, the default.  The CameraInfo handed to setCameraInfo() is the BINNED one (include/mod_sf.h
  // states the relation; sensor_msgs/CameraInfo's binning_x / binning_y describe the same thing).  estimateDisparity(),
  // estimateOpticalFlow() and submitStereo() compare the message's size with the camera's and so refuse full-resolution messages:
  // use the two submits above.  Throws where the library refuses the values; frames already submitted keep the setting of their submit.
  void setImageBinning(int bx, int by, int mode = MOD_BIN_MEAN) {
    const ModImageBinning b{bx, by, mode, 0};
    check(mod_set_image_binning(ctx_, &b));
  }
  bool estimateDisparity(const mod_host::Image *left_image, const mod_host::Image *right_image, const mod_host::CameraInfo &left_camera_info,
                         const mod_host::CameraInfo &right_camera_info, mod_host::DisparityImage *disparity, std::vector<float> *pixels) {
    if (!left_image || !right_image || !left_image->data || !right_image->data) return false;
    if (left_image->width != left_camera_info.width || left_image->height != left_camera_info.height ||
        right_image->width != left_image->width || right_image->height != left_image->height) return false;
    // the library copies the CONTEXT's width x height bytes from each image: an image of another size than the configured camera
    // would be over-read (setCameraInfo() ran on the first frame, scene_flow_constructor.cpp:368-375)
    if (image_width_ > 0 && (left_image->width != image_width_ || left_image->height != image_height_)) return false;
    if (!useLayout(*left_image, *right_image, 0, 0)) return false;   // the context reads the images as this message describes them
    pixels->resize((size_t)left_image->width * left_image->height);
    const int rc = mod_sgm_compute_host(ctx_, left_image->data, right_image->data, &sgm_, pixels->data());
    if (rc > 0) return false;
    check(rc);
    disparity->header = left_image->header;
    disparity->width = left_image->width; disparity->height = left_image->height;
    disparity->data = pixels->data();
    disparity->f = (float)left_camera_info.P[0];
    disparity->T = (float)(-right_camera_info.P[3] / right_camera_info.P[0]);
    disparity->min_disparity = (float)disparity_offset_;
    disparity->max_disparity = (float)(disparity_offset_ + sgm_.disparities - 1);
    return true;
  }

  // construct() (scene_flow_constructor.cpp:91-147).  Null pointers play the role of the reference's empty shared_ptrs.
  // Returns true when a cloud was produced ("published"); false when the reference would have published nothing.
  bool construct(const mod_host::DisparityImage *disparity_now, const mod_host::DisparityImage *disparity_previous,
                 const mod_host::FlowImage *left_flow, const mod_host::Transform *transform_prev2now,
                 mod_host::PointCloud2 *pc_with_velocity, std::vector<int32_t> *labels = nullptr,
                 mod_host::MovingObjectArray *moving_objects = nullptr, std::vector<float> *depth_image = nullptr) {
    // ~depth goes out whenever disparity_now exists, before the guards that end the frame (:110-123)
    if (depth_image) {
      depth_image->clear();
      if (disparity_now) {
        depth_image->resize((size_t)image_width_ * image_height_);
        const int drc = mod_depth_image_host(ctx_, disparity_now->data, depth_image->data());
        check(drc);
        if (drc > 0) depth_image->clear();   // a message without pixels: the reference publishes no depth image either
      }
    }
    const ModTransform tf = transform_prev2now ? mod_host::to_mod(*transform_prev2now) : ModTransform{};
    // time_between_frames = stamp_now - stamp_previous (scene_flow_constructor.cpp:162-164)
    const double dt = (disparity_now && disparity_previous) ? mod_host::duration_sec(disparity_now->header.stamp, disparity_previous->header.stamp) : 0.0;
    const size_t n = (size_t)image_width_ * image_height_;
    if (pc_with_velocity) pc_with_velocity->data.resize(n * 32);
    if (labels) labels->resize(n);
    std::vector<ModObject> objs(max_objects_);
    int32_t n_obj = 0;
    const int rc = mod_process_frame_host(ctx_, disparity_now ? disparity_now->data : nullptr,
                                          disparity_previous ? disparity_previous->data : nullptr,
                                          left_flow ? left_flow->data : nullptr, transform_prev2now ? &tf : nullptr, dt,
                                          pc_with_velocity ? pc_with_velocity->data.data() : nullptr,
                                          labels ? labels->data() : nullptr, objs.data(), (int32_t)objs.size(), &n_obj);
    if (rc > 0) return false;          // an input is missing: nothing is published (:104,110,122,127,133)
    check(rc);
    // publishPointcloud (:351-362): organized cloud, header of the flow image
    if (pc_with_velocity) mod_host::describe_cloud(*pc_with_velocity, left_flow->header, image_width_, image_height_);
    if (moving_objects) mod_host::fill_objects(*moving_objects, left_flow->header, objs.data(), n_obj, objs.size());
    return true;
  }

  // The part of stereoCallback() that carries state across frames (:389-398): the caller hands in this frame's estimator
  // outputs; the previous disparity is remembered here.  Frame 0 has no previous disparity / flow -> returns false.
  bool stereoCallback(const mod_host::DisparityImage *disparity_now, const mod_host::FlowImage *left_flow,
                      const mod_host::Transform *transform_prev2now, mod_host::PointCloud2 *pc_with_velocity,
                      mod_host::MovingObjectArray *moving_objects = nullptr) {
    const mod_host::DisparityImage *prev = have_previous_ ? &disparity_previous_ : nullptr;
    const bool ok = construct(disparity_now, prev, left_flow, transform_prev2now, pc_with_velocity, nullptr, moving_objects);
    if (disparity_now) {               // disparity_previous_ = disparity_now_ (:398); the pixels are copied: the message dies
      previous_pixels_.assign(disparity_now->data, disparity_now->data + (size_t)disparity_now->width * disparity_now->height);
      disparity_previous_ = *disparity_now;
      disparity_previous_.data = previous_pixels_.data();
      have_previous_ = true;
    } else {
      have_previous_ = false;          // estimateDisparity failed: disparity_now_.reset() (:272-276)
    }
    return ok;
  }

  // Pipelined stereoCallback(): the reference runs construct() of frame t on construct_thread_ while the estimators of
  // frame t+1 run (:389-392).  submit() enqueues the frame (copies and kernels proceed on the GPU's streams) and returns a
  // ticket, or -1 where nothing will be published; collect() joins it and fills the messages handed to submit().  The
  // previous disparity stays resident in HBM (disparity_previous_ = disparity_now_, :397-398) instead of being copied on
  // the host.  Up to MOD_PIPELINE_DEPTH frames may be in flight; tickets are collected in order.  The message buffers
  // (disparity, flow, cloud) should be page-locked (mod_host_malloc) for the copies to overlap.
  int submit(const mod_host::DisparityImage *disparity_now, const mod_host::FlowImage *left_flow,
             const mod_host::Transform *transform_prev2now, mod_host::PointCloud2 *pc_with_velocity,
             mod_host::MovingObjectArray *moving_objects = nullptr) {
    if (!disparity_now) {
      check(mod_forget_previous(ctx_));   // estimateDisparity failed: disparity_now_.reset() (:272-276)
      have_stamp_ = false; have_parked_ = false;
      return -1;
    }
    const size_t n = (size_t)image_width_ * image_height_;
    if (pc_with_velocity && pc_with_velocity->data.size() != n * 32) pc_with_velocity->data.resize(n * 32);
    const ModTransform tf = transform_prev2now ? mod_host::to_mod(*transform_prev2now) : ModTransform{};
    return submitFrame(&disparity_now->header.stamp, left_flow ? &left_flow->header : nullptr, pc_with_velocity, moving_objects,
                       [&](Pending &, double dt, void *cloud, ModObject *objects, int32_t max_objects, int32_t *ticket) {
      // previous disparity: resident in HBM from the last enqueued frame, or the host copy parked by a skipped frame
      const int rc = mod_submit_frame_host(ctx_, disparity_now->data, have_parked_ ? parked_.data() : nullptr, left_flow ? left_flow->data : nullptr,
                                           transform_prev2now ? &tf : nullptr, dt, cloud, nullptr, objects, max_objects, ticket);
      if (rc == MOD_OK) {
        have_parked_ = false;
      } else if (rc > 0) {
        // nothing was enqueued, so this disparity never reached HBM — yet it IS the next frame's previous one
        // (disparity_previous_ = disparity_now_ runs whatever construct() did, :398): park a host copy
        check(mod_forget_previous(ctx_));
        parked_.assign(disparity_now->data, disparity_now->data + n);
        have_parked_ = true;
      }
      return rc;
    });
  }
  // Pipelined stereoCallback() with the estimator on the GPU (BASELINE config 5): estimateDisparity() + construct() of one frame
  // in a single submission — images go in, the disparity plane is produced in HBM, serves as `now` here and as `previous` of the
  // next frame (disparity_previous_ = disparity_now_, :397-398) and never crosses the host link (estimateDisparity() + submit()
  // carry it to the host and back).  Returns a ticket for collect(), or -1 where nothing will be published; a missing or
  // mis-sized image plays the part of a failed estimateDisparity() (:272-276).
  int submitStereo(const mod_host::Image *left_image, const mod_host::Image *right_image, const mod_host::FlowImage *left_flow,
                   const mod_host::Transform *transform_prev2now, mod_host::PointCloud2 *pc_with_velocity,
                   mod_host::MovingObjectArray *moving_objects = nullptr) {
    if (side_by_side_ && !right_image) right_image = left_image;   // one message holds both eyes
    const int panes = side_by_side_ ? 2 : 1;
    const bool images = left_image && right_image && left_image->data && right_image->data && left_image->width == panes * image_width_ &&
                        left_image->height == image_height_ && right_image->width == panes * image_width_ &&
                        right_image->height == image_height_ && useLayout(*left_image, *right_image, 0, 0);
    const size_t n = (size_t)image_width_ * image_height_;
    if (images && pc_with_velocity && pc_with_velocity->data.size() != n * 32) pc_with_velocity->data.resize(n * 32);
    const ModTransform tf = transform_prev2now ? mod_host::to_mod(*transform_prev2now) : ModTransform{};
    return submitFrame(images ? &left_image->header.stamp : nullptr, left_flow ? &left_flow->header : nullptr, pc_with_velocity, moving_objects,
                       [&](Pending &, double dt, void *cloud, ModObject *objects, int32_t max_objects, int32_t *ticket) {
      have_parked_ = false;                         // the previous disparity lives in HBM (or is gone with the images)
      return mod_submit_stereo_host(ctx_, images ? left_image->data : nullptr, images ? right_image->data : nullptr, &sgm_,
                                    left_flow ? left_flow->data : nullptr, transform_prev2now ? &tf : nullptr, dt, cloud, nullptr, objects, max_objects,
                                    nullptr, ticket);
    });
  }
  // Pipelined stereoCallback() with every estimator on the GPU: images in (any encoding the library takes, rows as the message
  // pads them, the camera-sized window at (x0, y0)), moving objects and the estimated camera motion out.  The layout is taken from
  // the left message (left and right must agree in encoding, size and step, as the reference asserts, scene_flow_constructor.cpp:
  // 224-226).  dt is the stamp difference of consecutive left images.  flow_out (optional, W * H * 2 floats): ~optical_flow;
  // disparity_out (optional, W * H floats): the disparity image (32FC1, -1 where no match).  Both are valid after collectOdometry().
  // Returns a ticket for collectOdometry(), or -1 where nothing will be published (first frame, missing or unusable images).
  int submitOdometry(const mod_host::Image *left_image, const mod_host::Image *right_image, mod_host::MovingObjectArray *moving_objects,
                     std::vector<float> *flow_out = nullptr, int x0 = 0, int y0 = 0, std::vector<float> *disparity_out = nullptr,
                     mod_host::PointCloud2 *pc_with_velocity = nullptr) {
    if (side_by_side_ && !right_image) right_image = left_image;   // one message holds both eyes
    const bool images = left_image && right_image && left_image->data && right_image->data && useLayout(*left_image, *right_image, x0, y0);
    sizeOutputs(flow_out, disparity_out, pc_with_velocity);   // always, also for a frame that will be skipped
    return submitFrame(images ? &left_image->header.stamp : nullptr, left_image ? &left_image->header : nullptr, pc_with_velocity, moving_objects,
                       [&](Pending &p, double dt, void *cloud, ModObject *objects, int32_t max_objects, int32_t *ticket) {
      have_parked_ = false;
      return mod_submit_odometry_host(ctx_, images ? left_image->data : nullptr, images ? right_image->data : nullptr, &sgm_, &flow_, &ego_, dt, cloud,
                                      nullptr, objects, max_objects, disparity_out ? disparity_out->data() : nullptr,
                                      flow_out ? flow_out->data() : nullptr, &p.tf, &p.ego, ticket);
    });
  }
  // RGB-D cameras (mod_submit_depth_host): the layout of the depth messages — `depth` is a sensor_msgs/Image with encoding "16UC1"
  // (millimetres) or "32FC1" (metres), little-endian; unit 0 = the REP 118 default — with the camera-sized window at (x0, y0), and the
  // optional registration of a depth camera with intrinsics and a pose of its own (null = off; set it before a layout of another size
  // than the camera's, with x0 = y0 = 0).  false / an exception where the library refuses the values.
  bool setDepthLayout(const mod_host::Image &depth, int x0 = 0, int y0 = 0, float unit = 0.0f) {
    const int enc = depth.encoding == "16UC1" ? MOD_DEPTH_16UC1 : depth.encoding == "32FC1" ? MOD_DEPTH_32FC1 : -1;
    if (enc < 0) return false;
    const ModDepthLayout lay{enc, depth.width, depth.height, depth.step > 0 ? depth.step : depth.width * (enc == MOD_DEPTH_16UC1 ? 2 : 4), x0, y0, unit};
    return mod_set_depth_layout(ctx_, &lay) == MOD_OK;
  }
  void setDepthRegistration(const ModDepthRegistration *registration) { check(mod_set_depth_registration(ctx_, registration)); }
  // a depth camera whose stream is not rectified (an Azure Kinect's depth/image_raw): the D of its CameraInfo, plumb_bob or
  // rational_polynomial, k1 k2 p1 p2 k3 k4 k5 k6; null = off (the default).  Needs setDepthRegistration(); refused while a distortion is
  // set and tickets are outstanding, so set it before the first submitDepth()
  void setDepthDistortion(const ModDepthDistortion *distortion) { check(mod_set_depth_distortion(ctx_, distortion)); }
  // a depth camera of fewer pixels than the image camera (a registration is set): every depth sample fills the image pixels inside its
  // projected footprint instead of one, depth_image_proc/register's fill_upsampling_holes; off by default, read at each submitDepth()
  void setDepthSplat(bool on) { check(mod_set_depth_splat(ctx_, on ? 1 : 0)); }
  // the range and flying-pixel filter of the depth messages, on the depth camera's own lattice ahead of the conversion and the
  // registration (include/mod_sf.h: ModDepthFilter); null = off (the default), read at each submitDepth()
  void setDepthFilter(const ModDepthFilter *filter) { check(mod_set_depth_filter(ctx_, filter)); }
  // the edge-preserving smoother and hole fill of the depth messages, behind the depth filter and in front of the temporal filter
  // (include/mod_sf.h: ModDepthSpatial); null = off (the default), read at each submitDepth()
  void setDepthSpatial(const ModDepthSpatial *spatial) { check(mod_set_depth_spatial(ctx_, spatial)); }
  // the decimation of the depth messages by integer factors, behind the filters and in front of the conversion: a depth image aligned to
  // the full-resolution colour image meets the camera that setImageBinning's image has (include/mod_sf.h: ModDepthDecimation; the depth
  // layout's window is then (dx W) x (dy H)); null or dx = dy = 1: off (the default), read at each submitDepth(); not with a registration
  void setDepthDecimation(const ModDepthDecimation *decimation) { check(mod_set_depth_decimation(ctx_, decimation)); }
  // the temporal filter with hold of the depth messages, behind the depth filter (include/mod_sf.h: ModDepthTemporal); null = off (the
  // default), read at each submitDepth(); every call empties the filter's per-pixel state
  void setDepthTemporal(const ModDepthTemporal *filter) { check(mod_set_depth_temporal(ctx_, filter)); }
  // submitOdometry() for an RGB-D camera: one image (any encoding the library takes, the window at (x0, y0)) and one depth image of the
  // layout setDepthLayout() set, in the disparity estimator's place the conversion fT / depth on the GPU.  transform_prev2now null: the
  // camera motion is estimated on the GPU (collectOdometry() joins the ticket and integrates it); else the caller's (collect()).
  // dt is the stamp difference of consecutive images.  Returns a ticket, or -1 where nothing will be published (first frame, a
  // missing image, setSideBySide() on).
  int submitDepth(const mod_host::Image *image, const mod_host::Image *depth, mod_host::MovingObjectArray *moving_objects,
                  const mod_host::Transform *transform_prev2now = nullptr, std::vector<float> *flow_out = nullptr, int x0 = 0, int y0 = 0,
                  std::vector<float> *disparity_out = nullptr, mod_host::PointCloud2 *pc_with_velocity = nullptr) {
    // while setSideBySide() is on an image is two panes: an RGB-D frame is then a missing image, like two distinct images elsewhere
    const bool images = !side_by_side_ && image && depth && image->data && depth->data && useLayout(*image, *image, x0, y0);
    sizeOutputs(flow_out, disparity_out, pc_with_velocity);   // always, like submitOdometry()
    const ModTransform tf = transform_prev2now ? mod_host::to_mod(*transform_prev2now) : ModTransform{};
    return submitFrame(images ? &image->header.stamp : nullptr, image ? &image->header : nullptr, pc_with_velocity, moving_objects,
                       [&](Pending &p, double dt, void *cloud, ModObject *objects, int32_t max_objects, int32_t *ticket) {
      have_parked_ = false;
      return mod_submit_depth_host(ctx_, images ? image->data : nullptr, images ? depth->data : nullptr, &flow_, &ego_, transform_prev2now ? &tf : nullptr, dt,
                                   cloud, nullptr, objects, max_objects, disparity_out ? disparity_out->data() : nullptr,
                                   flow_out ? flow_out->data() : nullptr, &p.tf, &p.ego, ticket);
    });
  }
  // collect() of an odometry ticket: fills the messages, integrates the pose (only when the estimate succeeded) and returns the
  // estimated motion prev -> now; false when visual odometry failed (nothing is published, the pose is unchanged, :251-255).
  bool collectOdometry(int ticket, mod_host::Transform *motion = nullptr) {
    for (Pending &p : pending_) {
      if (p.ticket != ticket) continue;
      const int rc = finish(p, ticket);
      if (motion) *motion = mod_host::from_mod(p.tf);
      return integrateEstimate(p.tf, rc == MOD_OK ? p.ego.status : MOD_EGO_DIVERGED);
    }
    throw std::runtime_error("collectOdometry(): unknown ticket");
  }

  // integrateAndBroadcastTF (scene_flow_constructor.cpp:246,320-348): integrated_pose_ *= motion.inverse().  base_to_camera: the
  // base_link -> camera transform (the reference's TF lookup, identity when it is not available).
  void integrate(const mod_host::Transform &motion) { integrated_pose_ = integrated_pose_ * mod_host::Pose::fromTransform(motion).inverse(); }
  // an estimate of the library: integrated only when it succeeded (the reference integrates inside `if (viso_success)`, :231-246)
  bool integrateEstimate(const ModTransform &tf, int ego_status) {
    if (ego_status != MOD_EGO_OK) return false;
    integrate(mod_host::from_mod(tf));
    return true;
  }
  void setBaseToCamera(const mod_host::Transform &base_to_camera) { base_to_camera_ = mod_host::Pose::fromTransform(base_to_camera); }
  const mod_host::Pose &integratedPose() const { return integrated_pose_; }
  // odom -> base_link, the transform the reference broadcasts: B * integrated * B^-1
  mod_host::Pose odomToBase() const { return base_to_camera_ * integrated_pose_ * base_to_camera_.inverse(); }
  // camera -> odom, B * integrated: what MovingObjectsTracker::movingObjectsCallback takes as to_odom
  mod_host::Pose cameraToOdom() const { return base_to_camera_ * integrated_pose_; }
  void setEgoParams(const ModEgoParams &p) { ego_ = p; }

  void collect(int ticket) {
    for (Pending &p : pending_) {
      if (p.ticket != ticket) continue;
      check(finish(p, ticket));
      return;
    }
    throw std::runtime_error("collect(): unknown ticket");
  }

  // The constructor's per-pixel views as bgr8 messages, colour-coded on the device (mod_flow_image_dev and its siblings; the rule is
  // in include/mod_sf.h): one frame from a DEVICE plane at the camera's size — ~optical_flow or ~synthetic_optical_flow (flow alone),
  // the residual the dynamic test thresholds (flow and static_flow), ~depth's disparity (disparity alone).  3 B/px come back instead of
  // the 8 or 4 B/px plane.  Fills *image like ClustererNodelet::publishClustersImage: frame_id and stamp of `header`, packed rows.
  // false: an input was null (nothing rendered, *image untouched), as the reference publishes nothing for a missing input.
  bool publishFlowImage(const mod_host::Header &header, const float *flow, const float *static_flow, float max_px, mod_host::OwnedImage *image) {
    return publishView(header, image, [&](uint8_t *bgr) {
      return static_flow ? mod_flow_residual_image_dev(ctx_, 1, flow, static_flow, max_px, bgr) : mod_flow_image_dev(ctx_, 1, flow, max_px, bgr);
    });
  }
  bool publishDisparityImage(const mod_host::Header &header, const float *disparity, mod_host::OwnedImage *image) {
    return publishView(header, image, [&](uint8_t *bgr) { return mod_disparity_image_dev(ctx_, 1, disparity, bgr); });
  }

  void setMaxObjects(int n) { max_objects_ = n; }
  int imageWidth() const { return image_width_; }
  int imageHeight() const { return image_height_; }

 private:
  // render(device bgr) into a device buffer of the camera's size, then the pixels and the message around them
  template <class Render> bool publishView(const mod_host::Header &header, mod_host::OwnedImage *image, Render render) {
    ModCamera cam{};
    check(mod_get_camera(ctx_, &cam));
    const size_t bytes = 3 * (size_t)cam.width * cam.height;
    struct Dev { ModContext *c; void *p = nullptr; ~Dev() { if (p) (void)mod_free(c, p); } } dev{ctx_};
    check(mod_malloc(ctx_, bytes, &dev.p));
    const int rc = render(static_cast<uint8_t *>(dev.p));
    check(rc);
    if (rc != MOD_OK) return false;
    image->pixels.resize(bytes);
    check(mod_memcpy_d2h(ctx_, image->pixels.data(), dev.p, bytes));
    mod_host::Image &v = image->view;
    v.header = mod_host::Header();
    v.header.frame_id = header.frame_id; v.header.stamp = header.stamp;
    v.width = cam.width; v.height = cam.height;
    v.encoding = "bgr8"; v.step = 3 * cam.width;
    v.data = image->pixels.data();
    return true;
  }

  struct Pending {
    int ticket = -1;
    mod_host::PointCloud2 *cloud = nullptr;
    mod_host::MovingObjectArray *objs = nullptr;
    mod_host::Header header;
    std::vector<ModObject> objects;
    ModTransform tf{};
    ModEgoResult ego{};
  };
  // mod_set_image_layout from the left message, the camera-sized window at (x0, y0); false when the library cannot take the images
  // (an unknown encoding, a window that does not fit) or left and right disagree in encoding, size or step (the reference asserts
  // the same, scene_flow_constructor.cpp:224-226).  Every image entry point of this class sets it: the layout is the context's.
  bool useLayout(const mod_host::Image &left, const mod_host::Image &right, int x0, int y0) {
    ModImageLayout lay{};
    if (!mod_host::image_layout(left, x0, y0, &lay, side_by_side_) || right.encoding != left.encoding || right.width != left.width ||
        right.height != left.height || right.step != left.step) return false;
    if (side_by_side_ && right.data != left.data) return false;
    // the library checks a layout against the side-by-side state in force and the state against the layout: set each while the
    // other allows it (off accepts every layout, and a two-pane layout accepts both states)
    if (!side_by_side_) check(mod_set_side_by_side(ctx_, 0));
    if (mod_set_image_layout(ctx_, &lay) != MOD_OK) return false;
    return !side_by_side_ || mod_set_side_by_side(ctx_, 1) == MOD_OK;
  }

  // collects a ticket and fills the messages handed to its submit; returns the collect status (< 0 thrown)
  int finish(Pending &p, int ticket) {
    int32_t n_obj = 0;
    const int rc = mod_collect_frame_host(ctx_, ticket, &n_obj);
    p.ticket = -1;
    if (rc < 0) check(rc);
    if (p.cloud) mod_host::describe_cloud(*p.cloud, p.header, image_width_, image_height_);
    if (p.objs) mod_host::fill_objects(*p.objs, p.header, p.objects.data(), n_obj, p.objects.size());
    return rc;
  }

  // One frame of a submit*(), the part the four entries share.  `stamp`: of the message that times the frame, null where the entry
  // found its inputs unusable — dt is then 0 and the stamp is forgotten, so the next frame has no previous one either; dt is formed
  // from the STORED stamp of the frame before.  `enqueue` makes the entry's one mod_submit_*_host call on the slot's buffers and returns
  // its code: a skip returns -1, an error throws, and only an enqueued frame takes the slot — its ticket carries `header` (read only
  // then) and the messages collect() fills.  have_parked_ is the entry's to set inside `enqueue`: submit() parks a host copy on a skip and
  // keeps what is parked on an error, the submits whose previous disparity lives in HBM clear it whatever the code.  cloud == nullptr: the 32-byte cloud is neither packed nor copied to the host (nobody
  // subscribes to ~scene_flow); objs == nullptr: no cluster output is asked for and the library runs the scene-flow stage alone.
  template <class Enqueue>
  int submitFrame(const mod_host::Time *stamp, const mod_host::Header *header, mod_host::PointCloud2 *cloud, mod_host::MovingObjectArray *objs,
                  Enqueue enqueue) {
    const double dt = (stamp && have_stamp_) ? mod_host::duration_sec(*stamp, previous_stamp_) : 0.0;
    Pending &p = pending_[next_slot_];
    p.objects.resize(max_objects_);
    int32_t ticket = -1;
    const int rc = enqueue(p, dt, cloud ? cloud->data.data() : nullptr, objs ? p.objects.data() : nullptr, objs ? (int32_t)p.objects.size() : 0, &ticket);
    have_stamp_ = stamp != nullptr;
    if (stamp) previous_stamp_ = *stamp;
    if (rc > 0) return -1;
    check(rc);
    p.ticket = ticket; p.cloud = cloud; p.objs = objs; p.header = *header;
    next_slot_ = (next_slot_ + 1) % MOD_PIPELINE_DEPTH;
    return ticket;
  }
  // the host copies submitOdometry() and submitDepth() were asked for, at the camera's size
  void sizeOutputs(std::vector<float> *flow_out, std::vector<float> *disparity_out, mod_host::PointCloud2 *pc_with_velocity) {
    const size_t n = (size_t)image_width_ * image_height_;
    if (flow_out) flow_out->resize(n * 2);
    if (disparity_out) disparity_out->resize(n);
    if (pc_with_velocity) pc_with_velocity->data.resize(n * 32);
  }
  Pending pending_[MOD_PIPELINE_DEPTH];
  int next_slot_ = 0;
  bool have_stamp_ = false, have_parked_ = false;
  bool side_by_side_ = false;
  mod_host::Time previous_stamp_;
  std::vector<float> parked_;

  ModParams currentParams() {
    ModParams p{};
    if (mod_get_params(ctx_, &p) != MOD_OK) {   // reference defaults (SceneFlowConstructor.cfg:8, Clusterer.cfg:8-11)
      p.dynamic_flow_diff = 5; p.cluster_size = 2500; p.neighbor_distance = 4; p.depth_diff = 0.15; p.dynamic_speed = 0.3;
    }
    return p;
  }
  void check(int rc) { if (rc < 0) throw std::runtime_error(std::string("libmod_sf: ") + mod_last_error(ctx_)); }

  ModContext *ctx_;
  ModSgmParams sgm_{128, 6, 96, 8, 1, 1};   // the published configuration of the estimator (oracle/sgm_ref.cpp)
  int disparity_offset_ = 0;                // setDisparityOffset(): what the context holds
  ModFlowParams flow_{4, 4, 5, 1, 1};       // include/mod_sf.h defaults
  int image_width_ = 0, image_height_ = 0;
  int max_objects_ = 1024;
  bool have_previous_ = false;
  ModEgoParams ego_{4, 256, 10, 50, 2.0f, 1.0f, 0u, 0};   // include/mod_sf.h defaults
  mod_host::Pose integrated_pose_, base_to_camera_;
  mod_host::DisparityImage disparity_previous_;
  std::vector<float> previous_pixels_;
};

}  // namespace scene_flow_constructor
