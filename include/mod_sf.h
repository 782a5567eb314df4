/*
 * mod_sf.h — C ABI of the MI355X-native scene-flow + moving-point clustering path.
 *
 * The reference (ActiveIntelligentSystemsLab/moving_object_detector) has no FFI: the path is a ROS-1 node
 * (scene_flow_constructor) plus a nodelet plugin (scene_flow_clusterer/scene_flow_clusterer,
 * scene_flow_clusterer/nodelet_plugins.xml:3-4) joined by the ~scene_flow PointCloud2 topic.  This header is the
 * boundary a maintainer binds instead of the CPU loops; every entry point cites the reference code it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the node/nodelet side of the binding.
 *
 * Conventions
 *   - plain C, POD structs, no exceptions cross the boundary;
 *   - return value: 0 = ok, >0 = "skipped, input missing" (the reference silently publishes nothing,
 *     scene_flow_constructor/src/scene_flow_constructor.cpp:104,110,122,127,133), <0 = error
 *     (mod_last_error() gives the text);
 *   - a context is single-caller (the reference runs construct() on one thread at a time, :389-392, and the
 *     clusterer on a single-threaded callback queue, clusterer_nodelet.cpp:25,35); distinct contexts are independent;
 *   - "_dev" entry points take DEVICE pointers (HBM-resident planes) and only enqueue work on the context's
 *     stream; "_host" entry points take host pointers, stage through the context and synchronise;
 *   - image planes are row-major, pitch == width, frames contiguous ([frames][H][W]).
 */
#ifndef MOD_SF_H_
#define MOD_SF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libmod_sf.so is built with -fvisibility=hidden: the declarations of this header are its whole dynamic symbol table
 * (tests/test_abi.py checks `nm -D --defined-only`). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define MOD_ABI_VERSION 2   /* 2: ModConfig.batch_chunks (was reserved), stage "select" folded into MOD_STAGE_CCL_MERGE, MOD_STAGE_CLUSTER_GROUP */

/* status codes */
#define MOD_OK                      0
#define MOD_SKIP_NO_DISPARITY_NOW   1  /* construct(): `if (disparity_now)` guard, scene_flow_constructor.cpp:110 */
#define MOD_SKIP_NO_DISPARITY_PREV  2  /* :104,127 */
#define MOD_SKIP_NO_FLOW            3  /* :122-123 */
#define MOD_SKIP_NO_TRANSFORM       4  /* :127 (visual odometry failed, :251-255) */
#define MOD_ERR_INVALID_ARGUMENT   -1
#define MOD_ERR_NOT_CONFIGURED     -2  /* camera/params not set */
#define MOD_ERR_CAPACITY           -3  /* frames / image larger than the context was created for */
#define MOD_ERR_DEVICE             -4  /* HIP runtime error */
#define MOD_ERR_NO_DEVICE          -5  /* no gfx950 device / library built without a usable device */

typedef struct ModContext ModContext;

#define MOD_MAX_WIDTH 16384   /* widest image a context accepts (one image row of census words must fit LDS; tested up to 8256) */

/* Context creation parameters. */
typedef struct ModConfig {
  int32_t device;       /* HIP device ordinal */
  int32_t max_width;    /* largest image width  the scratch is sized for, <= MOD_MAX_WIDTH */
  int32_t max_height;   /* largest image height the scratch is sized for */
  int32_t max_frames;   /* largest batch (frames per call), <= 65535; max_width * max_height < 2^27 */
  int32_t max_objects;  /* per-frame capacity of the ModObject output; 0 -> max_width*max_height/100 (Clusterer.cfg:8 lower bound).
                           mod_set_params rejects a cluster_size with max_width*max_height/cluster_size > max_objects, so no
                           cluster can ever be dropped */
  int32_t batch_chunks; /* mod_process_dev on a large batch: 2..4 -> the cluster stage runs in that many chunks of frames, side by side
                           on streams of the context's own, so that its waiting kernels (cross-tile links, root merge, median
                           selection, tie replay) share the GPU with the streaming kernels of another chunk; forked from and joined
                           to `stream` with events — the call is ordered on `stream` like any other; a chunk has at least 32 frames.
                           0 or 1 -> one piece (the default).  Results do not depend on it.  Worth 1 - 3 % of a 512-pair step in a
                           long-running process and nothing in a process's first calls (csrc/mod_sf.hip process_chunked). */
  void   *stream;       /* hipStream_t to enqueue on; NULL -> the context creates its own */
} ModConfig;

/*
 * Camera + disparity-message constants.
 *   fx..Ty : left CameraInfo projection matrix P (P[0],P[5],P[2],P[6],P[3],P[7]) as used by
 *            image_geometry::PinholeCameraModel::projectPixelTo3dRay / project3dToPixel
 *            (call sites disparity_image_processor.cpp:45, scene_flow_constructor.cpp:84);
 *   disp_* : stereo_msgs/DisparityImage f, T, min_disparity, max_disparity
 *            (disparity_image_processor.cpp:25-27,41-42).
 */
typedef struct ModCamera {
  int32_t width, height;
  double  fx, fy, cx, cy, Tx, Ty;
  float   disp_f, disp_T, min_disparity, max_disparity;
} ModCamera;

/*
 * dynamic_reconfigure parameters, read by value inside the hot loops
 * (scene_flow_constructor/cfg/SceneFlowConstructor.cfg:8, scene_flow_clusterer/cfg/Clusterer.cfg:8-11).
 * cluster_size must be >= 1 (the reference's range is [100,10000]).
 */
typedef struct ModParams {
  int32_t dynamic_flow_diff;   /* default 5   [px]  */
  int32_t cluster_size;        /* default 2500 [px] */
  int32_t neighbor_distance;   /* default 4   [px], 1..MOD_MAX_NEIGHBOR_DISTANCE */
  int32_t reserved;
  double  depth_diff;          /* default 0.15 [m]  */
  double  dynamic_speed;       /* default 0.3 [m/s] */
} ModParams;
#define MOD_MAX_NEIGHBOR_DISTANCE 16

/* geometry_msgs/Transform previous->now (scene_flow_constructor.cpp:248-249,411): translation + quaternion x,y,z,w. */
typedef struct ModTransform {
  double t[3];
  double q[4];
} ModTransform;

/* moving_object_msgs/MovingObject (moving_object_msgs/msg/MovingObject.msg:3-7); orientation is always (0,0,0,1). */
typedef struct ModObject {
  int32_t id;
  int32_t n_points;       /* cluster size (not in the message; handy for tests/tracing) */
  double  center[3];
  double  orientation[4];
  double  velocity[3];
  double  bounding_box[3];
} ModObject;

/* The four values handed to SceneFlowConstructor::construct (scene_flow_constructor.cpp:91-97,392), batched. */
typedef struct ModFrameBatch {
  int32_t      frames;
  int32_t      reserved;
  const float *disparity_now;    /* dev [frames][H][W] 32FC1; NULL -> MOD_SKIP_NO_DISPARITY_NOW  */
  const float *disparity_prev;   /* dev [frames][H][W] 32FC1; NULL -> MOD_SKIP_NO_DISPARITY_PREV; for a sequence D[0..F]
                                    pass prev = D, now = D + H*W */
  const float *flow;             /* dev [frames][H][W][2] 32FC2 (x then y, scene_flow_constructor/README.md:35-40); NULL -> skip */
  const ModTransform *transforms;/* HOST [frames]; NULL -> MOD_SKIP_NO_TRANSFORM */
  const double *dt;              /* HOST [frames]: stamp_now - stamp_previous in seconds (scene_flow_constructor.cpp:162-164) */
} ModFrameBatch;

/* ~scene_flow as SoA planes (+ optional reference-layout outputs). All device pointers, [frames][H][W]. */
typedef struct ModSceneFlowPlanes {
  float    *x, *y, *z, *vx, *vy, *vz;  /* required — except x and y in mod_process_dev (both or neither): the reference builds and ships
                                          the cloud only for subscribers (scene_flow_constructor.cpp:141-142); a caller that serves the
                                          moving objects alone passes x = y = NULL, the scene-flow kernel then writes 16 instead of 24
                                          bytes per pixel and the cluster stage recomputes its members' x, y from z (bit-identical) */
  uint64_t *dynamic_mask;  /* optional [frames][H][mod_mask_words(W)]: bit b of word k of a row = pixel 64k+b is dynamic
                              (calculateDynamicMap, clusterer_nodelet.cpp:40-54).  The bits of a row's last word at columns >= W
                              must be 0 in a caller's mask (mod_cluster_dev reads the words whole and takes every set bit for a
                              pixel of that row: a set bit there addresses memory beyond the row, beyond the planes in the last
                              one); the library's own masks (mod_scene_flow_dev, mod_process_dev, mod_dynamic_mask_dev) have them 0 */
  void     *cloud_aos;     /* optional [frames][H][W] 32-byte pcl::PointXYZVelocity records
                              (scene_flow_constructor/pcl_point_xyz_velocity.h:8-34: x@0 y@4 z@8 vx@16 vy@20 vz@24) */
  float    *depth;         /* optional ~depth image (disparity_image_processor.cpp:105-120) */
  float    *static_flow;   /* optional ~synthetic_optical_flow 32FC2 (scene_flow_constructor.cpp:65-89) */
} ModSceneFlowPlanes;

/* Output of the clusterer (clusterer_nodelet.cpp:85-95,324-343). Device pointers. */
typedef struct ModClusterOut {
  int32_t   *labels;      /* optional [frames][H][W]: -1 = none, 0..K-1 in the reference's order (removeSmallClusters, :354-393).
                             The reference renders its cluster image only while somebody subscribes to it
                             (publishClustersImage, :235-236,292-322): pass NULL and the 4 B/px plane is never written.
                             mod_set_cluster_image draws that image from this plane on the device. */
  ModObject *objects;     /* [frames][max_objects] */
  int32_t   *n_objects;   /* [frames] accepted objects (publishMovingObjects, :324-343) */
  int32_t   *n_clusters;  /* [frames] K = clusters surviving the size filter (may be NULL) */
} ModClusterOut;

static inline int32_t mod_mask_words(int32_t width) { return (width + 63) / 64; }

/* ---- context ---------------------------------------------------------------------------------------------- */
int  mod_abi_version(void);
int  mod_create(const ModConfig *cfg, ModContext **out_ctx);
void mod_destroy(ModContext *ctx);
const char *mod_last_error(const ModContext *ctx);          /* never NULL */
int  mod_set_camera(ModContext *ctx, const ModCamera *cam); /* stereoCallback first-frame block, scene_flow_constructor.cpp:368-375 */
int  mod_set_params(ModContext *ctx, const ModParams *prm); /* reconfigureCB, scene_flow_constructor.cpp:401-407, clusterer_nodelet.cpp:345-352 */
int  mod_get_camera(const ModContext *ctx, ModCamera *cam);
int  mod_get_params(const ModContext *ctx, ModParams *prm);
int  mod_synchronize(ModContext *ctx);                      /* wait for everything enqueued on the context's stream */

/* ---- hot path, device-resident ---------------------------------------------------------------------------- */
/* construct(): toPointCloud x2 + transformPCPreviousToNow + calculateStaticOpticalFlow + constructVelocityPC
 * (scene_flow_constructor.cpp:91-147) as one fused kernel; also emits the dynamic mask when requested. */
int  mod_scene_flow_dev(ModContext *ctx, const ModFrameBatch *in, const ModSceneFlowPlanes *out);

/* ~depth alone: toDepthImage (disparity_image_proc/src/disparity_image_processor.cpp:105-120).  construct() publishes it whenever
 * disparity_now exists — also on frames that end at one of its guards without scene flow (scene_flow_constructor.cpp:110-123).
 * mod_scene_flow_dev / mod_process_dev follow that: when they return a skip code other than MOD_SKIP_NO_DISPARITY_NOW and
 * out->depth was requested, the depth plane HAS been enqueued (all other outputs are untouched).  These two entry points
 * give the depth image without a batch (device planes [frames][H][W]; host: one frame).  NULL disparity -> MOD_SKIP_NO_DISPARITY_NOW. */
int  mod_depth_image_dev(ModContext *ctx, int32_t frames, const float *disparity_now, float *depth);
int  mod_depth_image_host(ModContext *ctx, const float *disparity_now, float *depth);

/* ~synthetic_optical_flow alone: calculateStaticOpticalFlow (scene_flow_constructor.cpp:65-89) — the flow a static scene would
 * show under the camera motion `transform`: previous cloud reprojected, moved, projected (32FC2, NaN where the previous point is
 * invalid).  construct() publishes it only for subscribers (:141-145); the batch entry points give it through
 * ModSceneFlowPlanes.static_flow, this one for a node that holds host buffers.  One frame, synchronous.
 * NULL disparity_prev -> MOD_SKIP_NO_DISPARITY_PREV, NULL transform -> MOD_SKIP_NO_TRANSFORM. */
int  mod_static_flow_host(ModContext *ctx, const float *disparity_prev, const ModTransform *transform, float *static_flow);

/* calculateDynamicMap (clusterer_nodelet.cpp:40-54) for a cloud that did not come from mod_scene_flow_dev. */
int  mod_dynamic_mask_dev(ModContext *ctx, int32_t frames, const float *vx, const float *vy, const float *vz,
                          uint64_t *dynamic_mask);

/* clustering() + publishMovingObjects() (clusterer_nodelet.cpp:85-95,324-343) on SoA planes.
 * planes->dynamic_mask may be NULL (computed internally). */
int  mod_cluster_dev(ModContext *ctx, int32_t frames, const ModSceneFlowPlanes *planes, const ModClusterOut *out);

/* Both stages back to back without the PointCloud2 round trip (the mask is produced by the scene-flow kernel).
 * planes->x and planes->y may both be NULL (objects-only: see ModSceneFlowPlanes). */
int  mod_process_dev(ModContext *ctx, const ModFrameBatch *in, const ModSceneFlowPlanes *planes, const ModClusterOut *out);

/* Per-cluster member lists, opt-in: what clustering() returns as pcl::IndicesClusters (clusterMap2IndicesCluster,
 * clusterer_nodelet.cpp:97-117) and what cluster2Marker reads for the ~clusters markers (:119-145).  Context state like
 * mod_set_disparity_filters.  NULL = off (the default): every call enqueues exactly what it did without this setting — no launch, no
 * memset, no allocation.
 *   Which calls write the lists: every later mod_cluster_dev and mod_process_dev, chunked (ModConfig.batch_chunks) or not, for all
 *     their frames; the synchronous host calls that run the cluster stage, mod_process_frame_host and mod_cluster_cloud_host, as
 *     frame 0.  Ordered on the context's stream like the other outputs.  The pipelined mod_submit_*_host calls never write the lists
 *     (several tickets in flight would share one buffer): submits enqueue exactly what they enqueue without the setting.
 *   offsets: for frame f with K = n_clusters[f] surviving clusters, offsets[f][0] = 0 and offsets[f][k+1] - offsets[f][k] is the size
 *     of cluster k, k being the label the labels plane carries (the reference's numbering by first_edge_key).  All K clusters are
 *     listed, accepted as objects or not.  offsets[f][k] = offsets[f][K] for K < k <= max_objects (the context's capacity:
 *     ModConfig.max_objects, or max_width * max_height / 100 when that was 0).
 *   indices: indices[f][offsets[f][k] .. offsets[f][k+1]) are cluster k's pixel indices v * W + u in the reference's order: u
 *     ascending, then v ascending (column-major, :104-114).  Entries of indices and points at and beyond offsets[f][K] are not written.
 *   points (optional): points[f][i] is the (x, y, z) of pixel indices[f][i], bit for bit what the x, y, z planes hold — NaN
 *     coordinates of a caller's cloud included.  In an objects-only call (planes->x == planes->y == NULL) x and y are recomputed
 *     from z and the ray tables with the scene-flow kernel's own two operations, as the cluster stage does for its boxes: identical
 *     to a six-plane call.
 *   MOD_ERR_INVALID_ARGUMENT (the setting stays as it was): offsets or indices NULL, reserved != 0.  Every context has a cluster
 *     stage (max_objects 0 selects the default capacity), so there is no context that refuses the setting as such.
 * Frames lie max_objects + 1 (offsets), H * W (indices) and 3 * H * W (points) elements apart, H * W being the camera's size at the
 * call, like the labels plane.  The launches are timed inside MOD_STAGE_FINAL. */
typedef struct ModClusterMembers {   /* 32 bytes; device pointers; the caller owns them */
  int32_t *offsets;   /* [frames][max_objects + 1] */
  int32_t *indices;   /* [frames][H * W] */
  float   *points;    /* optional [frames][H * W][3]: x, y, z of indices[i], F32 as in the planes */
  int64_t  reserved;  /* must be 0 */
} ModClusterMembers;
int  mod_set_cluster_members(ModContext *ctx, const ModClusterMembers *out);   /* NULL = off (the default) */
/* *out: the setting in force (zeroed while off); *enabled: 0 / 1.  Either may be NULL. */
int  mod_get_cluster_members(const ModContext *ctx, ModClusterMembers *out, int32_t *enabled);

/* The cluster image and the markers' colours, opt-in: what publishClustersImage draws (~clusters_image, BGR8, one colour per cluster,
 * black elsewhere; clusterer_nodelet.cpp:292-322) and the colour cluster2Marker gives marker k (:119-145, color_set.cpp).  Context
 * state like mod_set_cluster_members.  NULL = off (the default): every call enqueues exactly what it did without this setting.
 *   The colour of label k in a frame with K = n_clusters[f] clusters is entry (k * 255) / K (integer division) of a 256-entry table:
 *     ColorSet::resize(K) per frame.  A label outside [0, K) — -1, anything else, every label when K <= 0 — is black (0, 0, 0) and
 *     never indexes the table.
 *   The built-in table (palette_bgr NULL) is this library's own hue wheel, NOT OpenCV's COLORMAP_HSV, whose 256 entries the reference
 *     reads from cv::applyColorMap: for i in 0..255, t = 6 i, s = t >> 8 (0..5), f = t & 255, g = 255 - f, and (R, G, B) is
 *     s = 0: (255, f, 0); 1: (g, 255, 0); 2: (0, 255, f); 3: (0, g, 255); 4: (f, 0, 255); 5: (255, 0, g); stored B, G, R.  Entry 0 is
 *     (0, 0, 255), entry 255 is (5, 0, 255) as B, G, R.  A caller who has OpenCV passes COLORMAP_HSV's 768 bytes as palette_bgr and gets
 *     the reference's bytes.  The table is copied at the call that takes it.
 *   Which calls write `image` (device): every later mod_cluster_dev and mod_process_dev, chunked or not, for all their frames, after
 *     the cluster stage, ordered on the context's stream.  They need out->labels and out->n_clusters: with either NULL while the
 *     setting is on and image is not NULL they return MOD_ERR_INVALID_ARGUMENT and enqueue nothing.
 *   Which calls write `host_image` (when not NULL): mod_process_frame_host and mod_cluster_cloud_host, frame 0, rendered from the
 *     staging's own label plane whether or not the caller passed `labels`; the image request alone makes them run the cluster stage.
 *     And, unlike the member lists, every pipelined submit (mod_submit_frame_host, _stereo_, _images_, _odometry_, _depth_host): the
 *     submit reads host_image and the table as they are when it is made, the frame in flight keeps both, and the image is valid after
 *     its ticket has been collected.  A caller rotates buffers by calling mod_set_cluster_image between submits, with tickets
 *     outstanding too.  A frame that ends at a guard (MOD_SKIP_*) or fails leaves host_image untouched.
 *   MOD_ERR_INVALID_ARGUMENT (the setting stays as it was): reserved != 0, image and host_image both NULL, image not 16-byte aligned.
 * The launches are timed inside MOD_STAGE_FINAL. */
typedef struct ModClusterImage {      /* 32 bytes */
  uint8_t       *image;        /* device [frames][H][W][3] BGR8, packed (no row padding); for the *_dev calls; 16-byte aligned */
  uint8_t       *host_image;   /* host  [H][W][3]; for the *_host calls (frame 0 / the ticket's frame) */
  const uint8_t *palette_bgr;  /* host, 256 x 3 bytes B,G,R, copied at the call; NULL = the built-in table */
  int64_t        reserved;     /* must be 0 */
} ModClusterImage;
int  mod_set_cluster_image(ModContext *ctx, const ModClusterImage *out);     /* NULL = off (the default) */
/* *out: the setting in force (zeroed while off; palette_bgr: the context's copy of a caller's table, or NULL); *enabled: 0 / 1. */
int  mod_get_cluster_image(const ModContext *ctx, ModClusterImage *out, int32_t *enabled);
/* The renderer alone, on any device label plane [frames][H * W] and device n_clusters [frames] at the camera's size, into
 * image [frames][H][W][3] (device, 16-byte aligned); ordered on the context's stream.  palette_bgr: host, 768 bytes, or NULL. */
int  mod_cluster_image_dev(ModContext *ctx, int32_t frames, const int32_t *labels, const int32_t *n_clusters,
                           const uint8_t *palette_bgr, uint8_t *image);
/* Host only, no context, no GPU: the colour of label k among n_clusters (marker k's r, g, b are bgr[2], bgr[1], bgr[0] over 255.0,
 * a = 1.0).  MOD_ERR_INVALID_ARGUMENT unless 0 <= k < n_clusters and bgr is not NULL. */
int  mod_cluster_color(int32_t k, int32_t n_clusters, const uint8_t *palette_bgr, uint8_t bgr[3]);
/* Host only: the built-in table, 256 x 3 bytes B, G, R. */
int  mod_cluster_palette(uint8_t palette_bgr[768]);

/* Flow and disparity images: the constructor's per-pixel views (~optical_flow, ~synthetic_optical_flow, ~depth;
 * scene_flow_constructor.cpp:45-48,100,118,145) colour-coded on the device, BGR8, 3 B/px out instead of the 8 or 4 B/px plane.
 * Calls of their own: nothing is enqueued unless one of them is made, and they keep no state.  All planes are device memory at the
 * camera's size, packed; every call is ordered on the context's stream and returns once its kernel is enqueued.
 *   The colour rule.  F32 throughout; every operation is one correctly rounded IEEE operation (add, subtract, multiply, divide,
 *     sqrtf, compare, truncation of a non-negative value): no atan2, no fused multiply-add.  For a vector (fx, fy) and max_px:
 *     invalid: fx or fy NaN or +-inf -> (0, 0, 0).
 *     magnitude: m = sqrtf(fx * fx + fy * fy), the two products and the sum rounded separately; m == 0 -> (255, 255, 255).
 *     strength: s = min(255, (int)(255 * (m / max_px))): one division, then one multiplication.  The comparison is made in F32
 *       ahead of the conversion — v = 255 * (m / max_px); s = v < 255 ? (int)v : 255 — so an m that overflowed to +inf gives 255.
 *     direction: A = |fx| + |fy|, t = fy / A (in [-1, 1]), and the "diamond angle" q in [0, 4]:
 *       fx >= 0 and fy >= 0: q = t;   fx < 0: q = 2 - t;   fx >= 0 and fy < 0: q = 4 + t   (a -0 component counts as >= 0);
 *       idx = min(255, (int)(q * 64)), again compared ahead of the conversion; 64 q is exact.
 *     palette: P = the built-in 256-entry hue wheel of mod_cluster_palette (no second table).
 *     blend, per channel c, in integers: out_c = 255 - ((255 - P[idx][c]) * s + 127) / 255: white at rest, the full hue at max_px
 *       and beyond.
 *   The residual image applies the rule to (flow - static_flow), subtracted per component in F32: the field the dynamic test
 *     thresholds (scene_flow_constructor.cpp:196-198).  NaN in either operand is black.
 *   The disparity image: d NaN, +-inf, d < min_disparity, d > max_disparity or d == 0 -> (0, 0, 0) (getDisparity's and getPoint3D's
 *     rejects); else idx = min(255, (int)(255 * ((d - min_disparity) / (max_disparity - min_disparity)))), compared ahead of the
 *     conversion, and the pixel is P[idx].  The range is the camera's (ModCamera.min_disparity .. max_disparity).
 *   Status, tested in this order: NULL ctx, frames outside 1 .. 65535, NULL output (or one not aligned: bgr 4 bytes, static_flow 8),
 *     max_px not finite or <= 0 -> MOD_ERR_INVALID_ARGUMENT; no camera set -> MOD_ERR_NOT_CONFIGURED (mod_disparity_image_dev: also
 *     max_disparity <= min_disparity); a NULL input plane -> the skip code of construct()'s guard for it (flow or static_flow:
 *     MOD_SKIP_NO_FLOW; disparity_prev: MOD_SKIP_NO_DISPARITY_PREV; disparity: MOD_SKIP_NO_DISPARITY_NOW; transforms:
 *     MOD_SKIP_NO_TRANSFORM); an input plane that is not 4-byte aligned (transforms: 8) -> MOD_ERR_INVALID_ARGUMENT.  Nothing is
 *     enqueued unless the call returns MOD_OK.  frames is not held to ModConfig.max_frames: the calls use no scratch. */
/* mod_static_flow_host on device planes: for every frame exactly that call's bytes (NaN where it writes NaN), from
 * disparity_prev [frames][H][W] and transforms [frames] IN DEVICE MEMORY (e.g. mod_egomotion_dev's) into static_flow [frames][H][W][2]. */
int  mod_static_flow_dev(ModContext *ctx, int32_t frames, const float *disparity_prev, const ModTransform *transforms, float *static_flow);
/* flow [frames][H][W][2] -> bgr [frames][H][W][3] */
int  mod_flow_image_dev(ModContext *ctx, int32_t frames, const float *flow, float max_px, uint8_t *bgr);
/* (flow - static_flow) -> bgr, one launch */
int  mod_flow_residual_image_dev(ModContext *ctx, int32_t frames, const float *flow, const float *static_flow, float max_px, uint8_t *bgr);
/* disparity [frames][H][W] -> bgr [frames][H][W][3] */
int  mod_disparity_image_dev(ModContext *ctx, int32_t frames, const float *disparity, uint8_t *bgr);
/* Host only, no context, no GPU: the colour of one vector by the same arithmetic (the legend of a flow image).
 * MOD_ERR_INVALID_ARGUMENT: bgr NULL, max_px not finite or <= 0. */
int  mod_flow_color(float fx, float fy, float max_px, uint8_t bgr[3]);

/* pcl::toROSMsg / pcl::fromROSMsg payload conversion (scene_flow_constructor.cpp:358-361, clusterer_nodelet.cpp:226). */
int  mod_pack_cloud_dev(ModContext *ctx, int32_t frames, const ModSceneFlowPlanes *planes, void *cloud_aos);
int  mod_unpack_cloud_dev(ModContext *ctx, int32_t frames, const void *cloud_aos, const ModSceneFlowPlanes *planes);

/* ---- on-GPU disparity (BASELINE config 5) ------------------------------------------------------------ */
/* The reference obtains disparity_now from sgm_gpu::SgmGpu::computeDisparity(left, right, left_info, right_info, disparity)
 * (scene_flow_constructor/src/scene_flow_constructor.cpp:35,267; package sgm_gpu of sgm_gpu_ros, not vendored).  Algorithm,
 * parameters and every choice the publication leaves open: oracle/sgm_ref.cpp (semi-global matching: centre-symmetric 9 x 7
 * census, Hamming cost, 8 paths with P1 / P2, winner-take-all, 3 x 3 median, left-right check).  Images are 8-bit, rectified,
 * [frames][H][W] of the configured camera size; the result is the `image` of a stereo_msgs/DisparityImage (32FC1, invalid
 * pixels -1 = min_disparity - 1) whose other fields are f, T of the camera, min_disparity 0, max_disparity disparities - 1
 * (with a disparity offset d0, mod_set_disparity_offset below: d0 and d0 + disparities - 1, invalid pixels still -1) —
 * exactly what mod_set_camera takes as disp_f, disp_T, min_disparity, max_disparity
 * (disparity_image_proc/src/disparity_image_processor.cpp:25-27,41-42). */
#define MOD_SGM_MAX_DISPARITIES 128
typedef struct ModSgmParams {
  int32_t disparities;   /* D <= 128; default 128 */
  int32_t p1, p2;        /* smoothness penalties; defaults 6, 96; 31 + p2 must fit uint8 */
  int32_t paths;         /* 8, or 4 (the horizontal and vertical ones) */
  int32_t lr_check;      /* left-right consistency check, tolerance 1 */
  int32_t median;        /* 3 x 3 median of the winner-take-all maps */
} ModSgmParams;
/* computeDisparity: device images in, device disparity plane out.  Ordered like any other work on the context's stream (the
 * aggregation paths run on streams of the context's own, forked from and joined to it with events).  Scratch — two sets of, per
 * frame of a group of up to 8 frames, one W*H*disparities uint8 cost volume per path, at most 24 GB — is allocated on first use.
 * Images at least 2 pixels wide.  NULL image -> MOD_SKIP_NO_DISPARITY_NOW, as a failed estimateDisparity. */
int  mod_sgm_compute_dev(ModContext *ctx, int32_t frames, const uint8_t *left, const uint8_t *right, const ModSgmParams *params,
                         float *disparity);
/* the same for one frame in host memory (what a ROS node holding sensor_msgs/Image buffers calls); synchronous */
int  mod_sgm_compute_host(ModContext *ctx, const uint8_t *left, const uint8_t *right, const ModSgmParams *params, float *disparity);
/* Sub-pixel disparity, opt-in: context state like the image layout, read when a call or a submit enqueues its estimator —
 * mod_sgm_compute_dev / _host, mod_submit_stereo_host, mod_submit_images_host, mod_submit_odometry_host; a frame in flight
 * completes with the setting of its own submit.  fraction_bits 0 (the default): whole disparities, as ever.  4: sixteenths of a
 * pixel — with S the summed path costs and d their first minimum, q = floor((16 num + den) / (2 den)), num = S(d-1) - S(d+1),
 * den = S(d-1) - 2 S(d) + S(d+1), for 1 <= d <= disparities - 2 (else 0; den >= 1 and |q| <= 8 because d is the FIRST minimum);
 * v = 16 d + q; the median runs on v; the left-right check on the nearest integer (v + 8) >> 4 against the (integer) right map;
 * the pixel is v / 16, exact in float, still inside [0, disparities - 1], or -1.  Integer arithmetic throughout:
 * tests/models/sgm_subpixel_model.py restates it bit for bit.  Any other value: MOD_ERR_INVALID_ARGUMENT. */
#define MOD_SGM_FRACTION_BITS 4
int  mod_set_disparity_subpixel(ModContext *ctx, int32_t fraction_bits);
int  mod_get_disparity_subpixel(const ModContext *ctx, int32_t *fraction_bits);
/* Rejection filters, opt-in: context state like the sub-pixel mode, read when a call or a submit enqueues its estimator (the same
 * five entry points); a frame in flight completes with the settings of its own submit.  All zero (the default): off — the estimator
 * enqueues the kernels it always did.  Integer arithmetic up to the final conversion: tests/models/sgm_filters_model.py restates
 * both bit for bit.
 *   uniqueness_ratio u (StereoSGBM's rule, left map only): with d the first minimum of the summed path costs S(x, .), m = S(x, d)
 *     and s2 = min S(x, d') over |d' - d| >= 2, the pixel is rejected iff such a d' exists and s2 * (100 - u) < m * 100.  A rejected
 *     pixel carries a marker (255; 65535 in the sub-pixel map) through the 3 x 3 median — as the largest value: an isolated rejection
 *     is replaced by its neighbourhood's median, a rejected patch stays — and leaves the left-right check as -1.
 *   speckle_size / speckle_range (the last stage, on the float plane): pixels that are finite and >= 0 take part; 4-neighbours that
 *     both take part are linked iff fabsf(a - b) <= (float)speckle_range (pairwise, not against a seed); every pixel of a connected
 *     region of at most speckle_size pixels becomes -1. */
typedef struct ModDisparityFilters {   /* 16 bytes; all zero = off */
  int32_t uniqueness_ratio;  /* 0..99 [%]; 0 = off */
  int32_t speckle_size;      /* regions of at most this many pixels are invalidated; 0 = off; <= max_width * max_height */
  int32_t speckle_range;     /* >= 0, whole disparities: neighbours link when they differ by at most this */
  int32_t reserved;          /* must be 0 */
} ModDisparityFilters;
/* NULL = all off.  Out-of-range values and a non-zero `reserved`: MOD_ERR_INVALID_ARGUMENT, and the settings stay as they were. */
int  mod_set_disparity_filters(ModContext *ctx, const ModDisparityFilters *filters);
int  mod_get_disparity_filters(const ModContext *ctx, ModDisparityFilters *filters);
/* Minimum-disparity offset, opt-in (minDisparity of StereoBM / StereoSGBM, min_disparity of stereo_image_proc): context state like
 * the sub-pixel mode, read when a call or a submit enqueues its estimator (the same five entry points) and by mod_sgm_path_dev; a
 * frame in flight completes with the offset of its own submit.  0 (the default): the window [0, disparities), the kernels and the
 * bytes of an estimator without the setting.  d0 in 0..128: index d in [0, disparities) of every volume and map stands for the
 * disparity d0 + d, the window is [d0, d0 + disparities).  Integer arithmetic as everywhere in the estimator
 * (tests/models/sgm_offset_model.py restates it bit for bit):
 *   matching cost   C(x, d) = popcount(cl(x) ^ cr(x - d0 - d)) if x - d0 - d >= 0, else the border cost 31.
 *   paths           unchanged over d: penalties, the first minimum dl(x) of the summed costs S(x, .), the fraction q, the uniqueness
 *                   test and the 3 x 3 median with its markers 255 / 65535.
 *   right map       dr(xr) = the first minimum over d of S(xr + d0 + d, d), taken over the d with xr + d0 + d < W; 0 if there is none.
 *   left-right      xs = x - d0 - dl(x).  With lr_check on, the pixel is valid iff xs >= 0 and |dr(xs) - dl(x)| <= 1 (the sub-pixel
 *                   mode checks (v + 8) >> 4 in dl's place); with lr_check off this rule rejects nothing, as without an offset.
 *   output          d0 + dl(x), or d0 + v / 16 in the sub-pixel mode: exact in float (at most 255.5).  An invalid pixel is -1 WHATEVER
 *                   d0 is — not min_disparity - 1: a caller whose camera keeps min_disparity 0 never sees a rejected pixel pass as a
 *                   disparity.  The estimator's speckle stage keeps its rule (>= 0 takes part, removed pixels become -1).
 *   DisparityImage  min_disparity = d0, max_disparity = d0 + disparities - 1.  The camera (mod_set_camera) is the caller's to set.
 * An image no wider than d0 is legal: every cost is 31.  Values outside 0..128: MOD_ERR_INVALID_ARGUMENT, and the offset stays as it
 * was.  MOD_SGM_MAX_DISPARITIES stays the width of the window, not its end. */
int  mod_set_disparity_offset(ModContext *ctx, int32_t min_disparity);
int  mod_get_disparity_offset(const ModContext *ctx, int32_t *min_disparity);
/* The speckle stage alone, in place, on any 32FC1 disparity planes [frames][H][W] of the camera's size (a caller's own matcher):
 * a pixel takes part iff it is finite and >= the camera's min_disparity; removed pixels become min_disparity - 1.  speckle_size 0:
 * nothing to do.  Ordered on the context's stream; scratch (8 bytes per pixel of max_frames frames) is allocated on first use.
 * NULL plane -> MOD_SKIP_NO_DISPARITY_NOW. */
int  mod_disparity_speckle_dev(ModContext *ctx, int32_t frames, float *disparity, int32_t speckle_size, int32_t speckle_range);
/* Edge-preserving smoother, opt-in: context state like the rejection filters, read when a call or a submit enqueues its estimator (the
 * same five entry points); a frame in flight completes with the setting of its own submit.  Every other stage behind the winner removes
 * disparities or copies measured words into holes; this one reduces the noise of the disparities that stay, which is what the scene flow
 * differentiates.  It works in the disparity domain, where matching noise is roughly uniform, so one gate in px serves near and far.  It
 * is the estimator's stage behind the speckle stage and in front of the hole fill (a fill then copies smoothed words).  The rule
 * (tests/models/disparity_smooth_model.py restates it bit for bit), for planes [F][H][W] float32, every step one
 * IEEE float32 operation:
 *   VALIDITY     a word w is valid iff it is finite and w >= lo.  Inside the estimator lo = 0.0f, what the hole fill uses at the same
 *                place: -1 is invalid whatever the disparity offset is, and -0.0 is valid.  In mod_disparity_smooth_dev lo is the camera's
 *                min_disparity, as in mod_disparity_fill_dev.
 *   INVALID      an invalid pixel: out = in, bit for bit — NaN payloads, +-inf and -1 pass through unchanged.  The smoother never fills a
 *                hole and never makes one.
 *   MEMBERS      for a valid pixel with word d: the valid words q of its window x window square (window 3, 5 or 7; the square is clipped
 *                to the image of the pixel's own frame, it never reaches into the next row's far end, the next frame or the plane before
 *                it) whose gate fabsf(q - d) <= tol holds, the subtraction rounded to float32.  The pixel is always its own member.
 *                n is the number of members.
 *   CONDITION    n < min_members (1..window^2): out = in, bit for bit.
 *   VALUE        otherwise sum = 0.0f; the members are added one at a time in row-major order of the window, top row first, left to
 *                right, each step sum = sum + q; out = fmaxf(sum / (float)n, lo).  The order is part of the rule (it is what makes
 *                arbitrary planes reproducible); the clamp keeps a valid pixel valid where rounding takes the mean below lo.  (A mean of
 *                -0.0 words is +0.0.  Words so large that the sum of a window's members overflows float32 give +inf: no disparity is.)
 *   SINGLE PASS  the smoother reads one plane and writes another; a smoothed pixel feeds no other pixel.
 * A gated mean also turns whole-number disparities on a slanted surface into fractions, with the sub-pixel mode off too.
 * NULL (or an all-zero struct, what the getter returns while off): off (the default) — the estimator allocates nothing, enqueues exactly
 * the kernels it did and writes the same bytes.  While on, the stages in front of the smoother work on a scratch plane of a group of
 * frames (4 bytes per pixel of the group, allocated at the first call with the smoother on, grow-only); the smoother writes the hole
 * fill's scratch plane where the fill is on and the caller's plane where it is off: no stage reads the plane it writes.  Consequences: the
 * ego-motion estimator and the gate of mod_set_flow_fill both see the SMOOTHED disparity; smoothed words are not multiples of 1/16.
 * A window other than 3, 5 or 7, a tol that is negative, NaN or infinite, min_members outside 1..window^2, a non-zero reserved:
 * MOD_ERR_INVALID_ARGUMENT, the setting stays as it was, and mod_last_error names the disparity smooth.  The defaults of the bindings
 * (window 5, tol 1, min_members 1) are not tuned on camera data. */
typedef struct ModDisparitySmooth {   /* 16 bytes; NULL: off (the default) */
  int32_t window;            /* 3, 5 or 7: the side of the square */
  int32_t min_members;       /* 1..window^2: with fewer members the pixel stays */
  float   tol;               /* >= 0, finite: the gate in px of disparity */
  int32_t reserved;          /* 0 */
} ModDisparitySmooth;
int  mod_set_disparity_smooth(ModContext *ctx, const ModDisparitySmooth *smooth);
/* as set; never set, or set with NULL: all zero */
int  mod_get_disparity_smooth(const ModContext *ctx, ModDisparitySmooth *smooth);
/* The smoother alone, on any 32FC1 disparity planes [frames][H][W] of the camera's size (a caller's own matcher) into disparity_out of
 * the same size, with lo = the camera's min_disparity.  smooth NULL: the context's.  Not in place: disparity_in == disparity_out or any
 * overlap of the planes, an invalid setting or none (nothing to do): MOD_ERR_INVALID_ARGUMENT; a NULL plane ->
 * MOD_SKIP_NO_DISPARITY_NOW.  Every pixel of disparity_out is stored, disparity_in is only read.  Ordered on the context's stream; keeps
 * no state, needs no scratch. */
int  mod_disparity_smooth_dev(ModContext *ctx, int32_t frames, const float *disparity_in, const ModDisparitySmooth *smooth, float *disparity_out);
/* Occlusion hole fill, opt-in (the "discontinuity preserving interpolation" of Hirschmueller's SGM refinement, without its
 * classification): context state like the rejection filters, read when a call or a submit enqueues its estimator (the same five entry
 * points); a frame in flight completes with the setting of its own submit.  The left-right check, the uniqueness, texture and speckle
 * rules only ever remove disparities; the check removes by design the strip left of every foreground object that the right camera
 * cannot see, and a pixel at -1 has no 3-D point, no velocity and no part in a cluster.  The fill is the LAST stage of the estimator,
 * behind the speckle stage.  The rule (tests/models/disparity_fill_model.py restates it bit for bit), for
 * planes [F][H][W] float32:
 *   VALIDITY     a word d is valid iff it is finite and d >= lo.  Inside the estimator lo = 0.0f, the speckle stage's rule: -1 is
 *                invalid whatever the disparity offset is, and -0.0 is valid.  In mod_disparity_fill_dev lo is the camera's
 *                min_disparity, as in mod_disparity_speckle_dev.
 *   SEARCH       an invalid pixel p = (x, y) walks each of the first `directions` of mod_sgm_path_dev's list, (+1,0) (-1,0) (0,+1)
 *                (0,-1) (+1,+1) (-1,-1) (-1,+1) (+1,-1): direction k visits p + s * (dx_k, dy_k) for s = 1 .. reach and stops at the
 *                first valid word v_k, or where the next step would leave the image of its own frame: a walk never wraps into the next
 *                row, the next frame or the plane before it.  n is the number of directions that found a word.
 *   CONDITION    p valid, or n < min_found: out = in, bit for bit — NaN payloads, +-inf and -1 pass through unchanged.
 *   VALUE        otherwise out is the element of rank r of the n found words in ascending order of the integer key
 *                k(b) = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000) of their bits (the flow median's order: -0.0 sorts before +0.0):
 *                MIN r = 0 (the background, the farthest surface in sight: an occlusion is never filled from the object that hides it),
 *                SECOND r = min(1, n - 1) (the paper's choice for an occlusion), MEDIAN r = (n - 1) >> 1 (its choice for a mismatch).
 *                No float arithmetic: every output word is one of the input plane's words, so a filled pixel lies inside the
 *                DisparityImage's [min_disparity, max_disparity].
 *   SINGLE PASS  the fill reads one plane and writes another; a filled pixel feeds no other fill.
 * reach 0 or NULL: off (the default) — the estimator allocates nothing, enqueues exactly the kernels it did and writes the same bytes.
 * While on, the stages in front of the fill work on a scratch plane of a group of frames (4 bytes per pixel of the group, allocated at
 * the first call with the fill on, grow-only) and the fill writes the caller's plane.  Consequences: the ego-motion estimator and the
 * gate of mod_set_flow_fill both see the FILLED disparity; the sub-pixel mode and the disparity offset need nothing special, the fill
 * copies float words.  reach outside 0..256, directions other than 2, 4 or 8, a mode other than the three, min_found outside
 * 1..directions (none of the three looked at while reach is 0): MOD_ERR_INVALID_ARGUMENT, the setting stays as it was, and
 * mod_last_error names the disparity fill. */
#define MOD_DISPARITY_FILL_MIN    0
#define MOD_DISPARITY_FILL_SECOND 1
#define MOD_DISPARITY_FILL_MEDIAN 2
typedef struct ModDisparityFill {   /* 16 bytes; NULL or reach 0: off (the default) */
  int32_t reach;             /* 0..256: the steps a direction may walk; 0 = off */
  int32_t directions;        /* 2, 4 or 8: the first so many of the list above */
  int32_t mode;              /* MOD_DISPARITY_FILL_MIN (0), _SECOND (1) or _MEDIAN (2) */
  int32_t min_found;         /* 1..directions: with fewer found words the hole stays */
} ModDisparityFill;
int  mod_set_disparity_fill(ModContext *ctx, const ModDisparityFill *fill);
/* as set; never set, or set with NULL: all zero */
int  mod_get_disparity_fill(const ModContext *ctx, ModDisparityFill *fill);
/* The fill alone, on any 32FC1 disparity planes [frames][H][W] of the camera's size (a caller's own matcher) into disparity_out of the
 * same size, with lo = the camera's min_disparity.  fill NULL: the context's.  Not in place: overlapping planes, an invalid fill or
 * reach 0 (nothing to do): MOD_ERR_INVALID_ARGUMENT; a NULL plane -> MOD_SKIP_NO_DISPARITY_NOW.  Every pixel of disparity_out is
 * stored, disparity_in is only read.  Ordered on the context's stream; keeps no state, needs no scratch. */
int  mod_disparity_fill_dev(ModContext *ctx, int32_t frames, const float *disparity_in, const ModDisparityFill *fill, float *disparity_out);
/* stages, for tests and tracing: centre-symmetric census (31 bits per pixel, 0 where the window leaves the image) ... */
int  mod_sgm_census_dev(ModContext *ctx, int32_t frames, const uint8_t *image, uint32_t *census);
/* ... and one aggregation path L_r [frames][H][W][disparities] uint8 over the Hamming cost of the census words; direction 0..7 =
 * (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,-1) (-1,+1) (+1,-1).  matching_cost (optional) receives C itself.  Both are those of
 * the disparity offset in force (mod_set_disparity_offset). */
int  mod_sgm_path_dev(ModContext *ctx, int32_t frames, const uint32_t *census_left, const uint32_t *census_right,
                      const ModSgmParams *params, int32_t direction, uint8_t *path_cost, uint8_t *matching_cost);

/* ---- on-GPU optical flow --------------------------------------------------------------------------------------------------- */
/* The reference obtains the flow from pwc_net_.estimateOpticalFlow(previous_left, left) (scene_flow_constructor.cpp:279-290), a
 * Caffe CNN whose weights this project does not have.  This estimator is NOT PWC-Net and claims no parity with it: coarse-to-fine
 * census block matching, deterministic and integer up to the sub-pixel step (tests/models/flow_model.py
 * restates it bit for bit).  Pyramid of `levels` (2 x 2 rounded mean), the SGM path's 9 x 7 census on every level, cost = sum of
 * Hamming distances over a window x window square (a prev sample outside the image costs 31), full search [-radius, radius]^2 on
 * the coarsest level and +-1 around twice the coarser winner on every finer one; largest displacement
 * radius * 2^(levels-1) + 2^(levels-1) - 1 px (39 at the defaults).  Sub-pixel: a parabola through the winner and its two
 * neighbours per axis.  Forward-backward check: the backward field must cancel the forward one within fb_check px, else NaN.
 * Output: 32FC2 (x then y) [frames][H][W][2] indexed at the NOW pixel, prev = now - flow — the `flow` every entry point above takes.
 * Images are 8-bit [frames][H][W] of the configured camera size.  Defaults: levels 4, radius 4, window 5, subpixel 1, fb_check 1. */
typedef struct ModFlowParams {
  int32_t levels;     /* 1..6; the coarsest level (W >> (levels-1), H >> (levels-1)) must be at least 16 px on either side */
  int32_t radius;     /* 1..8: search radius on the coarsest level */
  int32_t window;     /* 3, 5 or 7: matching window */
  int32_t subpixel;   /* 0 / 1: sub-pixel parabola on level 0 */
  int32_t fb_check;   /* tolerance of the forward-backward check in px; < 0 = off */
} ModFlowParams;
/* estimateOpticalFlow on device images.  Ordered on the context's stream; scratch (pyramids, census planes, integer flow planes for
 * max_width x max_height x max_frames) is allocated on first use.  frames <= max_frames and <= 32767.  NULL image ->
 * MOD_SKIP_NO_FLOW, as a failed estimateOpticalFlow. */
int  mod_flow_compute_dev(ModContext *ctx, int32_t frames, const uint8_t *prev, const uint8_t *now, const ModFlowParams *params,
                          float *flow);
/* the same for one frame in host memory; synchronous */
int  mod_flow_compute_host(ModContext *ctx, const uint8_t *prev, const uint8_t *now, const ModFlowParams *params, float *flow);
/* Neighbour-seed propagation, opt-in: context state like mod_set_disparity_filters, read when a call or a submit enqueues the flow —
 * mod_flow_compute_dev / _host, mod_submit_images_host, mod_submit_odometry_host; a frame in flight completes with the setting of
 * its own submit.  seeds 1 (the default): as described above — the estimator enqueues the kernels it always did.  seeds 5: on
 * every finer level a pixel also tries the winners of its parent's four neighbours, so a pixel near a motion boundary whose parent
 * chose the other layer's motion can still find its own (tests/models/flow_prop_model.py restates it bit
 * for bit).  The coarsest level is the same for either value.  On a finer level l (W x H; level l+1 is W1 x H1 with winners F_{l+1}),
 * for pixel (x, y):
 *   parent   (X, Y) = (min(x >> 1, W1 - 1), min(y >> 1, H1 - 1));
 *   seeds    k = 0..4 with offset (ox, oy) = (0,0), (-1,0), (+1,0), (0,-1), (0,+1); seed k's parent is
 *            (clamp(X + ox, 0, W1 - 1), clamp(Y + oy, 0, H1 - 1)) and its centre c_k = 2 F_{l+1}(that parent);
 *   winner   each seed's nine candidates c_k + [-1, 1]^2 are scored as ever, and each seed picks its own winner by the usual key
 *            (cost, then |ex| + |ey|, then raster index); the pixel's winner is the seed winner with the smallest COST, ties to the
 *            lowest k (a seed whose centre equals that of a lower k can therefore never win);
 *   sub-pixel (level 0): the terms come from the winning seed's own 3 x 3 costs; per axis both neighbours exist only when the
 *            winner is that seed's centre candidate on that axis.
 * Both directions use the rule, so the forward-backward check compares two propagated fields.  Largest displacement, pyramid,
 * census, border costs and the finishing step are unchanged; ModFlowParams keeps its layout.  Any other value:
 * MOD_ERR_INVALID_ARGUMENT, and the setting stays as it was. */
#define MOD_FLOW_SEEDS 5
int  mod_set_flow_propagation(ModContext *ctx, int32_t seeds);
int  mod_get_flow_propagation(const ModContext *ctx, int32_t *seeds);

/* ---- texture threshold of the on-GPU estimators ---------------------------------------------------------------------------- */
/* Opt-in rejection of pixels without image texture, for both estimators above (textureThreshold of StereoBM / stereo_image_proc's
 * texture_threshold in idea): where the image is flat every census word is the same, every candidate costs the same, and the
 * winner is decided by tie rules and the smoothness term.  The rule, integers throughout (tests/models/texture_model.py restates it
 * bit for bit) — for a grey plane I (uint8, W x H), a window w, a cap c and a threshold t:
 *   g(x, y) = min(|I(min(x + 1, W - 1), y) - I(max(x - 1, 0), y)|, c)      the horizontal central difference, columns CLAMPED
 *   T(x, y) = sum of g(x + i, y + j) over |i|, |j| <= (w - 1) / 2          window positions outside the image add 0
 *   rejected(x, y)  iff  T(x, y) < t
 * T <= 15 * 15 * 255 = 57375 fits a uint16.  Only the horizontal gradient counts: the vertical one says nothing about a horizontal
 * search.  Positions outside the image add 0, so the border band is rejected more readily; the census words there are 0 in both
 * images anyway.  The formula is this library's own: it is StereoBM's idea (a sum of capped horizontal gradient magnitudes over the
 * matching window), and bit parity with OpenCV's Sobel-prefiltered textureThreshold is NOT claimed.
 *
 * mod_set_texture_filter: context state like mod_set_disparity_filters, read when a call or a submit enqueues its estimator; a
 * frame in flight completes with the setting of its own submit, and the setting may change while tickets are outstanding.  NULL or
 * threshold 0: off (the default) — every entry point enqueues the kernels it always did and writes the same bytes.  With threshold 0
 * the other fields are still checked.  Out-of-range values, an even window or `apply` outside 1..3: MOD_ERR_INVALID_ARGUMENT, and
 * the setting stays as it was.
 *   apply & MOD_TEXTURE_DISPARITY  every entry point that runs the disparity estimator (mod_sgm_compute_dev / _host,
 *       mod_submit_stereo_host, mod_submit_images_host, mod_submit_odometry_host): behind the left-right check and BEFORE the speckle
 *       stage (StereoBM's order: a rejected pixel splits regions for the speckle filter), every pixel whose T of the LEFT image is below
 *       t becomes -1, the estimator's "invalid" whatever the disparity offset is.  The disparity mod_submit_depth_host converts from a
 *       depth image is not filtered: a depth sensor does not fail on flat surfaces.
 *   apply & MOD_TEXTURE_FLOW       every entry point that runs the flow estimator (mod_flow_compute_dev / _host, mod_submit_images_host,
 *       mod_submit_odometry_host, mod_submit_depth_host): behind the finishing step, every pixel whose T of the NOW image (the flow is
 *       indexed at the now pixel) is below t becomes (NaN, NaN), both words 0x7fc00000 like every other invalid flow pixel. */
#define MOD_TEXTURE_DISPARITY 1
#define MOD_TEXTURE_FLOW      2
typedef struct ModTextureFilter {   /* 16 bytes; NULL or threshold 0: off (the default) */
  int32_t threshold;                /* 0..57375 */
  int32_t window;                   /* odd, 3..15 */
  int32_t cap;                      /* 1..255 */
  int32_t apply;                    /* MOD_TEXTURE_DISPARITY | MOD_TEXTURE_FLOW, at least one */
} ModTextureFilter;
int  mod_set_texture_filter(ModContext *ctx, const ModTextureFilter *filter);
/* as set; never set, or set with NULL: {0, 9, 31, MOD_TEXTURE_DISPARITY | MOD_TEXTURE_FLOW} */
int  mod_get_texture_filter(const ModContext *ctx, ModTextureFilter *filter);
/* T itself, [frames][H][W] uint16, of grey planes [frames][H][W] of the camera's size: what one looks at to choose a threshold.
 * filter NULL: the context's; only window and cap are used and checked.  Ordered on the context's stream; keeps no state, needs no
 * scratch. */
int  mod_texture_dev(ModContext *ctx, int32_t frames, const uint8_t *grey, const ModTextureFilter *filter, uint16_t *texture);
/* The rule alone, in place, on a caller's own planes (another matcher's output), like mod_disparity_speckle_dev: where T of `grey`
 * is below the threshold, `disparity` [frames][H][W] becomes the camera's min_disparity - 1 and `flow` [frames][H][W][2] (NaN, NaN).
 * Either plane may be NULL (the planes given decide, not `apply`, which is checked all the same); both NULL, or a NULL `grey`:
 * MOD_SKIP_NO_DISPARITY_NOW.  filter NULL: the context's.  threshold 0: nothing is enqueued.  No other pixel of either plane is read
 * or written. */
int  mod_texture_reject_dev(ModContext *ctx, int32_t frames, const uint8_t *grey, const ModTextureFilter *filter, float *disparity,
                            float *flow);

/* ---- min-eigenvalue (aperture) threshold of the on-GPU optical flow -------------------------------------------------------- */
/* Opt-in rejection of flow pixels whose displacement the image does not determine in BOTH axes.  The texture rule above sums
 * horizontal gradients, which is right for a horizontal search and not for a 2-D one: a pixel on a vertical edge passes it although
 * its motion along the edge is undetermined (the aperture problem), and a pixel on a horizontal edge fails it although its vertical
 * motion is determined.  This rule asks what a 2-D tracker asks (Shi-Tomasi's measure; minEigThreshold of calcOpticalFlowPyrLK in
 * idea): whether the gradient structure tensor over the window has two large eigenvalues.  Integers throughout
 * (tests/models/corner_model.py restates it bit for bit) — for a grey plane I (uint8, W x H), an odd window
 * w, a cap c and a threshold t:
 *   gx(x, y) = clamp(I(min(x + 1, W - 1), y) - I(max(x - 1, 0), y), -c, c)     signed; columns CLAMPED as in the texture rule
 *   gy(x, y) = clamp(I(x, min(y + 1, H - 1)) - I(x, max(y - 1, 0)), -c, c)     rows CLAMPED
 *   A = sum gx^2,  B = sum gx gy,  C = sum gy^2    over |i|, |j| <= (w - 1) / 2; window positions outside the image add 0
 *   S = A + C,  D = (A - C)^2 + 4 B^2,  r = the smallest integer with r^2 >= D
 *   E(x, y) = (S - r) >> 1                 the floor of the tensor's smaller eigenvalue; S >= r always (the tensor is PSD)
 *   rejected(x, y)  iff  E(x, y) < t       equivalently, with no square root: not (S - 2 t >= 0 and (S - 2 t)^2 >= D)
 * A, C and |B| are at most 225 * 255^2 = 14630625 = MOD_CORNER_MAX (int32), so is E (stored as uint32); D is below 1.1e15 (int64, and
 * below 2^53).  E = 0 on a flat image and on stripes or a step edge of either direction.  The formula is this library's own: bit
 * parity with OpenCV's cornerMinEigenVal is NOT claimed.
 *
 * mod_set_flow_corner_filter: context state like mod_set_texture_filter, read when a call or a submit enqueues the flow estimator; a
 * frame in flight completes with the setting of its own submit, and the setting may change while tickets are outstanding.  NULL or
 * threshold 0: off (the default) — every entry point enqueues the kernels it always did and writes the same bytes.  With threshold 0
 * the other fields are still checked.  Out-of-range values, an even window or reserved != 0: MOD_ERR_INVALID_ARGUMENT, the setting
 * stays as it was, and mod_last_error names the corner filter.  Every entry point that runs the flow estimator (mod_flow_compute_dev /
 * _host, mod_submit_images_host, mod_submit_odometry_host, mod_submit_depth_host): behind the finishing step, and behind the texture
 * rule when that is on, every pixel whose E of the NOW image is below t becomes (NaN, NaN), both words 0x7fc00000.  The rule stores
 * only where it rejects and never reads the flow, so its order against the texture rule changes no byte.  The ego-motion estimator
 * below skips non-finite flow and is unchanged: with the filter on, its correspondences are the pixels whose flow the image
 * determines in both axes. */
#define MOD_CORNER_MAX 14630625
typedef struct ModCornerFilter {   /* 16 bytes; NULL or threshold 0: off (the default) */
  int32_t threshold;               /* 0..MOD_CORNER_MAX */
  int32_t window;                  /* odd, 3..15; default 9 */
  int32_t cap;                     /* 1..255; default 31 */
  int32_t reserved;                /* must be 0 */
} ModCornerFilter;
int  mod_set_flow_corner_filter(ModContext *ctx, const ModCornerFilter *filter);
/* as set; never set, or set with NULL: {0, 9, 31, 0} */
int  mod_get_flow_corner_filter(const ModContext *ctx, ModCornerFilter *filter);
/* E itself, [frames][H][W] uint32, of grey planes [frames][H][W] of the camera's size: what one looks at to choose a threshold.
 * filter NULL: the context's; only window and cap are used and checked.  A NULL grey or strength plane: MOD_ERR_INVALID_ARGUMENT.
 * Ordered on the context's stream; keeps no state, needs no scratch. */
int  mod_flow_corner_dev(ModContext *ctx, int32_t frames, const uint8_t *grey, const ModCornerFilter *filter, uint32_t *strength);
/* The rule alone, in place, on a caller's own flow [frames][H][W][2] (another matcher's output): where E of `grey` is below the
 * threshold the pixel becomes (NaN, NaN).  A NULL `grey` or `flow`: MOD_SKIP_NO_FLOW.  filter NULL: the context's.  threshold 0:
 * nothing is enqueued.  No other pixel is read or written. */
int  mod_flow_corner_reject_dev(ModContext *ctx, int32_t frames, const uint8_t *grey, const ModCornerFilter *filter, float *flow);

/* ---- NaN-aware median filter of the on-GPU optical flow --------------------------------------------------------------------- */
/* Opt-in post-filter of the finished flow.  The forward-backward check and the two rules above remove vectors the image cannot
 * determine; none removes a vector the image did determine, wrongly — the isolated outlier a block matcher leaves inside a smooth
 * field, which the dynamic test downstream turns into a "moving" pixel.  The cure is the small median every classical flow pipeline
 * carries behind its matcher (cv::medianBlur on the two channels in idea; bit parity with it is NOT claimed: this one knows invalid
 * pixels and clips its window).  The rule (tests/models/flow_median_model.py restates it bit for bit):
 *   A flow pixel is VALID when both of its components are finite; any NaN or +-inf makes it invalid (the rule mod_flow_image_dev
 *   draws black by).  For a pixel p of frame f let S be the valid pixels of the window x window square centred on p, CLIPPED to the
 *   image — no replication, no wrap, no other frame — and n = |S|.
 *     p invalid:                  the output pixel is the input pixel, bit for bit, both words, payloads included: no hole is filled
 *     p valid and n < min_valid:  the output is (NaN, NaN), both words 0x7fc00000, as the texture and corner rules write it
 *     otherwise:                  out.x is the LOWER MEDIAN of the x components of S and out.y the lower median of the y components,
 *                                 taken independently: the element of index (n - 1) / 2 (integer division) in ascending order
 *   "Ascending" is the order of the integer key k(b) = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000) of the float's 32 bits b, compared
 *   as uint32: for finite floats the numeric order with -0.0 before +0.0.  It does not depend on denormal flushing and makes the
 *   selected BIT PATTERN unique: every output word of a filtered pixel is one of the input words of S.
 * window: 0 (off, the default), 3 or 5.  min_valid: 0 .. window^2; 0 and 1 mean "no isolation test" (a valid p counts itself).
 *
 * mod_set_flow_median: context state like mod_set_flow_corner_filter, read when a call or a submit enqueues the flow estimator; a
 * frame in flight completes with the setting of its own submit.  NULL or window 0: off — every entry point enqueues the kernels it
 * always did, allocates nothing and writes the same bytes.  A window other than 0 / 3 / 5, min_valid outside 0 .. window^2 or a
 * non-zero reserved word: MOD_ERR_INVALID_ARGUMENT, the setting stays as it was, and mod_last_error names the flow median.  Every
 * entry point that runs the flow estimator (mod_flow_compute_dev / _host, mod_submit_images_host, mod_submit_odometry_host,
 * mod_submit_depth_host) filters LAST, behind the finishing step, the texture rule and the min-eigenvalue rule, so that a rejected
 * vector never votes: those write a scratch plane of max_frames x max_width x max_height x 8 bytes (allocated at the first call with
 * the filter on, never when off), and the filter writes the caller's plane.  The ego-motion and the scene flow of the odometry and
 * depth streams consume the filtered flow. */
typedef struct ModFlowMedian {     /* 16 bytes; NULL or window 0: off (the default) */
  int32_t window;                  /* 0, 3 or 5 */
  int32_t min_valid;               /* 0 .. window * window */
  int32_t reserved[2];             /* must be 0 */
} ModFlowMedian;
int  mod_set_flow_median(ModContext *ctx, const ModFlowMedian *filter);
/* as set; never set, or set with NULL: {0, 0, {0, 0}} */
int  mod_get_flow_median(const ModContext *ctx, ModFlowMedian *filter);
/* The filter alone, on a caller's own flow [frames][H][W][2] (another matcher's output) into flow_out of the same size.  filter NULL:
 * the context's.  A stencil cannot run in place: flow_in and flow_out must not overlap.  A NULL plane, overlapping planes, an invalid
 * filter or window 0 (nothing to do): MOD_ERR_INVALID_ARGUMENT.  Every pixel of flow_out is stored; flow_in is only read.  Ordered on
 * the context's stream; keeps no state, needs no scratch. */
int  mod_flow_median_dev(ModContext *ctx, int32_t frames, const float *flow_in, const ModFlowMedian *filter, float *flow_out);

/* ---- disparity-gated hole fill of the on-GPU optical flow ------------------------------------------------------------------- */
/* Opt-in last stage of the flow in the submits that hold the same frame's disparity.  The forward-backward check, the texture rule,
 * the min-eigenvalue rule and the median above only ever remove vectors; the scene flow gives a pixel without a vector no velocity
 * and the clusterer counts it as static.  The rejections fall on the border of a moving object (occluded or revealed background)
 * and on its flat interior, the pixels the windowed clusterer needs.  A blind fill would carry motion across the object's edge, so a
 * hole is filled only from valid neighbours ON THE SAME SURFACE: those whose disparity lies within a gate of the hole's own.  The
 * rule (tests/models/flow_fill_model.py restates it bit for bit), for a flow [F][H][W][2] float32 and the
 * disparity planes of the same frames [F][H][W] float32:
 *   A flow pixel is VALID when both of its components are finite (mod_flow_median_dev's definition).  A disparity word d is VALID
 *   when it is finite and d > 0: the rejected pixels' -1, 0, NaN and +-inf are invalid; the camera's range is not consulted.
 *   The gate of a pixel p with disparity d_p is g = tol_abs + tol_rel * d_p, computed as two float32 operations, a multiply and then
 *   an add, each rounded (never one fma).  A neighbour q PASSES when the float32 result of fabsf(d_q - d_p) is <= g.
 *   S is the set of pixels q != p of the window x window square centred on p, CLIPPED to the image — no replication, no wrap, no
 *   other frame — that have a valid flow, a valid disparity and pass the gate; n = |S|.
 *     p valid:                                        the output pixel is the input pixel, both words, bit for bit: the fill never
 *                                                     changes a measured vector
 *     p invalid with an invalid disparity, or n < min_valid:  the same: NaN payloads and +-inf stay exactly as they came
 *     any other invalid p:                            FILLED: out.x is the LOWER MEDIAN of the x components of S and out.y the lower
 *                                                     median of the y components, each taken on its own: the element of index
 *                                                     (n - 1) / 2 (integer division) in ascending order of the key
 *                                                     k(b) = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000) of the float's bits, the
 *                                                     median filter's order.  Every filled word is one of the input words of S.
 *   ONE PASS: the fill reads the input plane and writes another; a filled pixel never feeds another fill, nothing cascades.
 * window: 0 (off, the default), 3, 5 or 7.  min_valid: 1 .. window^2 - 1 (not looked at while window is 0).  tol_abs, tol_rel:
 * finite, >= 0, in disparity pixels / per disparity pixel.
 *
 * mod_set_flow_fill: context state like mod_set_flow_median, read when a submit is made; a frame in flight completes with the setting
 * of its own submit.  NULL or window 0: off — every entry point enqueues the kernels it always did, allocates nothing and writes the
 * same bytes.  A window other than 0 / 3 / 5 / 7, min_valid out of range, a negative or non-finite tolerance or a non-zero reserved
 * word: MOD_ERR_INVALID_ARGUMENT, the setting stays as it was, and mod_last_error names the flow fill.  While on, the fill runs in the
 * three submits that hold the flow and the same frame's disparity in HBM: mod_submit_images_host, mod_submit_odometry_host and
 * mod_submit_depth_host.  It is the LAST flow stage, behind the median, and reads the disparity of the NOW frame, the pixel the flow is
 * addressed at.  In the odometry and depth streams it runs behind the ego-motion estimate, which sees measured vectors only (a filled
 * vector is a copy of a measured one and would vote twice), and in front of the scene flow, which sees the filled flow.  The flow
 * plane a submit hands back (flow_out) is the FILLED one.  The measured flow goes to a plane of max_width x max_height x 8 bytes,
 * allocated at the first submit with the fill on and never when off.  mod_flow_compute_dev / _host have no disparity and are NOT
 * affected, and neither is mod_submit_stereo_host, whose flow is the caller's. */
typedef struct ModFlowFill {       /* 24 bytes; NULL or window 0: off (the default) */
  int32_t window;                  /* 0, 3, 5 or 7 */
  int32_t min_valid;               /* 1 .. window * window - 1 */
  float   tol_abs, tol_rel;        /* finite, >= 0; disparity pixels */
  int32_t reserved[2];             /* must be 0 */
} ModFlowFill;
int  mod_set_flow_fill(ModContext *ctx, const ModFlowFill *fill);
/* as set; never set, or set with NULL: all zero */
int  mod_get_flow_fill(const ModContext *ctx, ModFlowFill *fill);
/* The fill alone, on a caller's own flow [frames][H][W][2] and the disparity planes [frames][H][W] of the same frames, into flow_out
 * of the flow's size.  fill NULL: the context's.  A stencil cannot run in place: flow_in and flow_out must not overlap.  A NULL
 * plane, overlapping planes, an invalid fill or window 0 (nothing to do): MOD_ERR_INVALID_ARGUMENT; before a camera is set:
 * MOD_ERR_NOT_CONFIGURED.  Every pixel of flow_out is stored; flow_in and disparity are only read.  Ordered on the context's stream;
 * keeps no state, needs no scratch. */
int  mod_flow_fill_dev(ModContext *ctx, int32_t frames, const float *flow_in, const float *disparity, const ModFlowFill *fill,
                       float *flow_out);

/* ---- on-GPU stereo ego-motion ---------------------------------------------------------------------------------------------- */
/* The reference obtains transform_prev2now_ from libviso2 (VisualOdometryStereo::process + getMotion(),
 * scene_flow_constructor.cpp:214-256), sparse features matched in four images on the CPU.  This estimator is NOT libviso2 and
 * claims no parity with it: it keeps libviso2's model (RANSAC, then Gauss-Newton on the stereo reprojection error of previous-frame
 * 3D points seen in the current pair) and its output convention (motion prev -> now, P_now = R P_prev + t), but works from the
 * dense correspondences already in HBM: disparity_prev, disparity_now and the flow of the frame.  Deterministic; integer stages
 * bit-exact with tests/models/ego_model.py, which restates every step:
 *   correspondences  now pixels on a `stride` grid with valid disparity now, finite flow, prev pixel roundf(x - flow) in the image
 *                    with valid disparity; valid = finite, >= max(camera min_disparity, min_disparity), <= max_disparity, > 0
 *   hypotheses       `hypotheses` triples drawn by splitmix64(seed, h, k); closed-form triad alignment of prev and now points
 *   scoring          inlier = all three residuals (left u, v, right u) of the moved point below inlier_threshold px; most inliers
 *                    wins, ties to the lowest h
 *   refinement       Gauss-Newton (rotation vector + t) on the best hypothesis's inliers, inliers selected again, Gauss-Newton
 *                    again; at most `iterations` steps in all; fixed-order f64 sums
 * The transform is the quaternion of tf2::Matrix3x3::getRotation (host/messages.hpp transform_from_motion), as the reference
 * hands construct() (scene_flow_constructor.cpp:248-249).  Failure: status != MOD_EGO_OK and an all-NaN transform. */
#define MOD_EGO_OK           0
#define MOD_EGO_FEW_POINTS   1   /* fewer than max(3, min_inliers) correspondences */
#define MOD_EGO_FEW_INLIERS  2   /* best (or refined) inlier count below min_inliers */
#define MOD_EGO_DIVERGED     3   /* singular or non-finite Gauss-Newton system */
#define MOD_EGO_MAX_HYPOTHESES 4096
typedef struct ModEgoParams {   /* defaults: 4, 256, 10, 50, 2.0f, 1.0f, 0, 0 */
  int32_t  stride;              /* 1..64: grid step of the now pixels */
  int32_t  hypotheses;          /* 1..MOD_EGO_MAX_HYPOTHESES */
  int32_t  iterations;          /* 0..100 Gauss-Newton steps in all */
  int32_t  min_inliers;         /* >= 0 */
  float    inlier_threshold;    /* > 0, px */
  float    min_disparity;       /* finite: correspondences need a larger disparity (far points carry little translation) */
  uint32_t seed;                /* RANSAC draws; independent of the frame's place in a batch */
  int32_t  reserved;
} ModEgoParams;
typedef struct ModEgoResult {
  int32_t status;               /* MOD_EGO_* */
  int32_t correspondences;
  int32_t inliers;              /* of the final motion (on failure: the count that failed) */
  int32_t iterations;           /* Gauss-Newton steps taken */
  double  rms_px;               /* rms of the inliers' residuals (NaN on failure) */
} ModEgoResult;
/* Device planes [frames][H][W] (flow [frames][H][W][2]); transforms: device [frames]; results: device [frames] or NULL.  Ordered on
 * the context's stream; scratch is allocated on first use (grows to the smallest stride seen).  NULL plane -> the skip code of
 * construct()'s guard for it (MOD_SKIP_NO_DISPARITY_PREV / _NOW, MOD_SKIP_NO_FLOW). */
int  mod_egomotion_dev(ModContext *ctx, int32_t frames, const float *disparity_prev, const float *disparity_now, const float *flow,
                       const ModEgoParams *params, ModTransform *transforms, ModEgoResult *results);
/* one frame in host memory; synchronous; MOD_SKIP_NO_TRANSFORM when the estimate failed (transform NaN, result says why) */
int  mod_egomotion_host(ModContext *ctx, const float *disparity_prev, const float *disparity_now, const float *flow,
                        const ModEgoParams *params, ModTransform *transform, ModEgoResult *result);

/* ---- camera images: encodings, windows, grey on the GPU --------------------------------------------------------------------- */
/* The reference subscribes to image_rect_color (bgr8 / rgb8 / bgra8, rows possibly padded) and converts with
 * cv_bridge::toCvCopy(..., MONO8) (scene_flow_constructor.cpp:220-221); its ZED launch crops a centred window first
 * (image_crop.cpp:24-40).  A ModImageLayout describes such a message and the camera-sized window (the context's W x H) taken from
 * it.  Grey = OpenCV's 8-bit BGR2GRAY, (1868 B + 9617 G + 4899 R + 8192) >> 14 (B = G = R = v gives v); alpha is ignored.
 * Packed YUV 4:2:2, what a UVC camera delivers without a vendor SDK, is taken as it arrives: two bytes per pixel, step >= 2 * width;
 * MOD_ENCODING_YUV422 (ROS "yuv422") is UYVY, bytes U0 Y0 V0 Y1, the luma of pixel x is byte 2x + 1 of its row;
 * MOD_ENCODING_YUV422_YUY2 ("yuv422_yuy2") is YUYV, bytes Y0 U0 Y1 V0, the luma of pixel x is byte 2x.  Grey = Y, unchanged (what
 * cv_bridge's COLOR_YUV2GRAY_UYVY / _YUY2 and image_proc's image_mono do); chroma is never read, and any width and x0 is legal, odd
 * ones included.  Under rectification Y is interpolated as one channel, like mono8: parity with "convert to BGR, rectify, convert to
 * grey" is not claimed.
 * 8-bit Bayer mosaics, what an industrial or MIPI sensor delivers, are demosaiced straight to grey: MOD_ENCODING_BAYER_RGGB8 /
 * _BGGR8 / _GBRG8 / _GRBG8 (ROS "bayer_rggb8", ...), one byte per pixel, step >= width, width >= 3 and height >= 3.  For
 * bayer_ABCD8, pixel (x, y) of the MESSAGE carries the colour ABCD[2 (y & 1) + (x & 1)].  With p(x, y) the message byte and
 * kR = 4899, kG = 9617, kB = 1868 (the grey weights above), an interior pixel (1 <= x <= width - 2, 1 <= y <= height - 2) is, in
 * uint32 arithmetic,
 *   at an R or B site (own weight kc, the opposite colour's ko):
 *       v = (4 p(x,y) kc + (the four edge neighbours' sum) kG + (the four diagonal neighbours' sum) ko + 32768) >> 16
 *   at a G site (kh: the weight of the colour that shares its row, kv: of the one that shares its column):
 *       v = (2 p(x,y) kG + (p(x-1,y) + p(x+1,y)) kh + (p(x,y-1) + p(x,y+1)) kv + 16384) >> 15
 * which is bilinear demosaicing and the grey above with a single rounding; a pixel of the message's one-pixel frame copies the
 * nearest interior result, v(clamp(x, 1, width - 2), clamp(y, 1, height - 2)).  The window is the message's demosaic, cropped
 * (debayer, then crop): a pixel at the window's edge uses the message's pixels outside the window, x0 and y0 of either parity are
 * legal, and only the message's own edge is a border.  Side by side (below), each pane is a message of its own: the colour at the
 * right pane's (0, 0) is the message's colour at column `width` (an odd width shifts the pattern by one column), the frame rule
 * applies at the pane's edges, and no output pixel of one eye depends on a byte of the other.  Under rectification the whole
 * message (or pane) is demosaiced to grey by this rule and then rectified as mono8 of step `width`.  This is the arithmetic of this
 * library; bit parity with OpenCV's Bayer conversions is not claimed.
 *   mod_set_image_layout   the layout of the HOST images every *_host image entry point reads (mod_sgm_compute_host,
 *                          mod_flow_compute_host, mod_submit_stereo_host, mod_submit_images_host, mod_submit_odometry_host),
 *                          read at call time like mod_set_params: a frame in flight completes with the layout of its own submit.
 *                          NULL = mono8, packed, W x H, origin 0 (the layout of a context that never set one).  Only the window
 *                          crosses PCIe (a Bayer window with its one-pixel apron, clamped to the message or pane); mono8 is copied
 *                          straight into the estimator's buffer, colour and Bayer are converted on the GPU.
 *   mod_get_image_layout   the layout in force (the NULL layout spelled out)
 *   mod_image_to_mono_dev  device frames stacked at step * height bytes -> grey planes [frames][H][W]; layout NULL = the context's.
 *                          Ordered on the context's stream.  NULL src -> MOD_SKIP_NO_DISPARITY_NOW, like a NULL image elsewhere.
 *                          It has no eye: for the right pane of side-by-side frames (below) the caller passes src + width * channels
 *                          (Bayer: and, for an odd width, the encoding as it lies there: rggb <-> grbg, bggr <-> gbrg); the
 *                          Bayer region is width x height at src, so the pane's edges are borders.
 * MOD_ERR_INVALID_ARGUMENT: unknown encoding, step < width * channels, a window that does not fit inside the message, a Bayer
 * layout with width < 3 or height < 3;
 * MOD_ERR_NOT_CONFIGURED: no camera yet (the window size is the camera's). */
#define MOD_ENCODING_MONO8 0
#define MOD_ENCODING_BGR8  1
#define MOD_ENCODING_RGB8  2
#define MOD_ENCODING_BGRA8 3
#define MOD_ENCODING_RGBA8 4
#define MOD_ENCODING_YUV422 5        /* UYVY */
#define MOD_ENCODING_YUV422_YUY2 6   /* YUYV */
#define MOD_ENCODING_BAYER_RGGB8 16  /* 8-bit Bayer mosaics, one byte per pixel; 7..15 and anything above 19 are unknown */
#define MOD_ENCODING_BAYER_BGGR8 17
#define MOD_ENCODING_BAYER_GBRG8 18
#define MOD_ENCODING_BAYER_GRBG8 19
typedef struct ModImageLayout {   /* 24 bytes */
  int32_t encoding;               /* MOD_ENCODING_* */
  int32_t width, height;          /* of the message (sensor_msgs/Image width, height); side by side: of one eye's pane */
  int32_t step;                   /* bytes per row, >= width * channels (side by side: of the whole row, >= 2 * width * channels) */
  int32_t x0, y0;                 /* top-left of the window taken; the window is the context's W x H */
} ModImageLayout;
int  mod_set_image_layout(ModContext *ctx, const ModImageLayout *layout);
int  mod_get_image_layout(const ModContext *ctx, ModImageLayout *layout);
int  mod_image_to_mono_dev(ModContext *ctx, int32_t frames, const uint8_t *src, const ModImageLayout *layout, uint8_t *mono);

/* ---- side-by-side stereo messages ------------------------------------------------------------------------------------------- */
/* A stereo head used as a plain UVC device delivers both eyes in ONE frame, the left half and the right half of every row.  Opt-in
 * context state like mod_set_disparity_subpixel: read at submit time, a frame in flight keeps the setting of its submit, and it may
 * change while tickets are outstanding.  on: 0 = off (the default; every call enqueues exactly what it did before), 1 = on.
 * While on, one message holds both eyes:
 *   - the layout's width and height describe ONE eye's image (what that eye's CameraInfo and, with a rectification, its
 *     calibration state); step is the pitch of the WHOLE row and must be >= 2 * width * channels;
 *   - the left eye's pane starts at byte 0 of each row, the right eye's at byte width * channels; (x0, y0) is the window inside a
 *     pane, the same for both eyes;
 *   - mod_sgm_compute_host, mod_submit_stereo_host, mod_submit_images_host and mod_submit_odometry_host take the message in `left`;
 *     `right` must be NULL or equal to `left` (anything else: MOD_ERR_INVALID_ARGUMENT); a NULL `left` skips as it always did;
 *   - mod_flow_compute_host reads the left pane of both of its messages (this follows from the layout);
 *   - without a rectification the two windows are copied, one from each pane: only the windows cross PCIe.  With one, the message
 *     crosses PCIe ONCE (height * step bytes) and is rectified twice, the left pane with the left map and the right pane with the
 *     right one; a tap outside a pane reads 0, never the other eye's pixel;
 *   - mod_rectify_dev: `eye` also selects the pane; frames > 1 are whole messages stacked at height * step bytes.
 * mod_set_side_by_side(1) under a layout whose step < 2 * width * channels (the default layout, mono8 packed at the camera's size, is
 * one), and such a layout (mod_set_image_layout, or one handed to mod_rectify_dev / mod_image_to_mono_dev) while on:
 * MOD_ERR_INVALID_ARGUMENT, the state stays
 * as it was.  Before a camera is set there is no layout to check: the check is then made at call time.  The rectification maps are
 * per eye and do not depend on this setting. */
int  mod_set_side_by_side(ModContext *ctx, int32_t on);
int  mod_get_side_by_side(const ModContext *ctx, int32_t *on);

/* ---- binning: camera images reduced by an integer factor ---------------------------------------------------------------------- */
/* image_proc/crop_decimate's step on the GPU: a 1080p or 2K stereo head runs the estimators at half resolution, so that
 * MOD_SGM_MAX_DISPARITIES spans twice as many full-resolution pixels and every per-pixel stage costs a quarter, without giving up
 * field of view as a crop does.  Opt-in context state like mod_set_side_by_side: read when a call or a submit is made, a frame in
 * flight completes with the binning of its own submit, and while off (the default) every call enqueues exactly what it did before.
 * One definition for every input path.  Let G be the full-resolution grey window that the path without binning would produce for a
 * camera of (bx W) x (by H) at the layout's (x0, y0): mono8, colour and YUV through the grey conversion above; Bayer through the
 * demosaic above (debayer, then crop, then bin: the rule for the window's edge applies to the FULL window); under a rectification,
 * the rectifier with a map of (bx W) x (by H) entries for that window.  The context's W x H image is then, in integers,
 *   MOD_BIN_MEAN     out(X, Y) = (sum over j < by, i < bx of G(bx X + i, by Y + j) + ((bx by) >> 1)) / (bx by)
 *                    (2 x 2: (a + b + c + d + 2) >> 2; half-way sums round up; cv::INTER_AREA at an integer factor)
 *   MOD_BIN_NEAREST  out(X, Y) = G(bx X, by Y)      (the block's top-left pixel: crop_decimate's default, interpolation NN)
 * tests/models/binning_model.py restates both.
 *   - Layouts: the layout's width, height, step, x0 and y0 keep describing the MESSAGE; the window taken from it is (bx W) x (by H),
 *     and that window must fit.  The default layout while binning is on is mono8 packed at (bx W) x (by H).
 *   - Side by side: each pane is binned on its own; no output pixel of one eye depends on a byte of the other.
 *   - Rectification: mod_rectify_map_host returns the full-window map [by H][bx W][2]; the cached map is keyed by the full window's
 *     size, so a change of binning that changes it forces a rebuild, which is refused while tickets are outstanding (the rule of the
 *     rectifier).  Without a rectification the binning may change between submits, like the layout.
 *   - Every *_host image call and every stereo, images, odometry and depth submit reads it; so do mod_image_to_mono_dev and
 *     mod_rectify_dev, whose output stays [frames][H][W].  The _dev estimator calls take grey planes and are untouched.
 *   - The camera given to mod_set_camera is the BINNED one (what image_geometry does with binning_x / binning_y): with the
 *     full-resolution P, fx_b = fx / bx, fy_b = fy / by, Tx_b = Tx / bx, Ty_b = Ty / by, disp_f_b = disp_f / bx;
 *     MOD_BIN_NEAREST: cx_b = (cx - x0) / bx, cy_b = (cy - y0) / by; MOD_BIN_MEAN: cx_b = (cx - x0 - (bx - 1) / 2) / bx,
 *     cy_b = (cy - y0 - (by - 1) / 2) / by (the block's centre).
 *   - Depth images are not binned by THIS setting: mod_submit_depth_host bins the image, and the depth message must match the binned
 *     camera, be reduced by mod_set_depth_decimation (below, a reduction of its own that knows about validity), or go through
 *     mod_set_depth_registration, whose scatter lands in whatever size the image camera has.
 *   - Capacity: bx W <= ModConfig.max_width and by H <= ModConfig.max_height, else MOD_ERR_CAPACITY; checked when the binning is
 *     set if a camera is known, and again at call time (the camera may have changed).
 *   mod_set_image_binning  NULL, or bx = by = 1 with either mode: off.  A factor outside 1..4, an unknown mode or a non-zero
 *                          `reserved`: MOD_ERR_INVALID_ARGUMENT, and the setting stays as it was.
 *   mod_get_image_binning  the binning in force (as it was set; never set, or set to NULL: bx = by = 1, MOD_BIN_MEAN) */
#define MOD_BIN_MEAN    0   /* rounded box mean (cv::INTER_AREA at an integer factor) */
#define MOD_BIN_NEAREST 1   /* the block's top-left pixel (crop_decimate's default, interpolation NN) */
typedef struct ModImageBinning {  /* 16 bytes; NULL or bx = by = 1: off (the default) */
  int32_t bx, by;                 /* 1..4 each */
  int32_t mode;                   /* MOD_BIN_* */
  int32_t reserved;               /* must be 0 */
} ModImageBinning;
int  mod_set_image_binning(ModContext *ctx, const ModImageBinning *binning);
int  mod_get_image_binning(const ModContext *ctx, ModImageBinning *binning);

/* ---- raw camera images: rectification on the GPU ---------------------------------------------------------------------------- */
/* The reference's launch files subscribe to image_rect_color: something upstream (image_proc, the ZED SDK) has rectified.  With a
 * rectification set, the library does that step itself, so the *_host image entry points take RAW, distorted messages.  Opt-in,
 * context state like the image layout; off by default, and while off every call enqueues exactly what it did before.
 * A ModRectifyCamera is what the sensor_msgs/CameraInfo of the raw image carries: width, height (the raw message's size, which is also
 * the rectified image's, as image_proc makes it); K (fx = K[0], fy = K[4], cx = K[2], cy = K[5]; the skew K[1] must be 0);
 * D = k1 k2 p1 p2 k3 k4 k5 k6 (plumb_bob: the first five, the rest 0; rational_polynomial: all eight; under
 * MOD_DISTORTION_EQUIDISTANT, below: k1 k2 k3 k4, the rest 0); R, the rectifying rotation;
 * P (fx' = P[0], fy' = P[5], cx' = P[2], cy' = P[6]).  The context's W x H window at the layout's (x0, y0) is a window of the
 * RECTIFIED image (image_crop runs behind the rectifier); the P given to mod_set_camera stays the cropped one.
 * Map (f64, built on the GPU by k_rectify_map, one lane per entry, from IEEE + - * / sqrt and rint alone; operations in this order,
 * no contraction; csrc/rectify_map.h is the one definition, for device and host, and tests/models/rectify_model.py restates it bit
 * for bit), for window pixel (u, v) with U = u + x0, V = v + y0:
 *   x = (U - cx') / fx';  y = (V - cy') / fy'
 *   X = R[0]*x + R[3]*y + R[6];  Y = R[1]*x + R[4]*y + R[7];  Wd = R[2]*x + R[5]*y + R[8];  x = X / Wd;  y = Y / Wd
 *   x2 = x*x; y2 = y*y; r2 = x2 + y2; xy2 = 2.0*x*y
 *   kr = (1.0 + ((k3*r2 + k2)*r2 + k1)*r2) / (1.0 + ((k6*r2 + k5)*r2 + k4)*r2)
 *   xd = x*kr + p1*xy2 + p2*(r2 + 2.0*x2);  yd = y*kr + p1*(r2 + 2.0*y2) + p2*xy2
 *   mx = fx*xd + cx;  my = fy*yd + cy;  qx = rint(mx * 32.0), qy = rint(my * 32.0)   (half to even)
 * clamped to [-2^24, 2^24], a non-finite value becomes -2^24: cv::initUndistortRectifyMap on cv::remap's 1/32-pixel grid (parity
 * with a particular OpenCV build is not claimed).
 * Under MOD_DISTORTION_EQUIDISTANT (mod_set_distortion_model; fisheye lenses, Kannala-Brandt, cv::fisheye, D = k1 k2 k3 k4) the lines
 * from x2 to yd are replaced by (tests/models/fisheye_model.py restates it bit for bit):
 *   if !(Wd > 0.0): qx = qy = -2^24                    (the ray is at or behind 90 degrees; cv::fisheye writes -inf there)
 *   r = sqrt(x*x + y*y);  if !(r <= 1048576.0): qx = qy = -2^24                    (also NaN; never inside a real image)
 *   th = atan_m(r);  t2 = th*th;  td = th * (1.0 + (((k4*t2 + k3)*t2 + k2)*t2 + k1)*t2)
 *   sc = (r == 0.0) ? 1.0 : td / r;  mx = fx*(x*sc) + cx;  my = fy*(y*sc) + cy
 * and quantised as above.  atan_m is the library's own arctangent, built from correctly rounded operations only, so that numpy, a host
 * compiler and the GPU agree in every bit (libm's and the device library's atan are not correctly rounded):
 *   t = r;  four times: t = t / (1.0 + sqrt(1.0 + t*t))                            (atan r = 16 atan t, t <= tan(pi/32))
 *   u = t*t;  s = c11;  for k = 10 .. 0: s = s*u + ck,  ck = (k even ? 1.0 : -1.0) / (double)(2k + 1);  atan_m = 16.0 * (t*s)
 * within 1.2e-15 absolute of the arctangent on [0, 2^20].  This is cv::fisheye::initUndistortRectifyMap's model on the same grid; bit
 * parity with a particular OpenCV build is not claimed here either.  The Wd and r guards apply to the equidistant model only; the
 * rational model's arithmetic is as it always was.  Sampling, all integers: ix = qx >> 5, ax = qx & 31 (the same for y); taps
 * p00 = (ix, iy), p01 = (ix+1, iy), p10 = (ix, iy+1), p11 = (ix+1, iy+1) of the raw message, a tap outside it reads 0 in every
 * channel; per channel top = (32-ax) p00 + ax p01, bot = (32-ax) p10 + ax p11, val = ((32-ay) top + ay bot + 512) >> 10; colour is
 * interpolated per channel and then converted to grey as above (image_proc rectifies the colour image, cv_bridge converts).
 *   mod_set_rectification  both NULL = off; one NULL = error.  While set, mod_sgm_compute_host, mod_submit_stereo_host,
 *                          mod_submit_images_host and mod_submit_odometry_host rectify `left` with the left map and `right` with the
 *                          right one, mod_flow_compute_host both images with the left one; the WHOLE message (height * step bytes)
 *                          crosses PCIe.  The _dev estimator calls take grey planes and are untouched.
 *   mod_get_rectification  *enabled and, when set, the calibrations (left / right may be NULL)
 *   mod_rectify_dev        as mod_image_to_mono_dev, rectified with the map of `eye`; layout NULL = the context's
 *   mod_rectify_map_host   the map of `eye` for the window of `layout` (NULL = the context's): host int32 [H][W][2] (qx, qy)
 *                          Each eye holds ONE map.  Either of these two calls with a layout whose window differs from the one the
 *                          *_host calls and submits use replaces that eye's map: the next of those rebuilds it (one short
 *                          kernel on the context's stream, no wait), and while tickets are outstanding such a call is
 *                          refused.  Trace maps with the layout in force, or on a context of their own.
 *   mod_set_distortion_model  MOD_DISTORTION_RATIONAL (the default) or MOD_DISTORTION_EQUIDISTANT: how D is read.  Context state
 *                          like mod_set_side_by_side; it holds for both eyes (a stereo head has one lens type) and is read when a
 *                          map is built.  It may be set before or after mod_set_rectification; whichever of the two calls comes
 *                          second checks the pair: equidistant with a non-zero D[4..7] in either eye is
 *                          MOD_ERR_INVALID_ARGUMENT, and so is any other value of `model`; the state stays as it was.  Changing
 *                          it invalidates both cached maps, so it is refused while tickets are outstanding.
 *   mod_get_distortion_model  the model in force
 * A map is built for the window in force (message size, x0, y0, W, H) and the distortion model, cached, and rebuilt at the next use
 * after any of those or the calibration changed.  A map that a frame in flight reads is never overwritten: mod_set_rectification,
 * mod_set_distortion_model, and any call that would rebuild a map, are refused (MOD_ERR_INVALID_ARGUMENT) while tickets are
 * outstanding; otherwise the rebuild is ordered on the context's stream behind every reader of the old map.
 * MOD_ERR_INVALID_ARGUMENT: non-finite entries; fx, fy, fx', fy' <= 0; K[1] != 0; width or height < 1 or > MOD_MAX_WIDTH; R with an
 * entry of R R^T - I above 1e-6 in magnitude (the setting stays as it was); an invalid eye; at call time a layout whose width /
 * height differ from the calibration's.  MOD_ERR_NOT_CONFIGURED: no camera, or (mod_rectify_dev, mod_rectify_map_host) no
 * rectification set. */
typedef struct ModRectifyCamera {   /* 312 bytes */
  int32_t width, height;
  double  K[9];
  double  D[8];
  double  R[9];
  double  P[12];
} ModRectifyCamera;
#define MOD_EYE_LEFT  0
#define MOD_EYE_RIGHT 1
int  mod_set_rectification(ModContext *ctx, const ModRectifyCamera *left, const ModRectifyCamera *right);
int  mod_get_rectification(const ModContext *ctx, ModRectifyCamera *left, ModRectifyCamera *right, int32_t *enabled);
int  mod_rectify_dev(ModContext *ctx, int32_t frames, const uint8_t *src, const ModImageLayout *layout, int32_t eye, uint8_t *mono);
int  mod_rectify_map_host(ModContext *ctx, int32_t eye, const ModImageLayout *layout, int32_t *map_qxqy);
#define MOD_DISTORTION_RATIONAL    0   /* plumb_bob / rational_polynomial: D = k1 k2 p1 p2 k3 k4 k5 k6 (the default; as ever) */
#define MOD_DISTORTION_EQUIDISTANT 1   /* fisheye (Kannala-Brandt, cv::fisheye): D = k1 k2 k3 k4, D[4..7] must be 0 */
int  mod_set_distortion_model(ModContext *ctx, int32_t model);
int  mod_get_distortion_model(const ModContext *ctx, int32_t *model);

/* ---- RGB-D cameras: depth images to disparity on the GPU --------------------------------------------------------------------- */
/* A RealSense, an Azure Kinect or a structured-light head delivers one image and one depth image (REP 118: 16UC1 millimetres with
 * 0 = no reading, 32FC1 metres with NaN = no reading), no stereo pair.  Everything behind the disparity ring works from disparity
 * alone, so for such a camera the estimator stage is a conversion, d = fT / z with fT the F32 product disp_f * disp_T of the camera
 * (any positive virtual baseline works; INTEGRATION.md says how to choose it).  Context state like the image layout: the depth layout
 * and the registration are read when a call or a submit is made, and a frame in flight keeps what its submit read.
 * A ModDepthLayout describes the depth message as a ModImageLayout describes an image: window pixel (u, v) reads message pixel
 * (u + x0, v + y0); frames of a batch are stacked at step * height bytes; samples are little-endian.
 * The plain path (no registration: the depth image is aligned to the image camera), all F32, -ffp-contract=off:
 *   16UC1: r = the uint16; z = (float)r * unit (one F32 multiply)          32FC1: z = value * unit
 *   unit == 0 selects the encoding's REP 118 default: 0.001f for 16UC1, 1.0f for 32FC1
 *   valid iff z > 0.0f and z is finite (0, -0.0, negatives, NaN and +-inf are not)
 *   valid: d = fT / z (the correctly rounded F32 division); invalid: d = min_disparity - 1.0f (the estimator's -1 at min_disparity 0,
 *   the convention of mod_disparity_speckle_dev).  Nothing is clipped to max_disparity: getDisparity rejects out-of-range values
 *   downstream (disparity_image_processor.cpp:25-28), and a d that underflows to 0 is rejected at :38.
 * The registered path (mod_set_depth_registration, opt-in: the depth camera has intrinsics and a pose of its own, what
 * depth_image_proc/register does on the CPU): the WHOLE depth message is scattered into a z-buffer of the context's W x H, and the
 * layout's x0, y0 must be 0.  For every message pixel (U, V) whose z is valid by the rule above, in F64, the operations in exactly
 * this order, no contraction (fx_d .. t: the registration; fx, fy, cx, cy, Tx, Ty: the context camera's, the cropped P given to
 * mod_set_camera, so results land in window coordinates; tests/models/depth_model.py restates both paths bit for bit):
 *   Z0 = (double)z;  X0 = ((U - cx_d) * Z0) / fx_d;  Y0 = ((V - cy_d) * Z0) / fy_d
 *   X = ((R[0]*X0 + R[1]*Y0) + R[2]*Z0) + t[0]      (R row-major, P_img = R P_depth + t)
 *   Y = ((R[3]*X0 + R[4]*Y0) + R[5]*Z0) + t[1];  Z = ((R[6]*X0 + R[7]*Y0) + R[8]*Z0) + t[2]
 *   drop unless Z > 0 and finite
 *   a = ((fx*X + Tx) / Z + cx) + 0.5;  b = ((fy*Y + Ty) / Z + cy) + 0.5
 *   drop unless 0 <= a < W and 0 <= b < H   (compared as doubles, before any conversion)
 *   ui = (int)floor(a); vi = (int)floor(b); zf = (float)Z (round to nearest even);  zbuf[vi][ui] = min(zbuf[vi][ui], zf)
 * The minimum is a 32-bit atomic minimum on the bit pattern of zf: positive floats order like their unsigned patterns and the
 * all-ones word stands for "empty", so the result does not depend on the order of the atomics.  Then d = fT / zbuf where a sample
 * landed and min_disparity - 1.0f where none did.  Holes are left as holes (no splatting, no fill: depth_image_proc/register's
 * default; parity with a particular depth_image_proc build is not claimed).  The z-buffer is scratch of the context's, allocated on
 * first use.
 * The footprint (mod_set_depth_splat, opt-in, off by default; depth_image_proc/register's fill_upsampling_holes): a depth camera of
 * fewer pixels than the image camera leaves a lattice of targets no sample lands on.  With the mode on, every message pixel (U, V)
 * whose z is valid and whose own Z passes "drop unless Z > 0 and finite" (a) does the above unchanged, the same drop tests and the same
 * zf, and (b) paints the target pixels whose centres lie inside the bounding box of its four projected corners, a fronto-parallel patch
 * at the sample's own Z0.  F64, no contraction, in this order:
 *   for the corners (U - 0.5, V - 0.5), (U - 0.5, V + 0.5), (U + 0.5, V - 0.5), (U + 0.5, V + 0.5), k = 0 .. 3: the chain X0 .. Z above
 *     with the corner in the place of (U, V) and the sample's Z0;  drop the footprint unless all four Z are > 0 and finite
 *   p_k = (fx*X + Tx) / Z + cx;  q_k = (fy*Y + Ty) / Z + cy                    (no + 0.5: a target is covered when its centre is inside)
 *   ulo = ceil(min(min(p0, p1), min(p2, p3)));  uhi = ceil(max(max(p0, p1), max(p2, p3))) - 1;  vlo, vhi likewise from q
 *   drop the footprint if one of the four bounds is not finite (a NaN propagates through min and max)
 *   drop it if (uhi - ulo) + 1 > MOD_DEPTH_SPLAT_MAX or (vhi - vlo) + 1 > MOD_DEPTH_SPLAT_MAX   (as doubles, BEFORE clipping: a sample
 *     that would paint more than 8 x 8 targets keeps its point alone)
 *   ulo = max(ulo, 0); uhi = min(uhi, W - 1); vlo = max(vlo, 0); vhi = min(vhi, H - 1)  (as doubles); drop it if ulo > uhi or vlo > vhi
 *   for every (u, v) of the closed rectangle [ulo, uhi] x [vlo, vhi]: zbuf[v][u] = min(zbuf[v][u], zf), the atomic minimum and the zf of (a)
 * A dropped footprint never drops the point, and a point outside the window does not drop its footprint.  The rectangle is half-open
 * in the image: at equal size and identity pose it is the sample's own pixel, at a ratio of 2 neighbouring samples tile the image.
 * Every target the point rule hits is still hit, and the result still does not depend on the order of the atomics.  Occlusion shadows
 * and pixels without a reading stay holes.  depth_image_proc's own rule paints floor(a1) .. floor(a2) inclusive and drops footprints
 * that cross the border: parity with it is not claimed.  tests/models/depth_splat_model.py restates the mode bit for bit.
 *   mod_set_depth_splat         on = 0 (the default) or 1; anything else: MOD_ERR_INVALID_ARGUMENT, the state stays as it was.  May be set
 *                               at any time; it has an effect only while a registration is in force (the plain path ignores it).  Context
 *                               state like the depth layout: read when mod_depth_to_disparity_dev is called and at the submit of
 *                               mod_submit_depth_host; a ticket in flight keeps the setting of its submit.
 *   mod_get_depth_splat         *on
 *   mod_set_depth_layout        NULL = 16UC1, packed, W x H, origin 0, unit 0 (the default)
 *   mod_set_depth_registration  NULL = off (the default).  Set the registration BEFORE a layout whose message is not the camera's
 *                               size: without one the W x H window must fit the message, with one x0 and y0 must be 0 and the
 *                               message may have any size.  Both rules are checked again when a call or a submit is made.
 *   mod_get_depth_registration  *enabled and, when set, the registration (may be NULL)
 *   mod_depth_to_disparity_dev  `frames` device depth messages -> disparity [frames][H][W] on the context's stream; layout NULL = the
 *                               context's; depth NULL: MOD_SKIP_NO_DISPARITY_NOW; `depth` must be aligned to its element size and
 *                               `disparity` to 4 bytes; frames <= ModConfig.max_frames
 * MOD_ERR_INVALID_ARGUMENT (the state stays as it was): an unknown encoding; width or height < 1 or > MOD_MAX_WIDTH; step < width *
 * 2 (or 4), not a multiple of 2 (or 4), or step * height >= 2^31; unit not finite or < 0; a window that does not fit the message;
 * non-finite registration entries, fx_d or fy_d <= 0, an entry of R R^T - I above 1e-6 in magnitude (the rectifier's rule); a
 * registration together with x0 or y0 != 0.  MOD_ERR_NOT_CONFIGURED: no camera set. */
#define MOD_DEPTH_16UC1 0
#define MOD_DEPTH_32FC1 1
typedef struct ModDepthLayout {   /* 28 bytes */
  int32_t encoding, width, height, step, x0, y0;
  float   unit;
} ModDepthLayout;
typedef struct ModDepthRegistration {   /* 128 bytes */
  double fx, fy, cx, cy;   /* the depth camera, of the full depth message; fx, fy > 0 */
  double R[9], t[3];       /* depth optical frame -> image optical frame */
} ModDepthRegistration;
int  mod_set_depth_layout(ModContext *ctx, const ModDepthLayout *layout);
int  mod_get_depth_layout(const ModContext *ctx, ModDepthLayout *layout);
int  mod_set_depth_registration(ModContext *ctx, const ModDepthRegistration *registration);
int  mod_get_depth_registration(const ModContext *ctx, ModDepthRegistration *registration, int32_t *enabled);
int  mod_depth_to_disparity_dev(ModContext *ctx, int32_t frames, const void *depth, const ModDepthLayout *layout, float *disparity);
#define MOD_DEPTH_SPLAT_MAX 8   /* targets per axis a footprint may paint */
int  mod_set_depth_splat(ModContext *ctx, int32_t on);
int  mod_get_depth_splat(const ModContext *ctx, int32_t *on);
/* A depth camera with a lens (mod_set_depth_distortion, opt-in, off by default; while it is off every call enqueues exactly what it
 * enqueues without this section).  The registered path back-projects a sample with a pinhole, which is right for a depth stream that
 * is already rectified (a RealSense) and wrong for one that is not: an Azure Kinect's depth/image_raw carries a rational_polynomial
 * CameraInfo with |k| of 3 to 6, and Kalibr-calibrated ToF and structured-light heads are in the same position.  Depth must not be
 * resampled bilinearly, so k_rectify is no help; what depth needs is the inverse lens model, an undistorted ray per depth sample, in
 * front of the z-buffer scatter.  D = k1 k2 p1 p2 k3 k4 k5 k6 as ModRectifyCamera.D under MOD_DISTORTION_RATIONAL (plumb_bob: k4 = k5 =
 * k6 = 0).  Only the rational model: an equidistant (fisheye) depth camera is not supported, because its inverse needs a
 * bit-reproducible tangent, which the library does not have (its arctangent, csrc/rectify_map.h, is the forward direction only).
 * The ray (x, y) of a lattice point (Uc, Vc) of the depth message, a pixel centre (U, V) or a pixel corner (U - 0.5, V - 0.5); F64, no
 * contraction, in exactly this order (fx_d .. cy_d: the registration's; csrc/depth_rays.h is the one definition, host and device):
 *   xd = (Uc - cx_d) / fx_d;  yd = (Vc - cy_d) / fy_d;  x = xd;  y = yd
 *   MOD_DEPTH_UNDISTORT_ITERS times:
 *     x2 = x*x; y2 = y*y; r2 = x2 + y2; xy2 = 2.0*x*y
 *     ic = (1.0 + ((k6*r2 + k5)*r2 + k4)*r2) / (1.0 + ((k3*r2 + k2)*r2 + k1)*r2)
 *     dx = p1*xy2 + p2*(r2 + 2.0*x2);  dy = p1*(r2 + 2.0*y2) + p2*xy2
 *     x = (xd - dx) * ic;  y = (yd - dy) * ic
 *   the check, the rectifier's forward lines at (x, y) in the operation order of csrc/rectify_map.h:
 *     x2 = x*x; y2 = y*y; r2 = x2 + y2; xy2 = 2.0*x*y
 *     kr = (1.0 + ((k3*r2 + k2)*r2 + k1)*r2) / (1.0 + ((k6*r2 + k5)*r2 + k4)*r2)
 *     xf = x*kr + p1*xy2 + p2*(r2 + 2.0*x2);  yf = y*kr + p1*(r2 + 2.0*y2) + p2*xy2
 *   valid iff fabs(fx_d*(xf - xd)) <= 1.0/64 and fabs(fy_d*(yf - yd)) <= 1.0/64   (a NaN fails);  invalid: x = y = NaN
 * This is the fixed-point iteration of cv::undistortPoints with a fixed count and a round-trip test; parity with an OpenCV build is
 * not claimed.  20 iterations leave at most 7e-5 px at every pixel of a 640 x 576 Kinect-like calibration (fx = fy = 504, cx = 320,
 * cy = 330, D = 5.4, 3.5, -5e-5, 1e-4, 0.18, 5.7, 5.2, 0.95; 10 iterations leave 0.05 px there) and 6e-8 px under a strong plumb-bob
 * lens (k1 = -0.28, k2 = 0.07).  With D = 0 the iteration is an exact fixed point (dx = dy = 0, ic = 1).  A lens whose forward map folds
 * inside the image has no inverse past the fold: the iteration misses the round trip there and those rays are invalid.
 * While a distortion is set the registered chain changes in one place,
 *   X0 = x * Z0;  Y0 = y * Z0      ((x, y): the ray of (U, V); REP 118 depth is measured along the optical axis, so Z0 stays as it is)
 * and a sample whose ray is invalid is dropped.  With mod_set_depth_splat on, the four corners of the footprint of (U, V) take their
 * rays from the corner lattice, points (U - 0.5, V - 0.5), (U - 0.5, V + 0.5), (U + 0.5, V - 0.5), (U + 0.5, V + 0.5) for k = 0 .. 3, at
 * the sample's own Z0; a footprint with an invalid corner ray is dropped, its point stays.  Everything after X0, Y0 is the rule above
 * word for word, so the result still does not depend on the order of the atomics.  A zero D set through this call is NOT bit-identical
 * to no distortion: ((U - cx_d) * Z0) / fx_d against ((U - cx_d) / fx_d) * Z0, the same geometry with one rounding in another place.
 * tests/models/depth_undistort_model.py restates the tables and the changed chain bit for bit.
 * The rays are tabulated: two tables of 16 bytes an entry, context scratch, built by one kernel on the context's stream at first use
 * and cached on D, on fx_d, fy_d, cx_d, cy_d and on the message's width and height; the corner table only once the splat is on (or
 * mod_depth_rays_host asks for it); freed in mod_destroy.  A table that a frame in flight reads is never overwritten (the rectifier's
 * rule): while a distortion is set and tickets are outstanding, mod_set_depth_distortion, a mod_set_depth_registration with other
 * intrinsics, a mod_set_depth_layout of another message size and any call or submit that would rebuild a table return
 * MOD_ERR_INVALID_ARGUMENT; collect every ticket first.  Without a distortion those setters behave as without this section.
 *   mod_set_depth_distortion    NULL = off (the default).  A non-finite D: MOD_ERR_INVALID_ARGUMENT, the state stays as it was.  A
 *                               distortion needs a registration (a camera whose depth is aligned to its own image passes R = I,
 *                               t = 0 and the depth intrinsics): mod_depth_to_disparity_dev, mod_depth_rays_host and
 *                               mod_submit_depth_host return MOD_ERR_INVALID_ARGUMENT while a distortion is set without one.
 *                               Context state like the registration; a ticket in flight keeps the setting of its submit.
 *   mod_get_depth_distortion    *enabled and, when set, the coefficients (d may be NULL)
 *   mod_depth_rays_host         the table the kernels read, like mod_rectify_map_host: lattice MOD_DEPTH_RAYS_CENTRES or
 *                               MOD_DEPTH_RAYS_CORNERS of the layout's message (NULL = the context's) to `rays` on the host, after a
 *                               synchronise of the context's stream.  MOD_ERR_NOT_CONFIGURED: no camera or no distortion set.
 * Not done: equidistant depth cameras; a distortion without a registration as a plain in-place path; interpolating rays from a coarse
 * table instead of tabulating every one; wiring the depth CameraInfo into the ROS node. */
typedef struct ModDepthDistortion { double D[8]; } ModDepthDistortion;   /* 64 bytes: k1 k2 p1 p2 k3 k4 k5 k6, as ModRectifyCamera.D */
int  mod_set_depth_distortion(ModContext *ctx, const ModDepthDistortion *d);
int  mod_get_depth_distortion(const ModContext *ctx, ModDepthDistortion *d, int32_t *enabled);
#define MOD_DEPTH_RAYS_CENTRES 0   /* [h][w][2] doubles: entry [V][U] is the ray of message pixel (U, V) */
#define MOD_DEPTH_RAYS_CORNERS 1   /* [h+1][w+1][2] doubles: entry [j][i] is the ray of (i - 0.5, j - 0.5) */
int  mod_depth_rays_host(ModContext *ctx, const ModDepthLayout *layout, int32_t lattice, double *rays);
#define MOD_DEPTH_UNDISTORT_ITERS 20
/* The depth filter (mod_set_depth_filter, opt-in, off by default; while it is off nothing is allocated and every call enqueues exactly
 * what it enqueues without this section).  Depth cameras report flying (mixed, shadow) pixels at depth discontinuities, samples
 * somewhere between foreground and background, and readings outside the range the sensor can be trusted in.  Both are removed on the
 * depth camera's own lattice, in front of everything else: the filter maps a depth MESSAGE to a depth message of the same encoding,
 * width, height and step, and the plain path, the registration, the splat and the distortion run unchanged on the result.  What
 * PCL's ShadowPoints, laser_filters' ScanShadowsFilter and the vendors' post-processing blocks are for; parity with none is claimed.
 * All F32, one operation at a time, -ffp-contract=off, for message pixel (U, V):
 *   z(U, V) by the rule above (16UC1: (float)r * unit; 32FC1: value * unit; unit == 0: the encoding's default);
 *   valid0 iff z > 0.0f and z is finite
 *   The range rule.  in_range iff valid0 and (z_min == 0 or z >= z_min) and (z_max == 0 or z <= z_max): both bounds inclusive
 *   The support rule (window = 3 or 5, R = window / 2), for a pixel p with in_range(p):
 *     t = tol_abs + tol_rel * z_p                                                   (one multiply, then one add)
 *     n = the number of pixels q != p with |Uq - Up| <= R, |Vq - Vp| <= R, q inside the message, in_range(q) and fabsf(z_q - z_p) <= t
 *     p is kept iff n >= min_support
 *   Support is counted on the INPUT, after the range rule only: a neighbour the support rule itself removes still supports, so the
 *   filter is one pass and does not cascade.  Pixels outside the message never support.
 *   Output: a kept sample is the input word, bit for bit.  A sample with valid0 that a rule removed becomes the encoding's "no reading"
 *   word: 0 for 16UC1, the bit pattern 0x7fc00000 for 32FC1.  A sample without valid0 (0, -0.0, negatives, NaNs of any payload, +-inf)
 *   is copied bit for bit: the filter only ever invalidates valid samples.  Bytes of a row beyond `width` samples are not defined.
 * The neighbourhood is the message's, not the window's: on the plain path with x0, y0 > 0, samples outside the W x H window but inside
 * the message support (mod_submit_depth_host sends the window's apron of R message pixels, clamped to the message, across PCIe with
 * it).  tests/models/depth_filter_model.py restates the rule word for word.
 *   mod_set_depth_filter        NULL, or z_min = z_max = 0 and window = 0: off (the default).  Context state like mod_set_depth_splat:
 *                               read when mod_depth_to_disparity_dev is called and at the submit of mod_submit_depth_host; a ticket in
 *                               flight keeps the filter of its own submit; may change while tickets are outstanding.
 *                               MOD_ERR_INVALID_ARGUMENT, the state stays as it was: a non-finite or negative z_min, z_max, tol_abs or
 *                               tol_rel; z_max != 0 and z_max < z_min; a window not in {0, 3, 5}; with window != 0 a min_support
 *                               outside 1 .. window * window - 1; a non-zero reserved.  With window == 0, min_support, tol_abs and
 *                               tol_rel are ignored, but tol_abs and tol_rel are still checked for finiteness and sign.
 *   mod_get_depth_filter        the filter in force; all zeros when it was never set or set to NULL
 *   mod_depth_filter_dev        the stage alone: `frames` device messages stacked at step * height bytes -> depth_out, same layout, on
 *                               the context's stream.  Not in place: depth_out != depth_in, and overlap is the caller's error.  layout
 *                               NULL = the context's (that needs a camera); its x0, y0 are ignored, the whole message is filtered, and
 *                               any message size passes.  filter NULL = the context's; a filter that is off copies the samples.
 *                               depth_in NULL: MOD_SKIP_NO_DISPARITY_NOW.  Both pointers aligned to the sample size;
 *                               frames <= ModConfig.max_frames.
 * The filtered messages are context scratch, allocated on first use with the filter on and freed in mod_destroy.
 * Not done: windows above 5; node parameters.  (The temporal filter and the spatial smoother with hole fill: below.) */
typedef struct ModDepthFilter {   /* 32 bytes; NULL, or z_min = z_max = 0 and window = 0: off (the default) */
  float   z_min, z_max;           /* range rule, in the units of z above (metres); 0 = that bound is off */
  int32_t window;                 /* support rule: 0 = off, else 3 or 5 */
  int32_t min_support;            /* 1 .. window * window - 1 */
  float   tol_abs, tol_rel;       /* >= 0, finite */
  int32_t reserved[2];            /* must be 0 */
} ModDepthFilter;
int  mod_set_depth_filter(ModContext *ctx, const ModDepthFilter *filter);
int  mod_get_depth_filter(const ModContext *ctx, ModDepthFilter *filter);
int  mod_depth_filter_dev(ModContext *ctx, int32_t frames, const void *depth_in, const ModDepthLayout *layout,
                          const ModDepthFilter *filter, void *depth_out);
/* The temporal depth filter with hold (mod_set_depth_temporal, opt-in, off by default; while it is off nothing is allocated and every
 * call enqueues exactly what it enqueues without this section).  The scene-flow stage differences two consecutive disparity planes, so
 * a depth camera's frame-to-frame noise goes straight into vz = dz / dt, and a pixel that drops out for a frame punches a hole into
 * both the `now` and the next `previous` plane.  This stage smooths each pixel over time where the scene stands still, restarts where it
 * changed, and can repeat a pixel's last average for a few frames.  It maps depth messages to depth messages of the same encoding,
 * width, height and step, behind the depth filter above (samples that filter removed never enter the state) and in front of the
 * registration, the distortion, the splat and the conversion.  In idea it is librealsense's temporal filter with persistence and the
 * Azure Kinect's post-processing; the rule is this library's own and parity with no SDK is claimed.
 * State, one per context, on the lattice of the messages the stage is handed, packed height x width whatever `step` is:
 *   s    F32, in raw units (the units of x below)
 *   age  u8: the consecutive frames without a reading since the last valid one; 255 = empty.  An empty pixel stores s = 0.0f.
 * The rule.  All F32, one operation at a time, -ffp-contract=off.  For a message pixel with input word w:
 *   x = (float)w for 16UC1, x = value for 32FC1;  z = x * unit (unit == 0: the encoding's default);  valid0(z) iff z > 0.0f and z is finite
 *   enc(s): 16UC1: (uint16)min(max(rintf(s), 1.0f), 65535.0f), ties to even;  32FC1: the bits of s
 * Frames of one call are consecutive in time, frame 0 oldest; calls and submits follow in program order.  Per pixel and frame:
 *   valid0 and empty state:       s = x, age = 0.  The output is w, bit for bit.
 *   valid0 and non-empty state:   zs = s * unit;  t = delta_abs + delta_rel * zs             (one multiply, then one add)
 *                                 if fabsf(z - zs) <= t:  s = s + alpha * (x - s)            (subtract, multiply, add)
 *                                 otherwise:              s = x                              (the scene changed: restart)
 *                                 in both cases age = 0 and the output is enc(s); when s == x that is the input word.
 *   not valid0, state non-empty and age < hold:   age += 1.  The output is enc(s), a held value.
 *   not valid0 otherwise:         the state becomes empty (age = 255, s = 0.0f).  The output is w, bit for bit: NaN payloads, -0.0,
 *                                 negatives and +-inf pass through, as in the depth filter.
 * Consequences: alpha == 1 with hold == 0 is the identity, bit for bit.  Only hold > 0 ever fills a hole.  Bytes of a row beyond `width`
 * samples are not defined.  tests/models/depth_temporal_model.py restates the rule word for word.
 * The context's state empties (the next launch neither reads nor trusts the planes: no memset races the stream) on every successful
 * mod_set_depth_temporal, on mod_reset_depth_temporal, on mod_forget_previous, when a depth submit is skipped for a NULL image or
 * depth, and when the geometry the stage sees changes: encoding, width, height, unit and, for the stream's staged window copy, the
 * staged region's origin in the camera's message (it moves with x0 / y0 and with the two spatial stages' aprons).  The synchronous call and
 * the stream share the one state, in program order on the context's stream.
 *   mod_set_depth_temporal      NULL or alpha == 0: off (the default).  Read when mod_depth_to_disparity_dev is called and at the submit
 *                               of mod_submit_depth_host; a ticket in flight keeps the parameters of its own submit; may change while
 *                               tickets are outstanding.  MOD_ERR_INVALID_ARGUMENT, parameters and state stay as they were: alpha
 *                               outside [0, 1] or NaN; a non-finite or negative delta_abs or delta_rel; hold outside 0 .. 254; a
 *                               non-zero reserved.
 *   mod_get_depth_temporal      the parameters in force; all zeros while it is off
 *   mod_reset_depth_temporal    empties the context's state, nothing else
 *   mod_depth_temporal_dev      the stage alone: `frames` consecutive device messages stacked at step * height bytes -> depth_out, same
 *                               layout, on the context's stream.  state_s (float[height * width]) and state_age (uint8[height * width])
 *                               are caller-owned device planes, updated in place (to start empty, fill state_age with 255); both NULL =
 *                               the context's state; one NULL is an error.  depth_out == depth_in is allowed: the rule is pointwise.
 *                               layout NULL = the context's (that needs a camera); its x0, y0 are ignored and any message size passes.
 *                               filter NULL = the context's; a filter that is off copies the samples and touches no state.
 *                               depth_in NULL: MOD_SKIP_NO_DISPARITY_NOW.  The messages aligned to the sample size, state_s to 4 bytes;
 *                               frames <= ModConfig.max_frames.
 * The state planes are allocated on first use with the filter on and freed in mod_destroy.  The library never writes a caller's input:
 * it works in place on its own copies (the filtered scratch, the slot's staged copy) or writes the filtered scratch.
 * Not done: motion-compensated state (the state is per pixel of the depth camera: under camera motion the gate restarts it); fusion
 * with k_depth_filter in one kernel; node parameters. */
typedef struct ModDepthTemporal {   /* 32 bytes; NULL or alpha == 0: off (the default) */
  float alpha, delta_abs, delta_rel;   /* the average's weight of the new sample, in (0, 1]; the gate, in the units of z (metres), >= 0 */
  int32_t hold;                        /* 0 .. 254: the frames a pixel without a reading repeats its average */
  int32_t reserved[4];                 /* must be 0 */
} ModDepthTemporal;
int  mod_set_depth_temporal(ModContext *ctx, const ModDepthTemporal *filter);
int  mod_get_depth_temporal(const ModContext *ctx, ModDepthTemporal *filter);
int  mod_reset_depth_temporal(ModContext *ctx);
int  mod_depth_temporal_dev(ModContext *ctx, int32_t frames, const void *depth_in, const ModDepthLayout *layout,
                            const ModDepthTemporal *filter, float *state_s, uint8_t *state_age, void *depth_out);
/* The spatial depth smoother and hole fill (mod_set_depth_spatial, opt-in, off by default; while it is off nothing is allocated and every
 * call enqueues exactly what it enqueues without this section).  The scene-flow stage differences two disparity planes, so per-pixel
 * depth noise becomes false vz; the temporal filter above removes it only where the camera stands still.  And the depth filter only
 * ever invalidates: every flying pixel it removes, and every occlusion shadow a structured-light head reports beside a foreground
 * edge, is a hole that takes the pixel out of the cloud.  This stage smooths each valid sample over the neighbours on its own surface
 * and puts a sample into a hole from the surface BEHIND it.  It maps a depth MESSAGE to a depth message of the same encoding, width,
 * height and step, behind the depth filter (flying pixels are gone before any mean is formed, and the holes they leave are refilled
 * from the background) and in front of the temporal filter (whose state then averages smoothed samples, and whose hold is left for
 * dropouts in time), the registration, the distortion, the splat and the conversion.
 * The rule.  All F32, one operation at a time, -ffp-contract=off.  For a message pixel with input word w:
 *   x = (float)w for 16UC1, x = value for 32FC1;  z = x * unit (unit == 0: the encoding's default);  valid0 iff z > 0.0f and z is finite
 *   enc(m): 16UC1: (uint16)min(max(rintf(m), 1.0f), 65535.0f), ties to even;  32FC1: the bits of m        (the temporal filter's enc)
 *   R = window / 2.  The neighbourhood of p: the pixels q with |Uq - Up| <= R and |Vq - Vp| <= R that lie inside the message, p
 *   included.  Pixels outside the message never take part.
 * Both rules below read the INPUT only, so the stage is one pass and cannot cascade: a filled hole never supports a neighbour, and a
 * smoothed value never enters another mean.
 *   Smoothing (smooth != 0, p has valid0): a gated box mean, Lee's sigma filter, a bilateral filter with box weights.
 *     t = tol_abs + tol_rel * z_p                                                   (one multiply, then one add)
 *     members: every q of the neighbourhood, p included, with valid0(q) and fabsf(z_q - z_p) <= t
 *     sum = 0.0f;  sum = sum + x_q member by member in row-major order: V ascending, then U ascending
 *     m = sum / (float)n;  the output is enc(m)
 *     A pixel whose only member is itself comes out bit for bit.  For 16UC1 the sum is exact (49 * 65535 < 2^24): the order is then
 *     immaterial and the output lies between the smallest and the largest member word.
 *   Hole fill (fill_min > 0, p lacks valid0): let V be the neighbours q with valid0.
 *     V empty: the output is w, bit for bit.
 *     a = the largest z_q over V;  t = tol_abs + tol_rel * a                        (one multiply, then one add)
 *     members: the q in V with a - z_q <= t                                         (one subtract)
 *     n >= fill_min: the output is enc(m) of the members, summed as above.  Otherwise the output is w, bit for bit.
 *     The anchor is the farthest surface on purpose: a hole beside a depth edge is the foreground's occlusion shadow on the background,
 *     or a flying pixel the depth filter removed, and filling it from the foreground would grow objects and invent moving pixels.  In
 *     idea this is librealsense's farthest_from_around; parity with no SDK is claimed.
 *   Every other sample is copied bit for bit: valid samples while smooth == 0, samples without valid0 while fill_min == 0 (NaN
 *   payloads, -0.0, negatives and +-inf).  Bytes of a row beyond `width` samples are not defined.
 * The neighbourhood is the message's, not the window's: on the plain path mod_submit_depth_host sends the window's apron of
 * R_filter + R_spatial message pixels (each 0 while its stage is off), clamped to the message per side, across PCIe, so a spatial
 * neighbour outside the window has itself been filtered with its full neighbourhood.  tests/models/depth_spatial_model.py restates
 * the rule word for word.
 *   mod_set_depth_spatial       NULL or window == 0: off (the default).  Context state like mod_set_depth_filter: read when
 *                               mod_depth_to_disparity_dev is called and at the submit of mod_submit_depth_host; a ticket in flight
 *                               keeps the setting of its own submit; may change while tickets are outstanding.
 *                               MOD_ERR_INVALID_ARGUMENT, the state stays as it was: a window not in {0, 3, 5, 7}; smooth not 0 or 1;
 *                               fill_min outside 0 .. window * window - 1; a window with neither smooth nor fill_min; a non-finite or
 *                               negative tol_abs or tol_rel; a non-zero reserved.  With window == 0 everything else is still checked
 *                               (smooth, fill_min == 0, the tolerances, reserved) and then ignored.
 *   mod_get_depth_spatial       the setting in force; all zeros while it is off
 *   mod_depth_spatial_dev       the stage alone: `frames` device messages stacked at step * height bytes -> depth_out, same layout, on
 *                               the context's stream.  Not in place: depth_out != depth_in, and overlap is the caller's error.  layout
 *                               NULL = the context's (that needs a camera); its x0, y0 are ignored, the whole message is processed, and
 *                               any message size passes.  spatial NULL = the context's; a stage that is off copies the samples.
 *                               depth_in NULL: MOD_SKIP_NO_DISPARITY_NOW.  Both pointers aligned to the sample size;
 *                               frames <= ModConfig.max_frames.
 * The stage reads neighbours, so it never works in place: behind the depth filter it reads the filtered scratch and writes a second
 * scratch, without it it reads the input and writes the filtered scratch; the second scratch is allocated on first use with both
 * stages on and freed in mod_destroy.  The library never writes a caller's input.
 * Not done: an iterated or cascaded fill; windows above 7; Gaussian weights; an image-guided gate; fusion with k_depth_filter; node
 * parameters. */
typedef struct ModDepthSpatial {   /* 32 bytes; NULL or window == 0: off (the default) */
  int32_t window;                  /* 0 = off, else 3, 5 or 7 */
  int32_t smooth;                  /* 0 or 1 */
  int32_t fill_min;                /* 0 = no hole fill, else 1 .. window * window - 1 */
  float   tol_abs, tol_rel;        /* the gate, in the units of z (metres); finite, >= 0 */
  int32_t reserved[3];             /* must be 0 */
} ModDepthSpatial;
int  mod_set_depth_spatial(ModContext *ctx, const ModDepthSpatial *spatial);
int  mod_get_depth_spatial(const ModContext *ctx, ModDepthSpatial *spatial);
int  mod_depth_spatial_dev(ModContext *ctx, int32_t frames, const void *depth_in, const ModDepthLayout *layout,
                           const ModDepthSpatial *spatial, void *depth_out);
/* The depth decimation (mod_set_depth_decimation, opt-in, off by default; while it is off nothing is allocated and every call and submit
 * enqueues exactly what it enqueues without this section).  mod_set_image_binning reduces the IMAGE of an RGB-D camera; this stage
 * reduces its DEPTH, so that a depth image aligned to the colour image at the colour camera's resolution (RealSense align_depth, Azure
 * Kinect depth_to_rgb, depth_registered/image_rect) meets the binned camera without a host loop.  Depth cannot take k_bin_mono's box
 * mean: a mean over a block that holds foreground, background and "no reading" words invents a surface between them, the flying pixel
 * the depth filter removes.  This reduction knows validity and picks, or averages, samples of one surface only; in idea it is
 * librealsense's decimation block and depth_image_proc-style pipelines, and parity with none is claimed.  It maps depth messages to
 * PACKED depth messages of the same encoding by integer factors dx, dy in 1..4 on the depth camera's lattice, and is the last
 * message-to-message stage: k_depth_filter -> k_depth_spatial -> k_depth_temporal -> k_depth_decimate -> k_depth_to_disparity.  The
 * filters stay at full resolution, so flying pixels are removed before a block can select one; the temporal state keeps its
 * full-resolution lattice and its keys; the conversion reads the decimated W x H message at origin (0, 0).
 * The rule.  All F32, one operation at a time, -ffp-contract=off.  x, z = x * unit, valid0 (z > 0 and finite) and enc(m) are those of
 * the spatial stage above.
 *   Output sample (X, Y) reads the block of message pixels (x0 + dx X + i, y0 + dy Y + j), i < dx, j < dy.  "Row-major order" is j
 *   ascending, then i ascending.  V is the set of the block's samples with valid0.  The "no reading" word is 0 for 16UC1 and
 *   0x7fc00000 for 32FC1.
 *   MOD_DEPTH_DECIMATE_MEDIAN (0, the default).  If |V| < max(min_valid, 1): no reading.  Otherwise sort V ascending by
 *     (z, row-major index).  The output is the INPUT WORD of element (|V| - 1) / 2, the lower median.  Every valid output word is one
 *     of the block's input words.
 *   MOD_DEPTH_DECIMATE_MIN (1).  Same min_valid test.  The output is the input word of the first element of that order, the nearest
 *     surface.  This is the z-buffer's rule, what the registered path does when several samples land on one pixel.
 *   MOD_DEPTH_DECIMATE_MEAN (2).  Same min_valid test.  a = the z of the lower median.  t = tol_abs + tol_rel * a, one multiply and
 *     then one add.  Members are the q in V with fabsf(z_q - a) <= t.  The median itself is always a member.
 *     sum = 0.0f; sum = sum + x_q, member by member in row-major order.  m = sum / (float)n.  The output is enc(m).
 *     For 16UC1 the sum is exact, because 16 * 65535 < 2^24.
 *   MOD_DEPTH_DECIMATE_NEAREST (3).  The output is the block's top-left input word, bit for bit, whatever it is.  This is
 *     crop_decimate's default.  min_valid and the tolerances are ignored.
 *   dx = dy = 1, or a NULL struct, means the stage is off.  The stage alone then copies the window's words bit for bit.
 * tests/models/depth_decimate_model.py restates the rule word for word.
 * In the chain (the plain path): the window taken from the depth message becomes (dx W) x (dy H) at the layout's (x0, y0), and that
 * window must fit; mod_submit_depth_host sends that window, plus the filters' apron of R message pixels clamped as before, across PCIe.
 * The default layout while decimation is on is 16UC1 packed at (dx W) x (dy H).  With a registration in force and decimation on,
 * mod_depth_to_disparity_dev and mod_submit_depth_host return MOD_ERR_INVALID_ARGUMENT: the scatter already lands a larger message in
 * the camera's size with a z-buffer minimum, and decimating ahead of it would need the registration's intrinsics and the ray tables
 * rescaled.
 * The camera is the caller's, as with binning (the section on binning has the formulas): MEDIAN, MIN and MEAN describe the block, so
 * the binned camera is MOD_BIN_MEAN's (the block's centre); NEAREST goes with MOD_BIN_NEAREST.  The library does not tie the two
 * settings together, and nothing forces dx == bx.
 *   mod_set_depth_decimation    NULL or dx = dy = 1: off (the default).  Context state like mod_set_depth_filter: read when
 *                               mod_depth_to_disparity_dev is called and at the submit of mod_submit_depth_host; a ticket in flight
 *                               keeps the setting of its own submit; may change while tickets are outstanding.
 *                               MOD_ERR_INVALID_ARGUMENT, the state stays as it was: a factor outside 1..4; an unknown mode; min_valid
 *                               outside 0 .. dx * dy; a non-finite or negative tol_abs or tol_rel; a non-zero reserved.
 *   mod_get_depth_decimation    the setting in force; dx = dy = 1 and zeros while it is off
 *   mod_depth_decimate_dev      the stage alone: `frames` device messages stacked at step * height bytes -> depth_out on the context's
 *                               stream.  It honours the layout's x0, y0 (the blocks start there) and any message size passes.  The
 *                               output is `frames` packed messages of the same encoding: out_w = (width - x0) / dx and
 *                               out_h = (height - y0) / dy (integer division), step out_w * B, frames stacked at out_w * B * out_h
 *                               bytes.  MOD_ERR_INVALID_ARGUMENT: out_w or out_h below 1; a NULL depth_out; pointers not aligned to
 *                               the sample size; depth_out == depth_in (overlap is the caller's error).  frames <=
 *                               ModConfig.max_frames.  depth_in NULL: MOD_SKIP_NO_DISPARITY_NOW.  decimation NULL = the context's;
 *                               layout NULL = the context's (that needs a camera).
 * The decimated messages are context scratch, [frames] W x H samples, allocated on first use with the stage on and freed in mod_destroy.
 * Not done: decimation under a registration or a distortion; factors above 4; fusion into k_depth_to_disparity; node parameters. */
#define MOD_DEPTH_DECIMATE_MEDIAN  0   /* the lower median of the block's valid samples */
#define MOD_DEPTH_DECIMATE_MIN     1   /* the nearest of them (the z-buffer's rule) */
#define MOD_DEPTH_DECIMATE_MEAN    2   /* the mean of those within the gate of the median */
#define MOD_DEPTH_DECIMATE_NEAREST 3   /* the block's top-left word (crop_decimate's default) */
typedef struct ModDepthDecimation {   /* 32 bytes; NULL or dx = dy = 1: off (the default) */
  int32_t dx, dy;            /* 1..4 each */
  int32_t mode;              /* MOD_DEPTH_DECIMATE_* */
  int32_t min_valid;         /* 0 (= 1) .. dx * dy */
  float   tol_abs, tol_rel;  /* MEAN's gate, metres; finite, >= 0 */
  int32_t reserved[2];       /* must be 0 */
} ModDepthDecimation;
int  mod_set_depth_decimation(ModContext *ctx, const ModDepthDecimation *decimation);
int  mod_get_depth_decimation(const ModContext *ctx, ModDepthDecimation *decimation);
int  mod_depth_decimate_dev(ModContext *ctx, int32_t frames, const void *depth_in, const ModDepthLayout *layout,
                            const ModDepthDecimation *decimation, void *depth_out);

/* ---- host-pointer convenience (what a ROS node with host-side messages calls) ----------------------------- */
/* One frame, host buffers in/out; any output pointer may be NULL.  Returns a skip code exactly where construct()
 * would publish nothing.  cloud_aos: W*H*32 bytes; labels: W*H int32; objects: capacity `max_objects`.
 * With labels == NULL, objects == NULL AND n_objects == NULL the clustering stage does not run at all (the reference's constructor
 * node does not cluster; its clusterer runs whenever a cloud arrives, clusterer_nodelet.cpp:231): a node that serves ~scene_flow
 * alone pays for the scene-flow stage only.  A caller that passes n_objects alone still gets the real count.  mod_submit_frame_host
 * and mod_submit_stereo_host have no count pointer at submit time: there labels == NULL and objects == NULL select the scene-flow
 * stage alone, and mod_collect_frame_host reports 0 objects for such a ticket. */
int  mod_process_frame_host(ModContext *ctx,
                            const float *disparity_now, const float *disparity_prev, const float *flow,
                            const ModTransform *transform, double dt,
                            void *cloud_aos, int32_t *labels,
                            ModObject *objects, int32_t max_objects, int32_t *n_objects);

/* Clusterer alone on a host PointCloud2 payload (ClustererNodelet::dataCB, clusterer_nodelet.cpp:221-242).
 * point_step/row_step as in sensor_msgs/PointCloud2; fields x,y,z,vx,vy,vz at offsets 0,4,8,16,20,24.
 * A context without a camera (a clusterer-only process: the nodelet) takes the image size from this call — the clusterer needs
 * nothing else of the camera; parameters must have been set.  With a camera set, a cloud of another size is an error. */
int  mod_cluster_cloud_host(ModContext *ctx, const void *cloud, int32_t width, int32_t height,
                            int32_t point_step, int32_t row_step,
                            int32_t *labels, ModObject *objects, int32_t max_objects, int32_t *n_objects);

/* ---- host streaming: frames in flight, copies overlapped with the kernels --------------------------------------- */
/* The reference overlaps construct() of frame t with the estimators of frame t+1 (construct_thread_,
 * scene_flow_constructor.cpp:389-392) and keeps disparity_previous_ from the last callback (:397-398).  Here up to
 * MOD_PIPELINE_DEPTH frames are in flight: the input copy of frame t+1 and the result copy of frame t-1 run on their own
 * HIP streams beside the kernels of frame t.
 *   mod_submit_frame_host  enqueues one frame and returns at once with a ticket.  Arguments as mod_process_frame_host,
 *       except: disparity_prev may be NULL, then the disparity_now of the previous submit (still resident in HBM) is used
 *       (MOD_SKIP_NO_DISPARITY_PREV if there was none); outputs are written asynchronously — every pointer must stay valid
 *       and untouched until the ticket is collected.  Skip codes as construct(); MOD_ERR_CAPACITY when MOD_PIPELINE_DEPTH
 *       frames are already in flight.  The large buffers (inputs, cloud, labels) should come from mod_host_malloc: a copy
 *       to or from pageable memory makes the call wait for that copy; `objects` may be ordinary memory (filled at collect time).
 *   mod_collect_frame_host waits for a ticket (tickets complete in submission order; the oldest one must be collected
 *       first) and reports its object count.
 * Reconfiguration while frames are in flight: the PARAMETERS may change between two submits (mod_set_params; the reference's
 * reconfigureCB runs between two stereoCallbacks, scene_flow_constructor.cpp:401-407) — every kernel takes them by value at
 * submit time, so a frame in flight completes with the parameters of ITS submit and the next submit uses the new ones
 * (tests/test_gpu_host_stream.py).  The CAMERA must not change while frames are in flight (its ray tables live in HBM and are
 * read by the kernels of the frames in flight): collect every ticket first. */
#define MOD_PIPELINE_DEPTH 3
int  mod_submit_frame_host(ModContext *ctx,
                           const float *disparity_now, const float *disparity_prev, const float *flow,
                           const ModTransform *transform, double dt,
                           void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects,
                           int32_t *ticket);
int  mod_collect_frame_host(ModContext *ctx, int32_t ticket, int32_t *n_objects);

/* Stereo images in, moving objects out: the device-resident form of stereoCallback() for BASELINE config 5
 * (scene_flow_constructor.cpp:365-399: estimateDisparity, then construct() on construct_thread_ beside the next frame's
 * estimators, then disparity_previous_ = disparity_now_).  The two 8-bit images go to the GPU on the copy stream, the on-GPU
 * estimator (mod_sgm_compute_dev) writes the disparity plane straight into the pipe's ring — where it serves as `now` of this frame
 * and as `previous` of the next — and scene flow + clustering follow on the context's stream: the disparity never crosses PCIe
 * (mod_sgm_compute_host + mod_submit_frame_host move it there and back: two trips of 4 bytes per pixel and frame).
 *   left / right    W*H bytes each, row-major (sensor_msgs/Image mono8), or messages of the layout mod_set_image_layout set
 *                   (colour, padded rows, a window; converted on the GPU); NULL = the estimator has nothing to work on:
 *                   MOD_SKIP_NO_DISPARITY_NOW, and the next frame has no previous disparity (disparity_now_.reset(), :272-276)
 *   sgm             estimator parameters; the camera's min / max_disparity must describe its output (0 and disparities - 1)
 *   flow, transform, dt, cloud_aos, labels, objects, max_objects, ticket: as mod_submit_frame_host.  A frame that ends at one
 *                   of construct()'s guards (no flow, no previous disparity, no transform) still had its disparity estimated:
 *                   it IS the next frame's previous one (:397-398)
 *   disparity       optional host copy of the disparity image (32FC1, -1 where no match was found), valid after collect
 * Collected with mod_collect_frame_host like any other ticket. */
int  mod_submit_stereo_host(ModContext *ctx, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm,
                            const float *flow, const ModTransform *transform, double dt,
                            void *cloud_aos, int32_t *labels, ModObject *objects, int32_t max_objects,
                            float *disparity, int32_t *ticket);
/* Stereo images in, moving objects out, with the flow estimated on the GPU too: mod_submit_stereo_host whose `flow` is
 * mod_flow_compute_dev(previous left image, this left image, flow_prm).  The left image stays resident in HBM (a ring indexed like
 * the disparity ring) as the next submit's previous image, and the flow goes straight into the frame's flow buffer: no flow crosses
 * PCIe.  Without a previous left image — the first frame, after mod_forget_previous, after a submit of another kind, after a frame
 * with a NULL image — the frame behaves exactly like mod_submit_stereo_host with flow = NULL (MOD_SKIP_NO_FLOW; its disparity and
 * left image still serve the next frame).  flow_prm is read at submit time.
 *   flow_out   optional host copy of the flow image (32FC2, the reference's ~optical_flow, scene_flow_constructor.cpp:99-100),
 *              valid after collect; like `disparity`, written for ticketed frames only
 * Other arguments, skip codes and collection as mod_submit_stereo_host. */
int  mod_submit_images_host(ModContext *ctx, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm,
                            const ModFlowParams *flow_prm, const ModTransform *transform, double dt, void *cloud_aos,
                            int32_t *labels, ModObject *objects, int32_t max_objects, float *disparity, float *flow_out,
                            int32_t *ticket);
/* Stereo images in, moving objects out, nothing else on the host: mod_submit_images_host whose transform is estimated on the GPU
 * (mod_egomotion_dev on the frame's disparity pair and flow, ego_prm).  sgm -> flow -> ego-motion -> scene flow + clusters on the
 * context's stream; the estimator's last kernel writes the frame's constants for the scene-flow kernel straight into HBM, so no
 * transform crosses PCIe before the scene flow runs.  First frame, mod_forget_previous, NULL images, a submit of another kind: as
 * mod_submit_images_host.  A frame whose estimate fails (visual odometry failed, scene_flow_constructor.cpp:251-255) still runs
 * with the NaN transform — every velocity NaN, every label -1, no object — and mod_collect_frame_host returns
 * MOD_SKIP_NO_TRANSFORM for its ticket with 0 objects.
 *   transform_out, ego_out   optional host copies of the estimate, valid after collect
 * Other arguments as mod_submit_images_host. */
int  mod_submit_odometry_host(ModContext *ctx, const uint8_t *left, const uint8_t *right, const ModSgmParams *sgm,
                              const ModFlowParams *flow_prm, const ModEgoParams *ego_prm, double dt, void *cloud_aos, int32_t *labels,
                              ModObject *objects, int32_t max_objects, float *disparity, float *flow_out, ModTransform *transform_out,
                              ModEgoResult *ego_out, int32_t *ticket);
/* One image and one depth image in, moving objects out: mod_submit_images_host (transform non-NULL) or mod_submit_odometry_host
 * (transform NULL; ego_prm is then required) with the disparity estimator replaced by the depth conversion above.  On the copy
 * stream, without a registration only the depth window crosses PCIe (W * H * 2 or 4 bytes); with one the whole message crosses.  On
 * the context's stream the conversion writes straight into the ring plane, `now` of this frame and `previous` of the next.
 *   image   a message of the context's image layout, in every encoding the library takes
 *   depth   a message of the context's depth layout
 * The left-image ring, the skip codes, a first frame, mod_forget_previous, "a submit of another kind", a NULL image or NULL depth
 * (MOD_SKIP_NO_DISPARITY_NOW, and the next frame has no previous), disparity / flow_out / transform_out / ego_out and collection:
 * as the two submits above.  MOD_ERR_INVALID_ARGUMENT (the state stays as it was): side by side is on; a rectification is set but
 * no registration (a depth image aligned to a raw image cannot be aligned to the rectified one; with a registration the image is
 * rectified with the left map and the registration's target is the rectified camera); transform and ego_prm both NULL; a NULL
 * flow_prm; what mod_depth_to_disparity_dev refuses of the depth layout in force. */
int  mod_submit_depth_host(ModContext *ctx, const uint8_t *image, const void *depth, const ModFlowParams *flow_prm,
                           const ModEgoParams *ego_prm, const ModTransform *transform, double dt, void *cloud_aos, int32_t *labels,
                           ModObject *objects, int32_t max_objects, float *disparity, float *flow_out, ModTransform *transform_out,
                           ModEgoResult *ego_out, int32_t *ticket);
/* disparity_now_.reset() of a failed estimateDisparity (scene_flow_constructor.cpp:272-276): the next submit without an
 * explicit disparity_prev reports MOD_SKIP_NO_DISPARITY_PREV instead of pairing with a stale frame. */
int  mod_forget_previous(ModContext *ctx);
int  mod_host_malloc(ModContext *ctx, uint64_t bytes, void **host_ptr);   /* page-locked host memory */
int  mod_host_free(ModContext *ctx, void *host_ptr);

/* ---- device memory helpers (so a non-HIP host language can own HBM buffers) ------------------------------- */
int  mod_malloc(ModContext *ctx, uint64_t bytes, void **dev_ptr);
int  mod_free(ModContext *ctx, void *dev_ptr);
int  mod_memcpy_h2d(ModContext *ctx, void *dev_dst, const void *host_src, uint64_t bytes);
int  mod_memcpy_d2h(ModContext *ctx, void *host_dst, const void *dev_src, uint64_t bytes);

/* ---- measurement ------------------------------------------------------------------------------------------ */
/* Stage timers: each stage selected by `stage_mask` (bit i = stage i; MOD_PROFILE_ALL for all of them, 0 = off) is
 * bracketed by HIP events on the context's stream in the calls that follow.  Every event pair costs a few microseconds of
 * stream time, so a throughput measurement should select only the stage it prices. */
#define MOD_STAGE_SCENE_FLOW  0   /* k_scene_flow_v4 / _v1: fused scene-flow kernel (+ dynamic mask)            */
#define MOD_STAGE_CCL_TILE    1   /* tile stage: k_ccl_bits<n> + k_ccl_tile_list (k_ccl_tile for n > 10): tile-local
                                     connected components (+ k_dynamic_mask / k_tile_flags for a caller's cloud)  */
#define MOD_STAGE_CCL_LINK    2   /* k_ccl_link: cross-tile unions                                              */
#define MOD_STAGE_CCL_MERGE   3   /* k_ccl_merge: root-level flatten + record folding, and the size filter with the
                                     reference numbering: in k_ccl_merge's last workgroup per frame for batches of up
                                     to 16 frames, as k_select behind it for larger ones (a stage of its own, "select",
                                     until ABI version 1)                                                        */
#define MOD_STAGE_FINAL       4   /* k_final: labels plane + member compaction + cluster boxes; with
                                     mod_set_cluster_members on, k_cluster_members: the ordered member lists; with
                                     mod_set_cluster_image on, k_cluster_image: the BGR8 cluster image           */
#define MOD_STAGE_MEDIAN      5   /* k_median + k_median_ties: median-velocity member; object ids               */
#define MOD_STAGE_CLUSTER_GROUP 6 /* the whole cluster stage of a call, first launch to last (stages 1..5 and, in a chunked
                                     mod_process_dev, the overlap of its chunks: see ModConfig.batch_chunks).  While a timer
                                     of one of the stages 1..5 is on, mod_process_dev runs un-chunked: side by side the kernels
                                     of different chunks would be priced with each other's load */
#define MOD_STAGE_COUNT       7
#define MOD_PROFILE_ALL        0x7f
int  mod_set_profiling(ModContext *ctx, int32_t stage_mask);
/* Accumulated milliseconds and launch count of a stage since the last reset (synchronises the stream). */
int  mod_get_stage_time(ModContext *ctx, int32_t stage, double *total_ms, int64_t *calls);
int  mod_reset_stage_times(ModContext *ctx);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MOD_SF_H_ */
