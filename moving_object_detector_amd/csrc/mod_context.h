// mod_context.h — the context behind the C ABI and what its host-side files share (internal to libmod_sf.so, not installed): mod_sf.hip (lifecycle, the batched scene-flow /
// cluster path), host_sgm.hip, host_flow.hip, host_ego.hip (the estimators), host_filters.hip (their stand-alone filters), host_images.hip (image layouts, rectification, the
// host images' way to grey), host_depth.hip (DepthOptions, ray tables, DepthPlan and the chain from depth messages to disparity), host_api.hip (*_host calls).
#pragma once
#include "../../include/mod_sf.h"
#include "frame_const.h"
#include "mod_launch.h"

#include <string>
#include <utility>
#include <vector>

constexpr int kRing = 4;        // pinned staging slots for the per-frame constants
constexpr int kMaxChunks = 4;   // mod_process_dev cuts a large batch into at most this many chunks (ModConfig.batch_chunks)

// One owner per GPU resource: a handle releases what it holds when it is reset or destroyed, and reads as the raw pointer / handle.
// put() releases the old resource and hands the slot to the hip*Malloc / hip*Create call that fills it.
template <class H, auto Release>
class Owned {
  H h_ = nullptr;

 public:
  Owned() = default;
  Owned(Owned &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Owned &operator=(Owned &&o) noexcept { std::swap(h_, o.h_); return *this; }
  ~Owned() { reset(); }
  operator H() const { return h_; }
  H get() const { return h_; }
  H *put() { reset(); return &h_; }
  void reset() { if (h_) (void)Release(h_); h_ = nullptr; }
};
template <class T> using DevPtr = Owned<T *, hipFree>;
template <class T> using HostPtr = Owned<T *, hipHostFree>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// allocates unless p already holds a buffer (lazily built buffer sets can be resumed after a failed attempt without leaking)
template <class T>
hipError_t dalloc(DevPtr<T> &p, size_t count) { return p ? hipSuccess : hipMalloc((void **)p.put(), count * sizeof(T)); }
inline hipError_t make_event(Event &e) { return e ? hipSuccess : hipEventCreateWithFlags(e.put(), hipEventDisableTiming); }
#define HIP_OK(expr) do { if (hipError_t e_ = (expr); e_ != hipSuccess) return e_; } while (0)   // in functions that return a hipError_t (entry points: HIP_TRY)

// An event and whether it has been recorded yet: wait() on a fence that never was is no call at all.  A fence stays armed (every
// later wait() waits again) unless its waiter takes it with wait_once().  record() makes the event where nobody has.
struct Fence {
  Event ev;
  bool armed = false;
  hipError_t record(hipStream_t s) {
    hipError_t e = make_event(ev);
    if (e == hipSuccess && (e = hipEventRecord(ev, s)) == hipSuccess) armed = true;
    return e;
  }
  hipError_t wait(hipStream_t s) const { return armed ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
  hipError_t wait_once(hipStream_t s) { return std::exchange(armed, false) ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
};

struct EventPair { Event a, b; };

// Scratch of the cluster stage and of the scene-flow epilogue that feeds it (what each buffer holds: mod_launch.h ClArgs).  Sized once, for the capacities
// below; a call's frames lie the CAMERA's strides apart inside it.  Its operations are in mod_sf.hip: cluster_alloc, cluster_grow_requests, cluster_carve.
struct ClusterScratch {
  size_t frames = 0, pixels = 0, mask_rows = 0, tiles = 0, max_objects = 0;   // capacities: frames; per frame pixels, mask words x rows, tiles, objects
  DevPtr<uint64_t> mask, lroot;             // [frames][mask_rows]
  DevPtr<float2> zrange;                    // [frames][mask_rows] depth range of the dynamic pixels of each mask word (fused path)
  DevPtr<int32_t> parent, rsize, rkey;      // [frames][pixels]; rsize, rkey: 4 + 4 B per pixel of address space, touched only at roots
  DevPtr<uint32_t> mbits, mpix;             // [frames][pixels]
  DevPtr<ClusterBox> cbox;                  // [frames][max_objects]
  DevPtr<ClusterInfo> clusters;             // [2][frames][max_objects]: the clusters, then (rank_scratch) what k_ccl_merge ranks them in
  DevPtr<uint32_t> worklist;                // [2][frames * max_objects]: all clusters of a launch, then (tielist) the ambiguous ones
  ClusterInfo *rank_scratch = nullptr; uint32_t *tielist = nullptr;   // the second halves of the two, set where they are allocated
  DevPtr<int32_t> counters, tilehdr;        // [frames][kClusterCounters], [frames][tiles][kTileHdrWords]
  DevPtr<uint32_t> tilelist;                // [frames * tiles]
  DevPtr<uint2> requests; size_t req_alloc = 0;   // [frames][tiles][ccl_request_capacity(neighbor_distance)], grown by mod_set_params; entries allocated
};

struct Buffers {
  DevPtr<double> rayx, rayy;
  DevPtr<FrameConst> fc;                    // [maxF]
  DevPtr<unsigned long long> dbg;           // [kDbgWords] diagnostic counters (mod_device.h)
  ClusterScratch cluster;
  struct Sgm {                              // on-GPU disparity (allocated on first use)
    DevPtr<uint32_t> census;                // kSgmCensusLead words, then two sets of [left, right][group][N] census planes
    DevPtr<uint8_t> maps;                   // SgmMaps of a group (mod_launch.h): sgm_maps_bytes(maps16) * N bytes per frame
    DevPtr<uint8_t> S;                      // two sets of [kSgmPaths][group][H][W][D] path cost volumes
    int D = 0, G = 0; bool maps16 = false;  // disparities / frames per group the scratch is sized for; the sub-pixel mode's 16-bit left maps: grow-only, all three
    // the aggregation paths are independent of each other: they run side by side on these streams (forked from / joined to the
    // context's stream with events), so that the waves of one path fill the SIMD slots another leaves idle
    Stream side[kSgmPaths];
    Event fork[2], join[2][kSgmPaths];      // per set (host_sgm.hip SgmSet)
    DevPtr<float> unsmoothed; int unsmoothed_frames = 0;   // [group][maxN] a group's disparity in front of the smoother (its output goes to `unfilled` with the hole fill on, else to the caller's plane); allocated at the first call with mod_set_disparity_smooth on, grow-only
    DevPtr<float> unfilled; int unfilled_frames = 0;   // [group][maxN] a group's disparity in front of the hole fill (the caller's plane takes the filled one); allocated at the first call with mod_set_disparity_fill on, grow-only
  } sgm;
  // speckle filter (disparity_filter.hip): union-find parents and region sizes of its own, [frames][maxN] each — a group of the
  // estimator or max_frames of mod_disparity_speckle_dev; allocated on first use with the filter on, grow-only (ensure_speckle_scratch)
  struct Speckle { DevPtr<int32_t> parent, size; int frames = 0; } spk;
  struct Flow {                             // on-GPU optical flow (allocated on first use, every level sized for max_width x max_height x max_frames: FlowPlan)
    DevPtr<uint8_t> img;                    // pyramid levels 1 .. kFlowMaxLevels - 1 of both images
    DevPtr<uint32_t> census;                // census planes of levels 0 .. kFlowMaxLevels - 1 of both images
    DevPtr<short2> winners;                 // [2 levels, ping-pong][2 directions][maxF][maxN] integer winners
    DevPtr<short4> sub;                     // [maxF][maxN] sub-pixel terms of level 0
    DevPtr<float2> unfiltered;              // [maxF][maxN] the flow in front of the median filter; allocated at the first call with mod_set_flow_median on
    DevPtr<float2> unfilled;                // [maxN] a submit's flow in front of the hole fill (the slot's buffer takes the filled one); allocated at the first submit with mod_set_flow_fill on
  } flow;
  struct Ego {                              // on-GPU ego-motion (allocated on first use; the correspondence buffers grow to the smallest stride seen: ensure_ego_scratch)
    DevPtr<double> corr, hyp;               // [maxF][9][cap], [maxF][MOD_EGO_MAX_HYPOTHESES][12]
    DevPtr<uint8_t> flag; size_t cap = 0;   // [maxF][cap]
    DevPtr<int32_t> blkcnt, ncorr, hcnt;    // [maxF][blocks of the grid at the smallest stride], [maxF], [maxF][MOD_EGO_MAX_HYPOTHESES]
    DevPtr<ModTransform> tf; DevPtr<ModEgoResult> res;   // [maxF] each: mod_egomotion_host / (res) a NULL `results` of mod_egomotion_dev
  } ego;
};

// The options of the two image estimators, one member per mod_set_* / mod_get_* pair and named like it (host_options.h); these initialisers are the defaults.
// Read when a call or submit enqueues its estimator; every kernel of the call is enqueued from the snapshot.  A zero threshold / window / speckle_size: that stage is off
struct EstimatorOptions {
  int32_t disparity_subpixel = 0, disparity_offset = 0; ModDisparityFilters disparity_filters{};   // disparity: fraction bits; where the window starts (mod_sgm_path_dev reads it too)
  ModDisparitySmooth disparity_smooth{};                                                           // window 0: off; sgm_finish's stage behind the speckle stage, in front of the fill
  ModDisparityFill disparity_fill{};                                                               // reach 0: off; the last stage of sgm_finish (host_sgm.hip)
  ModTextureFilter texture_filter{0, 9, 31, MOD_TEXTURE_DISPARITY | MOD_TEXTURE_FLOW};             // both, as `apply` says
  int32_t flow_propagation = 1; ModCornerFilter flow_corner_filter{0, 9, 31, 0}; ModFlowMedian flow_median{}; ModFlowFill flow_fill{};   // flow: seeds of a search (1: the parent's winner alone); the fill runs in the submits only (host_api.hip)
};

// The settings of the depth input (RGB-D cameras), one member per mod_set_depth_* / mod_get_depth_* pair and named like it (host_depth.hip); these initialisers
// are the defaults.  Read when a call or submit is made: depth_plan() takes the snapshot, and everything the call or the ticket enqueues runs from that DepthPlan
struct DepthOptions {
  ModDepthLayout layout{}; bool has_layout = false;                       // while false: 16UC1 packed at the camera's size (layout_in_force)
  ModDepthRegistration registration{}; bool has_registration = false;     // opt-in: the whole message is scattered into the image camera (no window)
  bool splat = false;                                                     // ... and paints footprints (k_depth_register_splat)
  ModDepthDistortion distortion{}; bool has_distortion = false;           // the depth camera's lens: the registered path reads ray tables (DepthRayTable)
  ModDepthFilter filter{};                                                // all zeros: off
  ModDepthSpatial spatial{};                                              // all zeros: off
  ModDepthTemporal temporal{};                                            // all zeros: off
  ModDepthDecimation decimation{1, 1, MOD_DEPTH_DECIMATE_MEDIAN, 0, 0.0f, 0.0f, {0, 0}};   // dx = dy = 1: off
};

// What one call or one ticket does with its depth messages: DepthOptions as they were when it was made, resolved (host_depth.hip depth_plan)
struct DepthPlan {
  ModDepthLayout lay;               // checked; of the messages the chain is handed (the stream: of the staged copy, once stage_depth has run)
  float unit;                       // metres per raw unit, resolved (lay.unit 0: the encoding's REP 118 default)
  bool registered; DepthRegArgs reg;   // a registration is in force; then its arguments with the image camera's, else unused
  bool splat;
  DepthRayTables rays;              // both null: no distortion
  ModDepthFilter filter;
  ModDepthSpatial spatial;
  ModDepthTemporal temporal;
  ModDepthDecimation decimation;    // dx = dy = 1: off; else lay's window is (dx W) x (dy H) and the conversion reads the decimated scratch
  int ox, oy;                       // where the messages the chain is handed begin in the camera's message (the temporal state's key)
  bool own_input;                   // the chain's input buffer is the library's own: a stage may write it in place (false: a caller's, never written)
};

// Every resource is a member handle: mod_destroy synchronizes the streams below, and `delete` releases the rest.
struct ModContext {
  ModConfig cfg{};
  ModCamera cam{};
  ModParams prm{};
  bool has_cam = false, has_prm = false;
  ModImageLayout layout{};                  // of the host images (mod_set_image_layout) ...
  bool has_layout = false;                  // ... or, while false, mono8 packed at the camera's size
  bool side_by_side = false;                // mod_set_side_by_side: one message holds both eyes; read when a call / submit is made
  // mod_set_image_binning: read when a call / submit is made ({1, 1, ..}: off).  The window every layout is checked against, the
  // converters run at and a rectification map is built for is then the full one, (bx W) x (by H): full_window()
  ModImageBinning binning{1, 1, MOD_BIN_MEAN, 0};
  EstimatorOptions opt;
  // mod_set_cluster_members: read by the calls that write the lists when they enqueue the cluster stage (members_on false: off)
  ModClusterMembers members{};
  bool members_on = false;
  // mod_set_cluster_image: read by mod_cluster_dev / mod_process_dev (image) and by the *_host calls and the submits (host_image) when
  // they enqueue their work; image_table: the table in force, a caller's copied at the set call (image_bytes: its bytes, for mod_get_cluster_image)
  ModClusterImage image{};
  bool image_on = false;
  label_palette::Table image_table{};
  uint8_t image_bytes[3 * label_palette::kEntries] = {};
  // mod_set_rectification: the calibrations and, per eye, the map in HBM with the window and the distortion model it was built for
  // (ensure_rectify_map builds it at the next use after the window, the calibration or the model changed, never under a frame in flight)
  struct Rectify {
    bool on = false;
    ModRectifyCamera cam[2]{};
    int32_t model = MOD_DISTORTION_RATIONAL;  // mod_set_distortion_model: both eyes'; read when a map is built
    struct Map {
      DevPtr<int32_t> q;                      // [H][W][2], allocated on first use for maxN pixels
      bool valid = false;
      int32_t width = 0, height = 0, x0 = 0, y0 = 0, W = 0, H = 0, model = 0;
    } map[2];
  } rect;
  // whole raw messages on their way to k_rectify: room for two of the layout in force (allocated on first use, grow-only); a
  // side-by-side message is one, and uses the first half
  struct RawStage { DevPtr<uint8_t> buf; size_t bytes = 0; };
  // Bayer messages under a rectification are demosaiced whole (debayer, then rectify): the grey planes k_rectify then samples, one
  // per frame of mod_rectify_dev (the host paths have their own, beside their raw stages); allocated on first use, grow-only
  RawStage bayer_grey;
  // with a binning set: the full-window grey planes the converters write and k_bin_mono reads, one per frame of
  // mod_image_to_mono_dev / mod_rectify_dev (the host paths have their own two, beside their raw stages); on first use, grow-only
  RawStage bin_grey;
  // RGB-D cameras (depth.hip): the mod_set_depth_* settings, then their resources.  Each is allocated on first use, grow-only, and written and
  // read on the context's stream alone, in program order: so one of each serves the synchronous calls and every slot of the stream
  DepthOptions depth;
  DevPtr<uint32_t> depth_zbuf;              // the registered path's z-buffer, [max_frames][maxN], of mod_depth_to_disparity_dev (a slot has its own: Slot::zbuf)
  RawStage depth_filtered;                  // the messages a filter of the chain wrote where it could not work in place (run_depth_chain)
  RawStage depth_smoothed;                  // ... and the spatial stage's where its input is depth_filtered (it never works in place)
  RawStage depth_decimated;                 // the decimation's packed [frames] W x H messages, which the conversion then reads (run_depth_chain)
  // the temporal filter's per-pixel state: packed [height][width] planes on the lattice of the messages the stage was last handed (s: F32; age: u8,
  // 255 = empty).  Its key is the geometry of that lattice: encoding, size, unit and the origin in the camera's message.  fresh: forget_depth_history
  struct DepthTemporalState {
    RawStage s, age;
    bool fresh = true;
    int32_t encoding = 0, width = 0, height = 0, ox = 0, oy = 0;
    float unit = 0.0f;
  } depth_tstate;
  // mod_set_depth_distortion: per lattice (MOD_DEPTH_RAYS_*) the ray table in HBM with the lens and the message size it was built for
  // (ensure_depth_rays builds it at the next use after one of them changed, never over a table that a frame in flight may read)
  struct DepthRayTable {
    DevPtr<double2> rays;                     // [rows][cols], allocated on first use for the message at hand, grow-only
    size_t entries = 0;                       // ... its capacity
    bool valid = false;
    depth_rays::Lens lens{};
    int32_t width = 0, height = 0;
  } depth_rays[2];
  Stream own_stream;                        // the stream the context created when ModConfig.stream was null (a caller's is never destroyed)
  hipStream_t stream = nullptr;             // own_stream or the caller's
  DevCam dc{};
  Buffers b;
  int max_objects = 0;
  size_t maxN = 0;
  // the device buffers of one host frame: the staging of the synchronous *_host entry points and each slot of the stream have a set
  struct FrameBuffers {
    DevPtr<float> dprev, flow, planes;
    DevPtr<void> aos;
    DevPtr<int32_t> labels, nobj;
    DevPtr<ModObject> objects;
    DevPtr<uint8_t> image;                  // mod_set_cluster_image: the frame's BGR8 cluster image, 3 maxN bytes, allocated when first needed
  };
  // one-frame staging of the synchronous entry points (allocated on first use; ready: the last allocation has succeeded)
  struct HostStaging : FrameBuffers { DevPtr<float> dnow; bool ready = false; RawStage raw, bayer_grey, bin_grey; } staging;
  // host streaming (mod_submit_frame_host and the mod_submit_*_host image entries): a slot per ticket, a ring of MOD_PIPELINE_DEPTH + 1
  // planes (frame t's plane is frame t+1's "previous"), two copy streams and the events and fences that order them with the kernels
  struct Pipe {
    struct EgoSlot { ModTransform tf; ModEgoResult res; };
    // What a ticket owns.  dprev: a caller's previous disparity; flow: copied in or estimated; planes: z, vx, vy, vz (see scene_flow_staged)
    struct Slot : FrameBuffers {
      HostPtr<int32_t> h_n;                          // pinned: object count of the slot's frame
      // pinned: its objects (the count is not known at submit time, and a pageable destination would make the submit wait); collect hands them on
      HostPtr<ModObject> h_obj;
      ModObject *user_obj = nullptr;
      int32_t user_cap = 0;
      Event ev_in, ev_done, ev_out;                  // inputs on the device (copy stream) / kernels enqueued / results on the host
      DevPtr<uint8_t> img;                           // image entries: the slot's two 8-bit images (the left one unless one is resident)
      // ... the estimator has been enqueued behind them (context stream).  A frame that ended at a guard took no ticket, so nobody
      // waited for its estimator: the next copy into img queues behind it
      Fence img_read;
      // colour images (mod_set_image_layout): the slot's two windows as they arrive, W * H * 4 bytes each (allocated on first use);
      // k_to_mono turns them into grey in img / the plane's left image on the context's stream, behind every older reader of those
      DevPtr<uint8_t> stage;
      Fence stage_read;                              // ... the kernels that read them have been enqueued (context stream)
      RawStage raw;                                  // with a rectification set: the slot's two raw messages instead, behind the same fence
      RawStage bayer_grey;                           // ... and, for Bayer messages, their two demosaiced grey planes (k_rectify samples these)
      RawStage bin_grey;                             // with a binning set: the frame's two full-window grey planes (k_bin_mono reads these), behind the same fence
      // mod_submit_depth_host: the slot's depth window (with a registration: whole message) as it arrives, and the kernels that read
      // it have been enqueued (context stream); the slot's z-buffer [maxN], written and read on the context's stream only
      RawStage depth;
      Fence depth_read;
      DevPtr<uint32_t> zbuf;
      // mod_submit_odometry_host: the slot's estimate on the device (its element of Pipe::ego, last copied out before the slot's
      // previous ticket was collected) and its pinned host copy; collect reads the status
      EgoSlot *ego = nullptr;
      HostPtr<EgoSlot> h_ego;
      bool odo = false;                              // the slot's ticket came from the odometry stream
      ModTransform *user_tf = nullptr;               // ... and where collect hands the estimate (either may be null)
      ModEgoResult *user_ego = nullptr;
    };
    // What lives one frame longer than its ticket.  A frame that ends at a guard takes a plane but no ticket: the slots would not do.
    struct RingPlane {
      DevPtr<float> disparity;
      // the plane may still be on its way to a caller's `disparity` buffer (result stream) when guard-skipped frames have advanced the
      // ring back to it: the plane's next writer waits for that copy, once
      Fence copied_out;
      DevPtr<uint8_t> left;                          // mod_submit_images_host / _odometry_host: the frame's left image, grey
      Fence left_read;                               // the last kernel that reads it (this frame's or the next one's) has been enqueued
    };
    struct Frame { Slot *s; RingPlane *now, *prev; };   // a frame's place in the pipe: its slot, the plane it fills, the plane before
    bool ready = false;
    Stream h2d, d2h;
    static constexpr int R = MOD_PIPELINE_DEPTH + 1;
    Slot slot[MOD_PIPELINE_DEPTH];
    RingPlane ring[R];
    DevPtr<EgoSlot> ego;                             // device [DEPTH], one element per slot (Slot::ego)
    // the last plane written by kernels (image entries; a frame they skipped took a plane without a ticket): mod_submit_frame_host's next copy waits
    Fence ring_written;
    int64_t dring = 0, seq = 0;                      // planes / tickets handed out so far
    int in_flight = 0;
    bool have_prev = false, have_prev_img = false;   // the plane before the next one holds the previous frame's disparity / left image
    bool prev_img_rgbd = false;                      // ... and that left image came from mod_submit_depth_host (it pairs with its own kind only)
    // The ring arithmetic, all of it: the slot of ticket number t, the plane the next frame fills and the one filled before it.
    Frame frame(int64_t t) { return {&slot[t % MOD_PIPELINE_DEPTH], &ring[dring % R], &ring[(dring + R - 1) % R]}; }
    // `now` becomes the next frame's previous plane (disparity_previous_ = disparity_now_, scene_flow_constructor.cpp:397-398).  An image frame
    // takes its plane once its estimator is enqueued and keeps it when it then ends at a guard; a disparity frame takes one only with its ticket.
    void advance_ring() { dring++; have_prev = true; }
  } pipe;
  HostPtr<FrameConst> pinned[kRing];
  Event pinned_ev[kRing];
  int ring_pos = 0;
  // chunks of a large batch (process_chunked): chunk 0 runs on the context's stream, chunk k > 0 on chunk_stream[k - 1], forked from
  // and joined to the context's stream with events, so the call keeps the stream semantics of every other entry point.  Made by
  // mod_create when the context may chunk.
  Stream chunk_stream[kMaxChunks - 1];
  Event ev_fork, ev_join[kMaxChunks - 1];
  // The tile headers (word 0) and the cluster counters are ZERO between calls: the context's first call clears them, and the cluster stage's
  // last readers (k_final; k_median_ties' last workgroup) clear what a call has set — two memsets less in front of every call, which
  // a small batch feels (a launch costs it ~8 us of GPU time whatever it does).  False while a call is being enqueued; a call that
  // failed half-way leaves it false and the next one clears the scratch itself.
  bool scratch_clean = false;
  // the odometry stream's estimator has written the frame's FrameConst into b.fc on the stream: the scene-flow launch reads it there
  bool fc_resident = false;
  int profiling = 0;                          // stage mask of mod_set_profiling
  std::vector<EventPair> pending[MOD_STAGE_COUNT];
  std::vector<EventPair> free_events;
  double stage_ms[MOD_STAGE_COUNT] = {};
  int64_t stage_calls[MOD_STAGE_COUNT] = {};
  std::string err;
};

inline int fail(ModContext *ctx, int code, const std::string &msg) {
  if (ctx) ctx->err = msg;
  return code;
}

#define HIP_TRY(ctx, expr)                                                                              \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return fail(ctx, MOD_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));              \
  } while (0)

inline int check_ready(ModContext *c, int frames) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!c->has_cam || !c->has_prm) return fail(c, MOD_ERR_NOT_CONFIGURED, "camera and parameters must be set first");
  if (frames < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "frames must be >= 1");
  if (frames > c->cfg.max_frames) return fail(c, MOD_ERR_CAPACITY, "frames exceeds ModConfig.max_frames");
  return MOD_OK;
}

inline int need_camera(ModContext *c) {
  return c->has_cam ? MOD_OK : fail(c, MOD_ERR_NOT_CONFIGURED, "the camera must be set first (the window is the camera's size)");
}

// construct()'s guards, in its order: nothing is published when an input is missing (scene_flow_constructor.cpp:104,110,122,127,133)
inline int construct_skip(bool flow, bool prev, bool transform, bool now) {
  if (!flow) return MOD_SKIP_NO_FLOW;
  if (!prev) return MOD_SKIP_NO_DISPARITY_PREV;
  if (!transform) return MOD_SKIP_NO_TRANSFORM;
  if (!now) return MOD_SKIP_NO_DISPARITY_NOW;
  return MOD_OK;
}

// mod_sf.hip
void refresh_devcam(ModContext *c);
int begin_cluster_scratch(ModContext *c);
// mem: where the member lists of the call's frames go, or null (none are written)
int run_cluster(ModContext *c, int frames, const ModSceneFlowPlanes *pl, const uint64_t *mask, bool mask_ready, bool flags_ready,
                const ModClusterOut *out, const ModClusterMembers *mem);
// mod_process_dev with the member lists stated by the caller: the setting in force for the calls that write them (cluster_members),
// null for the pipelined submits — several tickets in flight would share one buffer
int process_dev(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *pl, const ModClusterOut *out, const ModClusterMembers *mem);
inline const ModClusterMembers *cluster_members(const ModContext *c) { return c->members_on ? &c->members : nullptr; }
// k_cluster_image over `frames` frames at the camera's size on the context's stream, timed inside MOD_STAGE_FINAL
int render_cluster_image(ModContext *c, int frames, const int32_t *labels, const int32_t *n_clusters, const label_palette::Table &table, uint8_t *image);
// where the *_host calls and the submits put the frame's image (mod_set_cluster_image), or null: no image is rendered
inline uint8_t *cluster_host_image(const ModContext *c) { return c->image_on ? c->image.host_image : nullptr; }
// the scene-flow stage of the host entry points: their SoA planes are internal staging that no caller sees (the cloud leaves as
// 32-byte records straight from the kernel's registers), so the x and y planes are not written at all
int scene_flow_staged(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *out);

// host_images.hip
// The window the image paths take from a message: the camera's size, or with a binning b its (bx W) x (by H)
struct Window { int w, h; size_t pixels() const { return (size_t)w * h; } };
inline bool binned(const ModImageBinning &b) { return b.bx * b.by > 1; }
inline Window full_window(const ModContext *c, const ModImageBinning &b) { return {b.bx * c->dc.W, b.by * c->dc.H}; }
// the layout the host image entry points read (the set one, or mono8 packed W x H), checked against the camera
int current_layout(ModContext *c, ModImageLayout *out);
// where the pane of `eye` starts in a row of a side-by-side message
inline size_t pane_offset(const ModImageLayout &l, int eye) { return eye == MOD_EYE_RIGHT ? (size_t)l.width * image_channels(l.encoding) : 0; }
// side by side (mod_set_side_by_side): `right` of a call that takes one message for both eyes must be NULL or that message
int check_one_message(ModContext *c, const uint8_t *left, const uint8_t *right);
// with a rectification set (the caller has checked that, and eye): the map of `eye` for the window of `l` (the full one of the binning in force) is in c->rect.map[eye].q when this returns MOD_OK (built, behind
// the context's stream, unless it is the cached one; refused while tickets are outstanding)
int ensure_rectify_map(ModContext *c, int eye, const ModImageLayout &l);
// room for `need` bytes in r; a buffer that has to grow is replaced once the context's streams have drained
int ensure_stage_bytes(ModContext *c, ModContext::RawStage &r, size_t need);
// the W x H window at (x0, y0) of a host image of bpp bytes a pixel to dst on stream s, as packed rows of W * bpp bytes: only the window crosses PCIe
hipError_t copy_window(const void *src, int32_t step, int32_t x0, int32_t y0, int bpp, int W, int H, void *dst, hipStream_t s);
size_t window_stage_bytes(const ModContext *c);   // what ImageIngest::stage must hold
// The one way of host images to grey, in two halves that a caller runs in order.  Where one call's / one frame's images go:
struct ImageIngest {
  ModImageLayout lay;
  ModImageBinning bin;              // the binning of this call / submit; while on, the converters write the full window into ...
  ModContext::RawStage *bin_grey;   // ... two planes here (ensure_bin_stage), mono8 windows are copied there, and k_bin_mono makes grey0 / grey1
  bool rectify, panes;              // a rectification is set; img0 holds both eyes side by side (img1 is not read)
  int eye1;                         // rectifying: the map of the second image
  uint8_t *stage;                   // colour windows / Bayer regions as they arrive (unused for mono8 and when rectifying)
  ModContext::RawStage *raw, *bayer_grey;   // rectifying: the whole messages, and the demosaiced planes of Bayer ones (ensure_raw_stages)
  uint8_t *grey0, *grey1;           // the results; without a binning mono8 windows are copied straight into them.  grey1 null: one image (RGB-D)
  // the caller's choice: the two colour windows become grey in ONE k_to_mono launch of two frames, not two launches of one.  It needs
  // grey1 == grey0 + W H (the staged windows are a window's bytes apart anyway); the synchronous calls ask for it, the stream never does
  bool batch2;
  // the images pass through a stage and kernels make the grey images (false: mono8 windows, copied straight into grey0 / grey1)
  bool staged() const { return rectify || lay.encoding != MOD_ENCODING_MONO8 || binned(bin); }
  // ... and that stage is `stage` (false: raw messages when rectifying; mono8 windows on their way to k_bin_mono lie in bin_grey)
  bool windows_staged() const { return !rectify && lay.encoding != MOD_ENCODING_MONO8; }
};
// rectifying: room for two raw messages of in.lay in *in.raw and, when they are Bayer mosaics, for their two grey planes in *in.bayer_grey
int ensure_raw_stages(ModContext *c, const ImageIngest &in);
// binning: room for the two full-window grey planes in *in.bin_grey (nothing to do while it is off)
int ensure_bin_stage(ModContext *c, const ImageIngest &in);
// the copies, on copy_stream: whole messages when rectifying, else Bayer regions / mono8 windows / colour windows
int ingest_copy(ModContext *c, const ImageIngest &in, const uint8_t *img0, const uint8_t *img1, hipStream_t copy_stream);
// the kernels, on the context's stream: k_rectify (behind k_bayer_to_mono), k_bayer_to_mono, k_to_mono, then k_bin_mono when binning; none unless in.staged()
int ingest_to_grey(ModContext *c, const ImageIngest &in);

// host_depth.hip
// The temporal depth filter's history is gone (a set or reset call, mod_forget_previous, a skipped depth submit, new planes, another lattice).
// A flag and not a memset, which would have to be ordered with the enqueued work: the next launch is told neither to read nor to trust the planes
inline void forget_depth_history(ModContext *c) { c->depth_tstate.fresh = true; }
// the depth layout the RGB-D entry points read (the set one, or 16UC1 packed W x H; with a decimation (dx W) x (dy H)), checked against the camera and the registration
int current_depth_layout(ModContext *c, ModDepthLayout *out);
// The snapshot of a call / submit whose messages have the checked layout `l`, made once its arguments are checked: the ray tables are built behind
// the context's stream unless they are the cached ones (refused without a registration, and when a table in use would have to be rebuilt while
// tickets are outstanding; p->rays stays null while no distortion is set)
int depth_plan(ModContext *c, const ModDepthLayout &l, bool own_input, DepthPlan *p);
// The one chain of device depth messages to disparity planes, on the context's stream: `frames` messages of p.lay through k_depth_filter, then
// k_depth_spatial, then k_depth_temporal (against the context's state, emptied first where the lattice differs from the last launch's), then
// k_depth_decimate (the window's blocks into a packed scratch of the camera's size, which the conversion reads at origin 0), then
// k_depth_to_disparity or, registered, the scatter through zbuf [frames][W H].  A stage that is off allocates and enqueues nothing.  The spatial
// stage never works in place (it writes the filtered scratch, or a second one where that is its input); the temporal stage works in place
// on the library's own buffers (p.own_input, the scratches) and writes the filtered scratch where its input is a caller's
int run_depth_chain(ModContext *c, int frames, const void *depth, const DepthPlan &p, uint32_t *zbuf, float *disparity);
// What of a host depth message crosses PCIe for a submit: copy_window's rectangle at (x, y) of w x h pixels of bpp bytes, and the layout of the
// staged copy, a message of its own that begins at (x, y) of the camera's.  Unregistered: the camera's window with its apron of R_filter + R_spatial
// message pixels (window / 2 of the filter's support rule and of the spatial stage, each 0 while it is off; with a decimation the window is (dx W) x (dy H)) clamped to the message per side: every
// sample of the window sees the neighbours the whole message would show it, and those neighbours theirs; rows packed.  Registered: the whole message as it is, rows of `step` bytes
struct DepthStage { int x, y, bpp, w, h; ModDepthLayout lay; size_t bytes() const { return (size_t)w * bpp * h; } };
DepthStage depth_stage(const ModContext *c, const DepthPlan &p);

// host_sgm.hip
int check_sgm_params(ModContext *c, const ModSgmParams *p);
// host_flow.hip
int check_flow_params(ModContext *c, const ModFlowParams *p, int frames);
// host_filters.hip
inline bool texture_applies(const ModTextureFilter &f, int to) { return f.threshold > 0 && (f.apply & to) != 0; }   // to: MOD_TEXTURE_DISPARITY / _FLOW
int ensure_speckle_scratch(ModContext *c, int frames);   // the speckle filter's planes for `frames` frames (grow-only)
int ensure_disparity_fill_scratch(ModContext *c, int frames);   // the disparity plane in front of the hole fill for `frames` frames (grow-only)
int ensure_disparity_smooth_scratch(ModContext *c, int frames);   // the disparity plane in front of the smoother for `frames` frames (grow-only)
// host_ego.hip
int check_ego_params(ModContext *c, const ModEgoParams *p);
// the ego-motion estimator over `frames` frames; tf == null: into b.ego.tf, res == null: into b.ego.res; fc != null: also the frames' scene-flow constants (with dt) into fc
int run_egomotion(ModContext *c, int frames, const float *dprev, const float *dnow, const float *flow, const ModEgoParams *p, ModTransform *tf, ModEgoResult *res, FrameConst *fc, double dt);
