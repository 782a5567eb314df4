// mod_launch.h — host-callable launchers of the gfx950 kernels (internal to libmod_sf.so).
#pragma once
#include "../../include/mod_sf.h"
#include "mod_device.h"
#include "label_palette.h"
#include "depth_rays.h"

struct SfArgs {
  const float *dnow, *dprev, *flow;   // [F][H][W], [F][H][W], [F][H][W][2]
  float *x, *y, *z, *vx, *vy, *vz;    // [F][H][W]
  uint64_t *mask;                     // [F][H][mask_words] or null
  float4 *aos;                        // [F][H][W][2 x float4] or null
  float *depth;                       // [F][H][W] or null
  float *sflow;                       // [F][H][W][2] or null
  const FrameConst *fc;               // [F] device
  int32_t *tilehdr;                   // [F][tiles][2] or null: header word 0 of every cluster tile with a dynamic pixel is set to 1
  int32_t tile_rows, tiles_x, tiles_per_frame;   // (zeroed by the caller beforehand); tile = 64 x tile_rows pixels
  float2 *zrange;                     // [F][H][mask_words] or null: (smallest, largest) depth z of the DYNAMIC pixels of every non-zero mask
                                      // word, written with the word (k_ccl_bits decides one-class tiles from it without loading a depth row)
  unsigned long long *dbg;            // the context's diagnostic counters (checked build: index assertion 16), unused by a product build
};

constexpr int kClusterCounters = 8;   // words per frame of ClArgs::counters
constexpr int kTileHdrWords = 2;      // words per tile of ClArgs::tilehdr / SfArgs::tilehdr

// Scratch the clustering kernels work in; all device pointers, sized by the context.
struct ClArgs {
  const float *x, *y, *z, *vx, *vy, *vz;  // input planes [F][H][W]
  const uint64_t *mask;       // [F][H][mask_words] dynamic bits
  const float2 *zrange;       // [F][H][mask_words] depth range of the dynamic pixels of every NON-ZERO mask word (the fused scene-flow
                              // kernel's epilogue writes it with the word; entries of zero words are undefined), or null: a caller's cloud
  uint64_t *lroot;            // [F][H][mask_words] pixel is the root of a tile-local component (owns a partial record)
  int32_t *parent;            // [F][N] union-find parents (only dynamic entries are ever touched)
  int32_t *rootlist;          // [F][N] pixel indices of the final roots (aliases `mpix`, dead before k_final)
  int32_t *labels;            // [F][N] output plane; used as the root/code plane in between
  int32_t *rsize;             // [F][N] member count of the component rooted at this pixel (sparse: only root entries are touched); after
                              // k_select, at the final root of a surviving cluster: start of the cluster's member segment
  int32_t *rkey;              // [F][N] its first_edge_key; after k_ccl_merge, at a tile root that is not final: its members' place inside the
                              // component's member segment; after k_select, at a final root: the new label, or -1
  ClusterBox *cbox;           // [F][max_objects] bounding boxes of the surviving clusters (k_select init, k_final atomics)
  int32_t *counters;          // [F][8]: 0 n_comps, 1 n_clusters, 2 workgroups of k_ccl_merge done with the frame (of frame 0, later: of
                              // k_median_ties done); of frame 0 also (counts of the whole launch): 3 cursor into `tilelist`, 4 its
                              // length, 5 k_median's cursor into `worklist`, 6 its length, 7 length of `tielist`.  ALL ZERO between
                              // calls: k_median_ties' last workgroup clears them
  ClusterInfo *clusters;      // [F][max_objects]
  uint32_t *mbits;            // [F][N] ||v|| bit patterns of the members, grouped per cluster (SoA with mpix)
  uint32_t *mpix;             // [F][N] pixel index of each member
  uint32_t *worklist;         // [F * max_objects] frame * max_objects + cluster of every cluster of the launch; count in counters[6]
  uint32_t *tielist;          // [F * max_objects] the clusters k_median flagged ambiguous;                count in counters[7]
  void *objects;              // [F][max_objects] ModObject
  int32_t *n_objects;         // [F]
  int32_t *n_clusters;        // [F] or null
  int32_t max_objects;
  int32_t xy_from_z;          // the planes are the fused scene-flow kernel's of this call: x, y of a valid pixel are functions of z
  uint2 *requests;            // [F][tiles][req_cap] cross-tile link requests (halo pixel, tile root)
  int32_t *tilehdr;           // [F][tiles][2]: 0 no dynamic pixel / 1 has one (set together with the mask words) / 2 done by k_ccl_bits;
                              // number of requests.  Word 0 is ZERO between calls: k_final, its last reader, clears it
  uint32_t *tilelist;         // [F * tiles] tiles that k_ccl_bits left to the union-find kernel (frame * tiles + tile)
  int32_t req_cap;
  unsigned long long *dbg;    // [96] diagnostic counters (mod_device.h): cycle counters when DevCam.debug & 128, index assertions of the checked build
};

// inline_consts: the frames' constants ride in the kernel arguments (frames <= MOD_SF_INLINE_FRAMES; a.fc is not read), or null
#define MOD_SF_INLINE_FRAMES 8
void launch_scene_flow(const DevCam &c, const SfArgs &a, int frames, const FrameConst *inline_consts, hipStream_t s);
void launch_dynamic_mask(const DevCam &c, int frames, const float *vx, const float *vy, const float *vz, uint64_t *mask,
                         hipStream_t s);
void launch_depth(const DevCam &c, int frames, const float *dnow, float *depth, hipStream_t s);
// n 8-byte words from (device-visible, e.g. pinned host) src to dst
void launch_copy_words(const unsigned long long *src, unsigned long long *dst, size_t n, hipStream_t s);
void launch_pack(size_t n, const float *x, const float *y, const float *z, const float *vx, const float *vy, const float *vz,
                 void *aos, hipStream_t s);
void launch_unpack(size_t n, const void *aos, float *x, float *y, float *z, float *vx, float *vy, float *vz, hipStream_t s);

// clustering kernels, one launcher per timed stage (include/mod_sf.h MOD_STAGE_*)
void launch_ccl_tile(const DevCam &c, const ClArgs &a, int frames, hipStream_t s);
void launch_tile_flags(const DevCam &c, const ClArgs &a, int frames, hipStream_t s);   // tile headers from a mask plane
void launch_ccl_link(const DevCam &c, const ClArgs &a, int frames, hipStream_t s);
void launch_ccl_merge(const DevCam &c, const ClArgs &a, int frames, ClusterInfo *rank_scratch, hipStream_t s);   // + size filter
void launch_final(const DevCam &c, const ClArgs &a, int frames, hipStream_t s);
void launch_median(const DevCam &c, const ClArgs &a, int frames, hipStream_t s);
// The member lists of the launch's clusters (ModClusterMembers, moved to the launch's first frame): offsets [F][max_objects + 1],
// indices [F][N], points [F][N][3] or null.  Between launch_final and launch_median: k_median_ties reuses the arrays it reads
struct ClusterMemberOut { int32_t *offsets, *indices; float *points; };
void launch_cluster_members(const DevCam &c, const ClArgs &a, const ClusterMemberOut &m, int frames, hipStream_t s);
// The cluster image (label_image.hip): labels [frames][W H] and n_clusters [frames] -> image [frames][W H][3] B, G, R (4-byte aligned);
// labels outside [0, n_clusters[f]) are black.  The table rides in the kernel's arguments
void launch_cluster_image(int W, int H, int frames, const int32_t *labels, const int32_t *n_clusters, const label_palette::Table &table,
                          uint8_t *image, hipStream_t s);
// The flow and disparity images (flow_image.hip; flow_color.h has the rule): flow [frames][W H][2] (minus still, same shape, when
// not null) or disparity [frames][W H] -> image [frames][W H][3] B, G, R (4-byte aligned); the planes 4-byte aligned
void launch_flow_image(int W, int H, int frames, const float *flow, const float *still, float max_px, uint8_t *image, hipStream_t s);
void launch_disparity_image(int W, int H, int frames, const float *disparity, float dmin, float dmax, uint8_t *image, hipStream_t s);
// calculateStaticOpticalFlow alone: dprev [frames][H][W], transforms [frames] in device memory -> static_flow [frames][H][W][2] (8-byte aligned)
void launch_static_flow(const DevCam &c, int frames, const float *dprev, const ModTransform *transforms, float *static_flow, hipStream_t s);
int ccl_tile_rows();                 // tile height of k_ccl_tile
int ccl_tiles(int mask_words, int H); // cluster tiles of a frame of H rows of mask_words words (a tile is one word wide)
int ccl_request_capacity(int n);     // link requests one tile can emit at neighbor_distance n

// on-GPU disparity (sgm.hip)
constexpr int kSgmPaths = 8;          // aggregation paths at most: the side streams, the join events and the volumes of a set count them
// words that must be readable in front of a right census plane `cr` when D == 128: the four-lines-per-wave kernels (the only ones for
// that count) read their census windows unconditionally, up to off + 127 <= kSgmCensusLead - 1 words to the left of a row (off: the
// disparity offset, at most kSgmMaxOffset); those words belong to disparities that do not exist and are never used
constexpr int kSgmMaxOffset = 128;    // mod_set_disparity_offset's largest value
constexpr int kSgmCensusLead = kSgmMaxOffset + 128;
void launch_sgm_census(int W, int H, int frames, const uint8_t *img, uint32_t *out, hipStream_t s);
// direction: the reference's numbering (sgm.hip kSgmDir); off: the disparity offset (index d stands for the disparity off + d)
void launch_sgm_path(int W, int H, int frames, int D, int off, int P1, int P2, int direction, const uint32_t *cl, const uint32_t *cr,
                     uint8_t *L, uint8_t *cost, hipStream_t s);
bool launch_sgm_paths_all(int W, int H, int frames, int D, int off, int P1, int P2, int paths, size_t path_stride, const uint32_t *cl, const uint32_t *cr,
                          uint8_t *L, hipStream_t s);

// The winner-take-all maps of a group and their 3 x 3 medians, [group][N] each, inside one allocation.  The left maps hold d in 8 bits
// or, in the sub-pixel mode, 16 d + q in 16 bits; the right maps are 8-bit in both.
struct SgmMaps {
  void *left, *left_median;           // uint8_t (left_bytes 1) or uint16_t (2)
  uint8_t *right, *right_median;
  int left_bytes;
};
constexpr size_t sgm_maps_bytes(bool subpixel) { return 2 * (subpixel ? 2 : 1) + 2; }   // per pixel of a frame: two left, two right maps
// 8-bit: left, right, left median, right median; sub-pixel: the two 16-bit left maps, then the two right maps
inline SgmMaps sgm_carve_maps(uint8_t *base, size_t N, int group, bool subpixel) {
  const size_t n = N * group;
  if (subpixel) return {base, base + 2 * n, base + 4 * n, base + 5 * n, 2};
  return {base, base + 2 * n, base + n, base + 3 * n, 1};
}
// winner-take-all, median, left-right check.  uniqueness: 0 = off, else the ratio in percent (mod_set_disparity_filters)
void launch_sgm_finish(int W, int H, int frames, int D, int off, int paths, size_t path_stride, int median, int lr_check, int uniqueness, const uint8_t *Lv,
                       const SgmMaps &m, float *disparity, hipStream_t s);

// speckle filter (disparity_filter.hip), in place on `disparity` [frames][H][W]: regions (4-connected, neighbours within speckle_range,
// pixels finite and >= lo) of at most speckle_size pixels become `invalid`.  parent / size: [frames][H][W] scratch of the filter's own
void launch_speckle(int W, int H, int frames, float lo, float invalid, int speckle_size, int speckle_range, float *disparity,
                    int32_t *parent, int32_t *size, unsigned long long *dbg, hipStream_t s);

// edge-preserving smoother of a finished disparity (disparity_smooth.hip): `in` [frames][H][W] -> `out` of the same size, a different plane
// (checked by the caller, as window 3 / 5 / 7, a finite tol >= 0 and min_members 1..window^2 are); a word is valid when it is finite and
// >= lo.  ONE launch; every pixel of `out` is stored, `in` is only read
void launch_disparity_smooth(int W, int H, int frames, float lo, int window, float tol, int min_members, const float *in, float *out, hipStream_t s);

// occlusion hole fill of a finished disparity (disparity_fill.hip): `in` [frames][H][W] -> `out` of the same size, a different plane
// (checked by the caller, as reach 1..256, directions 2 / 4 / 8, the mode and min_found 1..directions are); a word is valid when it is
// finite and >= lo.  ONE launch; every pixel of `out` is stored, `in` is only read
void launch_disparity_fill(int W, int H, int frames, float lo, int reach, int directions, int mode, int min_found, const float *in, float *out,
                           hipStream_t s);

// texture measure (texture.hip) of grey planes [frames][H][W]: T = the window x window sum of the horizontal central differences capped
// at `cap` (window odd in 3..15, cap in 1..255; checked by the caller).  ONE launch: `texture` non-null: T itself into [frames][H][W]
// uint16; else every pixel with T < threshold becomes `invalid` in `disparity` [frames][H][W] and (NaN, NaN) in `flow` [frames][H][W][2]
// (either may be null), and nothing else of the two planes is read or written
void launch_texture(int W, int H, int frames, int window, int cap, int threshold, const uint8_t *grey, uint16_t *texture, float *disparity,
                    float invalid, float *flow, hipStream_t s);

// min-eigenvalue measure (corner.hip) of grey planes [frames][H][W]: E = the floor of the smaller eigenvalue of the window x window sum
// of the gradient structure tensor, gradients capped at +-`cap` (window odd in 3..15, cap in 1..255; checked by the caller).  ONE
// launch: `strength` non-null: E itself into [frames][H][W] uint32; else every pixel with E < threshold becomes (NaN, NaN) in `flow`
// [frames][H][W][2], and nothing else of it is read or written
void launch_corner(int W, int H, int frames, int window, int cap, int threshold, const uint8_t *grey, uint32_t *strength, float *flow,
                   hipStream_t s);

// NaN-aware median of a finished flow (flow_median.hip): `in` [frames][H][W][2] -> `out` of the same size, a different plane (a
// stencil cannot run in place; checked by the caller, as window 3 or 5 and min_valid 0 .. window^2 are).  ONE launch; every pixel of
// `out` is stored, `in` is only read
void launch_flow_median(int W, int H, int frames, int window, int min_valid, const float *in, float *out, hipStream_t s);

// disparity-gated hole fill of a finished flow (flow_fill.hip): `in` [frames][H][W][2] and the disparity planes of the same frames
// [frames][H][W] -> `out` of the flow's size, a different plane (checked by the caller, as window 3, 5 or 7, min_valid 1 .. window^2 - 1
// and the two tolerances are).  ONE launch; every pixel of `out` is stored, `in` and `disparity` are only read
void launch_flow_fill(int W, int H, int frames, int window, int min_valid, float tol_abs, float tol_rel, const float *in, const float *disparity,
                      float *out, hipStream_t s);

// on-GPU optical flow (flow.hip).  Pyramid level of both images: src0 / src1 [frames][Hs][Ws] -> dst [2][frames][H][W].
void launch_flow_pyramid(int Ws, int Hs, int W, int H, int frames, const uint8_t *src0, const uint8_t *src1, uint8_t *dst, hipStream_t s);
// one level, `dirs` directions (1: forward, 2: + backward); coarse == nullptr: the coarsest level.  census [2][frames][H][W] (prev, now),
// coarse [dirs][frames][H1][W1], out [dirs][frames][H][W], sub [frames][H][W] or null.  seeds (finer levels): 1 = the parent's winner,
// 5 = + the winners of the parent's four neighbours (mod_set_flow_propagation)
void launch_flow_match(int W, int H, int W1, int H1, int frames, int dirs, int window, int radius, int seeds, const uint32_t *census,
                       const short2 *coarse, short2 *out, short4 *sub, hipStream_t s);
// level 0 winners (+ backward field G when fb >= 0, + sub-pixel terms) -> flow [frames][H][W][2] f32
void launch_flow_finish(int W, int H, int frames, const short2 *F, const short2 *G, const short4 *sub, int fb, float *flow, hipStream_t s);

// on-GPU stereo ego-motion (egomotion.hip).  One launch sequence for `frames` frames; all pointers device.
struct EgoArgs {
  int W, H, frames, stride, gw, gh;   // grid of now pixels: gw = ceil(W / stride) columns, gh rows
  int cap;                            // correspondences per frame the scratch holds (>= gw * gh)
  int hyps, iterations, min_inliers;
  uint32_t seed;
  float dlo, dhi;                     // disparity range: max(camera min_disparity, min_disparity), camera max_disparity
  double th;                          // inlier_threshold
  double fx, fy, cx, cy, Tx, Ty, fT;  // fT = f64 of the F32 product disp_f * disp_T (DevCam.fT)
  const float *dprev, *dnow, *flow;   // [F][H][W], [F][H][W], [F][H][W][2]
  double *corr;                       // [F][9][cap]: P xyz, Q xyz, O (u, v, u_r) of the kept samples, raster order
  int32_t *blkcnt;                    // [F][ego_grid_blocks]: kept samples per block
  int32_t *ncorr;                     // [F]
  double *hyp;                        // [F][hyps][12]: row-major 3 x 4 motion of every hypothesis
  int32_t *hcnt;                      // [F][hyps]: inlier count, -1 = invalid hypothesis
  uint8_t *flag;                      // [F][cap]: inlier of the refinement's current selection
  double *tf;                         // [F][7] ModTransform
  ModEgoResult *res;                  // [F]
  FrameConst *fc;                     // [F] or null: the frames' scene-flow constants from the estimate, with dt
  double dt;
};
int ego_grid_blocks(int gw, int gh);   // blocks of the correspondence kernels per frame
void launch_egomotion(const EgoArgs &a, hipStream_t s);

// camera images to grey (ingest.hip).  Window W x H at (x0, y0) of each 8-bit frame (row pitch `step`, frames frame_bytes apart)
// -> dst [frames][H][W]; encoding MOD_ENCODING_*
int image_channels(int encoding);   // bytes per pixel; 0: unknown encoding
void launch_to_mono(int encoding, int W, int H, int frames, const uint8_t *src, size_t frame_bytes, int step, int x0, int y0, uint8_t *dst,
                    hipStream_t s);

// 8-bit Bayer mosaics to grey (bayer.hip).  Region rw x rh bytes (row pitch `step`, frames frame_bytes apart; rw, rh >= 3) whose
// byte (0, 0) lies `phase` into the RGGB tile; the window W x H at (x0, y0) of it -> dst [frames][H][W].  Pixels of the region's
// one-pixel frame copy the nearest interior result
void launch_bayer_to_mono(int W, int H, int frames, const uint8_t *src, size_t frame_bytes, int step, int rw, int rh, int x0, int y0, int phase,
                          uint8_t *dst, hipStream_t s);
// the phase of a region whose (0, 0) is pixel (x, y) of a MOD_ENCODING_BAYER_* message; -1: not a Bayer encoding
int bayer_phase(int encoding, int x, int y);
inline bool is_bayer(int encoding) { return bayer_phase(encoding, 0, 0) >= 0; }

// grey planes reduced by an integer factor (binning.hip).  src: packed planes [frames][by H][bx W] -> dst [frames][H][W]; b: factors
// and mode, checked by the caller (mod_set_image_binning)
void launch_bin_mono(const ModImageBinning &b, int W, int H, int frames, const uint8_t *src, uint8_t *dst, hipStream_t s);

// raw camera images to rectified grey (rectify.hip). map: device int32 [H][W][2], where each pixel of the W x H window lies in the
// width x height message (1/32 pixel; launch_rectify_map fills it for the window at (x0, y0)) -> dst [frames][H][W].
// Frames lie frame_bytes apart; `extent` bytes from a frame's first one may be loaded (step * height, or less for a pane of a
// side-by-side message: src then points at the pane and width is the pane's)
void launch_rectify(int encoding, int W, int H, int frames, const uint8_t *src, size_t frame_bytes, size_t extent, int step, int width,
                    int height, const int32_t *map, uint8_t *dst, hipStream_t s);
// k_rectify_map on s: the map of `cam` under distortion model `model` (MOD_DISTORTION_*) for the W x H window at (x0, y0)
hipError_t launch_rectify_map(int model, const ModRectifyCamera &cam, int x0, int y0, int W, int H, int32_t *map, hipStream_t s);
const char *check_distortion(int model, const ModRectifyCamera &cam);   // null: cam's D fits the model, else what is wrong with it
const char *check_rectify_camera(const ModRectifyCamera &cam);   // null: valid, else what is wrong with it

// depth images to disparity (depth.hip).  Window W x H at (x0, y0) of each depth frame (MOD_DEPTH_*, row pitch `step`, frames
// frame_bytes apart) -> dst [frames][H][W]: fT / (sample * unit) where that is positive and finite, else `invalid`
int depth_bytes(int encoding);      // bytes per sample; 0: unknown encoding
void launch_depth_to_disparity(int encoding, int W, int H, int frames, const void *src, size_t frame_bytes, int step, int x0, int y0, float unit,
                               float fT, float invalid, float *dst, hipStream_t s);
// the range and flying-pixel filter (depth_filter.hip, mod_set_depth_filter): `frames` whole width x height messages of row pitch
// `step`, step * height bytes apart, src -> dst of the same layout (not in place); flt is valid; window 0 and both bounds 0: a copy
void launch_depth_filter(int encoding, int width, int height, int frames, const void *src, int step, float unit, const ModDepthFilter &flt,
                         void *dst, hipStream_t s);
// the edge-preserving smoother and hole fill (depth_spatial.hip, mod_set_depth_spatial): `frames` whole width x height messages of row
// pitch `step`, step * height bytes apart, src -> dst of the same layout (not in place); sp is valid and on (window 3, 5 or 7)
void launch_depth_spatial(int encoding, int width, int height, int frames, const void *src, int step, float unit, const ModDepthSpatial &sp,
                          void *dst, hipStream_t s);
// the temporal filter with hold (depth_temporal.hip, mod_set_depth_temporal): `frames` consecutive whole width x height messages of row
// pitch `step`, step * height bytes apart, src -> dst of the same layout (dst == src is allowed); state_s / state_age are packed
// height x width planes, updated in place; fresh: they are not read and every pixel starts empty; t is valid and on (alpha != 0)
void launch_depth_temporal(int encoding, int width, int height, int frames, const void *src, int step, float unit, const ModDepthTemporal &t,
                           bool fresh, float *state_s, uint8_t *state_age, void *dst, hipStream_t s);
// the decimation (depth_decimate.hip, mod_set_depth_decimation): the d.dx x d.dy blocks that start at (x0, y0) of `frames` messages of row
// pitch `step`, frame_bytes apart -> dst, PACKED messages of out_w x out_h samples (x0 + d.dx out_w <= width, y0 + d.dy out_h <= height:
// checked by the caller, as d is); not in place; d.dx = d.dy = 1: a copy of the window
void launch_depth_decimate(int encoding, int out_w, int out_h, int frames, const void *src, size_t frame_bytes, int step, int x0, int y0, float unit,
                           const ModDepthDecimation &d, void *dst, hipStream_t s);
// the depth camera (of the whole message) and its pose, then the image camera whose W x H window the samples land in
struct DepthRegArgs { double fxd, fyd, cxd, cyd, R[9], t[3], fx, fy, cx, cy, Tx, Ty; };
// the registered path: every sample of the whole width x height messages (frames step * height bytes apart) through g into the
// z-buffer zbuf [frames][H][W] (cleared here), the nearest sample of every target -> dst as above, targets nothing hit -> `invalid`;
// splat: every sample paints its footprint too (k_depth_register_splat, mod_set_depth_splat)
// rays.centres non-null (mod_set_depth_distortion): X0, Y0 come from the depth camera's ray tables instead of the pinhole
// (k_depth_register_rays, k_depth_register_splat_rays; the splat reads rays.corners too)
struct DepthRayTables {
  const double2 *centres;   // [height][width]: the ray of message pixel (U, V); null: no distortion
  const double2 *corners;   // [height + 1][width + 1]: entry [j][i] is the ray of (i - 0.5, j - 0.5); read by the splat only
};
hipError_t launch_depth_register(int encoding, int W, int H, int frames, const void *src, int width, int height, int step, float unit,
                                 const DepthRegArgs &g, bool splat, const DepthRayTables &rays, float fT, float invalid, uint32_t *zbuf,
                                 float *dst, hipStream_t s);
// k_depth_rays on s: table [rows][cols], entry [j][i] = the ray of lattice point (i + offset, j + offset) of the depth message
// (offset 0: pixel centres, cols x rows the message's size; offset -0.5: pixel corners, one more per axis)
hipError_t launch_depth_rays(const depth_rays::Lens &lens, double offset, int cols, int rows, double2 *table, hipStream_t s);
