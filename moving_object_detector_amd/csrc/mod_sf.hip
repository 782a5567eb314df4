// mod_sf.hip — C ABI (include/mod_sf.h) over the gfx950 kernels: context lifecycle and configuration, the batched scene-flow /
// cluster / process path, parameter folding, stage timers, memory helpers.  Host-side only; the kernels live in sceneflow.hip and
// the clusterer's ccl_*.hip / cluster_*.hip, the estimators' entry points in estimators.hip, the host-pointer calls in host_api.hip.
#include "mod_context.h"
#include "exact_div.h"
#include "mod_sf_debug.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

namespace {

constexpr int kChunkMinFrames = 32; // mod_process_dev's chunks have at least this many frames each (a chunk must still fill the GPU on its own)
constexpr int kAutoChunks = 1;      // ModConfig.batch_chunks == 0: one piece (see process_chunked for what two chunks gain, and when)

// smallest float t with (double)t >= th: for float a, ((double)a >= th) <=> (a >= t)
float ceil_to_f32(double th) {
  if (std::isnan(th)) return std::nanf("");
  float t = (float)th;
  if ((double)t < th) t = std::nextafterf(t, INFINITY);
  return t;
}
// largest float t with (double)t <= th: for float a, ((double)a > th) <=> (a > t)
float floor_to_f32(double th) {
  if (std::isnan(th)) return std::nanf("");
  float t = (float)th;
  if ((double)t > th) t = std::nextafterf(t, -INFINITY);
  return t;
}

// Smallest F32 a >= 0 with sqrtf(a) >= th, so that the kernels test a sum of squares instead of taking its root:
// sqrtf is correctly rounded (host libm and the device build alike) and therefore monotone, which makes the two tests
// agree on every input (a NaN fails both; th <= 0 accepts every sum of squares, which is >= +0).
float sqrt_threshold_sq(float th) {
  if (std::isnan(th)) return th;                            // never true, like the original comparison
  if (!(th > 0.0f)) return 0.0f;
  const float inf = std::numeric_limits<float>::infinity();
  if (std::isinf(th)) return inf;
  float a = (float)((double)th * (double)th);
  while (a > 0.0f && sqrtf(std::nextafterf(a, 0.0f)) >= th) a = std::nextafterf(a, 0.0f);
  while (a < inf && !(sqrtf(a) >= th)) a = std::nextafterf(a, inf);
  return a;
}

struct StageTimer {
  ModContext *c; int stage; hipStream_t s; EventPair ev{}; bool on;
  StageTimer(ModContext *ctx, int st, hipStream_t stream) : c(ctx), stage(st), s(stream), on((ctx->profiling >> st) & 1) {
    if (!on) return;
    if (!c->free_events.empty()) { ev = std::move(c->free_events.back()); c->free_events.pop_back(); }
    else { (void)hipEventCreate(ev.a.put()); (void)hipEventCreate(ev.b.put()); }
    (void)hipEventRecord(ev.a, s);
  }
  ~StageTimer() {
    if (!on) return;
    (void)hipEventRecord(ev.b, s);
    c->pending[stage].push_back(std::move(ev));
  }
};

void drain_timers(ModContext *c) {
  for (int s = 0; s < MOD_STAGE_COUNT; s++) {
    for (EventPair &ev : c->pending[s]) {
      (void)hipEventSynchronize(ev.b);
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) { c->stage_ms[s] += ms; c->stage_calls[s] += 1; }
      c->free_events.push_back(std::move(ev));
    }
    c->pending[s].clear();
  }
}

void fill_frame_const(FrameConst &h, const ModTransform &tf, double dt) { fill_frame_const(h, tf.t, tf.q, dt); }   // frame_const.h

// The per-frame constants of a batch.  Up to MOD_SF_INLINE_FRAMES frames: into `inl`, which the scene-flow launch passes in its
// kernel arguments (inl->used) — nothing is copied, nothing waited for.  Larger batches: through the pinned ring into c->b.fc.
struct InlineConsts { FrameConst v[MOD_SF_INLINE_FRAMES]; bool used = false; };

int upload_frame_consts(ModContext *c, const ModFrameBatch *in, InlineConsts *inl) {
  if (c->fc_resident) return MOD_OK;
  if (inl && in->frames <= MOD_SF_INLINE_FRAMES) {
    for (int f = 0; f < in->frames; f++) fill_frame_const(inl->v[f], in->transforms[f], in->dt[f]);
    inl->used = true;
    return MOD_OK;
  }
  const int slot = c->ring_pos;
  c->ring_pos = (c->ring_pos + 1) % kRing;
  HIP_TRY(c, hipEventSynchronize(c->pinned_ev[slot]));   // the slot's previous copy has left the host buffer
  FrameConst *h = c->pinned[slot];
  for (int f = 0; f < in->frames; f++) fill_frame_const(h[f], in->transforms[f], in->dt[f]);
  // a kernel of ours reads the pinned slot over the host link (hipHostMalloc memory is mapped into the device's address space):
  // the runtime's own host-to-device copy is a blit kernel too, and the kernel behind it started 5 us after it had ended
  launch_copy_words((const unsigned long long *)h, (unsigned long long *)c->b.fc.get(), sizeof(FrameConst) / 8 * (size_t)in->frames, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(c->pinned_ev[slot], c->stream));
  return MOD_OK;
}

int check_batch(ModContext *c, const ModFrameBatch *in) {
  if (!in) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null batch");
  int rc = check_ready(c, in->frames);
  if (rc) return rc;
  return construct_skip(in->flow, in->disparity_prev, in->transforms && in->dt, in->disparity_now);
}

// frames [f0, f0 + n) of a batch: every per-frame pointer of the launch moves to the chunk's first frame, so that "frame 0 of the
// launch" — where the clustering kernels keep their launch-wide counters and lists — is the chunk's own
struct Chunk { int f0, n; };

int check_scene_flow_out(ModContext *c, const ModSceneFlowPlanes *out, bool xy_optional) {
  if (!out || !out->z || !out->vx || !out->vy || !out->vz)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "scene-flow output planes z,vx,vy,vz are required");
  // x and y: both or neither; neither only where the call says so (mod_process_dev: the cluster stage recomputes them from z)
  if ((out->x == nullptr) != (out->y == nullptr) || (!out->x && !xy_optional))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, xy_optional ? "scene-flow output planes x and y: pass both or neither" : "scene-flow output planes x,y,z,vx,vy,vz are required");
  return MOD_OK;
}

// the scene-flow kernel over one chunk of the batch (the per-frame constants of the WHOLE batch are in c->b.fc by now)
void enqueue_scene_flow(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *out, uint64_t *mask, bool tile_flags, Chunk ch,
                        hipStream_t s, const InlineConsts *inl = nullptr) {
  const size_t N = (size_t)c->dc.W * c->dc.H, f0 = (size_t)ch.f0, MWH = (size_t)c->dc.mask_words * c->dc.H;
  SfArgs a;
  a.dnow = in->disparity_now + f0 * N; a.dprev = in->disparity_prev + f0 * N; a.flow = in->flow + f0 * N * 2;
  a.x = out->x ? out->x + f0 * N : nullptr; a.y = out->y ? out->y + f0 * N : nullptr;
  a.z = out->z + f0 * N; a.vx = out->vx + f0 * N; a.vy = out->vy + f0 * N; a.vz = out->vz + f0 * N;
  a.mask = mask ? mask + f0 * MWH : nullptr;
  a.aos = out->cloud_aos ? (float4 *)out->cloud_aos + f0 * N * 2 : nullptr;
  a.depth = out->depth ? out->depth + f0 * N : nullptr;
  a.sflow = out->static_flow ? out->static_flow + f0 * N * 2 : nullptr;
  a.fc = c->b.fc + f0;
  a.tilehdr = nullptr; a.zrange = nullptr; a.tile_rows = ccl_tile_rows(); a.tiles_x = c->dc.mask_words;
  a.tiles_per_frame = c->dc.mask_words * ((c->dc.H + ccl_tile_rows() - 1) / ccl_tile_rows());
  a.dbg = c->b.dbg;
  if (tile_flags && mask) {      // the clustering follows: the kernel's epilogue also marks the cluster tiles that hold a dynamic pixel
    a.tilehdr = c->b.tilehdr + f0 * 2 * (size_t)a.tiles_per_frame;   // (all zero: ModContext::scratch_clean)
    a.zrange = c->b.zrange + f0 * MWH; // ... and leaves the depth range of every non-zero mask word's dynamic pixels for the tile stage
  }
  StageTimer t(c, MOD_STAGE_SCENE_FLOW, s);
  launch_scene_flow(c->dc, a, ch.n, (inl && inl->used) ? inl->v : nullptr, s);
}

int run_scene_flow(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *out, uint64_t *mask, bool tile_flags, bool xy_optional) {
  int rc = check_scene_flow_out(c, out, xy_optional);
  if (rc) return rc;
  InlineConsts inl;
  if ((rc = upload_frame_consts(c, in, &inl))) return rc;
  enqueue_scene_flow(c, in, out, mask, tile_flags, Chunk{0, in->frames}, c->stream, &inl);   // (tile_flags: the caller has called begin_cluster_scratch)
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int check_cluster_io(ModContext *c, const ModSceneFlowPlanes *pl, bool flags_ready, const ModClusterOut *out) {
  // flags_ready: the planes are this call's own scene-flow output (mod_process_dev), where x, y are functions of z and may be absent
  if (!pl || !pl->z || !pl->vx || !pl->vy || !pl->vz || (!flags_ready && (!pl->x || !pl->y)))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster input planes x,y,z,vx,vy,vz are required");
  if (!out || !out->objects || !out->n_objects)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster outputs objects, n_objects are required");
  return MOD_OK;
}

// The clustering of one chunk on stream s.
void enqueue_cluster(ModContext *c, Chunk ch, const ModSceneFlowPlanes *pl, const uint64_t *mask, bool mask_ready, bool flags_ready,
                    const ModClusterOut *out, hipStream_t s) {
  const size_t N = (size_t)c->dc.W * c->dc.H, f0 = (size_t)ch.f0, MWH = (size_t)c->dc.mask_words * c->dc.H, MO = (size_t)c->max_objects;
  const size_t tiles = (size_t)c->dc.mask_words * ((c->dc.H + ccl_tile_rows() - 1) / ccl_tile_rows());
  const int frames = ch.n;
  ClArgs a;
  a.x = pl->x ? pl->x + f0 * N : nullptr; a.y = pl->y ? pl->y + f0 * N : nullptr;
  a.z = pl->z + f0 * N; a.vx = pl->vx + f0 * N; a.vy = pl->vy + f0 * N; a.vz = pl->vz + f0 * N;
  a.mask = mask + f0 * MWH; a.zrange = flags_ready ? c->b.zrange + f0 * MWH : nullptr; a.lroot = c->b.lroot + f0 * MWH;
  a.parent = c->b.parent + f0 * N; a.rootlist = (int32_t *)c->b.mpix.get() + f0 * N;
  a.labels = out->labels ? out->labels + f0 * N : nullptr; a.rsize = c->b.rsize + f0 * N; a.rkey = c->b.rkey + f0 * N;
  a.cbox = c->b.cbox + f0 * MO; a.counters = c->b.counters + f0 * 8; a.clusters = c->b.clusters + f0 * MO;
  a.mbits = c->b.mbits + f0 * N; a.mpix = c->b.mpix + f0 * N;
  a.worklist = c->b.worklist + f0 * MO; a.tielist = c->b.worklist + (size_t)c->cfg.max_frames * MO + f0 * MO;
  a.objects = (ModObject *)out->objects + f0 * MO; a.n_objects = out->n_objects + f0;
  a.n_clusters = out->n_clusters ? out->n_clusters + f0 : nullptr; a.max_objects = c->max_objects; a.dbg = c->b.dbg;
  a.xy_from_z = flags_ready ? 1 : 0;                  // only mod_process_dev's fused path hands over its own scene-flow planes
  const int req_cap = ccl_request_capacity(c->prm.neighbor_distance);
  a.requests = c->b.requests + f0 * tiles * (size_t)req_cap; a.tilehdr = c->b.tilehdr + f0 * tiles * 2; a.tilelist = c->b.tilelist + f0 * tiles;
  a.req_cap = req_cap;
  ClusterInfo *const rank_scratch = c->b.clusters + (size_t)c->cfg.max_frames * MO + f0 * MO;   // second half of the allocation
  {
    StageTimer t(c, MOD_STAGE_CCL_TILE, s);
    if (!mask_ready) launch_dynamic_mask(c->dc, frames, a.vx, a.vy, a.vz, (uint64_t *)a.mask, s);
    if (!flags_ready) launch_tile_flags(c->dc, a, frames, s);
    launch_ccl_tile(c->dc, a, frames, s);                 // (the counters are zero: ModContext::scratch_clean)
  }
  { StageTimer t(c, MOD_STAGE_CCL_LINK, s); launch_ccl_link(c->dc, a, frames, s); }
  { StageTimer t(c, MOD_STAGE_CCL_MERGE, s); launch_ccl_merge(c->dc, a, frames, rank_scratch, s); }
  { StageTimer t(c, MOD_STAGE_FINAL, s); launch_final(c->dc, a, frames, s); }
  { StageTimer t(c, MOD_STAGE_MEDIAN, s); launch_median(c->dc, a, frames, s); }
}

// How many chunks a fused call of `frames` frames runs in (ModConfig.batch_chunks; mod_sf.h).  One chunk while a per-kernel
// cluster timer is on: the kernels of different chunks run side by side, and a timer would price its kernel with its neighbours' load.
int chunk_count(const ModContext *c, int frames) {
  const int want = c->cfg.batch_chunks;
  const int per_kernel = ((1 << MOD_STAGE_CCL_TILE) | (1 << MOD_STAGE_CCL_LINK) | (1 << MOD_STAGE_CCL_MERGE) | (1 << MOD_STAGE_FINAL) |
                          (1 << MOD_STAGE_MEDIAN));
  if (c->profiling & per_kernel) return 1;
  int n = want ? want : kAutoChunks;
  n = std::min(n, kMaxChunks);
  while (n > 1 && frames / n < kChunkMinFrames) n--;
  return std::max(n, 1);
}

// mod_process_dev on a large batch, cluster stage in chunks (ModConfig.batch_chunks >= 2; opt-in).  The cluster stage ends in kernels
// that wait instead of moving bytes (cross-tile links, the root merge + size filter, the median selection, the tie replay: a few
// workgroups chasing pointers) and begins with one that is bound by workgroup dispatch (three quarters of the tiles are empty).  Cut
// into chunks of frames whose kernel chains run side by side on streams of their own, the waiting kernels of one chunk share the GPU
// with the streaming kernels of another; the hardware interleaves them as their workgroups come.  Measured (round 5, 512 pairs,
// profiles/README.md): in a process that has been running for a second or more, 2 chunks take 0.7 - 2.9 % off the step (in-process
// A/B on four boxes: tools/chunk_ab.py, tools/step_trace.py; bench.py --steps 200 --warmup 50: 5.11 - 5.18 vs 5.23 ms); in the first
// ~25 calls of a fresh process they ADD 2 % (bench.py --steps 20 --warmup 5: 5.28 - 5.31 vs 5.15 - 5.21 ms) — the first calls show
// hitches of ~0.9 ms each (the host falls behind while the runtime grows what the new streams need; a burst of fills and fork /
// join rounds at stream creation did not remove them).  Hence not the default.  Also measured with switches that have left the
// code again (commit d9702f0 of round 5 has them: ModConfig.batch_chunks bits 8 and 9): chains held one kernel apart by events — no better than free-running ones; 3 or
// 4 chunks like 2; the scene-flow kernel cut into the chunks too — +0.5 ... +3 % (it is bandwidth-bound throughout and gains
// nothing from company), so it stays ONE launch over the whole batch ahead of the chunks.
int process_chunked(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *pl, uint64_t *mask, const ModClusterOut *out, int C) {
  int rc = upload_frame_consts(c, in, nullptr);
  if (rc) return rc;
  enqueue_scene_flow(c, in, pl, mask, true, Chunk{0, in->frames}, c->stream);
  StageTimer group(c, MOD_STAGE_CLUSTER_GROUP, c->stream);
  HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
  hipError_t e = hipSuccess;
  int started = 1;                  // chunks enqueued behind the fork (chunk 0: the context's stream)
  for (int k = 0; k < C; k++) {
    const Chunk ch{(int)((int64_t)in->frames * k / C), (int)((int64_t)in->frames * (k + 1) / C - (int64_t)in->frames * k / C)};
    hipStream_t s = k ? c->chunk_stream[k - 1] : c->stream;
    if (k && (e = hipStreamWaitEvent(s, c->ev_fork, 0)) != hipSuccess) break;
    started = k + 1;
    enqueue_cluster(c, ch, pl, mask, true, true, out, s);
  }
  // join every chunk stream that has started, after a failure too: the next call's scratch memsets (begin_cluster_scratch) must
  // queue behind the cluster kernels already enqueued
  for (int k = 1; k < started; k++) {
    hipError_t j = hipEventRecord(c->ev_join[k - 1], c->chunk_stream[k - 1]);
    if (j == hipSuccess) j = hipStreamWaitEvent(c->stream, c->ev_join[k - 1], 0);
    if (e == hipSuccess) e = j;
  }
  if (e != hipSuccess) return fail(c, MOD_ERR_DEVICE, std::string("process_chunked fork / join: ") + hipGetErrorString(e));
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

}  // namespace

int check_layout(ModContext *c, const ModImageLayout &l, bool panes) {
  const int C = image_channels(l.encoding);
  if (!C) return fail(c, MOD_ERR_INVALID_ARGUMENT, "unknown image encoding");
  if (l.width < 1 || l.height < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "image size must be positive");
  if (is_bayer(l.encoding) && (l.width < 3 || l.height < 3))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "a Bayer image must be at least 3 x 3 (a pixel of its frame copies an interior one)");
  if ((int64_t)l.step < (int64_t)l.width * C) return fail(c, MOD_ERR_INVALID_ARGUMENT, "step is smaller than width * channels");
  if (panes && (int64_t)l.step < 2 * (int64_t)l.width * C)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "side by side: step is smaller than 2 * width * channels (width is one eye's)");
  if (l.x0 < 0 || l.y0 < 0 || (int64_t)l.x0 + c->dc.W > l.width || (int64_t)l.y0 + c->dc.H > l.height)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the camera-sized window does not fit inside the image");
  return MOD_OK;
}

int current_layout(ModContext *c, ModImageLayout *out) {
  *out = c->has_layout ? c->layout : ModImageLayout{MOD_ENCODING_MONO8, c->dc.W, c->dc.H, c->dc.W, 0, 0};
  if (!c->has_layout && !c->side_by_side) return MOD_OK;
  return check_layout(c, *out, c->side_by_side);   // the camera may have changed since the layout was set
}

// (callers have checked that a rectification is set and that eye is one of the two)
int ensure_rectify_map(ModContext *c, int eye, const ModImageLayout &l) {
  const ModRectifyCamera &cam = c->rect.cam[eye];
  if (l.width != cam.width || l.height != cam.height)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the image layout's width / height differ from the rectification's");
  ModContext::Rectify::Map &m = c->rect.map[eye];
  const int W = c->dc.W, H = c->dc.H;
  if (m.valid && m.width == l.width && m.height == l.height && m.x0 == l.x0 && m.y0 == l.y0 && m.W == W && m.H == H) return MOD_OK;
  if (c->pipe.in_flight > 0)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the rectification map must be rebuilt while frames are in flight: collect every ticket first");
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // kernels of calls and of frames that ended at a guard may still read the old map
  HIP_TRY(c, dalloc(m.q, 2 * c->maxN));
  m.valid = false;
  std::vector<int32_t> host(2 * (size_t)W * H);
  build_rectify_map(cam, l.x0, l.y0, W, H, host.data());
  HIP_TRY(c, hipMemcpyAsync(m.q, host.data(), sizeof(int32_t) * host.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // `host` is stack-owned
  m.width = l.width; m.height = l.height; m.x0 = l.x0; m.y0 = l.y0; m.W = W; m.H = H;
  m.valid = true;
  return MOD_OK;
}

int ensure_raw_stage(ModContext *c, ModContext::RawStage &r, const ModImageLayout &l) {
  return ensure_stage_bytes(c, r, 2 * (size_t)l.step * l.height);
}

int ensure_stage_bytes(ModContext *c, ModContext::RawStage &r, size_t need) {
  if (r.bytes >= need) return MOD_OK;
  for (hipStream_t q : {c->stream, (hipStream_t)c->pipe.h2d}) if (q) HIP_TRY(c, hipStreamSynchronize(q));
  r.buf.reset(); r.bytes = 0;
  HIP_TRY(c, dalloc(r.buf, need));
  r.bytes = need;
  return MOD_OK;
}

int rectify_bayer(ModContext *c, const ModImageLayout &l, int frames, const uint8_t *src, int pane, uint8_t *grey, const int32_t *map,
                  uint8_t *mono) {
  const size_t G = (size_t)l.width * l.height;
  launch_bayer_to_mono(l.width, l.height, frames, src, (size_t)l.step * l.height, l.step, l.width, l.height, 0, 0,
                       bayer_phase(l.encoding, pane == MOD_EYE_RIGHT ? l.width : 0, 0), grey, c->stream);
  launch_rectify(MOD_ENCODING_MONO8, c->dc.W, c->dc.H, frames, grey, G, G, l.width, l.width, l.height, map, mono, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

// registered: a registration is in force (the whole message is scattered: no window, any message size)
static int check_depth_layout(ModContext *c, const ModDepthLayout &l, bool registered) {
  const int B = depth_bytes(l.encoding);
  if (!B) return fail(c, MOD_ERR_INVALID_ARGUMENT, "unknown depth encoding");
  if (l.width < 1 || l.height < 1 || l.width > MOD_MAX_WIDTH || l.height > MOD_MAX_WIDTH)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: width and height must be in 1..MOD_MAX_WIDTH");
  if ((int64_t)l.step < (int64_t)l.width * B || l.step % B) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: step must be a multiple of the sample size and >= width * sample size");
  if ((int64_t)l.step * l.height > INT32_MAX) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: step * height must be below 2^31");
  if (!std::isfinite(l.unit) || l.unit < 0.0f) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: unit must be 0 (the REP 118 default) or finite and positive");
  if (registered) {
    if (l.x0 || l.y0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth image: x0 and y0 must be 0 while a depth registration is set (the whole message is registered)");
  } else if (l.x0 < 0 || l.y0 < 0 || (int64_t)l.x0 + c->dc.W > l.width || (int64_t)l.y0 + c->dc.H > l.height) {
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the camera-sized window does not fit inside the depth image");
  }
  return MOD_OK;
}

static ModDepthLayout default_depth_layout(const ModContext *c) { return ModDepthLayout{MOD_DEPTH_16UC1, c->dc.W, c->dc.H, 2 * c->dc.W, 0, 0, 0.0f}; }

int current_depth_layout(ModContext *c, ModDepthLayout *out) {
  *out = c->has_depth_layout ? c->depth_layout : default_depth_layout(c);
  return check_depth_layout(c, *out, c->has_depth_reg);   // the camera or the registration may have changed since the layout was set
}

int run_depth_to_disparity(ModContext *c, int frames, const void *depth, const ModDepthLayout &l, bool splat, uint32_t *zbuf, float *disparity) {
  const float unit = l.unit != 0.0f ? l.unit : l.encoding == MOD_DEPTH_16UC1 ? 0.001f : 1.0f;
  const float invalid = c->dc.dmin - 1.0f;
  if (c->has_depth_reg) {
    const ModDepthRegistration &r = c->depth_reg;
    DepthRegArgs g{};
    g.fxd = r.fx; g.fyd = r.fy; g.cxd = r.cx; g.cyd = r.cy;
    for (int i = 0; i < 9; i++) g.R[i] = r.R[i];
    for (int i = 0; i < 3; i++) g.t[i] = r.t[i];
    g.fx = c->cam.fx; g.fy = c->cam.fy; g.cx = c->cam.cx; g.cy = c->cam.cy; g.Tx = c->cam.Tx; g.Ty = c->cam.Ty;
    HIP_TRY(c, launch_depth_register(l.encoding, c->dc.W, c->dc.H, frames, depth, l.width, l.height, l.step, unit, g, splat, c->dc.fT, invalid, zbuf,
                                     disparity, c->stream));
  } else {
    launch_depth_to_disparity(l.encoding, c->dc.W, c->dc.H, frames, depth, (size_t)l.step * l.height, l.step, l.x0, l.y0, unit, c->dc.fT, invalid,
                              disparity, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

void refresh_devcam(ModContext *c) {
  DevCam &d = c->dc;
  d.W = c->cam.width; d.H = c->cam.height;
  d.mask_words = mod_mask_words(d.W);
  d.n = c->prm.neighbor_distance;
  d.cluster_size = c->prm.cluster_size;
#if defined(MOD_PHASE_COUNTERS) || defined(MOD_ABLATION)
  { const char *e = getenv("MOD_DEBUG"); d.debug = e ? atoi(e) : 0; }   // diagnostic builds only (mod_sf_debug.h)
#else
  d.debug = 0;
#endif
  d.fT = c->cam.disp_f * c->cam.disp_T;               // F32 product, exactly the reference's `focal_length * baseline`
  d.dmin = c->cam.min_disparity; d.dmax = c->cam.max_disparity;
  d.flow_th_sq = sqrt_threshold_sq((float)c->prm.dynamic_flow_diff);
  d.speed_th_sq = sqrt_threshold_sq(ceil_to_f32(c->prm.dynamic_speed));
  d.depth_th = floor_to_f32(c->prm.depth_diff);
  d.speed_th_d = c->prm.dynamic_speed;
  d.fx = c->cam.fx; d.fy = c->cam.fy; d.cx = c->cam.cx; d.cy = c->cam.cy; d.Tx = c->cam.Tx; d.Ty = c->cam.Ty;
  d.rayx = c->b.rayx; d.rayy = c->b.rayy;
}

int begin_cluster_scratch(ModContext *c) {
  if (!c->scratch_clean) {
    const size_t tiles = (size_t)c->max_mask_words * ((c->cfg.max_height + ccl_tile_rows() - 1) / ccl_tile_rows());
    HIP_TRY(c, hipMemsetAsync(c->b.tilehdr, 0, sizeof(int32_t) * 2 * tiles * c->cfg.max_frames, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->b.counters, 0, sizeof(int32_t) * 8 * c->cfg.max_frames, c->stream));
  }
  c->scratch_clean = false;
  return MOD_OK;
}

int run_cluster(ModContext *c, int frames, const ModSceneFlowPlanes *pl, const uint64_t *mask, bool mask_ready, bool flags_ready,
                const ModClusterOut *out) {
  int rc = check_cluster_io(c, pl, flags_ready, out);
  if (rc) return rc;
  StageTimer t(c, MOD_STAGE_CLUSTER_GROUP, c->stream);
  enqueue_cluster(c, Chunk{0, frames}, pl, mask, mask_ready, flags_ready, out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

// construct() publishes ~depth as soon as disparity_now exists, before the guards that end a frame without scene flow
// (scene_flow_constructor.cpp:110-123): on a skipped frame the depth plane is still produced when the caller asked for it.
static int depth_on_skip(ModContext *c, int skip, const ModFrameBatch *in, const ModSceneFlowPlanes *out) {
  if (skip <= 0 || skip == MOD_SKIP_NO_DISPARITY_NOW || !out || !out->depth || !in->disparity_now) return skip;
  launch_depth(c->dc, in->frames, in->disparity_now, out->depth, c->stream);
  HIP_TRY(c, hipGetLastError());
  return skip;
}

// the scene-flow stage alone: mod_scene_flow_dev, and with xy_optional the host entry points (scene_flow_staged)
static int scene_flow_alone(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *out, bool xy_optional) {
  int rc = check_batch(c, in);
  if (rc) return depth_on_skip(c, rc, in, out);
  return run_scene_flow(c, in, out, out ? out->dynamic_mask : nullptr, false, xy_optional);
}

int scene_flow_staged(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *out) { return scene_flow_alone(c, in, out, true); }

extern "C" {

int mod_abi_version(void) { return MOD_ABI_VERSION; }

int mod_create(const ModConfig *cfg, ModContext **out_ctx) {
  if (!cfg || !out_ctx) return MOD_ERR_INVALID_ARGUMENT;
  *out_ctx = nullptr;
  if (cfg->max_width < 1 || cfg->max_height < 1 || cfg->max_frames < 1) return MOD_ERR_INVALID_ARGUMENT;
  // launch geometry and index widths: frames ride in grid.y / grid.z (<= 65535), the scene-flow kernel addresses a frame's
  // planes with 32-bit byte offsets (32 B/px for the AoS cloud), cluster work items are frame * max_objects + cluster in 32 bits
  if (cfg->max_frames > 65535 || cfg->max_width > MOD_MAX_WIDTH) return MOD_ERR_INVALID_ARGUMENT;
  if (cfg->batch_chunks < 0 || cfg->batch_chunks > kMaxChunks) return MOD_ERR_INVALID_ARGUMENT;
  if ((uint64_t)cfg->max_width * (uint64_t)cfg->max_height >= (1ull << 27)) return MOD_ERR_INVALID_ARGUMENT;
  if (cfg->max_objects > 0 && (uint64_t)cfg->max_objects * (uint64_t)cfg->max_frames >= (1ull << 31)) return MOD_ERR_INVALID_ARGUMENT;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device || cfg->device < 0) return MOD_ERR_NO_DEVICE;
  if (hipSetDevice(cfg->device) != hipSuccess) return MOD_ERR_NO_DEVICE;
  ModContext *c = new ModContext();
  c->cfg = *cfg;
  const size_t N = (size_t)cfg->max_width * cfg->max_height;
  const int F = cfg->max_frames;
  c->maxN = N;
  c->max_mask_words = mod_mask_words(cfg->max_width);
  c->max_objects = cfg->max_objects > 0 ? cfg->max_objects : (int)std::max<size_t>(1, N / 100);
  if (cfg->stream) c->stream = (hipStream_t)cfg->stream;
  else { if (hipStreamCreate(c->own_stream.put()) != hipSuccess) { delete c; return MOD_ERR_DEVICE; } c->stream = c->own_stream; }
  const size_t mw = (size_t)F * cfg->max_height * c->max_mask_words;
  bool ok = true;
  ok &= dalloc(c->b.rayx, cfg->max_width + 4) == hipSuccess;
  ok &= dalloc(c->b.rayy, cfg->max_height + 4) == hipSuccess;
  ok &= dalloc(c->b.fc, F) == hipSuccess;
  ok &= dalloc(c->b.mask, mw) == hipSuccess;
  ok &= dalloc(c->b.lroot, mw) == hipSuccess;
  ok &= dalloc(c->b.zrange, mw) == hipSuccess;
  ok &= dalloc(c->b.parent, (size_t)F * N) == hipSuccess;
  ok &= dalloc(c->b.rsize, (size_t)F * N) == hipSuccess;   // 4 + 4 B per pixel of address space, touched only at roots
  ok &= dalloc(c->b.rkey, (size_t)F * N) == hipSuccess;
  ok &= dalloc(c->b.cbox, (size_t)F * c->max_objects) == hipSuccess;
  ok &= dalloc(c->b.counters, (size_t)F * 8) == hipSuccess;
  ok &= dalloc(c->b.clusters, (size_t)2 * F * c->max_objects) == hipSuccess;
  ok &= dalloc(c->b.mbits, (size_t)F * N) == hipSuccess;
  ok &= dalloc(c->b.mpix, (size_t)F * N) == hipSuccess;
  ok &= dalloc(c->b.worklist, (size_t)2 * F * c->max_objects) == hipSuccess;
  {
    const size_t tiles = (size_t)c->max_mask_words * ((cfg->max_height + ccl_tile_rows() - 1) / ccl_tile_rows());
    ok &= dalloc(c->b.tilehdr, (size_t)F * tiles * 2) == hipSuccess;
    ok &= dalloc(c->b.tilelist, (size_t)F * tiles) == hipSuccess;
  }
  ok &= dalloc(c->b.dbg, kDbgWords) == hipSuccess;
  if (ok) ok &= hipMemset(c->b.dbg, 0, kDbgWords * 8) == hipSuccess;
  // (tile headers and counters are cleared by the first call: scratch_clean starts false)
  if (ok) ok &= hipMemset((char *)c->b.dbg.get() + 42 * 8, 0xFF, 8) == hipSuccess;   // slot 42 is a minimum
  for (int i = 0; i < kRing && ok; i++) {
    ok &= hipHostMalloc((void **)c->pinned[i].put(), sizeof(FrameConst) * F, hipHostMallocDefault) == hipSuccess;
    ok &= hipEventCreateWithFlags(c->pinned_ev[i].put(), hipEventDisableTiming) == hipSuccess;
    if (ok) ok &= hipEventRecord(c->pinned_ev[i], c->stream) == hipSuccess;
  }
  // the chunk streams of process_chunked, on cfg->device; a few fork / join rounds, once: the runtime builds the cross-stream
  // signalling of the new streams here, not inside the first call
  if (ok && (cfg->batch_chunks ? cfg->batch_chunks : kAutoChunks) >= 2) {
    for (int k = 0; k < kMaxChunks - 1 && ok; k++)
      ok = hipStreamCreateWithFlags(c->chunk_stream[k].put(), hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(c->ev_join[k].put(), hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(c->ev_fork.put(), hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 16 && ok; i++) {
      ok = hipEventRecord(c->ev_fork, c->stream) == hipSuccess;
      for (int k = 0; k < kMaxChunks - 1 && ok; k++)
        ok = hipStreamWaitEvent(c->chunk_stream[k], c->ev_fork, 0) == hipSuccess &&
             hipEventRecord(c->ev_join[k], c->chunk_stream[k]) == hipSuccess && hipStreamWaitEvent(c->stream, c->ev_join[k], 0) == hipSuccess;
    }
  }
  if (!ok) { mod_destroy(c); return MOD_ERR_DEVICE; }
  *out_ctx = c;
  return MOD_OK;
}

void mod_destroy(ModContext *c) {
  if (!c) return;
  // every stream the context uses drains first; then the members' handles release everything (mod_context.h)
  for (hipStream_t q : {c->stream, (hipStream_t)c->pipe.h2d, (hipStream_t)c->pipe.d2h}) if (q) (void)hipStreamSynchronize(q);
  for (hipStream_t q : c->b.sgm_side) if (q) (void)hipStreamSynchronize(q);
  for (hipStream_t q : c->chunk_stream) if (q) (void)hipStreamSynchronize(q);
  delete c;
}

const char *mod_last_error(const ModContext *c) { return c ? c->err.c_str() : "null context"; }

int mod_set_camera(ModContext *c, const ModCamera *cam) {
  if (!c || !cam) return MOD_ERR_INVALID_ARGUMENT;
  if (cam->width < 1 || cam->height < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "camera size must be positive");
  if (cam->width > c->cfg.max_width || cam->height > c->cfg.max_height || (size_t)cam->width * cam->height > c->maxN)
    return fail(c, MOD_ERR_CAPACITY, "camera larger than ModConfig.max_width/max_height");
  c->cam = *cam;
  // projectPixelTo3dRay (image_geometry, melodic): ((u - cx - Tx)/fx, (v - cy - Ty)/fy, 1) in F64 — only a function of
  // the column / the row, so the two F64 divides per pixel of the reference become two table reads.
  std::vector<double> rx(cam->width + 4, 0.0), ry(cam->height + 4, 0.0);
  for (int u = 0; u < cam->width; u++) rx[u] = ((double)u - cam->cx - cam->Tx) / cam->fx;
  for (int v = 0; v < cam->height; v++) ry[v] = ((double)v - cam->cy - cam->Ty) / cam->fy;
  HIP_TRY(c, hipMemcpyAsync(c->b.rayx, rx.data(), sizeof(double) * rx.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->b.rayy, ry.data(), sizeof(double) * ry.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // rx/ry are stack-owned
  c->has_cam = true;
  refresh_devcam(c);
  return MOD_OK;
}

int mod_set_params(ModContext *c, const ModParams *p) {
  if (!c || !p) return MOD_ERR_INVALID_ARGUMENT;
  if (p->neighbor_distance < 1 || p->neighbor_distance > MOD_MAX_NEIGHBOR_DISTANCE)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "neighbor_distance must be in 1..16");
  if (p->cluster_size < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster_size must be >= 1");
  // at most N / cluster_size clusters can survive the size filter: the object arrays must hold them all, so that no
  // cluster is ever dropped (the default capacity N/100 covers the reference's whole range cluster_size >= 100)
  if (c->maxN / (size_t)p->cluster_size > (size_t)c->max_objects)
    return fail(c, MOD_ERR_CAPACITY, "ModConfig.max_objects is smaller than max_width*max_height / cluster_size");
  {   // link-request scratch grows with neighbor_distance
    const size_t tiles = (size_t)c->max_mask_words * ((c->cfg.max_height + ccl_tile_rows() - 1) / ccl_tile_rows());
    const size_t need = (size_t)c->cfg.max_frames * tiles * ccl_request_capacity(p->neighbor_distance);
    if (need > c->b.req_alloc) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      c->b.requests.reset(); c->b.req_alloc = 0;
      HIP_TRY(c, dalloc(c->b.requests, need));
      c->b.req_alloc = need;
    }
  }
  c->prm = *p;
  c->has_prm = true;
  refresh_devcam(c);
  return MOD_OK;
}

int mod_get_camera(const ModContext *c, ModCamera *cam) {
  if (!c || !cam || !c->has_cam) return MOD_ERR_NOT_CONFIGURED;
  *cam = c->cam;
  return MOD_OK;
}
int mod_get_params(const ModContext *c, ModParams *p) {
  if (!c || !p || !c->has_prm) return MOD_ERR_NOT_CONFIGURED;
  *p = c->prm;
  return MOD_OK;
}

int mod_set_image_layout(ModContext *c, const ModImageLayout *l) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!c->has_cam) return fail(c, MOD_ERR_NOT_CONFIGURED, "the camera must be set first (the window is the camera's size)");
  const ModImageLayout packed{MOD_ENCODING_MONO8, c->dc.W, c->dc.H, c->dc.W, 0, 0};   // (holds no two panes: refused while side by side)
  int rc = check_layout(c, l ? *l : packed, c->side_by_side);
  if (rc) return rc;
  if (l) c->layout = *l;
  c->has_layout = l != nullptr;
  return MOD_OK;
}

int mod_set_side_by_side(ModContext *c, int32_t on) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (on != 0 && on != 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "side by side must be 0 or 1");
  if (on && c->has_cam) {           // the layout in force must hold two panes (without a camera there is none yet: checked at call time)
    const ModImageLayout l = c->has_layout ? c->layout : ModImageLayout{MOD_ENCODING_MONO8, c->dc.W, c->dc.H, c->dc.W, 0, 0};
    if (int rc = check_layout(c, l, true)) return rc;
  }
  c->side_by_side = on != 0;
  return MOD_OK;
}

int mod_get_side_by_side(const ModContext *c, int32_t *on) {
  if (!c || !on) return MOD_ERR_INVALID_ARGUMENT;
  *on = c->side_by_side;
  return MOD_OK;
}

int mod_get_image_layout(const ModContext *c, ModImageLayout *l) {
  if (!c || !l) return MOD_ERR_INVALID_ARGUMENT;
  if (!c->has_cam) return MOD_ERR_NOT_CONFIGURED;
  *l = c->has_layout ? c->layout : ModImageLayout{MOD_ENCODING_MONO8, c->dc.W, c->dc.H, c->dc.W, 0, 0};
  return MOD_OK;
}

int mod_image_to_mono_dev(ModContext *c, int32_t frames, const uint8_t *src, const ModImageLayout *layout, uint8_t *mono) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!c->has_cam) return fail(c, MOD_ERR_NOT_CONFIGURED, "the camera must be set first (the window is the camera's size)");
  if (frames < 1 || frames > 65535) return fail(c, MOD_ERR_INVALID_ARGUMENT, "frames must be in 1..65535");
  if (!src) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!mono) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null grey planes");
  ModImageLayout l;
  int rc = layout ? check_layout(c, *layout, c->side_by_side) : current_layout(c, &l);
  if (rc) return rc;
  if (layout) l = *layout;
  if (is_bayer(l.encoding))        // the region is the message (side by side: the pane src points at, with the pattern as it lies there)
    launch_bayer_to_mono(c->dc.W, c->dc.H, frames, src, (size_t)l.step * l.height, l.step, l.width, l.height, l.x0, l.y0,
                         bayer_phase(l.encoding, 0, 0), mono, c->stream);
  else
    launch_to_mono(l.encoding, c->dc.W, c->dc.H, frames, src, (size_t)l.step * l.height, l.step, l.x0, l.y0, mono, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_set_rectification(ModContext *c, const ModRectifyCamera *left, const ModRectifyCamera *right) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!left != !right) return fail(c, MOD_ERR_INVALID_ARGUMENT, "rectification: both eyes or neither");
  for (const ModRectifyCamera *cam : {left, right})
    if (const char *what = cam ? check_rectify_camera(*cam) : nullptr) return fail(c, MOD_ERR_INVALID_ARGUMENT, what);
  if (c->pipe.in_flight > 0)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the rectification cannot change while frames are in flight: collect every ticket first");
  c->rect.on = left != nullptr;
  if (left) { c->rect.cam[MOD_EYE_LEFT] = *left; c->rect.cam[MOD_EYE_RIGHT] = *right; }
  for (ModContext::Rectify::Map &m : c->rect.map) m.valid = false;   // rebuilt at the next use, behind the context's stream
  return MOD_OK;
}

int mod_get_rectification(const ModContext *c, ModRectifyCamera *left, ModRectifyCamera *right, int32_t *enabled) {
  if (!c || !enabled) return MOD_ERR_INVALID_ARGUMENT;
  *enabled = c->rect.on;
  if (c->rect.on && left) *left = c->rect.cam[MOD_EYE_LEFT];
  if (c->rect.on && right) *right = c->rect.cam[MOD_EYE_RIGHT];
  return MOD_OK;
}

// the layout a rectifying call works on (the given one, or the context's) and the map of `eye` for its window
static int rectify_setup(ModContext *c, const ModImageLayout *layout, int32_t eye, ModImageLayout *l) {
  if (!c->has_cam) return fail(c, MOD_ERR_NOT_CONFIGURED, "the camera must be set first (the window is the camera's size)");
  if (eye != MOD_EYE_LEFT && eye != MOD_EYE_RIGHT) return fail(c, MOD_ERR_INVALID_ARGUMENT, "eye must be MOD_EYE_LEFT or MOD_EYE_RIGHT");
  if (!c->rect.on) return fail(c, MOD_ERR_NOT_CONFIGURED, "no rectification is set");
  int rc = layout ? check_layout(c, *layout, c->side_by_side) : current_layout(c, l);
  if (rc) return rc;
  if (layout) *l = *layout;
  return ensure_rectify_map(c, eye, *l);
}

int mod_rectify_dev(ModContext *c, int32_t frames, const uint8_t *src, const ModImageLayout *layout, int32_t eye, uint8_t *mono) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (frames < 1 || frames > 65535) return fail(c, MOD_ERR_INVALID_ARGUMENT, "frames must be in 1..65535");
  ModImageLayout l;
  if (int rc = rectify_setup(c, layout, eye, &l)) return rc;
  if (!src) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!mono) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null grey planes");
  const size_t M = (size_t)l.step * l.height, pane = c->side_by_side ? pane_offset(l, eye) : 0;   // side by side: eye selects the pane too
  if (is_bayer(l.encoding)) {      // debayer, then rectify: the whole messages (or panes) to grey planes of the context's, k_rectify from those
    if (int rc = ensure_stage_bytes(c, c->bayer_grey, (size_t)frames * l.width * l.height)) return rc;
    return rectify_bayer(c, l, frames, src + pane, c->side_by_side ? eye : MOD_EYE_LEFT, c->bayer_grey.buf, c->rect.map[eye].q, mono);
  }
  launch_rectify(l.encoding, c->dc.W, c->dc.H, frames, src + pane, M, M - pane, l.step, l.width, l.height, c->rect.map[eye].q, mono, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_rectify_map_host(ModContext *c, int32_t eye, const ModImageLayout *layout, int32_t *map_qxqy) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!map_qxqy) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null map");
  ModImageLayout l;
  if (int rc = rectify_setup(c, layout, eye, &l)) return rc;
  HIP_TRY(c, hipMemcpyAsync(map_qxqy, c->rect.map[eye].q, sizeof(int32_t) * 2 * (size_t)c->dc.W * c->dc.H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}

int mod_set_depth_layout(ModContext *c, const ModDepthLayout *l) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!c->has_cam) return fail(c, MOD_ERR_NOT_CONFIGURED, "the camera must be set first (the window is the camera's size)");
  if (int rc = check_depth_layout(c, l ? *l : default_depth_layout(c), c->has_depth_reg)) return rc;
  if (l) c->depth_layout = *l;
  c->has_depth_layout = l != nullptr;
  return MOD_OK;
}

int mod_get_depth_layout(const ModContext *c, ModDepthLayout *l) {
  if (!c || !l) return MOD_ERR_INVALID_ARGUMENT;
  if (!c->has_cam) return MOD_ERR_NOT_CONFIGURED;
  *l = c->has_depth_layout ? c->depth_layout : default_depth_layout(c);
  return MOD_OK;
}

int mod_set_depth_registration(ModContext *c, const ModDepthRegistration *r) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (r) {
    for (const double v : {r->fx, r->fy, r->cx, r->cy}) if (!std::isfinite(v)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: non-finite intrinsics");
    for (const double v : r->R) if (!std::isfinite(v)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: non-finite entry in R");
    for (const double v : r->t) if (!std::isfinite(v)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: non-finite entry in t");
    if (r->fx <= 0.0 || r->fy <= 0.0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: the focal lengths must be positive");
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const double d = r->R[3 * i] * r->R[3 * j] + r->R[3 * i + 1] * r->R[3 * j + 1] + r->R[3 * i + 2] * r->R[3 * j + 2];
        if (std::fabs(d - (i == j ? 1.0 : 0.0)) > 1e-6)
          return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth registration: R is not a rotation (R R^T differs from I by more than 1e-6)");
      }
    c->depth_reg = *r;
  }
  c->has_depth_reg = r != nullptr;
  return MOD_OK;
}

int mod_get_depth_registration(const ModContext *c, ModDepthRegistration *r, int32_t *enabled) {
  if (!c || !enabled) return MOD_ERR_INVALID_ARGUMENT;
  *enabled = c->has_depth_reg;
  if (c->has_depth_reg && r) *r = c->depth_reg;
  return MOD_OK;
}

int mod_depth_to_disparity_dev(ModContext *c, int32_t frames, const void *depth, const ModDepthLayout *layout, float *disparity) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (!c->has_cam) return fail(c, MOD_ERR_NOT_CONFIGURED, "the camera must be set first (the window is the camera's size)");
  if (frames < 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "frames must be >= 1");
  if (frames > c->cfg.max_frames) return fail(c, MOD_ERR_CAPACITY, "frames exceeds ModConfig.max_frames");
  ModDepthLayout l;
  int rc = layout ? check_depth_layout(c, *layout, c->has_depth_reg) : current_depth_layout(c, &l);
  if (rc) return rc;
  if (layout) l = *layout;
  if (!depth) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!disparity) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null disparity planes");
  if ((uintptr_t)depth % depth_bytes(l.encoding) || (uintptr_t)disparity % 4)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth must be aligned to its sample size and disparity to 4 bytes");
  if (c->has_depth_reg) HIP_TRY(c, dalloc(c->depth_zbuf, (size_t)c->cfg.max_frames * c->maxN));
  return run_depth_to_disparity(c, frames, depth, l, c->depth_splat, c->depth_zbuf, disparity);
}

int mod_set_depth_splat(ModContext *c, int32_t on) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (on != 0 && on != 1) return fail(c, MOD_ERR_INVALID_ARGUMENT, "depth splat: on must be 0 or 1");
  c->depth_splat = on != 0;
  return MOD_OK;
}

int mod_get_depth_splat(const ModContext *c, int32_t *on) {
  if (!c || !on) return MOD_ERR_INVALID_ARGUMENT;
  *on = c->depth_splat;
  return MOD_OK;
}

int mod_synchronize(ModContext *c) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}

int mod_scene_flow_dev(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *out) { return scene_flow_alone(c, in, out, false); }

int mod_depth_image_dev(ModContext *c, int32_t frames, const float *disparity_now, float *depth) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!disparity_now) return MOD_SKIP_NO_DISPARITY_NOW;
  if (!depth) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null depth plane");
  launch_depth(c->dc, frames, disparity_now, depth, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_dynamic_mask_dev(ModContext *c, int32_t frames, const float *vx, const float *vy, const float *vz, uint64_t *mask) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!vx || !vy || !vz || !mask) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null plane");
  launch_dynamic_mask(c->dc, frames, vx, vy, vz, mask, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_cluster_dev(ModContext *c, int32_t frames, const ModSceneFlowPlanes *pl, const ModClusterOut *out) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  const bool have = pl && pl->dynamic_mask;
  if ((rc = check_cluster_io(c, pl, false, out)) || (rc = begin_cluster_scratch(c))) return rc;
  if ((rc = run_cluster(c, frames, pl, have ? pl->dynamic_mask : c->b.mask.get(), have, false, out))) return rc;
  c->scratch_clean = true;
  return MOD_OK;
}

int mod_process_dev(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *pl, const ModClusterOut *out) {
  int rc = check_batch(c, in);
  if (rc) return depth_on_skip(c, rc, in, pl);
  uint64_t *mask = (pl && pl->dynamic_mask) ? pl->dynamic_mask : c->b.mask.get();
  const int chunks = chunk_count(c, in->frames);
  if ((rc = check_scene_flow_out(c, pl, true)) || (rc = check_cluster_io(c, pl, true, out)) || (rc = begin_cluster_scratch(c))) return rc;
  if (chunks > 1) rc = process_chunked(c, in, pl, mask, out, chunks);
  else if (!(rc = run_scene_flow(c, in, pl, mask, true, true))) rc = run_cluster(c, in->frames, pl, mask, true, true, out);
  if (rc) return rc;
  c->scratch_clean = true;
  return MOD_OK;
}

int mod_pack_cloud_dev(ModContext *c, int32_t frames, const ModSceneFlowPlanes *pl, void *aos) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!pl || !aos || !pl->x || !pl->y || !pl->z || !pl->vx || !pl->vy || !pl->vz) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null plane");
  launch_pack((size_t)frames * c->dc.W * c->dc.H, pl->x, pl->y, pl->z, pl->vx, pl->vy, pl->vz, aos, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_unpack_cloud_dev(ModContext *c, int32_t frames, const void *aos, const ModSceneFlowPlanes *pl) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!pl || !aos || !pl->x || !pl->y || !pl->z || !pl->vx || !pl->vy || !pl->vz) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null plane");
  launch_unpack((size_t)frames * c->dc.W * c->dc.H, aos, pl->x, pl->y, pl->z, pl->vx, pl->vy, pl->vz, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

// ---- memory helpers --------------------------------------------------------------------------------------------------
int mod_host_malloc(ModContext *c, uint64_t bytes, void **p) {
  if (!c || !p) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipHostMalloc(p, bytes, hipHostMallocDefault));
  return MOD_OK;
}
int mod_host_free(ModContext *c, void *p) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipHostFree(p));
  return MOD_OK;
}
int mod_malloc(ModContext *c, uint64_t bytes, void **p) {
  if (!c || !p) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipMalloc(p, bytes));
  return MOD_OK;
}
int mod_free(ModContext *c, void *p) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipFree(p));
  return MOD_OK;
}
int mod_memcpy_h2d(ModContext *c, void *d, const void *h, uint64_t bytes) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}
int mod_memcpy_d2h(ModContext *c, void *h, const void *d, uint64_t bytes) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MOD_OK;
}

#if defined(MOD_PHASE_COUNTERS) || defined(MOD_ABLATION) || defined(MOD_CHECKED)
// diagnostic builds only (declared in mod_sf_debug.h; a product build does not export them)
// copy an internal buffer to the host (0 member norms, 4 member pixels, 1 clusters, 2 counters; ego-motion: 5 correspondence counts,
// 6 correspondences, 7 hypothesis inlier counts)
int mod_debug_read(ModContext *c, int which, void *dst, unsigned long long bytes) {
  if (!c || !dst) return MOD_ERR_INVALID_ARGUMENT;
  const void *src = which == 0 ? (const void *)c->b.mbits : which == 4 ? (const void *)c->b.mpix : which == 1 ? (const void *)c->b.clusters
                  : which == 5 ? (const void *)c->b.ego_ncorr : which == 6 ? (const void *)c->b.ego_corr : which == 7 ? (const void *)c->b.ego_hcnt
                  : (const void *)c->b.counters;
  if (!src) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return MOD_OK;
}

int mod_debug_counters(ModContext *c, unsigned long long *out32) {
  if (!c || !out32) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out32, c->b.dbg, kDbgWords * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemset(c->b.dbg, 0, kDbgWords * 8));
  HIP_TRY(c, hipMemset((char *)c->b.dbg.get() + 42 * 8, 0xFF, 8));
  return MOD_OK;
}
#endif

// ---- measurement -------------------------------------------------------------------------------------------------------
int mod_set_profiling(ModContext *c, int32_t stage_mask) {
  if (!c || (stage_mask & ~MOD_PROFILE_ALL)) return MOD_ERR_INVALID_ARGUMENT;
  c->profiling = stage_mask;
  // events for the next 64 calls are created here, not inside the calls that are being timed (an event pair costs tens of
  // microseconds to create; later calls create what they lack)
  const size_t want = (size_t)64 * (size_t)__builtin_popcount((unsigned)stage_mask);
  while (c->free_events.size() < want) {
    EventPair ev;
    if (hipEventCreate(ev.a.put()) != hipSuccess || hipEventCreate(ev.b.put()) != hipSuccess) break;   // (ev releases a half-made pair)
    c->free_events.push_back(std::move(ev));
  }
  return MOD_OK;
}
int mod_get_stage_time(ModContext *c, int32_t stage, double *total_ms, int64_t *calls) {
  if (!c || stage < 0 || stage >= MOD_STAGE_COUNT) return MOD_ERR_INVALID_ARGUMENT;
  drain_timers(c);
  if (total_ms) *total_ms = c->stage_ms[stage];
  if (calls) *calls = c->stage_calls[stage];
  return MOD_OK;
}
int mod_reset_stage_times(ModContext *c) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  drain_timers(c);
  for (int s = 0; s < MOD_STAGE_COUNT; s++) { c->stage_ms[s] = 0; c->stage_calls[s] = 0; }
  return MOD_OK;
}

}  // extern "C"
