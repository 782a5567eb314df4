// mod_sf.hip — C ABI (include/mod_sf.h) over the gfx950 kernels: context lifecycle, camera and parameters, the batched scene-flow /
// cluster / process path, parameter folding, stage timers, memory helpers.  Host-side only; the kernels live in sceneflow.hip and
// the clusterer's ccl_*.hip / cluster_*.hip, the estimators in host_sgm.hip / host_flow.hip / host_ego.hip and their stand-alone filters in host_filters.hip, image input in host_images.hip, depth input in host_depth.hip, the *_host calls in host_api.hip.
#include "mod_context.h"
#include "exact_div.h"
#include "flow_color.h"
#include "mod_sf_debug.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

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

// frame f0 of a plane whose frames lie `stride` elements apart; a plane the caller did not pass stays null
template <class T> T *at(T *p, size_t f0, size_t stride) { return p ? p + f0 * stride : nullptr; }

// The cluster scratch (mod_context.h ClusterScratch): allocate, grow requests, carve; begin_cluster_scratch clears.
hipError_t cluster_alloc(ClusterScratch &s, const ModConfig &cfg, int max_objects) {
  s.frames = (size_t)cfg.max_frames; s.pixels = (size_t)cfg.max_width * cfg.max_height; s.max_objects = (size_t)max_objects;
  s.mask_rows = (size_t)mod_mask_words(cfg.max_width) * cfg.max_height; s.tiles = (size_t)ccl_tiles(mod_mask_words(cfg.max_width), cfg.max_height);
  const size_t F = s.frames, FN = F * s.pixels, FM = F * s.mask_rows, FO = F * s.max_objects, FT = F * s.tiles;
  HIP_OK(dalloc(s.mask, FM)); HIP_OK(dalloc(s.lroot, FM)); HIP_OK(dalloc(s.zrange, FM));
  HIP_OK(dalloc(s.parent, FN)); HIP_OK(dalloc(s.rsize, FN)); HIP_OK(dalloc(s.rkey, FN));
  HIP_OK(dalloc(s.cbox, FO)); HIP_OK(dalloc(s.counters, F * kClusterCounters));
  HIP_OK(dalloc(s.clusters, 2 * FO)); s.rank_scratch = s.clusters + FO;   // the second halves: stated here, and nowhere else
  HIP_OK(dalloc(s.mbits, FN)); HIP_OK(dalloc(s.mpix, FN));
  HIP_OK(dalloc(s.worklist, 2 * FO)); s.tielist = s.worklist + FO;
  HIP_OK(dalloc(s.tilehdr, FT * kTileHdrWords));
  return dalloc(s.tilelist, FT);
}

// room in `requests` for what every tile can emit at neighbor_distance n: grow-only, replaced once `stream` has drained
hipError_t cluster_grow_requests(ClusterScratch &s, int n, hipStream_t stream) {
  const size_t need = s.frames * s.tiles * ccl_request_capacity(n);
  if (need <= s.req_alloc) return hipSuccess;
  HIP_OK(hipStreamSynchronize(stream));
  s.requests.reset(); s.req_alloc = 0;
  HIP_OK(dalloc(s.requests, need));
  s.req_alloc = need; return hipSuccess;
}

// A chunk's part of the scratch, of the planes, the mask and the outputs (out == null: the scene-flow launch, which reads only what
// follows `a`).  The frames of a call lie the camera's strides apart, whatever the capacity.
struct Carved { ClArgs a; ClusterInfo *rank_scratch; float2 *zrange; int tiles; ClusterMemberOut members; };   // zrange: a.zrange for its writer (a.zrange is null unless flags_ready); tiles: of a frame; members: all null unless the call writes the lists

Carved cluster_carve(const Buffers &b, const DevCam &dc, Chunk ch, const ModSceneFlowPlanes *pl, const uint64_t *mask, bool flags_ready, const ModClusterOut *out,
                     const ModClusterMembers *mem) {
  const ClusterScratch &s = b.cluster;
  const size_t N = (size_t)dc.W * dc.H, f0 = (size_t)ch.f0, MWH = (size_t)dc.mask_words * dc.H, MO = s.max_objects, tiles = (size_t)ccl_tiles(dc.mask_words, dc.H);
  static const ModClusterOut no_out{}; if (!out) out = &no_out;
  Carved v{{}, s.rank_scratch + f0 * MO, s.zrange + f0 * MWH, (int)tiles, {}}; ClArgs &a = v.a;
  if (mem) v.members = {at(mem->offsets, f0, MO + 1), at(mem->indices, f0, N), at(mem->points, f0, 3 * N)};
  a.x = at(pl->x, f0, N); a.y = at(pl->y, f0, N); a.z = at(pl->z, f0, N); a.vx = at(pl->vx, f0, N); a.vy = at(pl->vy, f0, N); a.vz = at(pl->vz, f0, N);
  a.mask = at(mask, f0, MWH); a.zrange = flags_ready ? v.zrange : nullptr; a.lroot = s.lroot + f0 * MWH;
  a.parent = s.parent + f0 * N; a.rootlist = (int32_t *)s.mpix.get() + f0 * N; a.rsize = s.rsize + f0 * N; a.rkey = s.rkey + f0 * N;
  a.cbox = s.cbox + f0 * MO; a.counters = s.counters + f0 * kClusterCounters; a.clusters = s.clusters + f0 * MO;
  a.mbits = s.mbits + f0 * N; a.mpix = s.mpix + f0 * N; a.worklist = s.worklist + f0 * MO; a.tielist = s.tielist + f0 * MO;
  a.labels = at(out->labels, f0, N); a.objects = at(out->objects, f0, MO); a.n_objects = at(out->n_objects, f0, 1); a.n_clusters = at(out->n_clusters, f0, 1);
  a.max_objects = (int32_t)MO; a.req_cap = ccl_request_capacity(dc.n); a.dbg = b.dbg; a.xy_from_z = flags_ready ? 1 : 0;   // only mod_process_dev's fused path hands over its own scene-flow planes
  a.requests = s.requests + f0 * tiles * (size_t)a.req_cap; a.tilehdr = s.tilehdr + f0 * tiles * kTileHdrWords; a.tilelist = s.tilelist + f0 * tiles;
  return v;
}

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
  const size_t N = (size_t)c->dc.W * c->dc.H, f0 = (size_t)ch.f0;
  const bool marks = tile_flags && mask;   // the clustering follows: the kernel's epilogue also marks the cluster tiles that hold a dynamic pixel
  const Carved cv = cluster_carve(c->b, c->dc, ch, out, mask, marks, nullptr, nullptr);
  SfArgs a;
  a.dnow = in->disparity_now + f0 * N; a.dprev = in->disparity_prev + f0 * N; a.flow = in->flow + f0 * N * 2;
  a.x = at(out->x, f0, N); a.y = at(out->y, f0, N); a.z = out->z + f0 * N; a.vx = out->vx + f0 * N; a.vy = out->vy + f0 * N; a.vz = out->vz + f0 * N;
  a.mask = at(mask, f0, (size_t)c->dc.mask_words * c->dc.H);
  a.aos = at((float4 *)out->cloud_aos, f0, N * 2); a.depth = at(out->depth, f0, N); a.sflow = at(out->static_flow, f0, N * 2);
  a.fc = c->b.fc + f0; a.dbg = c->b.dbg;
  a.tilehdr = marks ? cv.a.tilehdr : nullptr;   // (all zero: ModContext::scratch_clean)
  a.zrange = marks ? cv.zrange : nullptr;       // ... and leaves the depth range of every non-zero mask word's dynamic pixels for the tile stage
  a.tile_rows = ccl_tile_rows(); a.tiles_x = c->dc.mask_words; a.tiles_per_frame = cv.tiles;
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

// The clustering of one chunk on stream s.  mem: where the member lists go (mod_set_cluster_members), or null: none are written
void enqueue_cluster(ModContext *c, Chunk ch, const ModSceneFlowPlanes *pl, const uint64_t *mask, bool mask_ready, bool flags_ready,
                    const ModClusterOut *out, const ModClusterMembers *mem, hipStream_t s) {
  const Carved cv = cluster_carve(c->b, c->dc, ch, pl, mask, flags_ready, out, mem);
  const ClArgs &a = cv.a;
  const int frames = ch.n;
  {
    StageTimer t(c, MOD_STAGE_CCL_TILE, s);
    if (!mask_ready) launch_dynamic_mask(c->dc, frames, a.vx, a.vy, a.vz, (uint64_t *)a.mask, s);
    if (!flags_ready) launch_tile_flags(c->dc, a, frames, s);
    launch_ccl_tile(c->dc, a, frames, s);                 // (the counters are zero: ModContext::scratch_clean)
  }
  { StageTimer t(c, MOD_STAGE_CCL_LINK, s); launch_ccl_link(c->dc, a, frames, s); }
  { StageTimer t(c, MOD_STAGE_CCL_MERGE, s); launch_ccl_merge(c->dc, a, frames, cv.rank_scratch, s); }
  {
    StageTimer t(c, MOD_STAGE_FINAL, s);
    launch_final(c->dc, a, frames, s);
    if (mem) launch_cluster_members(c->dc, a, cv.members, frames, s);   // before launch_median: the tie replay reuses the member arrays
  }
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
int process_chunked(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *pl, uint64_t *mask, const ModClusterOut *out,
                    const ModClusterMembers *mem, int C) {
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
    enqueue_cluster(c, ch, pl, mask, true, true, out, mem, s);
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

hipError_t reset_dbg(unsigned long long *dbg) {   // the diagnostic counters as a context starts with them: zero, slot 42 (a minimum) all ones
  HIP_OK(hipMemset(dbg, 0, kDbgWords * sizeof(*dbg))); return hipMemset(dbg + 42, 0xFF, sizeof(*dbg));
}

// the chunk streams of process_chunked, on cfg->device; a few fork / join rounds, once: the runtime builds the cross-stream
// signalling of the new streams here, not inside the first call
hipError_t create_chunk_streams(ModContext *c) {
  for (int k = 0; k < kMaxChunks - 1; k++) { HIP_OK(hipStreamCreateWithFlags(c->chunk_stream[k].put(), hipStreamNonBlocking)); HIP_OK(hipEventCreateWithFlags(c->ev_join[k].put(), hipEventDisableTiming)); }
  HIP_OK(hipEventCreateWithFlags(c->ev_fork.put(), hipEventDisableTiming));
  for (int i = 0; i < 16; i++) {
    HIP_OK(hipEventRecord(c->ev_fork, c->stream));
    for (int k = 0; k < kMaxChunks - 1; k++) {
      HIP_OK(hipStreamWaitEvent(c->chunk_stream[k], c->ev_fork, 0)); HIP_OK(hipEventRecord(c->ev_join[k], c->chunk_stream[k]));
      HIP_OK(hipStreamWaitEvent(c->stream, c->ev_join[k], 0));
    }
  }
  return hipSuccess;
}

// what mod_create gives a context whose configuration, capacities and stream are set
hipError_t create_resources(ModContext *c, const ModConfig &cfg) {
  HIP_OK(dalloc(c->b.rayx, cfg.max_width + 4)); HIP_OK(dalloc(c->b.rayy, cfg.max_height + 4)); HIP_OK(dalloc(c->b.fc, cfg.max_frames));
  HIP_OK(cluster_alloc(c->b.cluster, cfg, c->max_objects));   // (tile headers and counters are cleared by the first call: scratch_clean starts false)
  HIP_OK(dalloc(c->b.dbg, kDbgWords)); HIP_OK(reset_dbg(c->b.dbg));
  for (int i = 0; i < kRing; i++) {
    HIP_OK(hipHostMalloc((void **)c->pinned[i].put(), sizeof(FrameConst) * cfg.max_frames, hipHostMallocDefault));
    HIP_OK(hipEventCreateWithFlags(c->pinned_ev[i].put(), hipEventDisableTiming)); HIP_OK(hipEventRecord(c->pinned_ev[i], c->stream));
  }
  return (cfg.batch_chunks ? cfg.batch_chunks : kAutoChunks) >= 2 ? create_chunk_streams(c) : hipSuccess;
}

}  // namespace

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
  if (const ClusterScratch &s = c->b.cluster; !c->scratch_clean) {   // the clear of the scratch: word 0 of the tile headers, the counters (whole capacity)
    HIP_TRY(c, hipMemsetAsync(s.tilehdr, 0, sizeof(int32_t) * kTileHdrWords * s.tiles * s.frames, c->stream));
    HIP_TRY(c, hipMemsetAsync(s.counters, 0, sizeof(int32_t) * kClusterCounters * s.frames, c->stream));
  }
  c->scratch_clean = false;
  return MOD_OK;
}

int run_cluster(ModContext *c, int frames, const ModSceneFlowPlanes *pl, const uint64_t *mask, bool mask_ready, bool flags_ready,
                const ModClusterOut *out, const ModClusterMembers *mem) {
  int rc = check_cluster_io(c, pl, flags_ready, out);
  if (rc) return rc;
  StageTimer t(c, MOD_STAGE_CLUSTER_GROUP, c->stream);
  enqueue_cluster(c, Chunk{0, frames}, pl, mask, mask_ready, flags_ready, out, mem, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int render_cluster_image(ModContext *c, int frames, const int32_t *labels, const int32_t *n_clusters, const label_palette::Table &table, uint8_t *image) {
  StageTimer t(c, MOD_STAGE_FINAL, c->stream);
  launch_cluster_image(c->dc.W, c->dc.H, frames, labels, n_clusters, table, image, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

// mod_set_cluster_image's device image, or null: mod_cluster_dev / mod_process_dev draw none
static uint8_t *dev_image(const ModContext *c) { return c->image_on ? c->image.image : nullptr; }
// ... which needs the label plane and the cluster counts of the call
static int check_image_io(ModContext *c, const ModClusterOut *out) {
  if (dev_image(c) && out && (!out->labels || !out->n_clusters))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "the cluster image is on (mod_set_cluster_image): cluster outputs labels and n_clusters are required");
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
  c->cfg = *cfg; c->maxN = (size_t)cfg->max_width * cfg->max_height;
  c->max_objects = cfg->max_objects > 0 ? cfg->max_objects : (int)std::max<size_t>(1, c->maxN / 100);
  if (cfg->stream) c->stream = (hipStream_t)cfg->stream;
  else { if (hipStreamCreate(c->own_stream.put()) != hipSuccess) { delete c; return MOD_ERR_DEVICE; } c->stream = c->own_stream; }
  if (create_resources(c, c->cfg) != hipSuccess) { mod_destroy(c); return MOD_ERR_DEVICE; }
  *out_ctx = c;
  return MOD_OK;
}

void mod_destroy(ModContext *c) {
  if (!c) return;
  // every stream the context uses drains first; then the members' handles release everything (mod_context.h)
  for (hipStream_t q : {c->stream, (hipStream_t)c->pipe.h2d, (hipStream_t)c->pipe.d2h}) if (q) (void)hipStreamSynchronize(q);
  for (hipStream_t q : c->b.sgm.side) if (q) (void)hipStreamSynchronize(q);
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
  HIP_TRY(c, cluster_grow_requests(c->b.cluster, p->neighbor_distance, c->stream));   // link-request scratch grows with neighbor_distance
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
  if ((rc = check_cluster_io(c, pl, false, out)) || (rc = check_image_io(c, out)) || (rc = begin_cluster_scratch(c))) return rc;
  if ((rc = run_cluster(c, frames, pl, have ? pl->dynamic_mask : c->b.cluster.mask.get(), have, false, out, cluster_members(c)))) return rc;
  c->scratch_clean = true;
  return dev_image(c) ? render_cluster_image(c, frames, out->labels, out->n_clusters, c->image_table, dev_image(c)) : MOD_OK;
}

int mod_process_dev(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *pl, const ModClusterOut *out) {
  if (!c || !dev_image(c)) return process_dev(c, in, pl, out, c ? cluster_members(c) : nullptr);
  // the image is drawn once, over all frames, behind the cluster stage (chunked: behind the join of its chunks)
  int rc = check_batch(c, in);
  if (!rc && (rc = check_image_io(c, out))) return rc;
  if ((rc = process_dev(c, in, pl, out, cluster_members(c)))) return rc;
  return render_cluster_image(c, in->frames, out->labels, out->n_clusters, c->image_table, dev_image(c));
}

int mod_set_cluster_image(ModContext *c, const ModClusterImage *m) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (m && m->reserved != 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster image: reserved must be 0");
  if (m && !m->image && !m->host_image) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster image: image or host_image is required");
  if (m && ((uintptr_t)m->image & 15)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster image: image must be 16-byte aligned");
  c->image_on = m != nullptr;
  c->image = m ? *m : ModClusterImage{};
  if (m && m->palette_bgr) {
    memcpy(c->image_bytes, m->palette_bgr, sizeof(c->image_bytes));
    c->image.palette_bgr = c->image_bytes;
  } else {
    label_palette::builtin_bytes(c->image_bytes);
  }
  label_palette::table_from_bytes(c->image_bytes, &c->image_table);
  return MOD_OK;
}
int mod_get_cluster_image(const ModContext *c, ModClusterImage *m, int32_t *enabled) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (m) *m = c->image;
  if (enabled) *enabled = c->image_on ? 1 : 0;
  return MOD_OK;
}

int mod_cluster_image_dev(ModContext *c, int32_t frames, const int32_t *labels, const int32_t *n_clusters, const uint8_t *palette_bgr, uint8_t *image) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if (!labels || !n_clusters || !image) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster image: labels, n_clusters and image are required");
  if ((uintptr_t)image & 15) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster image: image must be 16-byte aligned");
  if ((uintptr_t)labels & 3) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster image: labels must be 4-byte aligned");
  label_palette::Table t;
  if (palette_bgr) label_palette::table_from_bytes(palette_bgr, &t);
  else { uint8_t b[3 * label_palette::kEntries]; label_palette::builtin_bytes(b); label_palette::table_from_bytes(b, &t); }
  return render_cluster_image(c, frames, labels, n_clusters, t, image);
}

int mod_cluster_color(int32_t k, int32_t n_clusters, const uint8_t *palette_bgr, uint8_t bgr[3]) {
  if (!bgr || k < 0 || k >= n_clusters) return MOD_ERR_INVALID_ARGUMENT;
  const uint32_t i = label_palette::palette_index((uint32_t)k, (uint32_t)n_clusters);
  const uint32_t v = palette_bgr ? (uint32_t)palette_bgr[3 * i] | ((uint32_t)palette_bgr[3 * i + 1] << 8) | ((uint32_t)palette_bgr[3 * i + 2] << 16)
                                 : label_palette::builtin_bgr(i);
  bgr[0] = (uint8_t)v; bgr[1] = (uint8_t)(v >> 8); bgr[2] = (uint8_t)(v >> 16);
  return MOD_OK;
}
int mod_cluster_palette(uint8_t palette_bgr[768]) {
  if (!palette_bgr) return MOD_ERR_INVALID_ARGUMENT;
  label_palette::builtin_bytes(palette_bgr);
  return MOD_OK;
}

// ---- the constructor's views on device planes: static flow, flow / residual / disparity images (flow_image.hip) ----
// What the four calls check in one order: context, frames (blockIdx.z carries them: 1 .. 65535), the output, then the camera
static int check_view(ModContext *c, int32_t frames, const void *out, size_t out_align, const char *what) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (frames < 1 || frames > 65535) return fail(c, MOD_ERR_INVALID_ARGUMENT, std::string(what) + ": frames must be 1 .. 65535");
  if (!out) return fail(c, MOD_ERR_INVALID_ARGUMENT, std::string(what) + ": null output");
  if ((uintptr_t)out & (out_align - 1)) return fail(c, MOD_ERR_INVALID_ARGUMENT, std::string(what) + ": output must be " + std::to_string(out_align) + "-byte aligned");
  return MOD_OK;
}
static int check_view_camera(ModContext *c, const char *what) {
  return c->has_cam ? MOD_OK : fail(c, MOD_ERR_NOT_CONFIGURED, std::string(what) + ": the camera must be set first");
}
static bool usable_max_px(float max_px) { return std::isfinite(max_px) && max_px > 0.0f; }

int mod_static_flow_dev(ModContext *c, int32_t frames, const float *disparity_prev, const ModTransform *transforms, float *static_flow) {
  int rc = check_view(c, frames, static_flow, 8, "static flow");
  if (rc || (rc = check_view_camera(c, "static flow"))) return rc;
  if (!disparity_prev) return MOD_SKIP_NO_DISPARITY_PREV;
  if (!transforms) return MOD_SKIP_NO_TRANSFORM;
  if (((uintptr_t)disparity_prev & 3) || ((uintptr_t)transforms & 7))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "static flow: disparity_prev must be 4-byte and transforms 8-byte aligned");
  launch_static_flow(c->dc, frames, disparity_prev, transforms, static_flow, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

static int flow_image(ModContext *c, int32_t frames, const float *flow, const float *still, bool residual, float max_px, uint8_t *bgr) {
  int rc = check_view(c, frames, bgr, 4, "flow image");
  if (rc) return rc;
  if (!usable_max_px(max_px)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow image: max_px must be finite and > 0");
  if ((rc = check_view_camera(c, "flow image"))) return rc;
  if (!flow || (residual && !still)) return MOD_SKIP_NO_FLOW;
  if (((uintptr_t)flow | (uintptr_t)still) & 3) return fail(c, MOD_ERR_INVALID_ARGUMENT, "flow image: the flow planes must be 4-byte aligned");
  launch_flow_image(c->dc.W, c->dc.H, frames, flow, residual ? still : nullptr, max_px, bgr, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}
int mod_flow_image_dev(ModContext *c, int32_t frames, const float *flow, float max_px, uint8_t *bgr) {
  return flow_image(c, frames, flow, nullptr, false, max_px, bgr);
}
int mod_flow_residual_image_dev(ModContext *c, int32_t frames, const float *flow, const float *static_flow, float max_px, uint8_t *bgr) {
  return flow_image(c, frames, flow, static_flow, true, max_px, bgr);
}

int mod_disparity_image_dev(ModContext *c, int32_t frames, const float *disparity, uint8_t *bgr) {
  int rc = check_view(c, frames, bgr, 4, "disparity image");
  if (rc || (rc = check_view_camera(c, "disparity image"))) return rc;
  if (!(c->dc.dmax > c->dc.dmin)) return fail(c, MOD_ERR_NOT_CONFIGURED, "disparity image: the camera's max_disparity must exceed its min_disparity");
  if (!disparity) return MOD_SKIP_NO_DISPARITY_NOW;
  if ((uintptr_t)disparity & 3) return fail(c, MOD_ERR_INVALID_ARGUMENT, "disparity image: the plane must be 4-byte aligned");
  launch_disparity_image(c->dc.W, c->dc.H, frames, disparity, c->dc.dmin, c->dc.dmax, bgr, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

int mod_flow_color(float fx, float fy, float max_px, uint8_t bgr[3]) {
  if (!bgr || !usable_max_px(max_px)) return MOD_ERR_INVALID_ARGUMENT;
  const uint32_t v = flow_color::flow_bgr(fx, fy, max_px, flow_color::Builtin());
  bgr[0] = (uint8_t)v; bgr[1] = (uint8_t)(v >> 8); bgr[2] = (uint8_t)(v >> 16);
  return MOD_OK;
}

int mod_set_cluster_members(ModContext *c, const ModClusterMembers *m) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (m && (!m->offsets || !m->indices)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster members: offsets and indices are required");
  if (m && m->reserved != 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "cluster members: reserved must be 0");
  c->members_on = m != nullptr;
  c->members = m ? *m : ModClusterMembers{};
  return MOD_OK;
}
int mod_get_cluster_members(const ModContext *c, ModClusterMembers *m, int32_t *enabled) {
  if (!c) return MOD_ERR_INVALID_ARGUMENT;
  if (m) *m = c->members;
  if (enabled) *enabled = c->members_on ? 1 : 0;
  return MOD_OK;
}

}  // extern "C"

int process_dev(ModContext *c, const ModFrameBatch *in, const ModSceneFlowPlanes *pl, const ModClusterOut *out, const ModClusterMembers *mem) {
  int rc = check_batch(c, in);
  if (rc) return depth_on_skip(c, rc, in, pl);
  uint64_t *mask = (pl && pl->dynamic_mask) ? pl->dynamic_mask : c->b.cluster.mask.get();
  const int chunks = chunk_count(c, in->frames);
  if ((rc = check_scene_flow_out(c, pl, true)) || (rc = check_cluster_io(c, pl, true, out)) || (rc = begin_cluster_scratch(c))) return rc;
  if (chunks > 1) rc = process_chunked(c, in, pl, mask, out, mem, chunks);
  else if (!(rc = run_scene_flow(c, in, pl, mask, true, true))) rc = run_cluster(c, in->frames, pl, mask, true, true, out, mem);
  if (rc) return rc;
  c->scratch_clean = true;
  return MOD_OK;
}

extern "C" {

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
  const void *src = which == 0 ? (const void *)c->b.cluster.mbits : which == 4 ? (const void *)c->b.cluster.mpix : which == 1 ? (const void *)c->b.cluster.clusters
                  : which == 5 ? (const void *)c->b.ego.ncorr : which == 6 ? (const void *)c->b.ego.corr : which == 7 ? (const void *)c->b.ego.hcnt
                  : (const void *)c->b.cluster.counters;
  if (!src) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return MOD_OK;
}

int mod_debug_counters(ModContext *c, unsigned long long *out32) {
  if (!c || !out32) return MOD_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out32, c->b.dbg, kDbgWords * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, reset_dbg(c->b.dbg));
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
