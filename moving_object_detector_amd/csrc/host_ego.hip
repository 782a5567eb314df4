// host_ego.hip — the C ABI's on-GPU stereo ego-motion estimator, host side (no kernel): its parameter check, the correspondence
// scratch, the one launch (run_egomotion: the synchronous call's and the odometry stream's) and mod_egomotion_dev.  The kernels live
// in egomotion.hip.
#include "mod_context.h"

#include <algorithm>
#include <cmath>

int check_ego_params(ModContext *c, const ModEgoParams *p) {
  if (!p) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null ego-motion parameters");
  if (p->stride < 1 || p->stride > 64) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion stride must be in 1..64");
  if (p->hypotheses < 1 || p->hypotheses > MOD_EGO_MAX_HYPOTHESES)
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion hypotheses must be in 1..4096");
  if (p->iterations < 0 || p->iterations > 100) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion iterations must be in 0..100");
  if (p->min_inliers < 0) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion min_inliers must be >= 0");
  if (!(p->inlier_threshold > 0.0f) || !std::isfinite(p->inlier_threshold))
    return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion inlier_threshold must be a positive number");
  if (!std::isfinite(p->min_disparity)) return fail(c, MOD_ERR_INVALID_ARGUMENT, "ego-motion min_disparity must be finite");
  return MOD_OK;
}

// Correspondence scratch for `stride` (max_width x max_height x max_frames / stride^2); grows, after a sync, when a smaller stride comes.
static int ensure_ego_scratch(ModContext *c, int stride) {
  Buffers::Ego &b = c->b.ego;
  const size_t F = (size_t)c->cfg.max_frames;
  const int gw = (c->cfg.max_width + stride - 1) / stride, gh = (c->cfg.max_height + stride - 1) / stride;
  const size_t cap = (size_t)gw * gh;
  if (cap > b.cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    b.corr.reset(); b.flag.reset(); b.blkcnt.reset(); b.cap = 0;
    HIP_TRY(c, dalloc(b.corr, F * 9 * cap));
    HIP_TRY(c, dalloc(b.flag, F * cap));
    HIP_TRY(c, dalloc(b.blkcnt, F * (size_t)ego_grid_blocks(gw, gh)));
    b.cap = cap;
  }
  if (!b.res) {
    HIP_TRY(c, dalloc(b.ncorr, F));
    HIP_TRY(c, dalloc(b.hyp, F * MOD_EGO_MAX_HYPOTHESES * 12));
    HIP_TRY(c, dalloc(b.hcnt, F * MOD_EGO_MAX_HYPOTHESES));
    HIP_TRY(c, dalloc(b.tf, F));
    HIP_TRY(c, dalloc(b.res, F));
  }
  return MOD_OK;
}

int run_egomotion(ModContext *c, int frames, const float *dprev, const float *dnow, const float *flow, const ModEgoParams *p,
                  ModTransform *tf, ModEgoResult *res, FrameConst *fc, double dt) {
  int rc = ensure_ego_scratch(c, p->stride);
  if (rc) return rc;
  Buffers::Ego &b = c->b.ego;
  EgoArgs a;
  a.W = c->dc.W; a.H = c->dc.H; a.frames = frames; a.stride = p->stride;
  a.gw = (a.W + p->stride - 1) / p->stride; a.gh = (a.H + p->stride - 1) / p->stride;
  a.cap = (int)b.cap;
  a.hyps = p->hypotheses; a.iterations = p->iterations; a.min_inliers = p->min_inliers; a.seed = p->seed;
  a.dlo = std::max(c->cam.min_disparity, p->min_disparity); a.dhi = c->cam.max_disparity;
  a.th = (double)p->inlier_threshold;
  a.fx = c->cam.fx; a.fy = c->cam.fy; a.cx = c->cam.cx; a.cy = c->cam.cy; a.Tx = c->cam.Tx; a.Ty = c->cam.Ty; a.fT = (double)c->dc.fT;
  a.dprev = dprev; a.dnow = dnow; a.flow = flow;
  a.corr = b.corr; a.blkcnt = b.blkcnt; a.ncorr = b.ncorr; a.hyp = b.hyp; a.hcnt = b.hcnt; a.flag = b.flag;
  a.tf = reinterpret_cast<double *>(tf ? tf : b.tf.get()); a.res = res ? res : b.res.get(); a.fc = fc; a.dt = dt;
  static_assert(sizeof(ModTransform) == 7 * sizeof(double), "ModTransform is 7 doubles");
  launch_egomotion(a, c->stream);
  HIP_TRY(c, hipGetLastError());
  return MOD_OK;
}

extern "C" {

int mod_egomotion_dev(ModContext *c, int32_t frames, const float *disparity_prev, const float *disparity_now, const float *flow,
                      const ModEgoParams *p, ModTransform *transforms, ModEgoResult *results) {
  int rc = check_ready(c, frames);
  if (rc) return rc;
  if ((rc = check_ego_params(c, p))) return rc;
  if (!transforms) return fail(c, MOD_ERR_INVALID_ARGUMENT, "null transforms");
  if ((rc = construct_skip(flow, disparity_prev, true, disparity_now))) return rc;
  return run_egomotion(c, frames, disparity_prev, disparity_now, flow, p, transforms, results, nullptr, 0.0);
}

}  // extern "C"
