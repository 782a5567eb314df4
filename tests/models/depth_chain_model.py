"""The chain from depth messages to disparity planes (run_depth_chain of csrc/host_depth.hip; include/mod_sf.h, "RGB-D cameras" and the
three stages behind it) as a composition of the stages' numpy models: depth_filter_model, then depth_spatial_model, then
depth_temporal_model with its state carried in and out, then depth_model.to_disparity or, registered, depth_model.register /
depth_splat_model.register_splat / depth_undistort_model.register.  TEST INFRASTRUCTURE ONLY.  It holds no arithmetic of its own: what
a stage computes is that stage's model, and a stage is on where the library says it is (a filter with a bound or a window, a spatial
window, an alpha).  The bytes of a row beyond `width` samples are not defined between stages; they are carried as the models carry
them (the input's), and nothing downstream reads them."""
import numpy as np

import depth_filter_model as dfm
import depth_model as dm
import depth_spatial_model as dsm
import depth_splat_model as dpm
import depth_temporal_model as dtm
import depth_undistort_model as dum

STAGES = ("filter", "spatial", "temporal")


def filter_on(flt):
    return flt is not None and (np.float32(flt.z_min) != 0 or np.float32(flt.z_max) != 0 or flt.window != 0)


def spatial_on(spa):
    return spa is not None and spa.window != 0


def temporal_on(tmp):
    return tmp is not None and np.float32(tmp.alpha) != 0


def stages(msgs, lay, flt, spa, tmp, state, frames):
    """the messages behind each stage that is on, in order: ({stage: uint8 [frames][height][step]}, the last of them (the input where
    none is on), state, counters as chain() returns them)"""
    m = np.ascontiguousarray(msgs).view(np.uint8).reshape(frames, lay.height, lay.step)
    behind, changed = {}, dict.fromkeys(STAGES, 0)
    counters = dict.fromkeys(dtm.COUNTERS, 0)

    def step(name, out):
        changed[name] = int(np.count_nonzero(dfm.words(out, lay, frames) != dfm.words(m, lay, frames)))
        behind[name] = out
        return out
    if filter_on(flt):
        m = step("filter", dfm.filter_messages(m, lay, flt, frames))
    if spatial_on(spa):
        m = step("spatial", dsm.spatial_messages(m, lay, spa, frames))
    if temporal_on(tmp):
        out, state, counters = dtm.filter_messages(m, lay, tmp, frames, state)
        m = step("temporal", out)
    counters = dict(counters, changed=changed)
    return behind, m, state, counters


def chain(msgs, lay, flt, spa, tmp, state, frames, *, W, H, fT, min_disparity, reg=None, splat=False, D=None, cam=None):
    """(disparity [frames][H][W] float32, state, counters) of `frames` consecutive messages of layout `lay` (a depth_model.Layout).
    flt / spa / tmp: a depth_filter_model.Filter, depth_spatial_model.Spatial, depth_temporal_model.Temporal, or None (off).  state:
    the temporal model's (s, age), None = empty; it is returned as the stage left it (as given while the stage is off) and the given
    planes are not modified.  reg None: the plain path, the W x H window at (lay.x0, lay.y0); else a depth_model.Registration with
    `cam` the image camera, `splat` the footprints and D the eight distortion coefficients or None.  counters: the temporal model's
    (all zero while it is off) and, under "changed", the number of sample words each stage changed."""
    _, m, state, counters = stages(msgs, lay, flt, spa, tmp, state, frames)
    if reg is None:
        d = dm.to_disparity(m, lay, W, H, fT, min_disparity, frames)
    elif D is not None:
        d, _ = dum.register(m, lay, reg, D, cam, W, H, fT, min_disparity, frames, splat)
    elif splat:
        d, _ = dpm.register_splat(m, lay, reg, cam, W, H, fT, min_disparity, frames)
    else:
        d, _ = dm.register(m, lay, reg, cam, W, H, fT, min_disparity, frames)
    assert d.dtype == np.float32 and d.shape == (frames, H, W)
    return d, state, counters
