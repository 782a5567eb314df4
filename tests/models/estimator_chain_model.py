"""The two estimator chains as csrc/host_sgm.hip and host_flow.hip enqueue them (sgm_finish; flow_finish), composed of the models of their
stages and of nothing else.  TEST INFRASTRUCTURE ONLY.

  disparity   winner-take-all, uniqueness, sub-pixel, 3 x 3 median, left-right check   sgm_filters_model.compute (with an offset:
                                                                                       sgm_offset_model.finish on that model's S)
              texture rule on the LEFT image, invalid = -1 whatever the offset         texture_model.reject_disparity
              speckle filter, lo = 0, invalid = -1 whatever the offset                 sgm_filters_model.speckle
  flow        pyramid, census, matching with 1 or 5 seeds, finish (sub-pixel, check)   flow_prop_model.flow
              texture rule on the NOW image                                            texture_model.reject_flow
              min-eigenvalue rule on the NOW image                                     corner_model.reject_flow
              NaN-aware median                                                         flow_median_model.median

Both take ONE frame: a batch is a loop over its frames, so no frame of a model can see another."""
from __future__ import annotations

import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corner_model as cm  # noqa: E402
import flow_median_model as mm  # noqa: E402
import flow_prop_model as fp  # noqa: E402
import sgm_filters_model as fm  # noqa: E402
import sgm_offset_model as om  # noqa: E402
import texture_model as tm  # noqa: E402

# paths: what S was summed over (the model does not use it).  texture: None or (threshold, window, cap, apply) with apply the bit
# mask of include/mod_sf.h; speckle: None or (size, range)
SgmSettings = collections.namedtuple("SgmSettings", "paths lr_check median fraction_bits uniqueness offset texture speckle")
# texture as above, corner: None or (threshold, window, cap), median: None or (window, min_valid)
FlowSettings = collections.namedtuple("FlowSettings", "texture corner median")
TEXTURE_DISPARITY, TEXTURE_FLOW = 1, 2                  # MOD_TEXTURE_DISPARITY, MOD_TEXTURE_FLOW
SGM_OFF = SgmSettings(8, True, True, 0, 0, 0, None, None)
FLOW_OFF = FlowSettings(None, None, None)


def texture_applies(texture, to):
    return texture is not None and texture[0] > 0 and (texture[3] & to) != 0


def unfiltered_disparity(S, settings):
    """the plane behind the left-right check: what the texture rule and the speckle filter start from"""
    s = settings
    if s.offset:
        return om.finish(S, s.offset, bool(s.lr_check), bool(s.median), s.fraction_bits, s.uniqueness)
    return fm.compute(S, bool(s.lr_check), bool(s.median), s.fraction_bits, s.uniqueness)


def disparity_filters(plane, left, settings, speckle_first=False):
    """the texture rule, then the speckle filter, on one float32 plane [H][W]; speckle_first: the WRONG order, for the case tests"""
    s = settings
    stages = []
    if texture_applies(s.texture, TEXTURE_DISPARITY):
        stages.append(lambda p: tm.reject_disparity(p, left, s.texture[0], s.texture[1], s.texture[2], invalid=-1.0))
    if s.speckle is not None and s.speckle[0] > 0:
        stages.append(lambda p: fm.speckle(p, s.speckle[0], s.speckle[1], lo=0.0, invalid=-1.0))
    out = np.array(plane, np.float32)
    for stage in (stages[::-1] if speckle_first else stages):
        out = stage(out)
    return out


def disparity(S, left, settings):
    """float32 [H][W] from the summed path costs S [H][W][D] of ONE frame (with an offset: sgm_offset_model's S under that offset) and
    its left image; invalid is -1 whatever the offset is"""
    assert S.ndim == 3 and left.shape == S.shape[:2]
    return disparity_filters(unfiltered_disparity(S, settings), left, settings)


def flow_filters(plane, now, settings, stages=False):
    """texture rule, min-eigenvalue rule, median on one float32 plane [H][W][2]; stages=True: the plane behind each of the three"""
    s = settings
    out = np.array(plane, np.float32)
    if texture_applies(s.texture, TEXTURE_FLOW):
        out = tm.reject_flow(out, now, s.texture[0], s.texture[1], s.texture[2])
    after_texture = out
    if s.corner is not None and s.corner[0] > 0:
        out = cm.reject_flow(out, now, *s.corner)
    after_corner = out
    if s.median is not None and s.median[0] > 0:
        out = mm.median(out, s.median[0], s.median[1])
    return (after_texture, after_corner, out) if stages else out


def flow(prev, now, params, seeds, settings):
    """float32 [H][W][2] of ONE image pair; params: flow_model.FlowParams"""
    assert prev.ndim == 2 and prev.shape == now.shape
    return flow_filters(fp.flow(prev, now, params, seeds), now, settings)
