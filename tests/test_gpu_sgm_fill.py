"""GPU: the occlusion hole fill inside the disparity estimator (mod_set_disparity_fill; include/mod_sf.h): mod_sgm_compute_dev with the
fill on equals, bit for bit, the estimator's models (tests/models/sgm_filters_model.compute_images; with an offset
sgm_offset_model.compute; the texture rule of texture_model and the speckle stage of sgm_filters_model behind them) followed by
tests/models/disparity_fill_model.fill with lo = 0 — on small layered stereo pairs (synth.make_stereo_images: foreground boxes, so that
the left-right check leaves an occlusion strip left of each), 96 x 48, D = 32 and 64, alone and combined with the sub-pixel mode, an
offset, uniqueness, texture and speckle, on 1, 3 and 11 frames (11: two groups of unequal size, both scratch sets).  A call with the fill
off made after one with it on writes the plain estimator's bytes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import disparity_fill_model as dm  # noqa: E402
import sgm_filters_model as sm  # noqa: E402
import sgm_offset_model as om  # noqa: E402
import texture_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
W, H = 96, 48
TEXTURE = (60, 5, 31)               # threshold, window, cap
SPECKLE = (12, 1)                   # size, range


def _ctx(F):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(synth.Params())
    return ctx


def _pairs(F, D, seed):
    from moving_object_detector_amd import synth
    p = [synth.make_stereo_images(W, H, seed + f, D, n_boxes=3) for f in range(F)]
    return np.stack([a for a, _, _ in p]), np.stack([b for _, b, _ in p])


def _estimate(ctx, left, right, D):
    from moving_object_detector_amd import capi
    out = torch.full(left.shape, -7.0, dtype=torch.float32, device=ctx.device)
    tl, tr = torch.from_numpy(left).to(ctx.device), torch.from_numpy(right).to(ctx.device)
    return ctx.estimate_disparity(tl, tr, capi.ModSgmParams(D, 6, 96, 8, 1, 1), out).cpu().numpy()


def _model(left, right, D, subpixel=False, offset=0, uniqueness=0, texture=False, speckle=False):
    """the estimator in front of the fill, one frame: the models of the stages in the estimator's order"""
    bits = 4 if subpixel else 0
    if offset:
        d = om.compute(left, right, D, 6, 96, 8, True, True, offset, bits, uniqueness)
    else:
        d = sm.compute_images(left, right, D, 6, 96, 8, True, True, bits, uniqueness)
    if texture:
        d = tm.reject_disparity(d, left, *TEXTURE, -1.0)
    if speckle:
        d = sm.speckle(d, SPECKLE[0], SPECKLE[1], 0.0, -1.0)
    return d


def _set(ctx, subpixel=False, offset=0, uniqueness=0, texture=False, speckle=False):
    from moving_object_detector_amd import capi
    ctx.set_disparity_subpixel(bool(subpixel))
    ctx.set_disparity_offset(offset)
    ctx.set_disparity_filters(uniqueness, SPECKLE[0] if speckle else 0, SPECKLE[1] if speckle else 0)
    ctx.set_texture_filter(*TEXTURE, capi.MOD_TEXTURE_DISPARITY) if texture else ctx.set_texture_filter()


CASES = [
    # D, F, options of the estimator, (reach, directions, mode, min_found)
    (32, 1, dict(), (16, 8, dm.MIN, 1)),
    (64, 1, dict(), (64, 2, dm.MIN, 1)),
    (32, 3, dict(), (8, 4, dm.MEDIAN, 2)),
    (32, 11, dict(), (32, 8, dm.SECOND, 3)),
    (32, 1, dict(subpixel=True), (16, 8, dm.MEDIAN, 1)),
    (32, 1, dict(offset=4), (16, 8, dm.MIN, 1)),
    (32, 1, dict(uniqueness=15), (16, 8, dm.MIN, 2)),
    (32, 1, dict(texture=True), (16, 4, dm.MIN, 1)),
    (32, 1, dict(speckle=True), (4, 8, dm.SECOND, 1)),
    (64, 3, dict(subpixel=True, uniqueness=10, texture=True, speckle=True), (24, 8, dm.MEDIAN, 2)),
    (32, 11, dict(subpixel=True, offset=3, speckle=True), (256, 8, dm.MIN, 8)),
]


@pytest.mark.parametrize("D,F,opts,fill", CASES, ids=[f"D{c[0]}-F{c[1]}-{'+'.join(c[2]) or 'alone'}" for c in CASES])
def test_estimator_with_the_fill_equals_the_models_composed(D, F, opts, fill):
    left, right = _pairs(F, D, seed=3 * D + F)
    ctx = _ctx(F)
    _set(ctx, **opts)
    plain = _estimate(ctx, left, right, D)                                     # the fill is off: the estimator as it always was
    ctx.set_disparity_fill(*fill)
    got = _estimate(ctx, left, right, D)
    ctx.set_disparity_fill()
    again = _estimate(ctx, left, right, D)                                     # off again, behind a call with it on
    holes = filled = 0
    for f in range(F):
        before = _model(left[f], right[f], D, **opts)
        assert dm.bits(plain[f]).tobytes() == dm.bits(before).tobytes(), (f, "the estimator in front of the fill")
        want, did = dm.fill(before, *fill, lo=0.0, return_filled=True)
        assert dm.bits(got[f]).tobytes() == dm.bits(want).tobytes(), (f, int((dm.bits(got[f]) != dm.bits(want)).sum()))
        holes, filled = holes + int((before < 0).sum()), filled + int(did.sum())
    print("holes", holes, "filled", filled, "of", F * W * H)
    assert holes > 0 and filled > 0                                            # an occlusion strip exists and something of it is filled
    assert again.tobytes() == plain.tobytes()
    ctx.close()


def test_the_setting_is_read_per_call_and_the_getter_returns_it():
    D, F = 32, 3
    left, right = _pairs(F, D, seed=7)
    ctx = _ctx(F)
    plain = _estimate(ctx, left, right, D)
    ctx.set_disparity_fill(16)
    g = ctx.get_disparity_fill()
    assert (g.reach, g.directions, g.mode, g.min_found) == (16, 8, 0, 1)
    on = _estimate(ctx, left, right, D)
    want = dm.fill(plain, 16, 8, dm.MIN, 1, 0.0)
    assert dm.bits(on).tobytes() == dm.bits(want).tobytes() and on.tobytes() != plain.tobytes()
    # a filled word is a measured one: inside the window, and nothing that was measured has changed
    assert (on[plain >= 0] == plain[plain >= 0]).all() and on.max() <= D - 1
    # the stand-alone call on the plain output gives the same planes (the camera's min_disparity is 0: the estimator's lo)
    alone = ctx.disparity_fill(torch.from_numpy(plain).to(ctx.device), ctx.get_disparity_fill()).cpu().numpy()
    assert alone.tobytes() == on.tobytes()
    ctx.close()
