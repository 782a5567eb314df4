"""GPU: the edge-preserving smoother inside the disparity estimator (mod_set_disparity_smooth; include/mod_sf.h): mod_sgm_compute_dev
with the smoother on equals, bit for bit, tests/models/disparity_smooth_model.smooth (lo = 0) applied to the output of the same call
with the smoother off — on 130 x 17 and 96 x 24 layered stereo pairs (synth.make_stereo_images), D = 16, 33 and 128, alone and combined
with the sub-pixel mode, an offset, the texture rule, the speckle stage and the hole fill behind it (then the two models composed in
the order smooth -> fill, tests/models/disparity_fill_model.fill), on 1 and 9 frames (9: two groups, both scratch sets).  A call with
the smoother off made after one with it on writes the plain estimator's bytes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import disparity_fill_model as dm  # noqa: E402
import disparity_smooth_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TEXTURE = (60, 5, 31)               # threshold, window, cap
SPECKLE = (12, 1)                   # size, range


def _ctx(W, H, F):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(synth.Params())
    return ctx


def _pairs(W, H, F, D, seed, offset=0):
    from moving_object_detector_amd import synth
    p = [synth.make_stereo_images(W, H, seed + f, D, n_boxes=3) for f in range(F)]
    left, right = np.stack([a for a, _, _ in p]), np.stack([b for _, b, _ in p])
    if offset:                       # the same scenes `offset` px nearer: right(x) = right0(x + offset)
        right = np.ascontiguousarray(right[:, :, np.minimum(np.arange(W) + offset, W - 1)])
    return left, right


def _estimate(ctx, left, right, D):
    from moving_object_detector_amd import capi
    out = torch.full(left.shape, -7.0, dtype=torch.float32, device=ctx.device)
    tl, tr = torch.from_numpy(left).to(ctx.device), torch.from_numpy(right).to(ctx.device)
    return ctx.estimate_disparity(tl, tr, capi.ModSgmParams(D, 6, 96, 8, 1, 1), out).cpu().numpy()


def _set(ctx, subpixel=False, offset=0, texture=False, speckle=False, fill=None):
    from moving_object_detector_amd import capi
    ctx.set_disparity_subpixel(bool(subpixel))
    ctx.set_disparity_offset(offset)
    ctx.set_disparity_filters(0, SPECKLE[0] if speckle else 0, SPECKLE[1] if speckle else 0)
    ctx.set_texture_filter(*TEXTURE, capi.MOD_TEXTURE_DISPARITY) if texture else ctx.set_texture_filter()


CASES = [
    # W, H, D, F, options of the estimator, (window, tol, min_members)
    (130, 17, 16, 1, dict(), (5, 1.0, 1)),
    (130, 17, 33, 1, dict(), (3, 2.0, 2)),
    (130, 17, 128, 1, dict(), (7, 1.0, 1)),
    (96, 24, 16, 1, dict(), (7, 4.0, 3)),
    (96, 24, 33, 1, dict(), (5, 1.0, 1)),
    (96, 24, 128, 1, dict(), (3, 1.0, 1)),
    (130, 17, 16, 1, dict(subpixel=True), (5, 1.0, 1)),
    (96, 24, 33, 1, dict(offset=3), (5, 1.0, 1)),
    (130, 17, 33, 1, dict(texture=True), (5, 2.0, 1)),
    (96, 24, 16, 1, dict(speckle=True), (3, 1.0, 1)),
    (130, 17, 128, 1, dict(fill=(16, 8, dm.MIN, 1)), (5, 1.0, 1)),
    (96, 24, 33, 1, dict(fill=(64, 4, dm.MEDIAN, 2)), (7, 1.0, 2)),      # (whole disparities: a tol below 1 would gather equal words only)
    (96, 24, 128, 3, dict(subpixel=True, offset=2, texture=True, speckle=True, fill=(24, 8, dm.SECOND, 1)), (5, 1.0, 1)),
    (96, 24, 33, 9, dict(), (5, 1.0, 1)),
    (130, 17, 16, 9, dict(subpixel=True, fill=(8, 8, dm.MIN, 1)), (7, 1.0, 4)),
]


@pytest.mark.parametrize("W,H,D,F,opts,smooth", CASES, ids=[f"{c[0]}x{c[1]}-D{c[2]}-F{c[3]}-{'+'.join(c[4]) or 'alone'}" for c in CASES])
def test_estimator_with_the_smoother_equals_the_model_on_its_plain_output(W, H, D, F, opts, smooth):
    left, right = _pairs(W, H, F, D, seed=3 * D + F, offset=opts.get("offset", 0))
    fill = opts.get("fill")
    ctx = _ctx(W, H, F)
    _set(ctx, **opts)
    plain = _estimate(ctx, left, right, D)                                     # the smoother and the fill are off: the estimator as it was
    ctx.set_disparity_smooth(*smooth)
    if fill:
        ctx.set_disparity_fill(*fill)
    got = _estimate(ctx, left, right, D)
    if fill:
        ctx.set_disparity_fill()
        alone = _estimate(ctx, left, right, D)                                 # the smoother without the fill behind it
    ctx.set_disparity_smooth()
    again = _estimate(ctx, left, right, D)                                     # off again, behind calls with it on
    smoothed = sm.smooth(plain, *smooth, lo=0.0)                               # per frame: the model never looks across frames
    want = dm.fill(smoothed, *fill, lo=0.0) if fill else smoothed
    changed = int((sm.bits(smoothed) != sm.bits(plain)).sum())
    print("valid", int((plain >= 0).sum()), "changed by the smoother", changed, "of", plain.size)
    assert sm.bits(got).tobytes() == sm.bits(want).tobytes(), int((sm.bits(got) != sm.bits(want)).sum())
    if fill:
        assert sm.bits(alone).tobytes() == sm.bits(smoothed).tobytes()
        assert ((smoothed < 0) & (want >= 0)).any()                            # the fill copied (smoothed) words into holes
    assert (plain >= 0).any() and changed > 0                                  # the comparison is the smoother's
    assert np.array_equal(plain >= 0, smoothed >= 0)                           # it fills no hole and makes none
    assert again.tobytes() == plain.tobytes()
    ctx.close()


def test_the_setting_is_read_per_call_and_the_stand_alone_call_agrees():
    W, H, D, F = 96, 24, 33, 3
    left, right = _pairs(W, H, F, D, seed=7)
    ctx = _ctx(W, H, F)
    ctx.set_disparity_subpixel(True)
    plain = _estimate(ctx, left, right, D)
    ctx.set_disparity_smooth(5)
    g = ctx.get_disparity_smooth()
    assert (g.window, g.min_members, g.tol, g.reserved) == (5, 1, 1.0, 0)
    on = _estimate(ctx, left, right, D)
    assert sm.bits(on).tobytes() == sm.bits(sm.smooth(plain, 5, 1.0, 1, 0.0)).tobytes() and on.tobytes() != plain.tobytes()
    # the stand-alone call on the plain output gives the same planes (the camera's min_disparity is 0: the estimator's lo)
    alone = ctx.disparity_smooth(torch.from_numpy(plain).to(ctx.device), g).cpu().numpy()
    assert alone.tobytes() == on.tobytes()
    ctx.close()
