"""GPU: the contract of the two image estimators' seven options (csrc/mod_context.h EstimatorOptions; their mod_set_* / mod_get_* pairs in
csrc/host_sgm.hip, host_flow.hip and host_filters.hip) through the C ABI on one 64 x 32 context: the defaults of a fresh context, a valid
value's round trip, every invalid value refused with the stored value left in force, NULL back to the default, and no setter touching
another option.  No kernel is launched, except in the last test: two fresh contexts, one of which had every option set and reset, must
compute bit-identical disparity and flow."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
W, H = 64, 32
BOTH = 3                                 # MOD_TEXTURE_DISPARITY | MOD_TEXTURE_FLOW


class Option:
    """One row of the table: the pair's name, the struct type (None: an int32 passed by value), the default as a tuple of fields, a valid
    non-default value, and the invalid values, each with the mod_last_error string it must leave (None: only the code is checked)"""

    def __init__(self, name, struct, default, valid, invalid):
        self.name, self.struct, self.default, self.valid, self.invalid = name, struct, default, valid, invalid

    def _make(self, capi, value):
        if self.name == "flow_median":
            return capi.ModFlowMedian(value[0], value[1], tuple(value[2:]))
        return getattr(capi, self.struct)(*value)

    def set(self, ctx, value):
        """the return code of the setter; value None: a NULL pointer (struct options only)"""
        from moving_object_detector_amd import capi
        fn = getattr(ctx.lib, "mod_set_" + self.name)
        if self.struct is None:
            return fn(ctx.h, value[0])
        if value is None:
            return fn(ctx.h, None)
        f = self._make(capi, value)
        return fn(ctx.h, C.byref(f))

    def get(self, ctx):
        from moving_object_detector_amd import capi
        fn = getattr(ctx.lib, "mod_get_" + self.name)
        if self.struct is None:
            v = C.c_int32(-77)
            assert fn(ctx.h, C.byref(v)) == 0
            return (v.value,)
        f = self._make(capi, (-77,) * len(self.default))
        assert fn(ctx.h, C.byref(f)) == 0
        if self.name == "flow_median":
            return (f.window, f.min_valid, f.reserved[0], f.reserved[1])
        return tuple(getattr(f, k) for k, _ in f._fields_)


def _window_cap(noun, threshold_max, last_name, last_bad):
    """the invalid values of the texture / corner filter: (threshold, window, cap, apply | reserved)"""
    w = noun.encode() + b" window must be odd and in 3..15"
    c = noun.encode() + b" cap must be in 1..255"
    return ([((100, window, 31, last_name), w) for window in (0, 4, 17, -3)]
            + [((100, 9, cap, last_name), c) for cap in (0, 256)]
            + [((threshold, 9, 31, last_name), None) for threshold in (-1, threshold_max + 1)]
            + [((100, 9, 31, bad), None) for bad in last_bad])


MEDIAN_WINDOW = b"flow median window must be 0, 3 or 5"
OPTIONS = [
    Option("disparity_subpixel", None, (0,), (4,), [((3,), None), ((-4,), None)]),
    Option("disparity_offset", None, (0,), (17,), [((129,), None), ((-1,), None)]),
    # uniqueness_ratio, speckle_size, speckle_range, reserved; the speckle size's upper end is the context's capacity, W * H pixels
    Option("disparity_filters", "ModDisparityFilters", (0, 0, 0, 0), (15, 40, 2, 0),
           [((100, 40, 2, 0), None), ((-1, 40, 2, 0), None), ((15, W * H + 1, 2, 0), None), ((15, -1, 2, 0), None), ((15, 40, -1, 0), None),
            ((15, 40, 2, 1), None)]),
    # threshold, window, cap, apply (0 and 4: neither estimator, an unknown one)
    Option("texture_filter", "ModTextureFilter", (0, 9, 31, BOTH), (400, 7, 63, 1), _window_cap("texture", 15 * 15 * 255, 1, (0, 4))),
    Option("flow_propagation", None, (1,), (5,), [((2,), None), ((0,), None)]),
    # threshold, window, cap, reserved
    Option("flow_corner_filter", "ModCornerFilter", (0, 9, 31, 0), (200, 5, 15, 0), _window_cap("corner", 15 * 15 * 255 * 255, 0, (1,))),
    # window, min_valid, reserved[2].  Window 0 is this filter's "off", a valid value: its bounds are an even number, 17 and a negative one
    Option("flow_median", "ModFlowMedian", (0, 0, 0, 0), (5, 13, 0, 0),
           [((window, 0, 0, 0), MEDIAN_WINDOW) for window in (4, 17, -3)]
           + [((3, 3 * 3 + 1, 0, 0), None), ((5, 5 * 5 + 1, 0, 0), None), ((5, -1, 0, 0), None), ((5, 13, 1, 0), None), ((5, 13, 0, 1), None)]),
]
IDS = [o.name for o in OPTIONS]


def _context():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(255.0)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    return ctx


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


def _all(ctx):
    return {o.name: o.get(ctx) for o in OPTIONS}


DEFAULTS = {o.name: o.default for o in OPTIONS}


def test_table_covers_the_seven_options():
    assert len(OPTIONS) == 7 and all(o.valid != o.default and len(o.valid) == len(o.default) for o in OPTIONS)
    assert DEFAULTS == {"disparity_subpixel": (0,), "disparity_offset": (0,), "disparity_filters": (0, 0, 0, 0), "texture_filter": (0, 9, 31, 3),
                        "flow_propagation": (1,), "flow_corner_filter": (0, 9, 31, 0), "flow_median": (0, 0, 0, 0)}


def test_fresh_context_has_the_defaults(ctx):
    assert _all(ctx) == DEFAULTS


@pytest.mark.parametrize("opt", OPTIONS, ids=IDS)
def test_set_get_invalid_reset(ctx, opt):
    from moving_object_detector_amd import capi
    assert _all(ctx) == DEFAULTS                               # (every case leaves the context as it found it)
    # (b) a valid value round-trips, (e) and no other getter's answer changes
    assert opt.set(ctx, opt.valid) == 0, ctx.lib.mod_last_error(ctx.h)
    expect = dict(DEFAULTS, **{opt.name: opt.valid})
    assert _all(ctx) == expect
    # (c) every invalid value fails and leaves (b) in force
    for value, message in opt.invalid:
        assert opt.set(ctx, value) == capi.MOD_ERR_INVALID_ARGUMENT, value
        if message is not None:
            assert ctx.lib.mod_last_error(ctx.h) == message, value
        assert _all(ctx) == expect, value
    # (d) NULL restores the default of a struct option; the scalar ones go back by their default value
    assert opt.set(ctx, None if opt.struct else opt.default) == 0
    assert _all(ctx) == DEFAULTS


def test_null_context_and_null_result_are_refused(ctx):
    import types
    from moving_object_detector_amd import capi
    null = types.SimpleNamespace(lib=ctx.lib, h=None)
    for o in OPTIONS:
        assert o.set(null, o.valid) == capi.MOD_ERR_INVALID_ARGUMENT
        assert getattr(ctx.lib, "mod_get_" + o.name)(ctx.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert _all(ctx) == DEFAULTS


def _pair():
    """a 64 x 32 textured pair, left and right: a disparity of 3 px (as prev and now: a flow of 3 px)"""
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (H, W + 8), dtype=np.uint8)
    base = ((base.astype(np.uint16) + np.roll(base, 1, 1) + np.roll(base, 1, 0)) // 3).astype(np.uint8)   # a little smoother than noise
    return np.ascontiguousarray(base[:, :W]), np.ascontiguousarray(base[:, 3:3 + W])


def _compute(ctx, a, b):
    from moving_object_detector_amd import capi
    left, right = torch.from_numpy(a[None]).to(ctx.device), torch.from_numpy(b[None]).to(ctx.device)
    disparity = ctx.estimate_disparity(left, right, capi.ModSgmParams(32, 6, 96, 8, 1, 1))
    flow = ctx.estimate_flow(right, left, capi.flow_params(levels=2))
    ctx.synchronize()
    return disparity.cpu().numpy().view(np.uint32), flow.cpu().numpy().view(np.uint32)


def test_reset_means_default_end_to_end(ctx):
    """every option at its default on a fresh context against a second fresh context on which every setter was called with a
    non-default value and then reset: mod_sgm_compute_dev and mod_flow_compute_dev give the same bits"""
    assert _all(ctx) == DEFAULTS
    a, b = _pair()
    want_d, want_f = _compute(ctx, a, b)
    assert (want_d.view(np.float32) >= 0).mean() > 0.25 and np.isfinite(want_f.view(np.float32)).mean() > 0.25   # the pair is matched, not all rejected
    other = _context()
    try:
        for o in OPTIONS:
            assert o.set(other, o.valid) == 0
        assert _all(other) == {o.name: o.valid for o in OPTIONS}
        for o in OPTIONS:
            assert o.set(other, None if o.struct else o.default) == 0
        assert _all(other) == DEFAULTS
        got_d, got_f = _compute(other, a, b)
    finally:
        other.close()
    assert np.array_equal(got_d, want_d) and np.array_equal(got_f, want_f)
