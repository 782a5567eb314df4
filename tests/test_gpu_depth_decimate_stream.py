"""GPU: mod_submit_depth_host through the Python stream driver with image binning 2 x 2 and depth decimation 2 x 2 median: full-size
256 x 192 image and aligned depth messages of a 128 x 96 camera, five frames, three in flight.  A second stream gets the same images
with the depth that tests/models/depth_decimate_model.py decimated on the host and decimation off.  Every collected output must be
identical: the first codes, the collect codes, the counts, the objects, labels, disparity and flow.  Then: a ticket in flight keeps the
decimation of its own submit when the setting is changed right behind the submit; full-size and host-decimated submits in turn; and a
submit with a registration set is refused and leaves the stream working."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_decimate_model as ddm  # noqa: E402
import depth_model as dm  # noqa: E402
from util import assert_same_stream  # noqa: E402
from moving_object_detector_amd import capi  # noqa: E402

W, H, BX, BY, FR, CAP, DT = 128, 96, 2, 2, 5, 64, 1.0 / 15.0
MW, MH = BX * W, BY * H
KEYS = ("labels", "disparity", "flow")
DEC = ddm.Decimation(2, 2, ddm.MEDIAN, 1)
FULL = dm.Layout("16UC1", MW, MH, 2 * MW)


@pytest.fixture(scope="module")
def scene():
    """synth.make_ego_images at the camera's size; the full-size image repeats every pixel 2 x 2 (its MOD_BIN_MEAN binning is the image
    again); the full-size depth repeats the millimetres of the true disparity 2 x 2 with +-3 mm of noise and 6 % holes, so the median
    has something to do"""
    from moving_object_detector_amd import synth
    m = synth.make_ego_images(W, H, seed=2, frames=FR, shift=(2, 3))
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(63.0)
    fT = np.float32(cam.disp_f) * np.float32(cam.disp_T)
    rng = np.random.default_rng(8)
    image, depth, small = [], [], []
    for f in range(FR):
        image.append(np.ascontiguousarray(np.kron(m[f"left{f}"], np.ones((BY, BX), np.uint8))))
        mm = np.rint(1000.0 * float(fT) / m[f"disparity{f}"].astype(np.float64)).astype(np.int64)
        full = np.kron(mm, np.ones((BY, BX), np.int64)) + rng.integers(-3, 4, size=(MH, MW))
        full[rng.random((MH, MW)) < 0.06] = 0
        full = np.ascontiguousarray(np.clip(full, 0, 65535).astype("<u2"))
        depth.append(full)
        small.append(np.ascontiguousarray(ddm.decimate_messages(full.view(np.uint8).reshape(1, MH, 2 * MW), FULL, DEC)[0]).view("<u2"))
        assert small[-1].shape == (H, W)
    tf = [None] + [(m["t"][f - 1], m["q"][f - 1]) for f in range(1, FR)]
    return {"cam": cam, "image": image, "depth": depth, "small": small, "tf": tf}


@pytest.fixture(scope="module")
def ctx(scene):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(MW, MH, max_frames=1, max_objects=1024)   # (the capacity check counts the full-size window)
    c.set_camera(scene["cam"])
    c.set_params(synth.Params(dynamic_flow_diff=2, cluster_size=50, dynamic_speed=0.2))
    c.set_image_binning(BX, BY, capi.MOD_BIN_MEAN)
    yield c
    c.close()


def _struct(d):
    return capi.depth_decimation(d.dx, d.dy, d.mode, d.min_valid, d.tol_abs, d.tol_rel) if d is not None else None


def _run(ctx, scene, depth_of, before=None, behind=None):
    """five submits of the full-size image f with depth_of(f); before(f) sets the context up in front of submit f (the oldest ticket
    has been collected by then where the pipe was full), behind(f) runs right after it, while its ticket is outstanding"""
    from moving_object_detector_amd.host_stream import HostStream
    s = HostStream(ctx, FR, CAP, outputs=KEYS)
    s.forget_previous()
    try:
        for f in range(FR):
            s.make_room()
            if before:
                before(f)
            s.submit_depth(f, scene["image"][f], depth_of(f), capi.flow_params(levels=2), None, scene["tf"][f] or scene["tf"][1], DT)
            if behind:
                behind(f)
        s.finish()
    finally:
        ctx.set_depth_decimation(None)
    return s


@pytest.fixture(scope="module")
def wanted(ctx, scene):
    """the host-decimated depth with decimation off: the stream as it was before the stage existed"""
    s = _run(ctx, scene, lambda f: scene["small"][f], lambda f: ctx.set_depth_decimation(None))
    assert s.first == [capi.MOD_SKIP_NO_FLOW, 0, 0, 0, 0], s.first
    assert all(rc == 0 for rc in s.rc[1:]), s.rc
    assert sum(s.n) > 0, "no object in any frame: the comparison would be weak"
    for f in range(1, FR):
        assert (s.disparity[f] > 0).mean() > 0.5
    return s


def test_the_stream_matches_the_host_decimated_depth(ctx, scene, wanted):
    got = _run(ctx, scene, lambda f: scene["depth"][f], lambda f: ctx.set_depth_decimation(_struct(DEC)))
    assert_same_stream(got, wanted, KEYS)
    # the setting decides: another mode gives another disparity
    other = _run(ctx, scene, lambda f: scene["depth"][f], lambda f: ctx.set_depth_decimation(_struct(ddm.Decimation(2, 2, ddm.MIN, 1))))
    assert any(other.disparity[f].tobytes() != wanted.disparity[f].tobytes() for f in range(1, FR))


def test_a_ticket_keeps_the_decimation_of_its_submit(ctx, scene, wanted):
    """median in front of every submit, MIN with min_valid 4 right behind it, while the ticket is outstanding"""
    got = _run(ctx, scene, lambda f: scene["depth"][f], lambda f: ctx.set_depth_decimation(_struct(DEC)),
               lambda f: ctx.set_depth_decimation(_struct(ddm.Decimation(2, 2, ddm.MIN, 4))))
    assert_same_stream(got, wanted, KEYS)


def test_full_size_and_host_decimated_submits_in_turn(ctx, scene, wanted):
    """the setting (and with it the default layout) changes between submits while tickets are outstanding"""
    got = _run(ctx, scene, lambda f: scene["depth"][f] if f % 2 == 0 else scene["small"][f],
               lambda f: ctx.set_depth_decimation(_struct(DEC) if f % 2 == 0 else None))
    assert_same_stream(got, wanted, KEYS)


def test_a_registration_refuses_the_submit_and_the_stream_goes_on(ctx, scene, wanted):
    from moving_object_detector_amd.host_stream import HostStream
    cam = scene["cam"]
    ctx.set_depth_decimation(_struct(DEC))
    ctx.set_depth_registration(capi.depth_registration(cam.fx, cam.fy, cam.cx, cam.cy))
    try:
        s = HostStream(ctx, 1, CAP, outputs=KEYS)
        with pytest.raises(capi.ModError) as e:
            s.submit_depth(0, scene["image"][0], scene["depth"][0], capi.flow_params(levels=2), None, scene["tf"][1], DT)
        assert e.value.code == capi.MOD_ERR_INVALID_ARGUMENT and "registration" in str(e.value)
    finally:
        ctx.set_depth_registration(None)
        ctx.set_depth_decimation(None)
    got = _run(ctx, scene, lambda f: scene["depth"][f], lambda f: ctx.set_depth_decimation(_struct(DEC)))
    assert_same_stream(got, wanted, KEYS)
