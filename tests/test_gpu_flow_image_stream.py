"""GPU: the views share no state with the pipeline.  A short HostStream images run (mod_submit_images_host: disparity, flow, scene
flow and clustering per frame, frames in flight) gives the same bytes and the same objects whether the new calls are never made or
are made after every submit and in front of every collect — on planes of their own, on the context's stream, between the frames'
kernels."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import flow_image_model as M  # noqa: E402
from util import assert_same_stream  # noqa: E402

W, H, FR, CAP, DT = 64, 40, 6, 16, 1.0 / 15.0
KEYS = ("cloud", "labels", "disparity", "flow")


def _scene(seed=11, far=3, near=9):
    """left / right grey images [FR][H][W]: a textured wall `far` pixels of disparity away and a textured box `near` away that moves
    two pixels a frame"""
    rng = np.random.default_rng(seed)
    ww = W + near + 2 * FR + 8
    wall = np.kron(rng.integers(0, 256, size=((H + 1) // 2, (ww + 1) // 2)), np.ones((2, 2), np.int64))[:H, :ww].astype(np.uint8)
    box = np.kron(rng.integers(0, 256, size=(8, 10)), np.ones((2, 2), np.int64)).astype(np.uint8)          # 16 x 20 pixels
    left, right = np.empty((FR, H, W), np.uint8), np.empty((FR, H, W), np.uint8)
    for f in range(FR):
        left[f], right[f] = wall[:, :W], wall[:, far:far + W]
        x = 12 + 2 * f
        left[f, 10:26, x:x + 20] = box
        right[f, 10:26, x - near:x - near + 20] = box
    return left, right


def _run(ctx, views):
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.host_stream import HostStream
    left, right = _scene()
    sp, fp = capi.ModSgmParams(16, 6, 96, 8, 1, 1), capi.flow_params(levels=1)
    made = []

    def view():
        if views is not None:
            made.append(views())

    s = HostStream(ctx, FR, CAP, transform=((0, 0, 0), (0, 0, 0, 1)), before_collect=view)
    s.forget_previous()
    for f in range(FR):
        s.submit_images(f, left[f], right[f], sp, fp, s.transforms[f], DT)
        view()
    s.finish()
    return s, made


def test_views_between_frames_change_nothing():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(15.0)
    ctx.set_camera(cam)
    prm = synth.Params()
    prm.cluster_size, prm.dynamic_flow_diff = 100, 1               # the box is 320 pixels and moves two a frame
    ctx.set_params(prm)
    rng = np.random.default_rng(2)
    flow = (rng.standard_normal((2, H, W, 2)) * 3).astype(np.float32)
    disp = (rng.random((2, H, W)) * 16).astype(np.float32)
    t_flow, t_disp = torch.from_numpy(flow).to(ctx.device), torch.from_numpy(disp).to(ctx.device)
    tf = torch.tensor([[0.01, 0, 0.1, 0, 0, 0, 1.0]] * 2, dtype=torch.float64, device=ctx.device)

    def views():
        still = ctx.static_flow(t_disp, tf)
        return ctx.flow_image(t_flow, 6.0), ctx.flow_image(t_flow, 6.0, static=still), ctx.disparity_image(t_disp), still

    plain, _ = _run(ctx, None)
    mixed, made = _run(ctx, views)
    assert any(rc == 0 for rc in plain.first) and any((plain.disparity[f] > 0).any() for f in range(FR))
    assert_same_stream(plain, mixed, KEYS)
    # ... and the frames in flight around them changed nothing in the views either
    ctx.synchronize()
    assert len(made) >= FR
    first = [t.cpu().numpy() for t in made[0]]
    for later in made[1:]:
        for a, b in zip(first, later):
            assert a.tobytes() == b.cpu().numpy().tobytes()
    assert np.array_equal(first[0], M.flow_image(flow, 6.0)) and np.array_equal(first[2], M.disparity_image(disp, 0.0, 15.0))
    assert np.array_equal(first[1], M.flow_image(flow, 6.0, static=first[3]))
    print("objects per frame:", plain.n)
    ctx.close()
