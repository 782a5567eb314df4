"""GPU: neighbour-seed propagation of the on-GPU optical flow (csrc/flow.hip k_flow_match_seeds, mod_set_flow_propagation) through
the C ABI — bit for bit against the numpy restatement (tests/models/flow_prop_model.py) over the shapes, windows and modes at which
the kernel can go wrong, the fixture, the context state, the two streams that estimate their flow, and the effect on moving boxes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
GOLD = os.path.join(HERE, "golden", "flow", "flow_prop_320x240.npz")
FRAMES = 3


def _ctx(W, H, F, seeds=None):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(synth.Params())
    if seeds is not None:
        ctx.set_flow_propagation(seeds)
    return ctx


def _gpu(ctx, prev, now, prm):
    F, H, W = now.shape
    dev = ctx.device
    tp, tn = torch.from_numpy(prev).to(dev), torch.from_numpy(now).to(dev)
    out = torch.full((F, H, W, 2), -7.0, dtype=torch.float32, device=dev)
    return ctx.estimate_flow(tp, tn, prm, out).cpu().numpy()   # (.cpu() waits: the context runs on torch\'s stream)


def _diff(a, b):
    """pixels that differ, compared as uint32 bits (the model's NaN is the kernel's: 0x7fc00000)"""
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).sum())


@pytest.mark.parametrize("window", [3, 5, 7])
@pytest.mark.parametrize("W,H", [(150, 77), (128, 64)])
def test_five_seeds_match_the_model_bit_for_bit(W, H, window):
    """150 x 77 at 3 levels: a ragged last 64 x 4 block and odd sizes on every level; 128 x 64: block-aligned, the coarsest level
    exactly 32 x 16.  Boxes moving by 4..12 px, so the seeds differ at their rims.  Three frames in one call (dir * frames + frame),
    sub-pixel on / off and forward-backward check off / on — all four finished from one pair of model fields per frame."""
    import flow_prop_model as fp
    from moving_object_detector_amd import capi, synth
    ms = [synth.make_moving_images(W, H, seed=W + f, n_boxes=2, shift=(4, 12)) for f in range(FRAMES)]
    prev, now = np.stack([m["left0"] for m in ms]), np.stack([m["left1"] for m in ms])
    base = fp.FlowParams(levels=3, window=window)
    five = [fp.fields(prev[f], now[f], base, seeds=5) for f in range(FRAMES)]
    one = [fp.integer_flow(prev[f], now[f], base, seeds=1) for f in range(FRAMES)]
    for f in range(FRAMES):                                       # the seeds must matter here, or the parity shows nothing
        assert ((five[f][0] != one[f][0]) | (five[f][1] != one[f][1])).any(), f
    ctx = _ctx(W, H, FRAMES, seeds=5)
    for subpixel in (0, 1):
        for fb in (-1, 1):
            got = _gpu(ctx, prev, now, capi.flow_params(levels=3, window=window, subpixel=subpixel, fb_check=fb))
            p = fp.FlowParams(levels=3, window=window, subpixel=subpixel, fb_check=fb)
            for f in range(FRAMES):
                want = fp.finish(*five[f], p)
                assert _diff(got[f], want) == 0, (subpixel, fb, f, _diff(got[f], want))
    ctx.close()


def test_fixture_and_state():
    """The GPU reproduces the fixture; set 5, compute, set 1, compute: the second result is a fresh context's default bit for bit."""
    from moving_object_detector_amd import capi
    g = np.load(GOLD)
    H, W = g["prev"].shape[1:]
    ctx = _ctx(W, H, 1)
    prms = [capi.ModFlowParams(*[int(v) for v in g["params"][k]]) for k in range(int(g["pairs"]))]
    default = [_gpu(ctx, g["prev"][k][None], g["now"][k][None], prms[k])[0] for k in range(len(prms))]
    ctx.close()
    ctx = _ctx(W, H, 1)
    ctx.set_flow_propagation(int(g["seeds"]))
    for k in range(len(prms)):
        got = _gpu(ctx, g["prev"][k][None], g["now"][k][None], prms[k])[0]
        assert _diff(got, g["flow"][k]) == 0, (k, _diff(got, g["flow"][k]))
        assert _diff(got, default[k]) > 0, k
        host = np.full((H, W, 2), -7.0, np.float32)               # the host form reads the same state
        pv, nw = np.ascontiguousarray(g["prev"][k]), np.ascontiguousarray(g["now"][k])
        assert ctx.flow_host(pv, nw, prms[k], host)[0] == 0
        assert _diff(host, got) == 0, k
    ctx.set_flow_propagation(1)
    for k in range(len(prms)):
        again = _gpu(ctx, g["prev"][k][None], g["now"][k][None], prms[k])[0]
        assert _diff(again, default[k]) == 0, (k, _diff(again, default[k]))
    ctx.close()


@pytest.mark.parametrize("stream", ["images", "odometry"])
def test_stream_frames_carry_the_seeds_of_their_submit(stream):
    """Submit A under 5 seeds, set 1, submit B, then collect both: A's flow_out is mod_flow_compute_dev's under 5 seeds on the same
    images, B's the one under 1 seed."""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    W, H, D, CAP = 320, 240, 128, 32
    m = synth.make_moving_images(W, H, seed=7, n_boxes=3, shift=(4, 12), frames=3)
    lefts = [np.ascontiguousarray(m["left%d" % k]) for k in range(3)]
    rights = [np.ascontiguousarray(m["right%d" % k]) for k in range(3)]
    fprm = capi.flow_params()
    ref = _ctx(W, H, 1)
    want = {}
    for seeds, (a, b) in ((5, (0, 1)), (1, (1, 2))):
        ref.set_flow_propagation(seeds)
        want[seeds] = _gpu(ref, lefts[a][None], lefts[b][None], fprm)[0]
    ref.set_flow_propagation(1)
    other = _gpu(ref, lefts[0][None], lefts[1][None], fprm)[0]
    ref.close()
    assert _diff(other, want[5]) > 0                              # the two settings are told apart on frame A
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(D - 1)
    sp, ep = capi.ModSgmParams(D, 6, 96, 8, 1, 1), capi.ego_params()
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params(cluster_size=150))
    flows = np.full((3, H, W, 2), -7.0, np.float32)
    objs = [(capi.ModObject * CAP)() for _ in range(3)]
    tfs, egos = [capi.ModTransform() for _ in range(3)], [capi.ModEgoResult() for _ in range(3)]
    t, n = C.c_int32(-1), C.c_int32(-1)
    tickets = []
    for f, seeds in enumerate((5, 5, 1)):                         # frame 0 only leaves its image behind; A = frame 1, B = frame 2
        ctx.set_flow_propagation(seeds)
        if stream == "images":
            rc = ctx.lib.mod_submit_images_host(ctx.h, lefts[f].ctypes.data, rights[f].ctypes.data, C.byref(sp), C.byref(fprm), C.byref(tf[0]),
                                                1.0 / 15.0, None, None, objs[f], CAP, None, flows[f].ctypes.data, C.byref(t))
        else:
            rc = ctx.lib.mod_submit_odometry_host(ctx.h, lefts[f].ctypes.data, rights[f].ctypes.data, C.byref(sp), C.byref(fprm), C.byref(ep),
                                                  1.0 / 15.0, None, None, objs[f], CAP, None, flows[f].ctypes.data, C.byref(tfs[f]),
                                                  C.byref(egos[f]), C.byref(t))
        if f == 0:
            assert rc == capi.MOD_SKIP_NO_FLOW and t.value == -1             # no previous image yet
        else:
            assert rc == 0, ctx.lib.mod_last_error(ctx.h)
            tickets.append(t.value)
    ctx.set_flow_propagation(5)                                   # changing it again before the collect changes nothing in flight
    for tk in tickets:
        assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) >= 0, ctx.lib.mod_last_error(ctx.h)   # (a failed ego-motion estimate is a skip code)
    ctx.close()
    assert _diff(flows[1], want[5]) == 0, (stream, "A", _diff(flows[1], want[5]))
    assert _diff(flows[2], want[1]) == 0, (stream, "B", _diff(flows[2], want[1]))


def test_effect_on_moving_boxes_at_640x480():
    """make_moving_images(640, 480, seed=1, shift=(8, 24)), subpixel 0, fb_check 1.  bad: truth and result finite and
    max(|dx|, |dy|) > 1; coverage: share of truth-valid pixels with a finite result.  The model gave 8134 bad pixels and coverage
    0.9499 with one seed, 3159 and 0.9869 with five; the GPU equals the model, so these counts are
    deterministic.  Both come from this run: the baseline is the default path."""
    import flow_prop_model as fp
    from moving_object_detector_amd import capi, synth
    W, H = 640, 480
    m = synth.make_moving_images(W, H, seed=1, shift=(8, 24))
    prm = capi.flow_params(subpixel=0, fb_check=1)
    ctx = _ctx(W, H, 1)
    one = fp.score(_gpu(ctx, m["left0"][None], m["left1"][None], prm)[0], m["flow"])
    ctx.set_flow_propagation(5)
    five = fp.score(_gpu(ctx, m["left0"][None], m["left1"][None], prm)[0], m["flow"])
    ctx.close()
    print("seeds 1:", one, "seeds 5:", five)
    assert five["bad"] <= 0.5 * one["bad"], (one, five)
    assert five["coverage"] > one["coverage"], (one, five)
