"""GPU: the host image paths fed 8-bit Bayer messages (csrc/host_api.hip: the window and its one-pixel apron cross PCIe,
k_bayer_to_mono runs on the staged region) give, bit for bit, what the same calls give when fed the model's grey
(tests/models/bayer_model.py) as mono8: mod_sgm_compute_host, mod_flow_compute_host and the stereo, images and odometry submits, on a
64 x 40 camera inside 80 x 52 messages at an odd origin and on a camera that is the whole message; a layout change between submits
while frames are in flight; side by side with an even and an odd pane width; the panes do not leak into each other; the C++ host
mirror (tests/cpp/bayer_mirror_test.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "moving_object_detector_amd")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import bayer_model as bm  # noqa: E402
from util import assert_same_stream  # noqa: E402

W, H, FR, CAP, DT = 64, 40, 4, 16, 1.0 / 15.0
PATTERNS = ("rggb", "bggr", "gbrg", "grbg")
KEYS = ("cloud", "labels", "disparity", "flow", "transform", "ego")      # (what a kind does not write keeps its sentinel)
# name: message width, height, row padding, window origin (the last one: the camera is the whole message)
CAMERAS = {"window": (80, 52, 5, 7, 5), "even origin": (80, 52, 0, 8, 6), "whole": (W, H, 3, 0, 0)}


def _colour_scene(mw, mh, frames, seed, shift=5):
    """left / right colour images [frames][mh][mw][3] of a textured plane `shift` pixels of disparity away that moves one pixel a
    frame: blocks of 2 x 2 and 6 x 6 pixels, the three channels a few levels apart"""
    rng = np.random.default_rng(seed)
    ww = mw + shift + frames + 8
    fine = np.kron(rng.integers(0, 120, size=((mh + 1) // 2, (ww + 1) // 2)), np.ones((2, 2), np.int64))[:mh, :ww]
    coarse = np.kron(rng.integers(0, 120, size=((mh + 5) // 6, (ww + 5) // 6)), np.ones((6, 6), np.int64))[:mh, :ww]
    base = np.clip((fine + coarse)[..., None] + rng.integers(-6, 7, size=(mh, ww, 3)), 0, 255).astype(np.uint8)
    left = np.stack([base[:, k:k + mw] for k in range(frames)])
    right = np.stack([base[:, k + shift:k + shift + mw] for k in range(frames)])
    return left, right


def _messages(name, pattern, seed):
    """per frame: the two Bayer messages [mh][step] and the grey the model makes of their windows; the layout dict"""
    from moving_object_detector_amd import synth
    mw, mh, pad, x0, y0 = CAMERAS[name]
    left, right = _colour_scene(mw, mh, FR, seed)
    rng = np.random.default_rng(seed + 1)
    lay = {"encoding": "bayer_%s8" % pattern, "width": mw, "height": mh, "step": mw + pad, "x0": x0, "y0": y0}
    out = []
    for f in range(FR):
        msgs, greys = [], []
        for eye in (left, right):
            m = rng.integers(0, 256, size=(mh, mw + pad), dtype=np.uint8)
            m[:, :mw] = synth.mosaic(eye[f], pattern)
            msgs.append(m)
            greys.append(bm.to_mono(m, bm.Layout(**lay), W, H)[0])
        out.append((msgs, greys))
    return out, lay


def _layout(lay):
    from moving_object_detector_amd import capi
    return capi.image_layout(lay["encoding"], lay["width"], lay["height"], lay["step"], lay["x0"], lay["y0"])


def _state(ctx, lay, sbs=False):
    if sbs:
        ctx.set_image_layout(_layout(lay))
        ctx.set_side_by_side(True)
    else:
        ctx.set_side_by_side(False)
        ctx.set_image_layout(_layout(lay) if lay is not None else None)


@pytest.fixture(scope="module")
def ctx():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    c = Context(W, H, max_frames=1)
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(15.0)
    c.set_camera(cam)
    c.set_params(synth.Params())
    yield c
    c.close()


def _params():
    from moving_object_detector_amd import capi
    return capi.ModSgmParams(16, 6, 96, 8, 1, 1), capi.flow_params(levels=1), capi.ego_params()


def _run(ctx, kind, frames, feed=None):
    """The `kind` stream ("stereo", "images", "odometry") over frames = [(left, right or None, layout dict or None, side by side)],
    up to MOD_PIPELINE_DEPTH in flight, the layout set in front of every submit.  feed: the odometry run whose flow and transform per
    frame a "stereo" / "images" run is given.  Returns the finished HostStream: every output of every frame."""
    from moving_object_detector_amd.host_stream import HostStream
    sp, fp, ep = _params()
    s = HostStream(ctx, len(frames), CAP, transform=((0, 0, 0), (0, 0, 0, 1)))
    s.forget_previous()
    for f, (l, r, lay, sbs) in enumerate(frames):
        s.make_room()
        _state(ctx, lay, sbs)
        if kind == "odometry":
            s.submit_odometry(f, l, r, sp, fp, ep, DT)                 # (a negative code raises: a skip code of construct()'s guards only)
        elif kind == "images":
            s.submit_images(f, l, r, sp, fp, feed.transforms[f], DT)
        else:
            s.submit_stereo(f, l, r, sp, feed.flow[f], feed.transforms[f], DT)
    s.finish()
    _state(ctx, None)
    return s


def _same(a, b):
    assert any(rc == 0 for rc in a.first), "no frame took a ticket: the comparison would be weak"
    assert_same_stream(a, b, KEYS)
    for f in range(len(a.first)):
        if a.first[f] == 0:
            assert (a.disparity[f] >= 0).any(), "no disparity at all: the comparison would be weak"


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_a_single_frame_host_calls(ctx, name, pattern):
    sp, fp, _ = _params()
    fr, lay = _messages(name, pattern, 31)
    (m0, g0), (m1, g1) = fr[0], fr[1]
    got_d, want_d = (np.full((H, W), -7, np.float32) for _ in range(2))
    got_f, want_f = (np.full((H, W, 2), -7, np.float32) for _ in range(2))
    try:
        _state(ctx, None)
        assert ctx.disparity_host(g1[0], g1[1], sp, want_d)[0] == 0
        assert ctx.flow_host(g0[0], g1[0], fp, want_f)[0] == 0
        assert (want_d >= 0).any()
        _state(ctx, lay)
        assert ctx.disparity_host(m1[0], m1[1], sp, got_d)[0] == 0
        assert ctx.flow_host(m0[0], m1[0], fp, got_f)[0] == 0
    finally:
        _state(ctx, None)
    assert got_d.tobytes() == want_d.tobytes() and got_f.tobytes() == want_f.tobytes()


@pytest.fixture(scope="module")
def mono_runs(ctx):
    """per camera and pattern: the messages, and the three streams fed the model's grey as mono8 (what every Bayer run must equal)"""
    out = {}
    for name in CAMERAS:
        for pattern in PATTERNS[:2] if name != "window" else PATTERNS:
            fr, lay = _messages(name, pattern, 41)
            grey = [(g[0], g[1], None, False) for _, g in fr]
            odo = _run(ctx, "odometry", grey)
            out[name, pattern] = (fr, lay, odo, {"odometry": odo, "images": _run(ctx, "images", grey, odo), "stereo": _run(ctx, "stereo", grey, odo)})
    return out


@pytest.mark.parametrize("kind", ["stereo", "images", "odometry"])
def test_b_streams_match_mono8(ctx, mono_runs, kind):
    for (name, pattern), (fr, lay, feed, want) in mono_runs.items():
        got = _run(ctx, kind, [(m[0], m[1], lay, False) for m, _ in fr], feed)
        _same(got, want[kind])


@pytest.mark.parametrize("kind", ["images", "odometry"])
def test_c_frames_in_flight_keep_their_layout(ctx, mono_runs, kind):
    """Bayer and mono8 submits in turn with three frames in flight, the layout switched in front of every submit (Bayer window,
    packed mono8, Bayer, mono8): each ticket keeps the layout of its own submit."""
    fr, lay, feed, want = mono_runs["window", "grbg"]
    frames = [(m[0], m[1], lay, False) if f % 2 == 0 else (g[0], g[1], None, False) for f, (m, g) in enumerate(fr)]
    _same(_run(ctx, kind, frames, feed), want[kind])
    fr2, lay2, _, _ = mono_runs["even origin", "rggb"]     # two Bayer layouts in turn: the same scene seed, another origin and pattern
    other = mono_runs["even origin", "rggb"][3][kind]
    mixed = _run(ctx, kind, [(fr[0][0][0], fr[0][0][1], lay, False)] + [(m[0], m[1], lay2, False) for m, _ in fr2[1:]], feed)
    for f in range(2, FR):                                  # (frame 1's flow has frame 0 of the other layout in front of it)
        assert mixed.disparity[f].tobytes() == other.disparity[f].tobytes()
        assert mixed.flow[f].tobytes() == other.flow[f].tobytes()


def _pane_messages(width, pattern, seed):
    """side-by-side messages of pane width `width` (height H + 2, the window at (width - W, 1) of each pane), per frame:
    (the message, the two panes cut out as packed messages, the model's grey of both windows); the layouts of the two forms"""
    from moving_object_detector_amd import synth
    mh, pad = H + 2, 3
    left, right = _colour_scene(width, mh, FR, seed)
    rng = np.random.default_rng(seed + 1)
    blay = {"encoding": "bayer_%s8" % pattern, "width": width, "height": mh, "step": 2 * width + pad, "x0": width - W, "y0": 1}
    right_pattern = bm.shifted(pattern, dx=width)
    out = []
    for f in range(FR):
        both = rng.integers(0, 256, size=(mh, 2 * width + pad), dtype=np.uint8)
        both[:, :width] = synth.mosaic(left[f], pattern)
        both[:, width:2 * width] = synth.mosaic(right[f], right_pattern)       # the pattern runs on across the seam
        greys = [bm.to_mono(both, bm.Layout(**blay), W, H, 1, pane)[0] for pane in (0, 1)]
        out.append((both, greys))
    return out, blay


@pytest.mark.parametrize("width", [W + 4, W + 5], ids=["even panes", "odd panes"])
@pytest.mark.parametrize("pattern", ["rggb", "gbrg"])
def test_d_side_by_side(ctx, width, pattern):
    """one message that holds both eyes (for an odd pane width the right pane's pattern is shifted by a column) against the
    model's grey of its panes as two mono8 messages: mod_sgm_compute_host and the odometry stream"""
    sp, _, _ = _params()
    fr, blay = _pane_messages(width, pattern, 51)
    want = _run(ctx, "odometry", [(g[0], g[1], None, False) for _, g in fr])
    _same(_run(ctx, "odometry", [(both, None, blay, True) for both, _ in fr]), want)
    got_d, want_d = (np.full((H, W), -7, np.float32) for _ in range(2))
    both, g = fr[1]
    try:
        _state(ctx, None)
        assert ctx.disparity_host(g[0], g[1], sp, want_d)[0] == 0
        _state(ctx, blay, True)
        assert ctx.disparity_host(both, None, sp, got_d)[0] == 0
    finally:
        _state(ctx, None)
    assert got_d.tobytes() == want_d.tobytes() and (want_d >= 0).any()


@pytest.mark.parametrize("width", [W + 4, W + 5], ids=["even panes", "odd panes"])
def test_e_panes_do_not_leak(ctx, width):
    """mod_image_to_mono_dev on each pane of device messages (it has no eye: the right pane is src + width with the pattern as it
    lies there): the model's grey, unchanged when every byte of the OTHER pane and of the padding is random anew."""
    from moving_object_detector_amd import capi
    rng = np.random.default_rng(61 + width)
    fr, blay = _pane_messages(width, "grbg", 61)
    both = fr[0][0]
    L = bm.Layout(**blay)
    ctx.set_side_by_side(False)
    for pane in (0, 1):
        enc = "bayer_%s8" % bm.shifted("grbg", dx=pane * width)
        lay = capi.image_layout(enc, width, blay["height"], blay["step"], blay["x0"], blay["y0"])
        for on in (False, True):                                   # the state does not matter to this call, the step rule aside
            if on:
                ctx.set_image_layout(_layout(blay))
                ctx.set_side_by_side(True)
            other = rng.integers(0, 256, size=both.shape, dtype=np.uint8)
            other[:, pane * width:(pane + 1) * width] = both[:, pane * width:(pane + 1) * width]
            for msg in (both, other):
                dev = torch.from_numpy(np.concatenate([msg.ravel(), np.zeros(width, np.uint8)])).to(ctx.device)
                got = ctx.image_to_mono(dev[pane * width:pane * width + msg.size], lay).cpu().numpy()
                assert np.array_equal(got, bm.to_mono(both, L, W, H, 1, pane)), (pane, on)
            _state(ctx, None)


def test_f_mirror_takes_bayer_images(tmp_path):
    """SceneFlowConstructor::submitOdometry with bayer_rggb8 Images (padded rows, the window at an odd origin) against the same
    stream fed the model's grey as mono8 Images; the program compares for itself."""
    from moving_object_detector_amd import synth
    W, H, mw, mh, pad = 160, 128, 176, 140, 5          # the mirror's flow pyramid has four levels: the coarsest must be 16 pixels
    lay = {"encoding": "bayer_rggb8", "width": mw, "height": mh, "step": mw + pad, "x0": 7, "y0": 5}
    scene = _colour_scene(mw, mh, FR, 71)
    rng = np.random.default_rng(72)
    cam = synth.make_camera(W, H)
    for k in range(FR):
        for eye, name in enumerate(("left", "right")):
            m = rng.integers(0, 256, size=(mh, mw + pad), dtype=np.uint8)
            m[:, :mw] = synth.mosaic(scene[eye][k], "rggb")
            (tmp_path / f"{name}{k}.bin").write_bytes(m.tobytes())
            (tmp_path / f"grey_{name}{k}.bin").write_bytes(bm.to_mono(m, bm.Layout(**lay), W, H)[0].tobytes())
    (tmp_path / "setup.txt").write_text(" ".join(str(v) for v in (
        W, H, FR, lay["encoding"], lay["width"], lay["height"], lay["step"], lay["x0"], lay["y0"], repr(float(cam.fx)), repr(float(cam.cx)),
        repr(float(cam.Tx)), repr(float(cam.fy)), repr(float(cam.cy)), repr(float(cam.Ty)), "%.9g" % cam.disp_f, "%.9g" % cam.disp_T, "0", "15")) + "\n")
    exe = str(tmp_path / "bayer_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", os.path.join(HERE, "cpp", "bayer_mirror_test.cpp"), "-o", exe, "-L" + PKG,
                           "-lmod_sf", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    word, seen = r.stdout.split()
    assert word == "disparities" and int(seen) > 0, "no valid disparity in the sequence: the comparison would be weak"


@pytest.mark.parametrize("pattern", ["rggb", "gbrg"])
def test_g_the_smallest_estimator_camera(pattern):
    """A 9 x 7 camera (the smallest the disparity estimator's own tests pin) that is the whole message, and in the corners of a 12 x 9
    one, where the staged region's edges are the message's: mod_sgm_compute_host (the synchronous staging) and two
    mod_submit_stereo_host frames (the slot's stage) against the model's grey as mono8."""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.host_stream import HostStream
    from moving_object_detector_amd.pipeline import Context
    w, h = 9, 7
    c = Context(w, h, max_frames=1)
    cam = synth.make_camera(w, h)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(7.0)
    c.set_camera(cam)
    c.set_params(synth.Params())
    sp = capi.ModSgmParams(8, 6, 96, 8, 1, 1)
    rng = np.random.default_rng(81)
    flow = np.zeros((h, w, 2), np.float32)
    tf = capi.ModTransform((0, 0, 0), (0, 0, 0, 1))

    def run(imgs, lay):
        """[(left, right)] * 2 -> the synchronous disparity of pair 1 and the streamed disparity of pair 1"""
        _state(c, lay)
        sync = np.full((h, w), -7, np.float32)
        assert c.disparity_host(imgs[1][0], imgs[1][1], sp, sync)[0] == 0
        s = HostStream(c, 2, 0, outputs=("disparity",))
        s.forget_previous()
        for k, (l, r) in enumerate(imgs):
            s.submit_stereo(k, l, r, sp, flow, tf, DT)
        s.finish()
        assert s.first == [capi.MOD_SKIP_NO_DISPARITY_PREV, 0] and s.rc[1] == 0
        _state(c, None)
        return sync.tobytes(), s.disparity[1].tobytes()

    try:
        for (mw, mh, pad, x0, y0) in [(w, h, 0, 0, 0), (w, h, 3, 0, 0), (12, 9, 1, 0, 0), (12, 9, 0, 3, 2), (12, 9, 2, 3, 0), (12, 9, 0, 1, 1)]:
            lay = {"encoding": "bayer_%s8" % pattern, "width": mw, "height": mh, "step": mw + pad, "x0": x0, "y0": y0}
            msgs = [[rng.integers(0, 256, size=(mh, mw + pad), dtype=np.uint8) for _ in range(2)] for _ in range(2)]
            greys = [[bm.to_mono(m, bm.Layout(**lay), w, h)[0] for m in pair] for pair in msgs]
            want, got = run(greys, None), run(msgs, lay)
            assert got == want, (mw, mh, pad, x0, y0)
    finally:
        c.close()
