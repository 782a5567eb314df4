"""GPU: the two routes of a host image to the estimators agree with each other.  The same two messages go to mod_sgm_compute_host (the
synchronous route: the context's staging, the context's stream) and to mod_submit_stereo_host with `disparity` asked for (the stream
route: a slot's stage, the copy stream, fences), and the two disparity planes are equal bit for bit: mono8 packed, bgr8 and one
yuv422 encoding in a larger message with padded rows and a window off the origin, one Bayer pattern with an odd origin; each with the
rectification off and with the distorted fixture calibration of tests/test_gpu_rectify.py on; mono8 and Bayer also side by side.  On
the smallest camera the estimators accept (9 x 7, tests/test_gpu_bayer_streams.py), one context per case, every ticket collected.
A 9 x 7 camera is the size of the census window and its disparity plane takes one or two values whatever the images are, so every
case runs on a 48 x 32 camera too.  There the scene is two bands 4 and 7 pixels of disparity away (under the fixture calibration,
whose new focal length is 0.8 of the old and whose principal points are 1.8 pixels apart, about 2 and 4): a plane that saw the
images is valid over most of the camera and holds both bands' disparities and the values between them, so at least half of its
pixels must be valid and at least three valid values distinct, rectified or not, before the planes are compared."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import rectify_model as rm  # noqa: E402

DT = 1.0 / 15.0
CAMERAS = ((9, 7), (48, 32))
# name: encoding, bytes per pixel, what the message is wider and higher than the camera (one eye's), row padding in bytes, window origin
CONFIGS = {"mono8": ("mono8", 1, 0, 0, 0, 0, 0), "bgr8": ("bgr8", 3, 5, 3, 5, 3, 2), "yuv422_yuy2": ("yuv422_yuy2", 2, 5, 3, 2, 4, 1),
           "bayer_grbg8": ("bayer_grbg8", 1, 4, 3, 3, 3, 1)}
CASES = [(cam, name, rect, sbs) for cam in CAMERAS for name in CONFIGS for rect in (False, True)
         for sbs in ((False, True) if CONFIGS[name][1] == 1 else (False,))]


def _pair(rng, mw, mh, bpp, pad, sbs):
    """Two messages [mh][step] (side by side: ONE, and None) of a texture of 2 x 2 blocks, the right one 4 pixels of disparity away in
    the upper half and 7 in the lower; the bytes of a pixel a few levels apart, the padding random."""
    base = np.kron(rng.integers(0, 250, size=((mh + 1) // 2, (mw + 8) // 2)), np.ones((2, 2), np.int64))[:mh, :mw + 7]
    eyes = []
    for shifts in ((0, 0), (4, 7)):
        px = np.concatenate([base[:mh // 2, shifts[0]:shifts[0] + mw], base[mh // 2:, shifts[1]:shifts[1] + mw]])
        px = np.clip(px[:, :, None] + rng.integers(-3, 4, size=(mh, mw, bpp)), 0, 255).astype(np.uint8)
        eyes.append(px.reshape(mh, mw * bpp))
    rows = [np.concatenate(eyes, axis=1)] if sbs else eyes
    msgs = [np.ascontiguousarray(np.concatenate([r, rng.integers(0, 256, size=(mh, pad), dtype=np.uint8)], axis=1)) for r in rows]
    return (msgs[0], None) if sbs else (msgs[0], msgs[1])


@pytest.mark.parametrize("cam,name,rect,sbs", CASES,
                         ids=["%dx%d-%s%s%s" % (*cm, n, "-rectified" if r else "", "-side_by_side" if s else "") for cm, n, r, s in CASES])
def test_the_synchronous_and_the_stream_route_give_the_same_disparity(cam, name, rect, sbs):
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.host_stream import HostStream
    from moving_object_detector_amd.pipeline import Context
    (W, H), (enc, bpp, dw, dh, pad, x0, y0) = cam, CONFIGS[name]
    mw, mh = W + dw, H + dh
    c = Context(W, H, max_frames=1)
    try:
        camera = synth.make_camera(W, H)
        camera.min_disparity, camera.max_disparity = np.float32(0.0), np.float32(7.0)
        c.set_camera(camera)
        c.set_params(synth.Params())
        step = (2 if sbs else 1) * mw * bpp + pad
        c.set_image_layout(capi.image_layout(enc, mw, mh, step, x0, y0))
        c.set_side_by_side(sbs)
        if rect:
            c.set_rectification(*[capi.rectify_camera(*rm.distorted(mw, mh, eye)) for eye in (0, 1)])
        rng = np.random.default_rng(17)
        pairs = [_pair(rng, mw, mh, bpp, pad, sbs) for _ in range(2)]
        sp = capi.ModSgmParams(8, 6, 96, 8, 1, 1)
        sync = np.full((H, W), -7, np.float32)
        left, right = pairs[1]
        assert c.disparity_host(left, right, sp, sync)[0] == 0
        flow = np.zeros((H, W, 2), np.float32)
        tf = capi.ModTransform((0, 0, 0), (0, 0, 0, 1))
        # the stream needs a first frame (it has no previous disparity: it takes a plane and no ticket); the estimator carries nothing
        # from one frame to the next, so the second frame's plane is the second pair's alone, as the synchronous call's is
        s = HostStream(c, 2, 0, outputs=("disparity",))
        for k, (l, r) in enumerate(pairs):
            s.submit_stereo(k, l, r, sp, flow, tf, DT)
        s.finish()
        assert s.first == [capi.MOD_SKIP_NO_DISPARITY_PREV, 0] and s.rc[1] == 0
        streamed = s.disparity[1]
        assert not (sync == -7).any() and not (streamed == -7).any()
        if (W, H) != CAMERAS[0]:      # the plane saw the images (see the module's docstring)
            valid = sync[sync >= 0]
            assert 2 * valid.size >= W * H and np.unique(valid).size >= 3, (valid.size, np.unique(valid))
        assert sync.tobytes() == streamed.tobytes()
    finally:
        c.close()
