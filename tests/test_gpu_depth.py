"""GPU: csrc/depth.hip against tests/models/depth_model.py, bit for bit.  The plain path (k_depth_to_disparity) on the shared cases
of tests/depth_cases.py: a 67 x 9 window at an odd origin of 80 x 12 messages with padded rows, 3 frames, both encodings, the default
and an explicit unit, every value without a depth, a denormal depth, disparities that are denormal or underflow to 0, a min_disparity
other than 0; the same window through every load path of the kernel (the message at device addresses 0, 2, 4 and 8 bytes past a
16-byte boundary, the output 0 and 4 bytes past a 32-byte one) and on a camera narrower than a run.  The registered path
(k_depth_register + k_zbuffer_to_disparity) on the shared registration, after the model has shown that the case holds a target hit
twice, samples outside the window and behind the camera, and empty targets.  The calls' argument errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_cases as dc  # noqa: E402
import depth_model as dm  # noqa: E402


def _context(W, H, frames, disp_f, disp_T, dmin, cam=None):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=frames)
    c = synth.make_camera(W, H)
    if cam is not None:
        c.fx, c.fy, c.cx, c.cy, c.Tx, c.Ty = cam.fx, cam.fy, cam.cx, cam.cy, cam.Tx, cam.Ty
    c.disp_f, c.disp_T, c.min_disparity, c.max_disparity = np.float32(disp_f), np.float32(disp_T), np.float32(dmin), np.float32(dmin + 64)
    ctx.set_camera(c)
    return ctx


def _layout(lay):
    from moving_object_detector_amd import capi
    return capi.depth_layout(lay.enc, lay.width, lay.height, lay.step, lay.x0, lay.y0, lay.unit)


def _run(ctx, msg, lay, frames, W, H, src_skew=0, dst_skew=0, use_context_layout=False):
    """the message bytes at a device address src_skew bytes past a 256-byte boundary, the planes dst_skew floats past one"""
    raw = torch.zeros(msg.size + 64, dtype=torch.uint8, device=ctx.device)
    raw[src_skew:src_skew + msg.size] = torch.from_numpy(np.ascontiguousarray(msg).reshape(-1)).to(ctx.device)
    out = torch.full((frames * H * W + 16,), -77.0, dtype=torch.float32, device=ctx.device)
    view = out[dst_skew:dst_skew + frames * H * W].view(frames, H, W)
    got = ctx.depth_to_disparity(raw[src_skew:src_skew + msg.size], None if use_context_layout else _layout(lay), out=view)
    ctx.synchronize()
    full = out.cpu().numpy()
    assert (full[:dst_skew] == -77.0).all() and (full[dst_skew + frames * H * W:] == -77.0).all(), "a store outside the planes"
    return got.cpu().numpy()


@pytest.mark.parametrize("camera", list(dc.CAMERAS))
@pytest.mark.parametrize("encoding,unit", [("16UC1", 0.0), ("16UC1", 0.00025), ("32FC1", 0.0), ("32FC1", 0.5)])
def test_plain_path_matches_the_model(encoding, unit, camera):
    f, T, dmin = dc.CAMERAS[camera]
    msg, lay = dc.plain_case(encoding, unit)
    want = dm.to_disparity(msg, lay, dc.W, dc.H, dm.f_times_T(f, T), dmin, dc.FRAMES)
    ctx = _context(dc.W, dc.H, dc.FRAMES, f, T, dmin)
    try:
        B = dm.BYTES[lay.enc]
        for src_skew in (0, B, 2 * B, 8):               # 16UC1: half-way into a dword (alignbyte / scalar), dwords, 16-byte words
            for dst_skew in (0, 1, 5):
                got = _run(ctx, msg, lay, dc.FRAMES, dc.W, dc.H, src_skew, dst_skew)
                assert got.tobytes() == want.tobytes(), (src_skew, dst_skew, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4])
        ctx.set_depth_layout(_layout(lay))              # ... and with the layout as context state
        assert _run(ctx, msg, lay, dc.FRAMES, dc.W, dc.H, use_context_layout=True).tobytes() == want.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
@pytest.mark.parametrize("W,H,x0", [(3, 2, 0), (5, 3, 2), (8, 2, 1), (16, 2, 0), (300, 5, 3)])
def test_plain_path_small_and_multi_block_cameras(encoding, W, H, x0):
    """cameras narrower than a run, exactly one and two runs wide, and more than one block of lanes; one frame and two"""
    enc = dm.ENCODINGS[encoding]
    B = dm.BYTES[enc]
    rng = np.random.default_rng(W * 31 + H)
    mw, mh = W + x0 + 1, H + 1
    lay = dm.Layout(encoding, mw, mh, mw * B + B, x0, 1, 0.0)
    img = rng.integers(0, 3000, size=(2, mh, mw)).astype("<u2") if enc == 0 else (rng.uniform(-0.2, 5.0, size=(2, mh, mw))).astype("<f4")
    msg = rng.integers(0, 256, size=(2, mh, lay.step), dtype=np.uint8)
    msg[:, :, :mw * B] = img.view(np.uint8).reshape(2, mh, mw * B)
    ctx = _context(W, H, 2, 70.0, 0.12, 0.0)
    try:
        for frames in (1, 2):
            want = dm.to_disparity(msg[:frames], lay, W, H, dm.f_times_T(70.0, 0.12), 0.0, frames)
            for dst_skew in (0, 3):
                assert _run(ctx, msg[:frames], lay, frames, W, H, 0, dst_skew).tobytes() == want.tobytes(), (frames, dst_skew)
    finally:
        ctx.close()


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_registered_path_matches_the_model(encoding):
    from moving_object_detector_amd import capi
    cam, reg = dc.REG_CAM, dc.REGISTRATION
    fT = dm.f_times_T(cam.disp_f, cam.disp_T)
    msg, lay = dc.registered_case(encoding)
    want, n = dm.register(msg, lay, reg, cam, dc.RW, dc.RH, fT, cam.min_disparity, 2)
    assert n["double_hits"] >= 1 and n["outside"] >= 1 and n["behind"] >= 1 and n["empty"] >= 1, n     # the model itself says so
    ctx = _context(dc.RW, dc.RH, 2, cam.disp_f, cam.disp_T, cam.min_disparity, cam)
    try:
        ctx.set_depth_registration(capi.depth_registration(reg.fx, reg.fy, reg.cx, reg.cy, reg.R, reg.t))
        for dst_skew in (0, 1):                          # the finishing kernel's 16-byte and scalar stores
            got = _run(ctx, msg, lay, 2, dc.RW, dc.RH, 0, dst_skew)
            assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
        one = _run(ctx, msg[1:], lay, 1, dc.RW, dc.RH)   # a second call finds the z-buffer cleared
        assert one.tobytes() == want[1:].tobytes()
        ctx.set_depth_registration(None)                 # off again: the plain path refuses the small message ...
        with pytest.raises(capi.ModError):
            _run(ctx, msg, lay, 2, dc.RW, dc.RH)
    finally:
        ctx.close()


def test_argument_errors_leave_the_output_untouched():
    from moving_object_detector_amd import capi
    ctx = _context(dc.W, dc.H, 1, 70.0, 0.12, 0.0)
    try:
        msg, lay = dc.plain_case("16UC1", 0.0)
        dev = torch.from_numpy(msg.reshape(-1)).to(ctx.device)
        out = torch.full((1, dc.H, dc.W), -77.0, dtype=torch.float32, device=ctx.device)
        L, E = ctx.lib, capi.MOD_ERR_INVALID_ARGUMENT
        cl = _layout(lay)
        assert L.mod_depth_to_disparity_dev(ctx.h, 2, dev.data_ptr(), C.byref(cl), out.data_ptr()) == capi.MOD_ERR_CAPACITY
        assert L.mod_depth_to_disparity_dev(ctx.h, 1, dev.data_ptr() + 1, C.byref(cl), out.data_ptr()) == E
        assert L.mod_depth_to_disparity_dev(ctx.h, 1, None, C.byref(cl), out.data_ptr()) == capi.MOD_SKIP_NO_DISPARITY_NOW
        for field, v in (("encoding", 7), ("step", lay.step - 8), ("step", lay.step + 1), ("x0", 14), ("y0", 4), ("unit", float("nan")), ("unit", -1.0)):
            b = _layout(lay)
            setattr(b, field, v)
            assert L.mod_depth_to_disparity_dev(ctx.h, 1, dev.data_ptr(), C.byref(b), out.data_ptr()) == E, (field, v)
        ctx.set_depth_registration(capi.depth_registration(60, 60, 20, 12))
        assert L.mod_depth_to_disparity_dev(ctx.h, 1, dev.data_ptr(), C.byref(cl), out.data_ptr()) == E        # x0, y0 != 0 with a registration
        ctx.synchronize()
        assert (out.cpu().numpy() == -77.0).all()
    finally:
        ctx.close()
