"""GPU: mod_set_depth_distortion (k_depth_rays, k_depth_register_rays, k_depth_register_splat_rays of csrc/depth.hip) against
tests/models/depth_undistort_model.py, bit for bit.  Both ray tables of a 40 x 24 message under the 80 x 48 camera and of a 300 x 5
message (wider than one block of lanes, rows that end inside a wave), NaN entries by bit pattern, one guard word in front of and
behind each table.  The registered disparity on the rigs of tests/depth_undistort_cases.py: both encodings, three frames a call,
the splat off and on, a roll of 1 degree and a translation of 2 cm, the lens past its fold (invalid rays), D = 0, and a message wider
than one block.  The cache: another D, other depth intrinsics or another message size rebuild the tables and the results follow;
clearing the distortion gives depth_model.register's planes exactly.  The calls' refusals."""
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
import depth_model as dm  # noqa: E402
import depth_splat_cases as sc  # noqa: E402
import depth_splat_model as sm  # noqa: E402
import depth_undistort_cases as uc  # noqa: E402
import depth_undistort_model as dum  # noqa: E402
from test_gpu_depth import _context, _layout, _run  # noqa: E402

GUARD = 0x5A5A5A5A5A5A5A5A


def _registered(ctx, reg, D):
    from moving_object_detector_amd import capi
    ctx.set_depth_registration(capi.depth_registration(reg.fx, reg.fy, reg.cx, reg.cy, reg.R, reg.t))
    ctx.set_depth_distortion(capi.depth_distortion(D) if D is not None else None)


def _table(ctx, lay, lattice):
    """mod_depth_rays_host into the middle of a guarded buffer: the table's words, after the guards were found intact"""
    n = (lay.height + lattice) * (lay.width + lattice) * 2
    buf = np.full(n + 2, GUARD, np.uint64)
    rc = ctx.lib.mod_depth_rays_host(ctx.h, C.byref(lay), lattice, buf[1:].ctypes.data)
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    assert buf[0] == GUARD and buf[-1] == GUARD, "a store outside the table"
    return buf[1:-1].reshape(lay.height + lattice, lay.width + lattice, 2)


def _differs(got, want):
    return np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]


TABLES = {
    "rig": uc.CALIBRATIONS["rig"],
    "fold": uc.FOLD,
    "zero": uc.CALIBRATIONS["rig"][:6] + (uc.ZERO,),
    "kinect 300 x 5": (300, 5) + uc.CALIBRATIONS["kinect"][2:],
}


@pytest.mark.parametrize("name", list(TABLES))
def test_tables_match_the_model(name):
    from moving_object_detector_amd import capi
    width, height, fx, fy, cx, cy, D = TABLES[name]
    reg = dm.Registration(fx, fy, cx, cy)
    ctx = _context(sc.W, sc.H, 1, sc.DISP_F, sc.DISP_T, 0.0, sc.CAM)
    try:
        _registered(ctx, reg, D)
        lay = capi.depth_layout("16UC1", width, height)
        for lattice in (dum.CENTRES, dum.CORNERS):
            want = dum.rays(D, reg, width, height, lattice).view(np.uint64)
            got = _table(ctx, lay, lattice)
            assert got.tobytes() == want.tobytes(), (lattice, np.argwhere(got != want)[:4])
            if name == "fold":
                assert (got == 0x7FF8000000000000).any()
        ctx.set_depth_layout(lay)                                      # the Python method, with the layout as context state
        assert ctx.depth_rays().tobytes() == dum.rays(D, reg, width, height).tobytes()
        assert ctx.depth_rays(lattice=capi.MOD_DEPTH_RAYS_CORNERS).shape == (height + 1, width + 1, 2)
    finally:
        ctx.close()


@pytest.mark.parametrize("splat", [False, True], ids=["points", "splat"])
@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
@pytest.mark.parametrize("name", uc.RIGS)
def test_registered_disparity_matches_the_model(name, encoding, splat):
    msg, lay, reg, D, cam, W, H, frames = uc.rig(name, encoding)
    assert frames == 3 and lay.step > lay.width * dm.BYTES[lay.enc]
    want, n = dum.register(msg, lay, reg, D, cam, W, H, sc.fT(cam), cam.min_disparity, frames, splat)
    assert n["kept"] > 0 and (name != "fold" or (n["invalid_ray"] > 0 and (not splat or n["invalid_corner"] > 0))), n
    ctx = _context(W, H, frames, cam.disp_f, cam.disp_T, cam.min_disparity, cam)
    try:
        _registered(ctx, reg, D)
        ctx.set_depth_splat(splat)
        for dst_skew in (0, 1):
            got = _run(ctx, msg, lay, frames, W, H, 0, dst_skew)
            assert got.tobytes() == want.tobytes(), (n, _differs(got, want))
        one = _run(ctx, msg[2:], lay, 1, W, H)                 # a second call finds the z-buffer cleared and the tables cached
        assert one.tobytes() == want[2:].tobytes()
    finally:
        ctx.close()


def test_the_cache_follows_the_lens_the_intrinsics_and_the_size():
    from moving_object_detector_amd import capi
    msg, lay, reg, D, cam, W, H, frames = uc.rig("rig", "16UC1")
    fT = sc.fT(cam)
    ctx = _context(W, H, frames, cam.disp_f, cam.disp_T, 0.0, cam)

    def check(reg, D, msg, lay, splat):
        want, _ = dum.register(msg, lay, reg, D, cam, W, H, fT, 0.0, frames, splat)
        got = _run(ctx, msg, lay, frames, W, H)
        assert got.tobytes() == want.tobytes(), _differs(got, want)
        return want
    try:
        ctx.set_depth_splat(True)
        _registered(ctx, reg, D)
        first = check(reg, D, msg, lay, True)
        D2 = (-0.2, 0.05, 1e-3, 0.0, 0.0, 0.0, 0.0, 0.0)              # another D
        _registered(ctx, reg, D2)
        assert check(reg, D2, msg, lay, True).tobytes() != first.tobytes()
        reg2 = dm.Registration(reg.fx * 1.05, reg.fy, reg.cx + 0.5, reg.cy, reg.R, reg.t)   # other depth intrinsics
        _registered(ctx, reg2, D2)
        check(reg2, D2, msg, lay, True)
        small, slay = sc.message(sc.scene(33, 17, 21), "16UC1")       # another message size
        check(reg2, D2, small, slay, True)
        check(reg2, D2, msg, lay, True)                               # ... and back
        ctx.set_depth_splat(False)                                    # the point rule reads the centre table alone
        check(reg2, D2, msg, lay, False)
        got = ctx.get_depth_distortion()
        assert got is not None and list(got.D) == list(D2)
        # cleared: today's kernels, bit for bit
        ctx.set_depth_distortion(None)
        assert ctx.get_depth_distortion() is None
        want, _ = dm.register(msg, lay, reg2, cam, W, H, fT, 0.0, frames)
        assert _run(ctx, msg, lay, frames, W, H).tobytes() == want.tobytes()
        ctx.set_depth_splat(True)
        want, _ = sm.register_splat(msg, lay, reg2, cam, W, H, fT, 0.0, frames)
        assert _run(ctx, msg, lay, frames, W, H).tobytes() == want.tobytes()
    finally:
        ctx.close()


def test_refusals_leave_the_state_and_the_output_untouched():
    from moving_object_detector_amd import capi
    msg, lay, reg, D, cam, W, H, frames = uc.rig("rig", "16UC1")
    ctx = _context(W, H, frames, cam.disp_f, cam.disp_T, 0.0, cam)
    try:
        L, E = ctx.lib, capi.MOD_ERR_INVALID_ARGUMENT
        on, d = C.c_int32(-7), capi.ModDepthDistortion()
        assert L.mod_get_depth_distortion(ctx.h, C.byref(d), C.byref(on)) == 0 and on.value == 0      # the default
        assert L.mod_get_depth_distortion(ctx.h, C.byref(d), None) == E
        cl, rays = _layout(lay), np.zeros(2 * 41 * 25)
        assert L.mod_depth_rays_host(ctx.h, C.byref(cl), 0, rays.ctypes.data) == capi.MOD_ERR_NOT_CONFIGURED   # no distortion set
        ctx.set_depth_distortion(capi.depth_distortion(D))
        for bad in (float("nan"), float("inf"), -float("inf")):                  # a non-finite D: the state stays as it was
            for k in (0, 3, 7):
                b = capi.depth_distortion(D)
                b.D[k] = bad
                assert L.mod_set_depth_distortion(ctx.h, C.byref(b)) == E and b"distortion" in L.mod_last_error(ctx.h)
        assert list(ctx.get_depth_distortion().D) == list(D)
        # a distortion without a registration: the call and the table are refused, nothing is written
        dev = torch.full((frames * H * W,), 1500, dtype=torch.int16, device=ctx.device)       # camera-sized messages: the plain path would take them
        out = torch.full((frames, H, W), -77.0, dtype=torch.float32, device=ctx.device)
        plain = capi.depth_layout("16UC1", W, H)
        assert L.mod_depth_to_disparity_dev(ctx.h, frames, dev.data_ptr(), C.byref(plain), out.data_ptr()) == E
        assert b"registration" in L.mod_last_error(ctx.h)
        assert L.mod_depth_rays_host(ctx.h, C.byref(cl), 0, rays.ctypes.data) == E and b"registration" in L.mod_last_error(ctx.h)
        ctx.synchronize()
        assert (out.cpu().numpy() == -77.0).all() and (rays == 0.0).all()
        _registered(ctx, reg, D)
        assert L.mod_depth_rays_host(ctx.h, C.byref(cl), 2, rays.ctypes.data) == E                     # an unknown lattice
        assert L.mod_depth_rays_host(ctx.h, C.byref(cl), 0, None) == E
        assert (rays == 0.0).all()
        want, _ = dum.register(msg, lay, reg, D, cam, W, H, sc.fT(cam), 0.0, frames)
        assert _run(ctx, msg, lay, frames, W, H).tobytes() == want.tobytes()
    finally:
        ctx.close()
