"""CPU: tests/models/depth_model.py, the numpy restatement of csrc/depth.hip that the GPU tests compare with bit for bit, against an
independent scalar Python loop; an identity registration equals the plain path; two samples on one target keep the nearer; the
values REP 118 and IEEE leave without a depth map to min_disparity - 1; the shared registered case produces every case of the scatter."""
import math
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_cases as dc  # noqa: E402
import depth_model as dm  # noqa: E402

f32 = np.float32


def _sample(msg, lay, f, U, V):
    """z of message pixel (U, V) of frame f, read byte by byte"""
    raw = np.ascontiguousarray(msg).view(np.uint8).reshape(-1)
    B = dm.BYTES[lay.enc]
    at = f * lay.step * lay.height + V * lay.step + U * B
    unit = f32(lay.unit) if lay.unit != 0.0 else f32(0.001) if lay.enc == 0 else f32(1.0)
    with np.errstate(all="ignore"):
        if lay.enc == 0:
            return f32(int(raw[at]) | int(raw[at + 1]) << 8) * unit
        return f32(struct.unpack("<f", bytes(raw[at:at + 4]))[0]) * unit


def _is_valid(z):
    return bool(z > 0) and math.isfinite(float(z))


def _scalar_plain(msg, lay, W, H, fT, dmin, frames):
    out = np.empty((frames, H, W), f32)
    for f in range(frames):
        for v in range(H):
            for u in range(W):
                z = _sample(msg, lay, f, u + lay.x0, v + lay.y0)
                with np.errstate(all="ignore"):
                    out[f, v, u] = f32(fT) / z if _is_valid(z) else f32(dmin) - f32(1.0)
    return out


def _scalar_register(msg, lay, reg, cam, W, H, fT, dmin, frames):
    """Python floats are IEEE doubles and Python evaluates one operation at a time"""
    best = {}
    R, t = [float(v) for v in reg.R], [float(v) for v in reg.t]
    for f in range(frames):
        for V in range(lay.height):
            for U in range(lay.width):
                z = _sample(msg, lay, f, U, V)
                if not _is_valid(z):
                    continue
                Z0 = float(z)
                X0 = ((U - reg.cx) * Z0) / reg.fx
                Y0 = ((V - reg.cy) * Z0) / reg.fy
                X = ((R[0] * X0 + R[1] * Y0) + R[2] * Z0) + t[0]
                Y = ((R[3] * X0 + R[4] * Y0) + R[5] * Z0) + t[1]
                Z = ((R[6] * X0 + R[7] * Y0) + R[8] * Z0) + t[2]
                if not (Z > 0 and math.isfinite(Z)):
                    continue
                a = ((cam.fx * X + cam.Tx) / Z + cam.cx) + 0.5
                b = ((cam.fy * Y + cam.Ty) / Z + cam.cy) + 0.5
                if not (0 <= a < W and 0 <= b < H):
                    continue
                key = (f, math.floor(b), math.floor(a))
                zf = f32(Z)
                if key not in best or zf < best[key]:
                    best[key] = zf
    out = np.full((frames, H, W), f32(dmin) - f32(1.0), f32)
    with np.errstate(all="ignore"):
        for key, zf in best.items():
            out[key] = f32(fT) / zf
    return out


def _same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("camera", list(dc.CAMERAS))
@pytest.mark.parametrize("encoding,unit", [("16UC1", 0.0), ("16UC1", 0.00025), ("32FC1", 0.0), ("32FC1", 0.5)])
def test_plain_model_matches_a_scalar_loop(encoding, unit, camera):
    f, T, dmin = dc.CAMERAS[camera]
    fT = dm.f_times_T(f, T)
    msg, lay = dc.plain_case(encoding, unit)
    got = dm.to_disparity(msg, lay, dc.W, dc.H, fT, dmin, dc.FRAMES)
    assert _same(got, _scalar_plain(msg, lay, dc.W, dc.H, fT, dmin, dc.FRAMES))
    bad = got == f32(dmin) - f32(1.0)
    assert bad.any() and (~bad).any()
    if camera == "tiny fT" and encoding == "32FC1":
        assert (got[~bad] == 0.0).any(), "no disparity underflows to 0"
        tiny = np.abs(got[~bad & (got != 0.0)])
        assert (tiny < np.finfo(f32).tiny).any(), "no denormal disparity"


def test_invalid_values_map_to_min_disparity_minus_one():
    for dmin in (0.0, 2.5, -3.0):
        want = f32(dmin) - f32(1.0)
        lay = dm.Layout("32FC1", 8, 1, 32)
        vals = np.array([math.nan, math.inf, -math.inf, -0.0, 0.0, -2.0, -1e-40, 1.0], "<f4")
        d = dm.to_disparity(vals.view(np.uint8), lay, 8, 1, f32(8.0), dmin)[0, 0]
        assert (d[:7] == want).all() and d[7] == f32(8.0)
        lay = dm.Layout("16UC1", 4, 1, 8)
        d = dm.to_disparity(np.array([0, 1, 65535, 1000], "<u2").view(np.uint8), lay, 4, 1, f32(8.0), dmin)[0, 0]
        assert d[0] == want and d[1] == f32(8.0) / (f32(1.0) * f32(0.001)) and d[2] == f32(8.0) / (f32(65535.0) * f32(0.001)) and d[3] == f32(8.0) / f32(1.0)
    # a denormal depth is a reading: positive and finite
    lay = dm.Layout("32FC1", 1, 1, 4)
    with np.errstate(all="ignore"):
        assert dm.to_disparity(np.array([1e-40], "<f4").view(np.uint8), lay, 1, 1, f32(8.0), 0.0)[0, 0, 0] == f32(8.0) / f32(1e-40)


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_registered_model_matches_a_scalar_loop_and_the_case_covers_the_scatter(encoding):
    cam = dc.REG_CAM
    fT = dm.f_times_T(cam.disp_f, cam.disp_T)
    msg, lay = dc.registered_case(encoding)
    got, n = dm.register(msg, lay, dc.REGISTRATION, cam, dc.RW, dc.RH, fT, cam.min_disparity, 2)
    assert n["double_hits"] >= 1 and n["outside"] >= 1 and n["behind"] >= 1 and n["empty"] >= 1 and n["kept"] >= 100, n
    assert _same(got, _scalar_register(msg, lay, dc.REGISTRATION, cam, dc.RW, dc.RH, fT, cam.min_disparity, 2))


@pytest.mark.parametrize("encoding,unit", [("16UC1", 0.0), ("32FC1", 0.0), ("32FC1", 0.5)])
def test_identity_registration_equals_the_plain_path(encoding, unit):
    """depth intrinsics = the camera's, R = I, t = 0, Tx = Ty = 0, the message the camera's size: every valid sample lands on its own
    pixel (floor(u + 0.5 + an error far below 0.5)) with its own z ((float)(double)z)"""
    from types import SimpleNamespace
    f, T, dmin = dc.CAMERAS["ordinary"]
    fT = dm.f_times_T(f, T)
    msg, lay = dc.plain_case(encoding, unit)
    whole = dm.Layout(encoding, lay.width, lay.height, lay.step, 0, 0, unit)
    cam = SimpleNamespace(fx=70.0, fy=71.0, cx=39.5, cy=5.25, Tx=0.0, Ty=0.0)
    reg = dm.Registration(cam.fx, cam.fy, cam.cx, cam.cy)
    got, n = dm.register(msg, whole, reg, cam, lay.width, lay.height, fT, dmin, dc.FRAMES)
    assert n["outside"] == 0 and n["behind"] == 0 and n["double_hits"] == 0
    assert _same(got, dm.to_disparity(msg, whole, lay.width, lay.height, fT, dmin, dc.FRAMES))


def test_two_samples_on_one_target_keep_the_nearer():
    """a 2 x 1 depth camera of twice the focal length: both samples land on pixel (1, 0) of a 3 x 1 image camera"""
    from types import SimpleNamespace
    cam = SimpleNamespace(fx=1.0, fy=1.0, cx=1.0, cy=0.0, Tx=0.0, Ty=0.0)
    reg = dm.Registration(4.0, 4.0, 0.5, 0.0)
    lay = dm.Layout("32FC1", 2, 1, 8)
    for near, far in ((1.25, 3.0), (3.0, 1.25)):
        d, n = dm.register(np.array([near, far], "<f4").view(np.uint8), lay, reg, cam, 3, 1, f32(8.0), 0.0)
        assert n["double_hits"] == 1 and n["empty"] == 2
        assert list(d[0, 0]) == [f32(-1.0), f32(8.0) / f32(1.25), f32(-1.0)]
