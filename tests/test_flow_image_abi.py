"""CPU: the ABI of the flow and disparity images (mod_static_flow_dev, mod_flow_image_dev, mod_flow_residual_image_dev,
mod_disparity_image_dev, mod_flow_color) — exports, what the header promises, the host-only legend against the model, and the
status table (the rows that need a context need a device: the one gpu-marked test here)."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mod_sf.h")
CSRC = os.path.join(ROOT, "moving_object_detector_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests", "models"))
import flow_image_model as M  # noqa: E402

NAMES = ("mod_static_flow_dev", "mod_flow_image_dev", "mod_flow_residual_image_dev", "mod_disparity_image_dev", "mod_flow_color")
f32 = np.float32


def test_header_declares_the_calls_and_the_version_stays():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, flags=re.M), name
    assert "#define MOD_ABI_VERSION 2" in src
    from moving_object_detector_amd import capi
    assert capi.load().mod_abi_version() == 2


def test_symbols_pass_the_export_map_and_are_bound():
    from moving_object_detector_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    assert re.search(r"global:\s*mod_\*;", text) and re.search(r"local:\s*\*;", text)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert name in names and name in capi.EXPORTS, name
    lib = capi.load()
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [5, 5, 6, 4, 4]


def test_header_states_the_rule():
    src = " ".join(re.sub(r"\n \*(?!/)", "\n", open(HEADER).read()).split())
    doc = src[src.index("Flow and disparity images"):src.index("int mod_static_flow_dev")]
    for phrase in ("m = sqrtf(fx * fx + fy * fy)", "m == 0 -> (255, 255, 255)", "s = min(255, (int)(255 * (m / max_px)))",
                   "A = |fx| + |fy|, t = fy / A", "fx < 0: q = 2 - t", "fx >= 0 and fy < 0: q = 4 + t", "idx = min(255, (int)(q * 64))",
                   "out_c = 255 - ((255 - P[idx][c]) * s + 127) / 255", "no atan2, no fused multiply-add", "mod_cluster_palette",
                   "(d - min_disparity) / (max_disparity - min_disparity)", "d == 0 -> (0, 0, 0)", "frames outside 1 .. 65535",
                   "MOD_SKIP_NO_FLOW", "MOD_SKIP_NO_DISPARITY_PREV", "MOD_SKIP_NO_DISPARITY_NOW", "MOD_ERR_NOT_CONFIGURED"):
        assert phrase in doc, phrase


def test_null_context_is_refused_without_a_device():
    from moving_object_detector_amd import capi
    lib, E = capi.load(), capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_static_flow_dev(None, 1, None, None, None) == E
    assert lib.mod_flow_image_dev(None, 1, None, 8.0, None) == E
    assert lib.mod_flow_residual_image_dev(None, 1, None, None, 8.0, None) == E
    assert lib.mod_disparity_image_dev(None, 1, None, None) == E


def _vectors(max_px):
    """(fx, fy) of the legend's test: the eight axis and diagonal directions at three lengths, zero, |v| at max_px, one float below
    and above it on the x axis and well above it, NaN and inf components."""
    r = f32(max_px)
    lo, hi = np.nextafter(r, f32(0)), np.nextafter(r, f32(np.inf))
    v = []
    for scale in (0.25 * max_px, 1.0, 3.0 * max_px):
        for dx, dy in ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)):
            v.append((dx * scale, dy * scale))
    v += [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
    v += [(r, 0.0), (lo, 0.0), (hi, 0.0), (0.0, -r), (0.0, lo), (-hi, 0.0), (0.6 * max_px, 0.8 * max_px), (1e6, -1e6), (3e38, 3e38)]
    nan, inf = float("nan"), float("inf")
    v += [(nan, 1.0), (1.0, nan), (nan, nan), (inf, 1.0), (1.0, -inf), (-inf, inf), (inf, nan)]
    v += [(1e-30, 0.0), (1e-40, 1e-41), (-1e-20, 2e-20)]
    return [(float(f32(a)), float(f32(b))) for a, b in v]


@pytest.mark.parametrize("max_px", [8.0, 1.0, 0.3, 1000.0])
def test_flow_color_equals_the_model(max_px):
    from moving_object_detector_amd import capi
    lib = capi.load()
    out = (C.c_uint8 * 3)()
    for fx, fy in _vectors(max_px):
        assert lib.mod_flow_color(fx, fy, max_px, out) == capi.MOD_OK
        assert tuple(out) == M.flow_color(fx, fy, max_px), (fx, fy, max_px)
        assert capi.flow_color(fx, fy, max_px) == tuple(out)


def test_flow_color_landmarks():
    """What the rule says in plain words, independent of the model: white at rest, black when invalid, the pure table entries of
    the four axes at max_px (idx 0, 64, 128, 192), and half strength half way."""
    from moving_object_detector_amd import capi
    lut = capi.cluster_palette()
    assert capi.flow_color(0.0, 0.0, 8.0) == (255, 255, 255)
    assert capi.flow_color(float("nan"), 0.0, 8.0) == (0, 0, 0) and capi.flow_color(0.0, float("-inf"), 8.0) == (0, 0, 0)
    for (fx, fy), idx in (((8, 0), 0), ((0, 8), 64), ((-8, 0), 128), ((0, -8), 192), ((80, 0), 0), ((0, -1e6), 192)):
        assert capi.flow_color(fx, fy, 8.0) == tuple(lut[idx]), (fx, fy)
    assert capi.flow_color(1.0, 1.0, 8.0) == tuple(M.blend(lut[32], 45))        # |v| = sqrt 2: (int)(255 * 0.17677669) = 45
    b, g, r = capi.flow_color(4.0, 0.0, 8.0)                                    # entry 0 is (0, 0, 255) B, G, R; s = 127
    assert (b, g, r) == (128, 128, 255)


@pytest.mark.parametrize("max_px", [0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_flow_color_refuses_a_useless_max_px(max_px):
    from moving_object_detector_amd import capi
    out = (C.c_uint8 * 3)(7, 7, 7)
    assert capi.load().mod_flow_color(1.0, 1.0, max_px, out) == capi.MOD_ERR_INVALID_ARGUMENT
    assert tuple(out) == (7, 7, 7)
    with pytest.raises(ValueError):
        capi.flow_color(1.0, 1.0, max_px)


def test_flow_color_refuses_a_null_output():
    from moving_object_detector_amd import capi
    assert capi.load().mod_flow_color(1.0, 1.0, 8.0, None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_the_kernels_and_the_legend_read_one_header():
    kernel = open(os.path.join(CSRC, "flow_image.hip")).read()
    host = open(os.path.join(CSRC, "mod_sf.hip")).read()
    assert '#include "flow_color.h"' in kernel and '#include "flow_color.h"' in host
    assert "flow_color::flow_bgr(" in kernel and "flow_color::flow_bgr(" in host and "flow_color::disparity_bgr(" in kernel
    hdr = open(os.path.join(CSRC, "flow_color.h")).read()
    assert '#include "label_palette.h"' in hdr and "#pragma clang fp contract(off)" in hdr
    assert not re.search(r"\b(atan2f?|fmaf?|__fdividef|__fsqrt_rn|rsqrtf?)\s*\(", hdr + kernel)
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()


@pytest.mark.gpu
def test_status_table():
    """(needs contexts, hence a device) every row of the header's table, through ctypes; nothing is written by a refused call."""
    torch = pytest.importorskip("torch")
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    W, H = 8, 4
    ctx = Context(W, H, max_frames=1)
    lib, E, NC = ctx.lib, capi.MOD_ERR_INVALID_ARGUMENT, capi.MOD_ERR_NOT_CONFIGURED
    flow = torch.zeros((2, H, W, 2), dtype=torch.float32, device=ctx.device)
    disp = torch.ones((2, H, W), dtype=torch.float32, device=ctx.device)
    tf = torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]] * 2, dtype=torch.float64, device=ctx.device)
    img = torch.full((2 * H * W * 3 + 16,), 0xA5, dtype=torch.uint8, device=ctx.device)
    sf = torch.full((2 * H * W * 2 + 4,), -7.0, dtype=torch.float32, device=ctx.device)
    F, D, T, I, S = flow.data_ptr(), disp.data_ptr(), tf.data_ptr(), img.data_ptr(), sf.data_ptr()
    # no camera yet
    assert lib.mod_flow_image_dev(ctx.h, 1, F, 8.0, I) == NC
    assert lib.mod_flow_residual_image_dev(ctx.h, 1, F, F, 8.0, I) == NC
    assert lib.mod_disparity_image_dev(ctx.h, 1, D, I) == NC
    assert lib.mod_static_flow_dev(ctx.h, 1, D, T, S) == NC
    # ... but the argument rows come first
    assert lib.mod_flow_image_dev(ctx.h, 0, F, 8.0, I) == E and lib.mod_flow_image_dev(ctx.h, 1, F, 8.0, None) == E
    cam = synth.make_camera(W, H)
    ctx.set_camera(cam)
    # the camera alone is enough (no parameters set), and frames is not held to max_frames = 1
    assert lib.mod_flow_image_dev(ctx.h, 2, F, 8.0, I) == 0
    assert lib.mod_flow_residual_image_dev(ctx.h, 2, F, F, 8.0, I) == 0
    assert lib.mod_disparity_image_dev(ctx.h, 2, D, I) == 0
    assert lib.mod_static_flow_dev(ctx.h, 2, D, T, S) == 0
    ctx.synchronize()
    assert (img.cpu().numpy()[-16:] == 0xA5).all() and (sf.cpu().numpy()[-4:] == -7.0).all()
    img.fill_(0xA5); sf.fill_(-7.0)
    for frames in (0, -1, 65536, 2**31 - 1):
        assert lib.mod_flow_image_dev(ctx.h, frames, F, 8.0, I) == E, frames
        assert lib.mod_flow_residual_image_dev(ctx.h, frames, F, F, 8.0, I) == E
        assert lib.mod_disparity_image_dev(ctx.h, frames, D, I) == E
        assert lib.mod_static_flow_dev(ctx.h, frames, D, T, S) == E
    assert b"frames" in lib.mod_last_error(ctx.h)
    assert lib.mod_flow_image_dev(ctx.h, 1, F, 8.0, None) == E
    assert lib.mod_flow_residual_image_dev(ctx.h, 1, F, F, 8.0, None) == E
    assert lib.mod_disparity_image_dev(ctx.h, 1, D, None) == E
    assert lib.mod_static_flow_dev(ctx.h, 1, D, T, None) == E
    assert lib.mod_flow_image_dev(ctx.h, 1, F, 8.0, I + 2) == E and lib.mod_static_flow_dev(ctx.h, 1, D, T, S + 4) == E   # alignment
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert lib.mod_flow_image_dev(ctx.h, 1, F, bad, I) == E, bad
        assert lib.mod_flow_residual_image_dev(ctx.h, 1, F, F, bad, I) == E, bad
    assert lib.mod_flow_image_dev(ctx.h, 1, None, 8.0, I) == capi.MOD_SKIP_NO_FLOW
    assert lib.mod_flow_residual_image_dev(ctx.h, 1, None, F, 8.0, I) == capi.MOD_SKIP_NO_FLOW
    assert lib.mod_flow_residual_image_dev(ctx.h, 1, F, None, 8.0, I) == capi.MOD_SKIP_NO_FLOW
    assert lib.mod_disparity_image_dev(ctx.h, 1, None, I) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert lib.mod_static_flow_dev(ctx.h, 1, None, T, S) == capi.MOD_SKIP_NO_DISPARITY_PREV
    assert lib.mod_static_flow_dev(ctx.h, 1, D, None, S) == capi.MOD_SKIP_NO_TRANSFORM
    # a camera whose disparity range is empty cannot colour a disparity
    cam.max_disparity = cam.min_disparity
    ctx.set_camera(cam)
    assert lib.mod_disparity_image_dev(ctx.h, 1, D, I) == NC
    assert lib.mod_flow_image_dev(ctx.h, 1, None, 8.0, I) == capi.MOD_SKIP_NO_FLOW
    ctx.synchronize()
    assert (img.cpu().numpy() == 0xA5).all() and (sf.cpu().numpy() == -7.0).all()
    ctx.close()
