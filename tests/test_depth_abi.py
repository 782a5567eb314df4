"""CPU: the RGB-D entry points are part of the C ABI: declared in include/mod_sf.h, let through by csrc/exports.map, exported by the
library, listed and typed by capi; the calls refuse a NULL context without a device.  GPU (they need a context): the settings'
defaults and round trips, and every argument error that needs no GPU work."""
import ctypes as C
import fnmatch
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_depth_layout", "mod_get_depth_layout", "mod_set_depth_registration", "mod_get_depth_registration",
         "mod_depth_to_disparity_dev", "mod_submit_depth_host")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mod_sf.h")).read(), flags=re.S)


def test_header_declares_the_calls_and_the_structs():
    src = _header()
    for name in NAMES:
        assert re.search(r"^\s*int\s+%s\s*\(\s*(const\s+)?ModContext\s*\*" % name, src, flags=re.M), name
    lay = re.search(r"typedef\s+struct\s+ModDepthLayout\s*\{(.*?)\}\s*ModDepthLayout\s*;", src, flags=re.S)
    assert re.sub(r"\s+", " ", lay.group(1)).strip() == "int32_t encoding, width, height, step, x0, y0; float unit;"
    reg = re.search(r"typedef\s+struct\s+ModDepthRegistration\s*\{(.*?)\}\s*ModDepthRegistration\s*;", src, flags=re.S)
    assert re.sub(r"\s+", " ", reg.group(1)).strip() == "double fx, fy, cx, cy; double R[9], t[3];"
    assert re.search(r"#define\s+MOD_DEPTH_16UC1\s+0\b", src) and re.search(r"#define\s+MOD_DEPTH_32FC1\s+1\b", src)
    assert re.search(r"#define\s+MOD_ABI_VERSION\s+2\b", src)                   # additions only: the version stays
    sub = re.search(r"int\s+mod_submit_depth_host\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", a).strip() for a in sub.split(",")] == [
        "ModContext *ctx", "const uint8_t *image", "const void *depth", "const ModFlowParams *flow_prm", "const ModEgoParams *ego_prm",
        "const ModTransform *transform", "double dt", "void *cloud_aos", "int32_t *labels", "ModObject *objects", "int32_t max_objects",
        "float *disparity", "float *flow_out", "ModTransform *transform_out", "ModEgoResult *ego_out", "int32_t *ticket"]


def test_exports_map_lets_them_through_and_the_library_has_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "exports.map")).read(), flags=re.S)
    globs = re.findall(r"([\w*?]+)\s*;", text.split("global:")[1].split("local:")[0])
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), (name, globs)
    from moving_object_detector_amd import capi
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= defined, set(NAMES) - defined


def test_capi_lists_and_types_them():
    from moving_object_detector_amd import capi
    for name in NAMES:
        assert name in capi.EXPORTS
    assert C.sizeof(capi.ModDepthLayout) == 28 and C.sizeof(capi.ModDepthRegistration) == 128
    assert (capi.ModDepthLayout.unit.offset, capi.ModDepthRegistration.R.offset, capi.ModDepthRegistration.t.offset) == (24, 32, 104)
    assert (capi.MOD_DEPTH_16UC1, capi.MOD_DEPTH_32FC1) == (0, 1)
    lib = capi.load()
    lay, reg, i32, vp = C.POINTER(capi.ModDepthLayout), C.POINTER(capi.ModDepthRegistration), C.c_int32, C.c_void_p
    assert lib.mod_set_depth_layout.argtypes == [vp, lay] and lib.mod_get_depth_layout.argtypes == [vp, lay]
    assert lib.mod_set_depth_registration.argtypes == [vp, reg]
    assert lib.mod_get_depth_registration.argtypes == [vp, reg, C.POINTER(i32)]
    assert lib.mod_depth_to_disparity_dev.argtypes == [vp, i32, vp, lay, vp]
    assert len(lib.mod_submit_depth_host.argtypes) == 16
    assert lib.mod_abi_version() == 2
    l = capi.depth_layout("32FC1", 80, 12, x0=5, y0=1, unit=0.5)
    assert (l.encoding, l.width, l.height, l.step, l.x0, l.y0, l.unit) == (1, 80, 12, 320, 5, 1, 0.5)
    assert capi.depth_layout("16UC1", 80, 12).step == 160 and capi.depth_layout(0, 80, 12, 166).step == 166
    r = capi.depth_registration(60, 61, 19.5, 11.25, [[1, 0, 0], [0, 1, 0], [0, 0, 1]], (0.05, 0, 0))
    assert list(r.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(r.t) == [0.05, 0, 0] and (r.fx, r.fy, r.cx, r.cy) == (60, 61, 19.5, 11.25)
    with pytest.raises(ValueError):
        capi.depth_registration(1, 1, 0, 0, [1] * 8)


def test_null_context_is_refused_without_a_device():
    from moving_object_detector_amd import capi
    lib = capi.load()
    lay, reg, on, t = capi.depth_layout("16UC1", 8, 8), capi.depth_registration(1, 1, 0, 0), C.c_int32(-7), C.c_int32(-7)
    buf = (C.c_int32 * 128)()
    fp = capi.flow_params()
    tf = capi.ModTransform((0, 0, 0), (0, 0, 0, 1))
    assert lib.mod_set_depth_layout(None, C.byref(lay)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_depth_layout(None, C.byref(lay)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_set_depth_registration(None, C.byref(reg)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_depth_registration(None, C.byref(reg), C.byref(on)) == capi.MOD_ERR_INVALID_ARGUMENT and on.value == -7
    assert lib.mod_depth_to_disparity_dev(None, 1, buf, C.byref(lay), buf) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_submit_depth_host(None, buf, buf, C.byref(fp), None, C.byref(tf), 0.1, None, None, None, 0, None, None, None, None,
                                     C.byref(t)) == capi.MOD_ERR_INVALID_ARGUMENT and t.value == -7


def _copy(s):
    out = type(s)()
    C.memmove(C.byref(out), C.byref(s), C.sizeof(s))
    return out


@pytest.mark.gpu
def test_settings_round_trip_and_argument_errors():
    """(needs a context, hence a device; no kernel runs) the defaults; round trips; every value include/mod_sf.h refuses is refused and
    leaves the state as it was; the submit's own refusals leave the stream's state as it was"""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    W, H = 64, 48
    ctx = Context(W, H, max_frames=2)
    L, E = ctx.lib, capi.MOD_ERR_INVALID_ARGUMENT
    lay, on = capi.ModDepthLayout(), C.c_int32(-1)
    # no camera yet
    assert L.mod_set_depth_layout(ctx.h, None) == capi.MOD_ERR_NOT_CONFIGURED
    assert L.mod_get_depth_layout(ctx.h, C.byref(lay)) == capi.MOD_ERR_NOT_CONFIGURED
    assert L.mod_depth_to_disparity_dev(ctx.h, 1, None, None, None) == capi.MOD_ERR_NOT_CONFIGURED
    ctx.set_camera(synth.make_camera(W, H))
    # defaults
    d = ctx.get_depth_layout()
    assert (d.encoding, d.width, d.height, d.step, d.x0, d.y0, d.unit) == (0, W, H, 2 * W, 0, 0, 0.0)
    assert ctx.get_depth_registration() is None
    assert L.mod_get_depth_registration(ctx.h, None, None) == E
    good = capi.depth_layout("32FC1", 80, 60, 80 * 4 + 8, 5, 7, 0.5)
    ctx.set_depth_layout(good)
    assert bytes(ctx.get_depth_layout()) == bytes(good)

    def bad_layouts():
        for enc in (-1, 2, 16):
            b = _copy(good); b.encoding = enc
            yield f"encoding {enc}", b
        for step in (80 * 4 - 4, 80 * 4 + 2, 0, -4):
            b = _copy(good); b.step = step
            yield f"step {step}", b
        b = capi.depth_layout("16UC1", 80, 60, 161)
        yield "odd step", b
        for unit in (math.nan, math.inf, -math.inf, -0.001):
            b = _copy(good); b.unit = unit
            yield f"unit {unit}", b
        for x0, y0 in ((-1, 0), (0, -1), (17, 0), (0, 13)):
            b = _copy(good); b.x0, b.y0 = x0, y0
            yield f"window at {x0}, {y0}", b
        for w, h in ((0, 60), (80, 0), (W - 1, 60), (80, H - 1), (capi.MOD_MAX_WIDTH + 1, 60)):
            b = _copy(good); b.width, b.height, b.step, b.x0, b.y0 = w, h, max(4, 4 * w), 0, 0
            yield f"size {w} x {h}", b

    dev = (C.c_int32 * 4)()     # stands for device pointers: every call below is refused before it is used
    n = 0
    for what, b in bad_layouts():
        assert L.mod_set_depth_layout(ctx.h, C.byref(b)) == E, what
        assert b"depth" in L.mod_last_error(ctx.h), what
        assert bytes(ctx.get_depth_layout()) == bytes(good), what
        assert L.mod_depth_to_disparity_dev(ctx.h, 1, dev, C.byref(b), dev) == E, what
        n += 1
    assert n == 21
    # frames and pointers of the _dev call
    assert L.mod_depth_to_disparity_dev(ctx.h, 0, dev, None, dev) == E
    assert L.mod_depth_to_disparity_dev(ctx.h, 3, dev, None, dev) == capi.MOD_ERR_CAPACITY
    assert L.mod_depth_to_disparity_dev(ctx.h, 1, None, None, dev) == capi.MOD_SKIP_NO_DISPARITY_NOW
    assert L.mod_depth_to_disparity_dev(ctx.h, 1, dev, None, None) == E
    assert L.mod_depth_to_disparity_dev(ctx.h, 1, C.c_void_p(C.addressof(dev) + 2), None, dev) == E       # 32FC1 at an address that is 2 mod 4
    assert L.mod_depth_to_disparity_dev(ctx.h, 1, dev, None, C.c_void_p(C.addressof(dev) + 2)) == E
    assert L.mod_depth_to_disparity_dev(ctx.h, 1, C.c_void_p(C.addressof(dev) + 1), C.byref(capi.depth_layout("16UC1", W, H)), dev) == E
    # registration
    reg = capi.depth_registration(60, 61, 19.5, 11.25, [1, 0, 0, 0, 1, 0, 0, 0, 1], (0.05, 0, 0))

    def bad_registrations():
        for field in ("fx", "fy", "cx", "cy"):
            for v in (math.nan, math.inf):
                b = _copy(reg); setattr(b, field, v)
                yield f"{field} = {v}", b
        for field, k in (("R", 0), ("R", 8), ("t", 0), ("t", 2)):
            for v in (math.nan, -math.inf):
                b = _copy(reg); getattr(b, field)[k] = v
                yield f"{field}[{k}] = {v}", b
        for field in ("fx", "fy"):
            for v in (0.0, -60.0):
                b = _copy(reg); setattr(b, field, v)
                yield f"{field} = {v}", b
        b = _copy(reg); b.R[0] += 3e-6
        yield "R scaled", b
        b = _copy(reg); b.R[1] += 2e-6
        yield "R sheared", b

    n = 0
    for what, b in bad_registrations():
        assert L.mod_set_depth_registration(ctx.h, C.byref(b)) == E, what
        assert b"depth registration" in L.mod_last_error(ctx.h), what
        assert ctx.get_depth_registration() is None, what
        n += 1
    assert n == 22
    ok = _copy(reg); ok.R[0] += 2e-7                                       # inside the 1e-6: accepted
    ctx.set_depth_registration(ok)
    assert bytes(ctx.get_depth_registration()) == bytes(ok)
    for what, b in bad_registrations():
        assert L.mod_set_depth_registration(ctx.h, C.byref(b)) == E and bytes(ctx.get_depth_registration()) == bytes(ok), what
    # a registration together with a window origin: at call time (the layout in force was set before the registration) and at set time
    assert L.mod_depth_to_disparity_dev(ctx.h, 1, dev, None, dev) == E and b"x0 and y0" in L.mod_last_error(ctx.h)
    assert L.mod_set_depth_layout(ctx.h, C.byref(good)) == E
    small = capi.depth_layout("16UC1", 40, 24)                              # ... but a message smaller than the camera is fine now
    ctx.set_depth_layout(small)
    ctx.set_depth_registration(None)
    assert ctx.get_depth_registration() is None
    assert L.mod_depth_to_disparity_dev(ctx.h, 1, dev, None, dev) == E and b"does not fit" in L.mod_last_error(ctx.h)   # at call time again
    assert L.mod_set_depth_layout(ctx.h, C.byref(small)) == E
    ctx.set_depth_layout(None)
    # the submit's own refusals
    ctx.set_params(synth.Params())
    fp, ep, tf, t = capi.flow_params(levels=2), capi.ego_params(), capi.ModTransform((0, 0, 0), (0, 0, 0, 1)), C.c_int32(-7)
    img, dep = (C.c_uint8 * (W * H))(), (C.c_uint16 * (W * H))()
    sub = lambda f=fp, e=ep, x=tf: L.mod_submit_depth_host(ctx.h, img, dep, C.byref(f) if f else None, C.byref(e) if e else None,
                                                           C.byref(x) if x else None, 0.1, None, None, None, 0, None, None, None, None, C.byref(t))
    assert sub(f=None) == E and sub(e=None, x=None) == E
    assert sub(f=capi.flow_params(window=4)) == E and sub(e=capi.ego_params(stride=0), x=None) == E
    assert L.mod_submit_depth_host(ctx.h, img, dep, C.byref(fp), None, C.byref(tf), 0.1, None, None, None, 0, None, None, None, None, None) == E
    ctx.set_image_layout(capi.image_layout("mono8", W, H, 2 * W))
    ctx.set_side_by_side(True)
    assert sub() == E and b"side by side" in L.mod_last_error(ctx.h) and t.value == -1
    ctx.set_side_by_side(False)
    ctx.set_image_layout(None)
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    rc = capi.rectify_camera(W, H, [50, 0, 32, 0, 50, 24, 0, 0, 1], [0.0] * 5, ident, [50, 0, 32, 0, 0, 50, 24, 0, 0, 0, 1, 0])
    ctx.set_rectification(rc, rc)
    assert sub() == E and b"registration" in L.mod_last_error(ctx.h)
    ctx.set_rectification()
    ctx.close()
