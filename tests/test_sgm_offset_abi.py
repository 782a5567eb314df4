"""The ABI of the disparity offset: mod_set_disparity_offset / mod_get_disparity_offset are declared, exported and bound (CPU), refuse
values outside 0..128 without changing the state and start at 0 (GPU: the state lives in a context, and a context needs a device)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_disparity_offset", "mod_get_disparity_offset")


def test_header_declares_the_two_calls_and_keeps_the_limits():
    src = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    assert re.search(r"^int\s+mod_set_disparity_offset\(ModContext \*ctx, int32_t min_disparity\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_get_disparity_offset\(const ModContext \*ctx, int32_t \*min_disparity\);", src, flags=re.M)
    assert re.search(r"^#define MOD_ABI_VERSION 2\b", src, flags=re.M)
    assert re.search(r"^#define MOD_SGM_MAX_DISPARITIES 128\b", src, flags=re.M)


def test_library_exports_and_python_binds_them():
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    i32p = C.POINTER(C.c_int32)
    assert capi.SIGNATURES["mod_set_disparity_offset"] == [C.c_void_p, C.c_int32]
    assert capi.SIGNATURES["mod_get_disparity_offset"] == [C.c_void_p, i32p]
    lib = capi.load()
    for name in NAMES:
        assert name in exported and name in capi.EXPORTS and hasattr(lib, name), name
    assert lib.mod_abi_version() == 2
    assert C.sizeof(capi.ModSgmParams) == 24                         # the offset is context state: the parameter block keeps its layout
    assert callable(Context.set_disparity_offset) and callable(Context.get_disparity_offset)
    # no context: an error code, not a crash
    d0 = C.c_int32(-5)
    assert lib.mod_set_disparity_offset(None, 5) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_disparity_offset(None, C.byref(d0)) == capi.MOD_ERR_INVALID_ARGUMENT and d0.value == -5


@pytest.mark.gpu
def test_values_outside_the_range_are_refused_and_change_nothing():
    pytest.importorskip("torch")
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(64, 48, max_frames=1)
    ctx.set_camera(synth.make_camera(64, 48))
    d0 = C.c_int32(-5)
    assert ctx.lib.mod_get_disparity_offset(ctx.h, C.byref(d0)) == 0 and d0.value == 0             # a fresh context
    assert ctx.get_disparity_offset() == 0
    for keep in (0, 77, 128):
        assert ctx.lib.mod_set_disparity_offset(ctx.h, keep) == 0
        for bad in (-1, 129, 255, -128, 1 << 20):
            assert ctx.lib.mod_set_disparity_offset(ctx.h, bad) == capi.MOD_ERR_INVALID_ARGUMENT, bad
            assert b"0..128" in ctx.lib.mod_last_error(ctx.h)
            assert ctx.lib.mod_get_disparity_offset(ctx.h, C.byref(d0)) == 0 and d0.value == keep   # a refused value changes nothing
    with pytest.raises(capi.ModError):
        ctx.set_disparity_offset(129)
    assert ctx.get_disparity_offset() == 128
    ctx.set_disparity_offset()                                       # the default: off
    assert ctx.get_disparity_offset() == 0
    assert ctx.lib.mod_get_disparity_offset(ctx.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
    ctx.close()
