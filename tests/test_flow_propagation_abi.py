"""CPU: the neighbour-seed propagation of the optical flow is part of the C ABI: declared in include/mod_sf.h, let through by
csrc/exports.map, exported by the library, listed and typed by capi; the setter refuses what it cannot do without a device."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_flow_propagation", "mod_get_flow_propagation")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mod_sf.h")).read(), flags=re.S)


def test_header_declares_both_calls_and_keeps_the_flow_parameters():
    src = _header()
    for name in NAMES:
        assert re.search(r"^\s*int\s+%s\s*\(\s*(const\s+)?ModContext\s*\*" % name, src, flags=re.M), name
    assert re.search(r"#define\s+MOD_FLOW_SEEDS\s+5\b", src)
    m = re.search(r"typedef\s+struct\s+ModFlowParams\s*\{(.*?)\}\s*ModFlowParams\s*;", src, flags=re.S)
    assert re.findall(r"int32_t\s+(\w+)\s*;", m.group(1)) == ["levels", "radius", "window", "subpixel", "fb_check"]
    assert re.search(r"#define\s+MOD_ABI_VERSION\s+2\b", src)                   # additions only: the version stays


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
    assert capi.MOD_FLOW_SEEDS == 5
    assert C.sizeof(capi.ModFlowParams) == 20
    lib = capi.load()
    assert lib.mod_set_flow_propagation.argtypes == [C.c_void_p, C.c_int32]
    assert lib.mod_get_flow_propagation.argtypes == [C.c_void_p, C.POINTER(C.c_int32)]
    assert lib.mod_abi_version() == 2


def test_null_context_is_refused_without_a_device():
    from moving_object_detector_amd import capi
    lib = capi.load()
    seeds = C.c_int32(-1)
    assert lib.mod_set_flow_propagation(None, 5) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_flow_propagation(None, C.byref(seeds)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert seeds.value == -1


@pytest.mark.gpu
def test_round_trip_and_invalid_values():
    """(needs a context, hence a device) default 1; 5 and 1 round-trip; anything else is refused and leaves the setting as it was."""
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(64, 64, max_frames=1)
    seeds = C.c_int32(-1)
    assert ctx.lib.mod_get_flow_propagation(ctx.h, C.byref(seeds)) == 0 and seeds.value == 1
    assert ctx.get_flow_propagation() == 1
    ctx.set_flow_propagation(5)
    assert ctx.get_flow_propagation() == 5
    for bad in (0, 2, 3, 4, 6, 9, -1, -5):
        assert ctx.lib.mod_set_flow_propagation(ctx.h, bad) == capi.MOD_ERR_INVALID_ARGUMENT, bad
        assert b"seeds" in ctx.lib.mod_last_error(ctx.h)
        assert ctx.get_flow_propagation() == 5, bad
    with pytest.raises(capi.ModError):
        ctx.set_flow_propagation(3)
    assert ctx.lib.mod_get_flow_propagation(ctx.h, None) == capi.MOD_ERR_INVALID_ARGUMENT
    ctx.set_flow_propagation()
    assert ctx.get_flow_propagation() == 1
    ctx.close()
