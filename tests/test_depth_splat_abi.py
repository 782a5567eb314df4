"""CPU: mod_set_depth_splat and mod_get_depth_splat are part of the C ABI: declared in include/mod_sf.h, let through by
csrc/exports.map, exported by the library, listed and typed by capi; MOD_DEPTH_SPLAT_MAX is the same number in the header and in capi;
the calls refuse a NULL context without a device."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_depth_splat", "mod_get_depth_splat")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mod_sf.h")).read(), flags=re.S)


def test_header_declares_the_calls_and_the_cap():
    src = _header()
    assert re.search(r"^\s*int\s+mod_set_depth_splat\s*\(\s*ModContext\s*\*\s*ctx\s*,\s*int32_t\s+on\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_get_depth_splat\s*\(\s*const\s+ModContext\s*\*\s*ctx\s*,\s*int32_t\s*\*\s*on\s*\)\s*;", src, flags=re.M)
    assert re.search(r"#define\s+MOD_DEPTH_SPLAT_MAX\s+8\b", src)
    assert re.search(r"#define\s+MOD_ABI_VERSION\s+2\b", src)                   # additions only: the version stays


def test_the_header_states_the_rule():
    """the footprint paragraph is an addition: the registered-path block keeps its sentences"""
    text = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    assert "Holes are left as holes (no splatting, no fill: depth_image_proc/register's" in text
    for phrase in ("mod_set_depth_splat", "ulo = ceil(min(min(p0, p1), min(p2, p3)))", "MOD_DEPTH_SPLAT_MAX", "BEFORE clipping"):
        assert phrase in text, phrase


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
    cap = int(re.search(r"#define\s+MOD_DEPTH_SPLAT_MAX\s+(\d+)", _header()).group(1))
    assert capi.MOD_DEPTH_SPLAT_MAX == cap == 8
    lib = capi.load()
    assert lib.mod_set_depth_splat.argtypes == [C.c_void_p, C.c_int32]
    assert lib.mod_get_depth_splat.argtypes == [C.c_void_p, C.POINTER(C.c_int32)]
    assert lib.mod_set_depth_splat.restype == C.c_int and lib.mod_get_depth_splat.restype == C.c_int
    assert lib.mod_abi_version() == 2


def test_null_context_is_refused_without_a_device():
    from moving_object_detector_amd import capi
    lib = capi.load()
    on = C.c_int32(-7)
    assert lib.mod_set_depth_splat(None, 1) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_depth_splat(None, C.byref(on)) == capi.MOD_ERR_INVALID_ARGUMENT and on.value == -7


def test_the_python_layer_and_the_host_mirror_have_the_switch():
    from moving_object_detector_amd.pipeline import Context
    assert callable(Context.set_depth_splat) and callable(Context.get_depth_splat)
    hpp = open(os.path.join(ROOT, "moving_object_detector_amd", "host", "scene_flow_constructor.hpp")).read()
    assert re.search(r"void\s+setDepthSplat\s*\(\s*bool\s+on\s*\)\s*\{\s*check\(mod_set_depth_splat\(ctx_,", hpp)
