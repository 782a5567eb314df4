"""CPU: mod_set_depth_filter, mod_get_depth_filter and mod_depth_filter_dev are part of the C ABI: declared in include/mod_sf.h, let
through by csrc/exports.map, exported by the library, listed and typed by capi; ModDepthFilter is 32 bytes in C and in ctypes; the ABI
version stays 2; the calls refuse a NULL context without a device (the setter's refusals of values need a context, which needs a
device: tests/test_gpu_depth_filter.py); the host mirror's setDepthFilter forwards."""
import ctypes as C
import fnmatch
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_depth_filter", "mod_get_depth_filter", "mod_depth_filter_dev")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mod_sf.h")).read(), flags=re.S)


def test_header_declares_the_calls_and_the_struct():
    src = _header()
    assert re.search(r"^\s*int\s+mod_set_depth_filter\s*\(\s*ModContext\s*\*\s*ctx\s*,\s*const\s+ModDepthFilter\s*\*\s*filter\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_get_depth_filter\s*\(\s*const\s+ModContext\s*\*\s*ctx\s*,\s*ModDepthFilter\s*\*\s*filter\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_depth_filter_dev\s*\(\s*ModContext\s*\*\s*ctx\s*,\s*int32_t\s+frames\s*,\s*const\s+void\s*\*\s*depth_in\s*,\s*"
                     r"const\s+ModDepthLayout\s*\*\s*layout\s*,\s*const\s+ModDepthFilter\s*\*\s*filter\s*,\s*void\s*\*\s*depth_out\s*\)\s*;", src, flags=re.M)
    assert re.search(r"typedef\s+struct\s+ModDepthFilter\s*\{\s*float\s+z_min\s*,\s*z_max\s*;\s*int32_t\s+window\s*;\s*int32_t\s+min_support\s*;\s*"
                     r"float\s+tol_abs\s*,\s*tol_rel\s*;\s*int32_t\s+reserved\[2\]\s*;\s*\}\s*ModDepthFilter\s*;", src)
    assert re.search(r"#define\s+MOD_ABI_VERSION\s+2\b", src)                   # additions only: the version stays


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    for phrase in ("t = tol_abs + tol_rel * z_p", "fabsf(z_q - z_p) <= t", "n >= min_support", "does not cascade", "0x7fc00000",
                   "Pixels outside the message never support", "The neighbourhood is the message's, not the window's"):
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
        assert name in capi.EXPORTS and name in capi.SIGNATURES
    lib = capi.load()
    P = C.POINTER
    assert lib.mod_set_depth_filter.argtypes == [C.c_void_p, P(capi.ModDepthFilter)]
    assert lib.mod_get_depth_filter.argtypes == [C.c_void_p, P(capi.ModDepthFilter)]
    assert lib.mod_depth_filter_dev.argtypes == [C.c_void_p, C.c_int32, C.c_void_p, P(capi.ModDepthLayout), P(capi.ModDepthFilter), C.c_void_p]
    assert all(getattr(lib, n).restype == C.c_int for n in NAMES)
    assert lib.mod_abi_version() == 2


def test_the_struct_is_32_bytes_in_c_and_in_ctypes(tmp_path):
    from moving_object_detector_amd import capi
    assert C.sizeof(capi.ModDepthFilter) == 32
    offsets = [getattr(capi.ModDepthFilter, n).offset for n in ("z_min", "z_max", "window", "min_support", "tol_abs", "tol_rel", "reserved")]
    assert offsets == [0, 4, 8, 12, 16, 20, 24]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mod_sf.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(ModDepthFilter), offsetof(ModDepthFilter, window), offsetof(ModDepthFilter, tol_abs), '
                   'offsetof(ModDepthFilter, reserved)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["32", "8", "16", "24"]


def test_the_helper_and_its_defaults():
    from moving_object_detector_amd import capi
    f = capi.depth_filter()
    assert (f.z_min, f.z_max, f.window, f.min_support, f.tol_abs, list(f.reserved)) == (0.0, 0.0, 0, 3, 0.0, [0, 0])
    assert abs(f.tol_rel - 0.02) < 1e-8
    assert "not tuned" in capi.depth_filter.__doc__.lower()
    g = capi.depth_filter(0.3, 6.0, 5, 7, 0.01, 0.03)
    assert (g.window, g.min_support) == (5, 7) and g.z_max == 6.0


def test_null_context_is_refused_without_a_device():
    from moving_object_detector_amd import capi
    lib = capi.load()
    f = capi.depth_filter(1.0, 2.0, 3, 3)
    before = bytes(f)
    assert lib.mod_set_depth_filter(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_depth_filter(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT and bytes(f) == before
    lay = capi.depth_layout("16UC1", 8, 4)
    assert lib.mod_depth_filter_dev(None, 1, None, C.byref(lay), C.byref(f), None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_the_python_layer_has_the_methods():
    from moving_object_detector_amd.pipeline import Context
    assert callable(Context.set_depth_filter) and callable(Context.get_depth_filter) and callable(Context.depth_filter)


def test_the_host_mirror_forwards(tmp_path):
    """a C++ program against host/ with a recording stub in the library's place: setDepthFilter(&f) hands f on, setDepthFilter(nullptr) NULL"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "depth_filter_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "depth_filter_mirror_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    out = [line for line in out if line.startswith(("mod_set_depth_filter", "refused"))]
    call = "mod_set_depth_filter 0.5 6 5 7 0.01 0.03 0 0"
    assert out == [call, "mod_set_depth_filter NULL", call, "refused: threw"], out
