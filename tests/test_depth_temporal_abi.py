"""CPU: mod_set_depth_temporal, mod_get_depth_temporal, mod_reset_depth_temporal and mod_depth_temporal_dev are part of the C ABI:
declared in include/mod_sf.h with the rule stated, let through by csrc/exports.map, exported by the library, listed and typed by capi;
ModDepthTemporal is 32 bytes in C and in ctypes; the ABI version stays 2; csrc/depth_temporal.hip is one of the Makefile's sources; the
calls refuse a NULL context without a device (the setter's refusals of values need a context, which needs a device:
tests/test_gpu_depth_temporal.py); the host mirror's setDepthTemporal forwards."""
import ctypes as C
import fnmatch
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_depth_temporal", "mod_get_depth_temporal", "mod_reset_depth_temporal", "mod_depth_temporal_dev")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mod_sf.h")).read(), flags=re.S)


def test_header_declares_the_calls_and_the_struct():
    src = _header()
    assert re.search(r"^\s*int\s+mod_set_depth_temporal\s*\(\s*ModContext\s*\*\s*ctx\s*,\s*const\s+ModDepthTemporal\s*\*\s*filter\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_get_depth_temporal\s*\(\s*const\s+ModContext\s*\*\s*ctx\s*,\s*ModDepthTemporal\s*\*\s*filter\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_reset_depth_temporal\s*\(\s*ModContext\s*\*\s*ctx\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_depth_temporal_dev\s*\(\s*ModContext\s*\*\s*ctx\s*,\s*int32_t\s+frames\s*,\s*const\s+void\s*\*\s*depth_in\s*,\s*"
                     r"const\s+ModDepthLayout\s*\*\s*layout\s*,\s*const\s+ModDepthTemporal\s*\*\s*filter\s*,\s*float\s*\*\s*state_s\s*,\s*"
                     r"uint8_t\s*\*\s*state_age\s*,\s*void\s*\*\s*depth_out\s*\)\s*;", src, flags=re.M)
    assert re.search(r"typedef\s+struct\s+ModDepthTemporal\s*\{\s*float\s+alpha\s*,\s*delta_abs\s*,\s*delta_rel\s*;\s*int32_t\s+hold\s*;\s*"
                     r"int32_t\s+reserved\[4\]\s*;\s*\}\s*ModDepthTemporal\s*;", src)
    assert re.search(r"#define\s+MOD_ABI_VERSION\s+2\b", src)                   # additions only: the version stays


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    for phrase in ("t = delta_abs + delta_rel * zs", "fabsf(z - zs) <= t", "s = s + alpha * (x - s)", "age < hold", "255 = empty",
                   "(uint16)min(max(rintf(s), 1.0f), 65535.0f)", "ties to even", "alpha == 1 with hold == 0 is the identity",
                   "Only hold > 0 ever fills a hole", "mod_forget_previous", "parity with no SDK is claimed"):
        assert phrase in text, phrase
    for lost in ("Not done: a temporal filter",):
        assert lost not in text
    for gained in ("motion-compensated state", "with k_depth_filter in one kernel", "node parameters"):
        assert gained in text, gained


def test_the_makefile_builds_the_kernels_source():
    mk = open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=((?:.*\\\n)*.*)$", mk, flags=re.M).group(1)
    assert "depth_temporal.hip" in srcs.split() or "depth_temporal.hip" in srcs.replace("\\", " ").split()
    src = open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "depth_temporal.hip")).read()
    assert "k_depth_temporal" in src and "__global__" in src


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
    assert lib.mod_set_depth_temporal.argtypes == [C.c_void_p, P(capi.ModDepthTemporal)]
    assert lib.mod_get_depth_temporal.argtypes == [C.c_void_p, P(capi.ModDepthTemporal)]
    assert lib.mod_reset_depth_temporal.argtypes == [C.c_void_p]
    assert lib.mod_depth_temporal_dev.argtypes == [C.c_void_p, C.c_int32, C.c_void_p, P(capi.ModDepthLayout), P(capi.ModDepthTemporal),
                                                   C.c_void_p, C.c_void_p, C.c_void_p]
    assert all(getattr(lib, n).restype == C.c_int for n in NAMES)
    assert lib.mod_abi_version() == 2


def test_the_struct_is_32_bytes_in_c_and_in_ctypes(tmp_path):
    from moving_object_detector_amd import capi
    assert C.sizeof(capi.ModDepthTemporal) == 32
    offsets = [getattr(capi.ModDepthTemporal, n).offset for n in ("alpha", "delta_abs", "delta_rel", "hold", "reserved")]
    assert offsets == [0, 4, 8, 12, 16]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mod_sf.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(ModDepthTemporal), offsetof(ModDepthTemporal, delta_rel), '
                   'offsetof(ModDepthTemporal, hold), offsetof(ModDepthTemporal, reserved)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["32", "8", "12", "16"]


def test_the_helper_and_its_defaults():
    from moving_object_detector_amd import capi
    f = capi.depth_temporal()
    assert (f.hold, f.delta_rel, list(f.reserved)) == (0, 0.0, [0, 0, 0, 0])
    assert abs(f.alpha - 0.4) < 1e-7 and abs(f.delta_abs - 0.02) < 1e-8
    assert "not tuned" in capi.depth_temporal.__doc__.lower()
    g = capi.depth_temporal(0.25, 0.5, 0.125, 3)
    assert (g.alpha, g.delta_abs, g.delta_rel, g.hold) == (0.25, 0.5, 0.125, 3)


def test_null_context_is_refused_without_a_device():
    from moving_object_detector_amd import capi
    lib = capi.load()
    f = capi.depth_temporal(0.5, 0.1, 0.0, 2)
    before = bytes(f)
    assert lib.mod_set_depth_temporal(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_depth_temporal(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT and bytes(f) == before
    assert lib.mod_reset_depth_temporal(None) == capi.MOD_ERR_INVALID_ARGUMENT
    lay = capi.depth_layout("16UC1", 8, 4)
    assert lib.mod_depth_temporal_dev(None, 1, None, C.byref(lay), C.byref(f), None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_the_python_layer_has_the_methods():
    from moving_object_detector_amd.pipeline import Context
    for name in ("set_depth_temporal", "get_depth_temporal", "reset_depth_temporal", "depth_temporal"):
        assert callable(getattr(Context, name))


def test_the_host_mirror_forwards(tmp_path):
    """a C++ program against host/ with a recording stub in the library's place: setDepthTemporal(&f) hands f on, setDepthTemporal(nullptr) NULL"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "depth_temporal_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "depth_temporal_mirror_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    out = [line for line in out if line.startswith(("mod_set_depth_temporal", "refused"))]
    call = "mod_set_depth_temporal 0.25 0.5 0.125 3 0 0 0 0"
    assert out == [call, "mod_set_depth_temporal NULL", call, "refused: threw"], out
