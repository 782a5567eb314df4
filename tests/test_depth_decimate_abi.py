"""CPU: mod_set_depth_decimation, mod_get_depth_decimation and mod_depth_decimate_dev are part of the C ABI: declared in include/mod_sf.h
with the rule stated, let through by csrc/exports.map, exported by the library, listed and typed by capi; ModDepthDecimation is 32
bytes in C and in ctypes with the header's offsets; the ABI version stays 2; csrc/depth_decimate.hip is one of the Makefile's sources;
the calls refuse a NULL context without a device (the setter's refusals of values need a context, which needs a device:
tests/test_gpu_depth_decimate.py); the host mirror's setDepthDecimation forwards."""
import ctypes as C
import fnmatch
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_depth_decimation", "mod_get_depth_decimation", "mod_depth_decimate_dev")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mod_sf.h")).read(), flags=re.S)


def test_header_declares_the_calls_and_the_struct():
    src = _header()
    assert re.search(r"^\s*int\s+mod_set_depth_decimation\s*\(\s*ModContext\s*\*\s*ctx\s*,\s*const\s+ModDepthDecimation\s*\*\s*decimation\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_get_depth_decimation\s*\(\s*const\s+ModContext\s*\*\s*ctx\s*,\s*ModDepthDecimation\s*\*\s*decimation\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_depth_decimate_dev\s*\(\s*ModContext\s*\*\s*ctx\s*,\s*int32_t\s+frames\s*,\s*const\s+void\s*\*\s*depth_in\s*,\s*"
                     r"const\s+ModDepthLayout\s*\*\s*layout\s*,\s*const\s+ModDepthDecimation\s*\*\s*decimation\s*,\s*void\s*\*\s*depth_out\s*\)\s*;", src, flags=re.M)
    assert re.search(r"typedef\s+struct\s+ModDepthDecimation\s*\{\s*int32_t\s+dx\s*,\s*dy\s*;\s*int32_t\s+mode\s*;\s*int32_t\s+min_valid\s*;\s*"
                     r"float\s+tol_abs\s*,\s*tol_rel\s*;\s*int32_t\s+reserved\[2\]\s*;\s*\}\s*ModDepthDecimation\s*;", src)
    for k, name in enumerate(("MEDIAN", "MIN", "MEAN", "NEAREST")):
        assert re.search(r"#define\s+MOD_DEPTH_DECIMATE_%s\s+%d\b" % (name, k), src)
    assert re.search(r"#define\s+MOD_ABI_VERSION\s+2\b", src)                   # additions only: the version stays


def test_the_header_states_the_rule_and_the_model_restates_it():
    text = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    model = open(os.path.join(ROOT, "tests", "models", "depth_decimate_model.py")).read()
    squeeze = lambda s: " ".join(s.replace(" * ", " ").split())  # noqa: E731  (the header's comment frame and line breaks)
    for phrase in ("(x0 + dx X + i, y0 + dy Y + j), i < dx, j < dy", "ascending, then i ascending", "If |V| < max(min_valid, 1): no reading",
                   "(z, row-major index)", "element (|V| - 1) / 2, the lower median", "one of the block's input words", "the nearest surface",
                   "the z-buffer's rule", "t = tol_abs + tol_rel * a, one multiply and", "fabsf(z_q - a) <= t", "The median itself is always a member",
                   "sum = 0.0f; sum = sum + x_q, member by member in row-major order", "m = sum / (float)n", "16 * 65535 < 2^24",
                   "top-left input word, bit for bit, whatever it is", "crop_decimate's default", "min_valid and the tolerances are ignored",
                   "copies the window's words bit for bit"):
        assert squeeze(phrase) in squeeze(text), phrase
        assert squeeze(phrase) in squeeze(model), phrase
    for phrase in ("tests/models/depth_decimate_model.py", "k_depth_filter -> k_depth_spatial -> k_depth_temporal -> k_depth_decimate -> k_depth_to_disparity",
                   "MOD_BIN_MEAN's", "NEAREST goes with MOD_BIN_NEAREST", "nothing forces dx == bx", "decimation under a registration or a distortion",
                   "factors above 4", "fusion into k_depth_to_disparity"):
        assert phrase in text, phrase
    assert "Depth images are NOT binned" not in text


def test_the_makefile_builds_the_kernels_source():
    mk = open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=((?:.*\\\n)*.*)$", mk, flags=re.M).group(1)
    assert "depth_decimate.hip" in srcs.replace("\\", " ").split()
    src = open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "depth_decimate.hip")).read()
    assert "k_depth_decimate" in src and "__global__" in src
    launch = open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "mod_launch.h")).read()
    assert "launch_depth_decimate" in launch and "launch_depth_decimate" in src


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
    assert lib.mod_set_depth_decimation.argtypes == [C.c_void_p, P(capi.ModDepthDecimation)]
    assert lib.mod_get_depth_decimation.argtypes == [C.c_void_p, P(capi.ModDepthDecimation)]
    assert lib.mod_depth_decimate_dev.argtypes == [C.c_void_p, C.c_int32, C.c_void_p, P(capi.ModDepthLayout), P(capi.ModDepthDecimation), C.c_void_p]
    assert all(getattr(lib, n).restype == C.c_int for n in NAMES)
    assert lib.mod_abi_version() == 2
    assert (capi.MOD_DEPTH_DECIMATE_MEDIAN, capi.MOD_DEPTH_DECIMATE_MIN, capi.MOD_DEPTH_DECIMATE_MEAN, capi.MOD_DEPTH_DECIMATE_NEAREST) == (0, 1, 2, 3)


def test_the_struct_is_32_bytes_in_c_and_in_ctypes(tmp_path):
    from moving_object_detector_amd import capi
    assert C.sizeof(capi.ModDepthDecimation) == 32
    offsets = [getattr(capi.ModDepthDecimation, n).offset for n in ("dx", "dy", "mode", "min_valid", "tol_abs", "tol_rel", "reserved")]
    assert offsets == [0, 4, 8, 12, 16, 20, 24]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "mod_sf.h"\n'
                   '_Static_assert(sizeof(ModDepthDecimation) == 32, "ModDepthDecimation is 32 bytes");\n'
                   '_Static_assert(offsetof(ModDepthDecimation, dx) == 0 && offsetof(ModDepthDecimation, dy) == 4 && '
                   'offsetof(ModDepthDecimation, mode) == 8 && offsetof(ModDepthDecimation, min_valid) == 12 && '
                   'offsetof(ModDepthDecimation, tol_abs) == 16 && offsetof(ModDepthDecimation, tol_rel) == 20 && '
                   'offsetof(ModDepthDecimation, reserved) == 24, "its members");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])


def test_the_helper_and_its_defaults():
    from moving_object_detector_amd import capi
    d = capi.depth_decimation()
    assert (d.dx, d.dy, d.mode, d.min_valid, d.tol_abs, list(d.reserved)) == (2, 2, capi.MOD_DEPTH_DECIMATE_MEDIAN, 1, 0.0, [0, 0])
    assert abs(d.tol_rel - 0.02) < 1e-8
    g = capi.depth_decimation(4, 3, "mean", 5, 0.25, 0.125)
    assert (g.dx, g.dy, g.mode, g.min_valid, g.tol_abs, g.tol_rel) == (4, 3, 2, 5, 0.25, 0.125)
    assert [capi.depth_decimation(mode=m).mode for m in ("median", "min", "mean", "nearest", 3)] == [0, 1, 2, 3, 3]


def test_null_context_is_refused_without_a_device():
    from moving_object_detector_amd import capi
    lib = capi.load()
    d = capi.depth_decimation(2, 2, "mean", 2, 0.03, 0.02)
    before = bytes(d)
    assert lib.mod_set_depth_decimation(None, C.byref(d)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_depth_decimation(None, C.byref(d)) == capi.MOD_ERR_INVALID_ARGUMENT and bytes(d) == before
    lay = capi.depth_layout("16UC1", 8, 4)
    assert lib.mod_depth_decimate_dev(None, 1, None, C.byref(lay), C.byref(d), None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert bytes(d) == before


def test_the_python_layer_has_the_methods():
    from moving_object_detector_amd.pipeline import Context
    for name in ("set_depth_decimation", "get_depth_decimation", "depth_decimate"):
        assert callable(getattr(Context, name))


def test_the_host_mirror_forwards(tmp_path):
    """a C++ program against host/ with a recording stub in the library's place: setDepthDecimation(&d) hands d on, setDepthDecimation(nullptr) NULL"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "depth_decimate_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "depth_decimate_mirror_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    out = [line for line in out if line.startswith(("mod_set_depth_decimation", "refused"))]
    call = "mod_set_depth_decimation 2 3 2 4 0.25 0.125 0 0"
    assert out == [call, "mod_set_depth_decimation NULL", call, "refused: threw"], out
