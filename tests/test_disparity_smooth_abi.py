"""CPU: the ABI of the disparity's edge-preserving smoother.  ModDisparitySmooth is 16 bytes with its fields at 0 / 4 / 8 / 12, the three
calls are declared in include/mod_sf.h, bound in capi.SIGNATURES / capi.EXPORTS and exported by the library, capi.disparity_smooth() has
the documented defaults and refuses what the library refuses, the three calls answer a NULL context with an error code — the one check
of theirs that needs no device — and the host mirror's setDisparitySmooth, compiled against a recording stub, hands the library the
struct it was given.  (The values the setter refuses need a context, hence a device: tests/test_gpu_disparity_smooth.py.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_disparity_smooth", "mod_get_disparity_smooth", "mod_disparity_smooth_dev")


def _fields(f):
    return (f.window, f.min_members, f.tol, f.reserved)


def test_struct_layout_and_the_helper():
    from moving_object_detector_amd import capi
    S = capi.ModDisparitySmooth
    assert C.sizeof(S) == 16
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("window", 0), ("min_members", 4), ("tol", 8), ("reserved", 12)]
    assert [t for _, t in S._fields_] == [C.c_int32, C.c_int32, C.c_float, C.c_int32]
    assert _fields(capi.disparity_smooth()) == (5, 1, 1.0, 0)
    assert _fields(capi.disparity_smooth(3)) == (3, 1, 1.0, 0)
    assert _fields(capi.disparity_smooth(7, 0.0625, 49)) == (7, 49, 0.0625, 0)
    assert _fields(capi.disparity_smooth(window=3, tol=0.0, min_members=9)) == (3, 9, 0.0, 0)
    assert "not tuned" in capi.disparity_smooth.__doc__
    for bad in ((0,), (1,), (4,), (9,), (-3,), (5, -1.0), (5, -1e-30), (5, float("nan")), (5, float("inf")), (5, -float("inf")), (5, 1e39), (5, 1.0, 0),
                (5, 1.0, -1), (5, 1.0, 26), (3, 1.0, 10), (7, 1.0, 50)):
        with pytest.raises(ValueError):
            capi.disparity_smooth(*bad)
    # the fill's struct and version are as they were
    assert C.sizeof(capi.ModDisparityFill) == 16 and [n for n, _ in capi.ModDisparityFill._fields_] == ["reach", "directions", "mode", "min_found"]
    assert C.sizeof(capi.ModSgmParams) == 24


def test_header_declares_the_calls_and_the_struct_and_states_the_rule():
    src = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    assert re.search(r"^int\s+mod_set_disparity_smooth\(ModContext \*ctx, const ModDisparitySmooth \*smooth\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_get_disparity_smooth\(const ModContext \*ctx, ModDisparitySmooth \*smooth\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_disparity_smooth_dev\(ModContext \*ctx, int32_t frames, const float \*disparity_in, const ModDisparitySmooth \*smooth, "
                     r"float \*disparity_out\);", src, flags=re.M)
    assert re.search(r"typedef struct ModDisparitySmooth \{[^}]*int32_t window;[^}]*int32_t min_members;[^}]*float   tol;[^}]*int32_t reserved;[^}]*"
                     r"\} ModDisparitySmooth;", src)
    assert re.search(r"^#define MOD_ABI_VERSION 2\b", src, flags=re.M)
    flat = re.sub(r"\s*\n \*\s*", " ", src)
    for phrase in ("a word w is valid iff it is finite and w >= lo", "-0.0 is valid", "an invalid pixel: out = in, bit for bit",
                   "never fills a hole and never makes one", "fabsf(q - d) <= tol", "the subtraction rounded to float32",
                   "The pixel is always its own member", "n < min_members (1..window^2): out = in, bit for bit", "sum = 0.0f",
                   "row-major order of the window, top row first, left to right", "each step sum = sum + q", "out = fmaxf(sum / (float)n, lo)",
                   "a smoothed pixel feeds no other pixel", "both see the SMOOTHED disparity", "behind the speckle stage and in front of the hole fill",
                   "not tuned on camera data"):
        assert phrase in flat, phrase


def test_library_exports_and_python_binds_them():
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "mod_*" in open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "exports.map")).read()      # the map exports the mod_ prefix
    lib = capi.load()
    for name in NAMES:
        assert name in exported and name in capi.EXPORTS and name in capi.SIGNATURES and hasattr(lib, name), name
    sp = C.POINTER(capi.ModDisparitySmooth)
    assert capi.SIGNATURES["mod_set_disparity_smooth"] == [C.c_void_p, sp] and capi.SIGNATURES["mod_get_disparity_smooth"] == [C.c_void_p, sp]
    assert capi.SIGNATURES["mod_disparity_smooth_dev"] == [C.c_void_p, C.c_int32, C.c_void_p, sp, C.c_void_p]
    assert lib.mod_abi_version() == 2
    for method in ("set_disparity_smooth", "get_disparity_smooth", "disparity_smooth"):
        assert callable(getattr(Context, method)), method
    # no context: an error code, not a crash, and nothing is written
    f = capi.disparity_smooth(7, 0.5, 3)
    assert lib.mod_set_disparity_smooth(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_disparity_smooth(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert _fields(f) == (7, 3, 0.5, 0)
    assert lib.mod_disparity_smooth_dev(None, 1, None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_the_kernel_file_is_built_and_holds_plain_loads_and_stores_only():
    csrc = os.path.join(ROOT, "moving_object_detector_amd", "csrc")
    assert re.search(r"^SRCS\s*=.*?\bdisparity_smooth\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M | re.S)
    kernel = open(os.path.join(csrc, "disparity_smooth.hip")).read()
    assert "getenv" not in kernel and "atomic" not in kernel.replace("no atomics", "") and "asm" not in kernel
    assert "k_disparity_smooth" in kernel and "__shared__" in kernel and "template <int Win>" in kernel
    assert "launch_disparity_smooth(" in open(os.path.join(csrc, "mod_launch.h")).read()
    sgm = open(os.path.join(csrc, "host_sgm.hip")).read()
    assert sgm.index("launch_speckle(") < sgm.index("launch_disparity_smooth(") < sgm.index("launch_disparity_fill(")     # the stage order
    assert "check_disparity_smooth" in open(os.path.join(csrc, "host_filters.hip")).read()


def test_the_host_mirror_has_the_setter(tmp_path):
    """a C++ program against host/ with a recording stub in the library's place: setDisparitySmooth hands the library the struct it was
    given, and a refusal becomes an exception"""
    hpp = open(os.path.join(ROOT, "moving_object_detector_amd", "host", "scene_flow_constructor.hpp")).read()
    assert "void setDisparitySmooth(int window, float tol, int min_members)" in hpp and "mod_set_disparity_smooth(ctx_" in hpp
    assert hpp.index("void setDisparityFilters(") < hpp.index("void setDisparitySmooth(") < hpp.index("void setDisparityFill(")
    exe = str(tmp_path / "disparity_smooth_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "disparity_smooth_mirror_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    out = [line for line in out if line.startswith(("mod_set_disparity_smooth", "refused"))]
    assert out == ["mod_set_disparity_smooth 5 1 1 0", "mod_set_disparity_smooth 7 49 0.0625 0", "mod_set_disparity_smooth NULL",
                   "mod_set_disparity_smooth 4 1 1 0", "refused: threw"], out
