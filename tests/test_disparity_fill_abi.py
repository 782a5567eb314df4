"""CPU: the ABI of the disparity's occlusion hole fill.  ModDisparityFill is 16 bytes with its fields at 0 / 4 / 8 / 12, the three calls
and the three mode constants are declared in include/mod_sf.h, bound in capi.SIGNATURES / capi.EXPORTS and exported by the library,
capi.disparity_fill() has the documented defaults and refuses what the library refuses, the three calls answer a NULL context with an
error code — the one check of theirs that needs no device — and the host mirror's setDisparityFill, compiled against a recording stub,
hands the library the struct it was given.  (The values the setter refuses need a context, hence a device:
tests/test_gpu_disparity_fill.py.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_disparity_fill", "mod_get_disparity_fill", "mod_disparity_fill_dev")


def _fields(f):
    return (f.reach, f.directions, f.mode, f.min_found)


def test_struct_layout_constants_and_the_helper():
    from moving_object_detector_amd import capi
    F = capi.ModDisparityFill
    assert C.sizeof(F) == 16
    assert [(n, getattr(F, n).offset) for n, _ in F._fields_] == [("reach", 0), ("directions", 4), ("mode", 8), ("min_found", 12)]
    assert (capi.MOD_DISPARITY_FILL_MIN, capi.MOD_DISPARITY_FILL_SECOND, capi.MOD_DISPARITY_FILL_MEDIAN) == (0, 1, 2)
    assert _fields(capi.disparity_fill(64)) == (64, 8, 0, 1)
    assert _fields(capi.disparity_fill(256, 4, "median", 3)) == (256, 4, 2, 3)
    assert _fields(capi.disparity_fill(1, 2, "second", 2)) == (1, 2, 1, 2)
    assert _fields(capi.disparity_fill(16, directions=8, mode=capi.MOD_DISPARITY_FILL_MEDIAN, min_found=8)) == (16, 8, 2, 8)
    assert _fields(capi.disparity_fill(0)) == (0, 8, 0, 1)
    assert "not tuned" in capi.disparity_fill.__doc__
    for bad in ((-1,), (257,), (16, 3), (16, 0), (16, 16), (16, 8, "mean"), (16, 8, 3), (16, 8, -1), (16, 8, "min", 0), (16, 8, "min", 9),
                (16, 4, "min", 5), (16, 2, "min", 3)):
        with pytest.raises(ValueError):
            capi.disparity_fill(*bad)
    # the rejection filters' struct is as it was
    assert C.sizeof(capi.ModDisparityFilters) == 16
    assert [n for n, _ in capi.ModDisparityFilters._fields_] == ["uniqueness_ratio", "speckle_size", "speckle_range", "reserved"]


def test_header_declares_the_calls_and_the_struct_and_states_the_rule():
    src = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    assert re.search(r"^int\s+mod_set_disparity_fill\(ModContext \*ctx, const ModDisparityFill \*fill\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_get_disparity_fill\(const ModContext \*ctx, ModDisparityFill \*fill\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_disparity_fill_dev\(ModContext \*ctx, int32_t frames, const float \*disparity_in, const ModDisparityFill \*fill, "
                     r"float \*disparity_out\);", src, flags=re.M)
    assert re.search(r"typedef struct ModDisparityFill \{[^}]*int32_t reach;[^}]*int32_t directions;[^}]*int32_t mode;[^}]*int32_t min_found;[^}]*"
                     r"\} ModDisparityFill;", src)
    for name, value in (("MIN", 0), ("SECOND", 1), ("MEDIAN", 2)):
        assert re.search(rf"^#define MOD_DISPARITY_FILL_{name}\s+{value}\b", src, flags=re.M)
    assert re.search(r"^#define MOD_ABI_VERSION 2\b", src, flags=re.M)
    flat = re.sub(r"\s*\n \*\s*", " ", src)
    for phrase in ("a word d is valid iff it is finite and d >= lo", "-0.0 is valid", "never wraps into the next row, the next frame or the plane before it",
                   "n < min_found: out = in, bit for bit", "SECOND r = min(1, n - 1)", "MEDIAN r = (n - 1) >> 1", "a filled pixel feeds no other fill",
                   "both see the FILLED disparity", "(+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,-1) (-1,+1) (+1,-1)"):
        assert phrase in flat, phrase


def test_library_exports_and_python_binds_them():
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = capi.load()
    for name in NAMES:
        assert name in exported and name in capi.EXPORTS and name in capi.SIGNATURES and hasattr(lib, name), name
    fp = C.POINTER(capi.ModDisparityFill)
    assert capi.SIGNATURES["mod_set_disparity_fill"] == [C.c_void_p, fp] and capi.SIGNATURES["mod_get_disparity_fill"] == [C.c_void_p, fp]
    assert capi.SIGNATURES["mod_disparity_fill_dev"] == [C.c_void_p, C.c_int32, C.c_void_p, fp, C.c_void_p]
    assert lib.mod_abi_version() == 2
    for method in ("set_disparity_fill", "get_disparity_fill", "disparity_fill"):
        assert callable(getattr(Context, method)), method
    # no context: an error code, not a crash, and nothing is written
    f = capi.disparity_fill(16, 4, "second", 2)
    assert lib.mod_set_disparity_fill(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_disparity_fill(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert _fields(f) == (16, 4, 1, 2)
    assert lib.mod_disparity_fill_dev(None, 1, None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_the_kernel_file_is_built_and_holds_plain_loads_and_stores_only():
    csrc = os.path.join(ROOT, "moving_object_detector_amd", "csrc")
    assert re.search(r"^SRCS\s*=.*?\bdisparity_fill\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M | re.S)
    kernel = open(os.path.join(csrc, "disparity_fill.hip")).read()
    assert "getenv" not in kernel and "atomic" not in kernel and "asm" not in kernel
    assert "k_disparity_fill" in kernel and "__ballot" in kernel
    assert "launch_disparity_fill(" in open(os.path.join(csrc, "mod_launch.h")).read()
    assert "launch_disparity_fill(" in open(os.path.join(csrc, "host_sgm.hip")).read()
    assert "check_disparity_fill" in open(os.path.join(csrc, "host_filters.hip")).read()


def test_the_host_mirror_has_the_setter(tmp_path):
    """a C++ program against host/ with a recording stub in the library's place: setDisparityFill hands the library the struct it was given,
    and a refusal becomes an exception"""
    hpp = open(os.path.join(ROOT, "moving_object_detector_amd", "host", "scene_flow_constructor.hpp")).read()
    assert "void setDisparityFill(int reach, int directions, int mode, int min_found)" in hpp and "mod_set_disparity_fill(ctx_" in hpp
    assert hpp.index("void setDisparityFilters(") < hpp.index("void setDisparityFill(")     # beside setDisparityFilters
    exe = str(tmp_path / "disparity_fill_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "disparity_fill_mirror_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    out = [line for line in out if line.startswith(("mod_set_disparity_fill", "refused"))]
    assert out == ["mod_set_disparity_fill 64 8 0 1", "mod_set_disparity_fill 256 4 2 3", "mod_set_disparity_fill 0 0 0 0",
                   "mod_set_disparity_fill 16 3 1 1", "refused: threw"], out
