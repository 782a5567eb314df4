"""CPU: the ABI of the flow's disparity-gated hole fill.  ModFlowFill is 24 bytes with its fields at 0 / 4 / 8 / 12 / 16, the three calls
are declared in include/mod_sf.h, bound in capi.SIGNATURES / capi.EXPORTS and exported by the library, capi.flow_fill() has the documented defaults, the three calls answer a
NULL context with an error code — the one check of theirs that needs no device — and the host mirror's setFlowFill, compiled against a
recording stub, hands the library the struct it was given.  (The values the setter refuses need a context, hence a device:
tests/test_gpu_flow_fill.py, case by case.)"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_flow_fill", "mod_get_flow_fill", "mod_flow_fill_dev")


def test_struct_layout_and_defaults():
    from moving_object_detector_amd import capi
    F = capi.ModFlowFill
    assert C.sizeof(F) == 24
    assert [(n, getattr(F, n).offset) for n, _ in F._fields_] == [("window", 0), ("min_valid", 4), ("tol_abs", 8), ("tol_rel", 12), ("reserved", 16)]
    f = capi.flow_fill()
    assert (f.window, f.min_valid, f.tol_abs, f.tol_rel, tuple(f.reserved)) == (5, 3, 1.0, 0.0, (0, 0))
    f = capi.flow_fill(7, 48, 0.5, 0.0625)
    assert (f.window, f.min_valid, f.tol_abs, f.tol_rel, tuple(f.reserved)) == (7, 48, 0.5, 0.0625, (0, 0))
    assert "not tuned" in capi.flow_fill.__doc__
    # the median's struct is as it was
    assert C.sizeof(capi.ModFlowMedian) == 16 and [n for n, _ in capi.ModFlowMedian._fields_] == ["window", "min_valid", "reserved"]


def test_header_declares_the_calls_and_the_struct_and_states_the_rule():
    src = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    assert re.search(r"^int\s+mod_set_flow_fill\(ModContext \*ctx, const ModFlowFill \*fill\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_get_flow_fill\(const ModContext \*ctx, ModFlowFill \*fill\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_flow_fill_dev\(ModContext \*ctx, int32_t frames, const float \*flow_in, const float \*disparity, "
                     r"const ModFlowFill \*fill,\s+float \*flow_out\);", src, flags=re.M)
    assert re.search(r"typedef struct ModFlowFill \{[^}]*int32_t window;[^}]*int32_t min_valid;[^}]*float   tol_abs, tol_rel;[^}]*"
                     r"int32_t reserved\[2\];[^}]*\} ModFlowFill;", src)
    assert re.search(r"^#define MOD_ABI_VERSION 2\b", src, flags=re.M)
    flat = re.sub(r"\s*\n \*\s*", " ", src)
    for phrase in ("g = tol_abs + tol_rel * d_p", "fabsf(d_q - d_p) is <= g", "finite and d > 0", "ONE PASS", "flow_out) is the FILLED one",
                   "mod_flow_compute_dev / _host have no disparity and are NOT affected"):
        assert phrase in flat, phrase


def test_library_exports_and_python_binds_them():
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = capi.load()
    for name in NAMES:
        assert name in exported and name in capi.EXPORTS and name in capi.SIGNATURES and hasattr(lib, name), name
    fp = C.POINTER(capi.ModFlowFill)
    assert capi.SIGNATURES["mod_set_flow_fill"] == [C.c_void_p, fp] and capi.SIGNATURES["mod_get_flow_fill"] == [C.c_void_p, fp]
    assert capi.SIGNATURES["mod_flow_fill_dev"] == [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, fp, C.c_void_p]
    assert lib.mod_abi_version() == 2
    for method in ("set_flow_fill", "get_flow_fill", "flow_fill"):
        assert callable(getattr(Context, method)), method
    # no context: an error code, not a crash, and nothing is written
    f = capi.flow_fill(3, 2, 0.25, 0.5)
    assert lib.mod_set_flow_fill(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_flow_fill(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert (f.window, f.min_valid, f.tol_abs, f.tol_rel) == (3, 2, 0.25, 0.5)
    assert lib.mod_flow_fill_dev(None, 1, None, None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_the_kernel_file_is_built_and_holds_plain_loads_and_stores_only():
    csrc = os.path.join(ROOT, "moving_object_detector_amd", "csrc")
    assert re.search(r"^SRCS\s*=.*?\bflow_fill\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M | re.S)
    kernel = open(os.path.join(csrc, "flow_fill.hip")).read()
    assert "getenv" not in kernel and "atomic" not in kernel and "asm" not in kernel
    for w in (3, 5, 7):
        assert f"k_flow_fill<{w}>" in kernel
    assert "launch_flow_fill(" in open(os.path.join(csrc, "mod_launch.h")).read()


def test_the_host_mirror_has_the_setter(tmp_path):
    """a C++ program against host/ with a recording stub in the library's place: setFlowFill hands the library the struct it was given, and a
    refusal becomes an exception"""
    hpp = open(os.path.join(ROOT, "moving_object_detector_amd", "host", "scene_flow_constructor.hpp")).read()
    assert "void setFlowFill(int window, int min_valid, float tol_abs, float tol_rel)" in hpp and "mod_set_flow_fill(ctx_" in hpp
    assert hpp.index("void setFlowMedian(") < hpp.index("void setFlowFill(") < hpp.index("void setDisparityFilters(")     # beside setFlowMedian
    exe = str(tmp_path / "flow_fill_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "flow_fill_mirror_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    out = [line for line in out if line.startswith(("mod_set_flow_fill", "refused"))]
    assert out == ["mod_set_flow_fill 5 3 1 0 0 0", "mod_set_flow_fill 7 48 0.25 0.0625 0 0", "mod_set_flow_fill 0 0 0 0 0 0",
                   "mod_set_flow_fill 4 1 1 0 0 0", "refused: threw"], out
