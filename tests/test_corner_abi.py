"""CPU: the ABI of the flow's min-eigenvalue threshold.  ModCornerFilter is 16 bytes with its fields at 0 / 4 / 8 / 12, the four calls
are declared in include/mod_sf.h, bound in capi.SIGNATURES / capi.EXPORTS and exported by the library, and capi.corner_filter() has
the header's defaults.  (The values the setter refuses need a context, hence a device: tests/test_gpu_corner.py.)"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_flow_corner_filter", "mod_get_flow_corner_filter", "mod_flow_corner_dev", "mod_flow_corner_reject_dev")


def test_struct_layout_and_defaults():
    from moving_object_detector_amd import capi
    F = capi.ModCornerFilter
    assert C.sizeof(F) == 16
    assert [(n, getattr(F, n).offset) for n, _ in F._fields_] == [("threshold", 0), ("window", 4), ("cap", 8), ("reserved", 12)]
    f = capi.corner_filter()
    assert (f.threshold, f.window, f.cap, f.reserved) == (0, 9, 31, 0)
    f = capi.corner_filter(200, 15, 255)
    assert (f.threshold, f.window, f.cap, f.reserved) == (200, 15, 255, 0)
    assert capi.MOD_CORNER_MAX == 14630625 == 225 * 255 * 255 < 1 << 31
    # the texture filter is as it was
    assert C.sizeof(capi.ModTextureFilter) == 16 and [n for n, _ in capi.ModTextureFilter._fields_] == ["threshold", "window", "cap", "apply"]


def test_header_declares_the_calls_and_the_struct():
    src = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    assert re.search(r"^int\s+mod_set_flow_corner_filter\(ModContext \*ctx, const ModCornerFilter \*filter\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_get_flow_corner_filter\(const ModContext \*ctx, ModCornerFilter \*filter\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_flow_corner_dev\(ModContext \*ctx, int32_t frames, const uint8_t \*grey, const ModCornerFilter \*filter, "
                     r"uint32_t \*strength\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_flow_corner_reject_dev\(ModContext \*ctx, int32_t frames, const uint8_t \*grey, const ModCornerFilter \*filter, "
                     r"float \*flow\);", src, flags=re.M)
    assert re.search(r"^#define MOD_CORNER_MAX 14630625\b", src, flags=re.M)
    assert re.search(r"typedef struct ModCornerFilter \{[^}]*int32_t threshold;[^}]*int32_t window;[^}]*int32_t cap;[^}]*int32_t reserved;[^}]*\} "
                     r"ModCornerFilter;", src)
    assert re.search(r"^#define MOD_ABI_VERSION 2\b", src, flags=re.M)
    assert "parity with OpenCV's cornerMinEigenVal is NOT claimed" in re.sub(r"\s*\n \*\s*", " ", src)


def test_library_exports_and_python_binds_them():
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = capi.load()
    for name in NAMES:
        assert name in exported and name in capi.EXPORTS and hasattr(lib, name), name
    fp = C.POINTER(capi.ModCornerFilter)
    assert capi.SIGNATURES["mod_set_flow_corner_filter"] == [C.c_void_p, fp] and capi.SIGNATURES["mod_get_flow_corner_filter"] == [C.c_void_p, fp]
    assert capi.SIGNATURES["mod_flow_corner_dev"] == [C.c_void_p, C.c_int32, C.c_void_p, fp, C.c_void_p]
    assert capi.SIGNATURES["mod_flow_corner_reject_dev"] == [C.c_void_p, C.c_int32, C.c_void_p, fp, C.c_void_p]
    assert lib.mod_abi_version() == 2
    for method in ("set_flow_corner_filter", "get_flow_corner_filter", "flow_corner", "flow_corner_reject"):
        assert callable(getattr(Context, method)), method
    # no context: an error code, not a crash
    f = capi.corner_filter(5)
    assert lib.mod_set_flow_corner_filter(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_flow_corner_filter(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT and f.threshold == 5
    assert lib.mod_flow_corner_dev(None, 1, None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_flow_corner_reject_dev(None, 1, None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_the_kernel_file_is_built_and_reads_no_environment():
    csrc = os.path.join(ROOT, "moving_object_detector_amd", "csrc")
    assert re.search(r"^SRCS\s*=.*?\bcorner\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M | re.S)
    kernel = open(os.path.join(csrc, "corner.hip")).read()
    assert "getenv" not in kernel and "atomic" not in kernel.replace("no atomics", "") and "asm" not in kernel
    assert "launch_corner(" in open(os.path.join(csrc, "mod_launch.h")).read()
    hpp = open(os.path.join(ROOT, "moving_object_detector_amd", "host", "scene_flow_constructor.hpp")).read()
    assert "void setFlowCornerFilter(int threshold, int window = 9, int cap = 31)" in hpp and "mod_set_flow_corner_filter(ctx_" in hpp
