"""CPU: the ABI of the texture threshold.  ModTextureFilter is 16 bytes with its fields at 0 / 4 / 8 / 12, the four calls are declared
in include/mod_sf.h, bound in capi.SIGNATURES / capi.EXPORTS and exported by the library, and capi.texture_filter() has the header's
defaults.  (The values the setter refuses need a context, hence a device: tests/test_gpu_texture.py.)"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_texture_filter", "mod_get_texture_filter", "mod_texture_dev", "mod_texture_reject_dev")


def test_struct_layout_and_defaults():
    from moving_object_detector_amd import capi
    F = capi.ModTextureFilter
    assert C.sizeof(F) == 16
    assert [(n, getattr(F, n).offset) for n, _ in F._fields_] == [("threshold", 0), ("window", 4), ("cap", 8), ("apply", 12)]
    assert (capi.MOD_TEXTURE_DISPARITY, capi.MOD_TEXTURE_FLOW) == (1, 2)
    f = capi.texture_filter()
    assert (f.threshold, f.window, f.cap, f.apply) == (0, 9, 31, 3)
    f = capi.texture_filter(400, 15, 255, capi.MOD_TEXTURE_FLOW)
    assert (f.threshold, f.window, f.cap, f.apply) == (400, 15, 255, 2)
    assert capi.MOD_TEXTURE_MAX == 57375 < 65536


def test_header_declares_the_calls_and_the_struct():
    src = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    assert re.search(r"^int\s+mod_set_texture_filter\(ModContext \*ctx, const ModTextureFilter \*filter\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_get_texture_filter\(const ModContext \*ctx, ModTextureFilter \*filter\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_texture_dev\(ModContext \*ctx, int32_t frames, const uint8_t \*grey, const ModTextureFilter \*filter, "
                     r"uint16_t \*texture\);", src, flags=re.M)
    assert re.search(r"^int\s+mod_texture_reject_dev\(ModContext \*ctx, int32_t frames, const uint8_t \*grey, const ModTextureFilter \*filter, "
                     r"float \*disparity,\s+float \*flow\);", src, flags=re.M)
    assert re.search(r"^#define MOD_TEXTURE_DISPARITY 1\b", src, flags=re.M) and re.search(r"^#define MOD_TEXTURE_FLOW\s+2\b", src, flags=re.M)
    assert re.search(r"typedef struct ModTextureFilter \{[^}]*int32_t threshold;[^}]*int32_t window;[^}]*int32_t cap;[^}]*int32_t apply;[^}]*\} "
                     r"ModTextureFilter;", src)
    assert re.search(r"^#define MOD_ABI_VERSION 2\b", src, flags=re.M)
    assert "parity with OpenCV's Sobel-prefiltered textureThreshold is NOT claimed" in src


def test_library_exports_and_python_binds_them():
    from moving_object_detector_amd import capi
    from moving_object_detector_amd.pipeline import Context
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = capi.load()
    for name in NAMES:
        assert name in exported and name in capi.EXPORTS and hasattr(lib, name), name
    fp = C.POINTER(capi.ModTextureFilter)
    assert capi.SIGNATURES["mod_set_texture_filter"] == [C.c_void_p, fp] and capi.SIGNATURES["mod_get_texture_filter"] == [C.c_void_p, fp]
    assert capi.SIGNATURES["mod_texture_dev"] == [C.c_void_p, C.c_int32, C.c_void_p, fp, C.c_void_p]
    assert capi.SIGNATURES["mod_texture_reject_dev"] == [C.c_void_p, C.c_int32, C.c_void_p, fp, C.c_void_p, C.c_void_p]
    assert lib.mod_abi_version() == 2
    for method in ("set_texture_filter", "get_texture_filter", "texture", "texture_reject"):
        assert callable(getattr(Context, method)), method
    # no context: an error code, not a crash
    f = capi.texture_filter(5)
    assert lib.mod_set_texture_filter(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_texture_filter(None, C.byref(f)) == capi.MOD_ERR_INVALID_ARGUMENT and f.threshold == 5
    assert lib.mod_texture_dev(None, 1, None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_texture_reject_dev(None, 1, None, None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_the_kernel_file_is_built_and_reads_no_environment():
    csrc = os.path.join(ROOT, "moving_object_detector_amd", "csrc")
    assert re.search(r"^SRCS\s*=.*?\btexture\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M | re.S)
    assert "getenv" not in open(os.path.join(csrc, "texture.hip")).read()
    hpp = open(os.path.join(ROOT, "moving_object_detector_amd", "host", "scene_flow_constructor.hpp")).read()
    assert "void setTextureFilter(int threshold" in hpp and "mod_set_texture_filter(ctx_" in hpp
