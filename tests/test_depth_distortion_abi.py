"""CPU: mod_set_depth_distortion, mod_get_depth_distortion and mod_depth_rays_host are part of the C ABI: declared in include/mod_sf.h,
let through by csrc/exports.map, exported by the library, listed and typed by capi; ModDepthDistortion is 64 bytes on both sides; the
ABI version stays 2; MOD_DEPTH_UNDISTORT_ITERS and the lattice names are the same numbers in the header and in capi; the calls refuse
what they can refuse without a device; the Python layer and the host mirror have the setter."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_depth_distortion", "mod_get_depth_distortion", "mod_depth_rays_host")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mod_sf.h")).read(), flags=re.S)


def test_header_declares_the_calls_the_struct_and_the_constants():
    src = _header()
    assert re.search(r"typedef\s+struct\s+ModDepthDistortion\s*\{\s*double\s+D\[8\];\s*\}\s*ModDepthDistortion\s*;", src)
    assert re.search(r"^\s*int\s+mod_set_depth_distortion\s*\(\s*ModContext\s*\*\s*ctx\s*,\s*const\s+ModDepthDistortion\s*\*\s*d\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_get_depth_distortion\s*\(\s*const\s+ModContext\s*\*\s*ctx\s*,\s*ModDepthDistortion\s*\*\s*d\s*,\s*int32_t\s*\*\s*enabled\s*\)\s*;",
                     src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_depth_rays_host\s*\(\s*ModContext\s*\*\s*ctx\s*,\s*const\s+ModDepthLayout\s*\*\s*layout\s*,\s*int32_t\s+lattice\s*,"
                     r"\s*double\s*\*\s*rays\s*\)\s*;", src, flags=re.M)
    assert re.search(r"#define\s+MOD_DEPTH_RAYS_CENTRES\s+0\b", src) and re.search(r"#define\s+MOD_DEPTH_RAYS_CORNERS\s+1\b", src)
    assert re.search(r"#define\s+MOD_DEPTH_UNDISTORT_ITERS\s+20\b", src)
    assert re.search(r"#define\s+MOD_ABI_VERSION\s+2\b", src)                   # additions only: the version stays


def test_the_header_states_the_arithmetic_and_what_is_left_undone():
    text = open(os.path.join(ROOT, "include", "mod_sf.h")).read()
    assert "Holes are left as holes (no splatting, no fill: depth_image_proc/register's" in text       # the older paragraphs keep their sentences
    for phrase in ("ic = (1.0 + ((k6*r2 + k5)*r2 + k4)*r2) / (1.0 + ((k3*r2 + k2)*r2 + k1)*r2)", "x = (xd - dx) * ic;  y = (yd - dy) * ic",
                   "<= 1.0/64", "X0 = x * Z0;  Y0 = y * Z0", "NOT bit-identical", "equidistant", "collect every ticket first"):
        assert phrase in text, phrase


def test_sizeof_is_64_on_both_sides(tmp_path):
    from moving_object_detector_amd import capi
    assert C.sizeof(capi.ModDepthDistortion) == 64
    src = tmp_path / "size.c"
    src.write_text('#include "mod_sf.h"\n#include <stdio.h>\nint main(void) { printf("%zu %d\\n", sizeof(ModDepthDistortion), MOD_DEPTH_UNDISTORT_ITERS); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["64", str(capi.MOD_DEPTH_UNDISTORT_ITERS)]


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
    iters = int(re.search(r"#define\s+MOD_DEPTH_UNDISTORT_ITERS\s+(\d+)", _header()).group(1))
    assert capi.MOD_DEPTH_UNDISTORT_ITERS == iters == 20
    assert (capi.MOD_DEPTH_RAYS_CENTRES, capi.MOD_DEPTH_RAYS_CORNERS) == (0, 1)
    lib = capi.load()
    assert lib.mod_set_depth_distortion.argtypes == [C.c_void_p, C.POINTER(capi.ModDepthDistortion)]
    assert lib.mod_get_depth_distortion.argtypes == [C.c_void_p, C.POINTER(capi.ModDepthDistortion), C.POINTER(C.c_int32)]
    assert lib.mod_depth_rays_host.argtypes == [C.c_void_p, C.POINTER(capi.ModDepthLayout), C.c_int32, C.c_void_p]
    assert all(getattr(lib, n).restype == C.c_int for n in NAMES)
    assert lib.mod_abi_version() == 2


def test_depth_distortion_pads_with_zeros():
    from moving_object_detector_amd import capi
    assert list(capi.depth_distortion([1, 2, 3, 4]).D) == [1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0]
    assert list(capi.depth_distortion([1, 2, 3, 4, 5]).D) == [1.0, 2.0, 3.0, 4.0, 5.0, 0.0, 0.0, 0.0]
    assert list(capi.depth_distortion(range(8)).D) == [float(k) for k in range(8)]
    for n in (0, 3, 6, 7, 9):
        with pytest.raises(ValueError):
            capi.depth_distortion([0.0] * n)


def test_null_arguments_are_refused_without_a_device():
    from moving_object_detector_amd import capi
    lib = capi.load()
    E = capi.MOD_ERR_INVALID_ARGUMENT
    d, on, out = capi.depth_distortion([0.1, 0.0, 0.0, 0.0]), C.c_int32(-7), (C.c_double * 2)()
    assert lib.mod_set_depth_distortion(None, C.byref(d)) == E and lib.mod_set_depth_distortion(None, None) == E
    bad = capi.depth_distortion([float("nan"), 0.0, 0.0, 0.0])
    assert lib.mod_set_depth_distortion(None, C.byref(bad)) == E
    assert lib.mod_get_depth_distortion(None, C.byref(d), C.byref(on)) == E and on.value == -7
    assert lib.mod_depth_rays_host(None, None, 0, out) == E and list(out) == [0.0, 0.0]


def test_the_python_layer_and_the_host_mirror_have_the_setter():
    from moving_object_detector_amd.pipeline import Context
    assert callable(Context.set_depth_distortion) and callable(Context.get_depth_distortion) and callable(Context.depth_rays)
    hpp = open(os.path.join(ROOT, "moving_object_detector_amd", "host", "scene_flow_constructor.hpp")).read()
    assert re.search(r"void\s+setDepthDistortion\s*\(\s*const\s+ModDepthDistortion\s*\*\s*distortion\s*\)\s*\{\s*check\(mod_set_depth_distortion\(ctx_,", hpp)
