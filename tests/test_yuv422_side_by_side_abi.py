"""CPU: the packed YUV 4:2:2 encodings and the side-by-side setting are part of the C ABI — the two macros against capi, the two
calls declared in include/mod_sf.h, let through by csrc/exports.map, exported by the library and typed by capi; the layout helper
knows two bytes per pixel; host/messages.hpp's name lookup and image_channels for all seven encodings, in a small program built with
the host compiler."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mod_set_side_by_side", "mod_get_side_by_side")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mod_sf.h")).read(), flags=re.S)


def test_the_two_macros_match_capi():
    from moving_object_detector_amd import capi
    src = _header()
    for macro, name, val in (("MOD_ENCODING_YUV422", "yuv422", 5), ("MOD_ENCODING_YUV422_YUY2", "yuv422_yuy2", 6)):
        m = re.search(r"#define\s+%s\s+(\d+)\s*$" % macro, src, flags=re.M)
        assert m and int(m.group(1)) == val == getattr(capi, macro) == capi.ENCODINGS[name]
        assert capi.CHANNELS[val] == 2
    assert sorted(capi.ENCODINGS.values()) == list(range(7)) and set(capi.CHANNELS) == set(capi.ENCODINGS.values())
    assert re.search(r"#define\s+MOD_ABI_VERSION\s+2\b", src)                   # additions only: the version stays


def test_layout_helper_knows_two_bytes_per_pixel():
    from moving_object_detector_amd import capi
    assert capi.image_layout("yuv422", 1280, 720).step == 2560
    l = capi.image_layout("yuv422_yuy2", 1281, 721, x0=1, y0=1)
    assert (l.encoding, l.step, l.x0, l.y0) == (capi.MOD_ENCODING_YUV422_YUY2, 2562, 1, 1)
    assert capi.image_layout("yuv422", 640, 480, step=2 * 2 * 640).step == 2560   # a side-by-side row: the caller's step stands


def test_header_declares_the_calls():
    src = _header()
    assert re.search(r"^\s*int\s+mod_set_side_by_side\s*\(\s*ModContext\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", src, flags=re.M)
    assert re.search(r"^\s*int\s+mod_get_side_by_side\s*\(\s*const\s+ModContext\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;", src, flags=re.M)


def test_exports_map_lets_them_through_and_the_library_has_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "exports.map")).read(), flags=re.S)
    globs = re.findall(r"([\w*?]+)\s*;", text.split("global:")[1].split("local:")[0])
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), (name, globs)
    from moving_object_detector_amd import capi
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= defined, set(NAMES) - defined


def test_capi_lists_types_and_refuses_a_null_context():
    from moving_object_detector_amd import capi
    for name in NAMES:
        assert name in capi.EXPORTS
    lib = capi.load()
    assert lib.mod_set_side_by_side.argtypes == [C.c_void_p, C.c_int32]
    assert lib.mod_get_side_by_side.argtypes == [C.c_void_p, C.POINTER(C.c_int32)]
    on = C.c_int32(-7)
    assert lib.mod_set_side_by_side(None, 1) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_side_by_side(None, C.byref(on)) == capi.MOD_ERR_INVALID_ARGUMENT and on.value == -7
    assert lib.mod_abi_version() == 2
    from moving_object_detector_amd.pipeline import Context
    assert callable(Context.set_side_by_side) and callable(Context.get_side_by_side)


PROGRAM = r"""
#include "messages.hpp"
#include <cstdio>
int main() {
  const char *names[7] = {"mono8", "bgr8", "rgb8", "bgra8", "rgba8", "yuv422", "yuv422_yuy2"};
  const int enc[7] = {MOD_ENCODING_MONO8, MOD_ENCODING_BGR8, MOD_ENCODING_RGB8, MOD_ENCODING_BGRA8, MOD_ENCODING_RGBA8, MOD_ENCODING_YUV422,
                      MOD_ENCODING_YUV422_YUY2};
  const int channels[7] = {1, 3, 3, 4, 4, 2, 2};
  int bad = 0;
  for (int i = 0; i < 7; i++) {
    if (enc[i] != i || mod_host::image_encoding(names[i]) != enc[i]) { std::printf("lookup %s\n", names[i]); bad++; }
    if (mod_host::image_channels(enc[i]) != channels[i]) { std::printf("channels %s: %d\n", names[i], mod_host::image_channels(enc[i])); bad++; }
  }
  if (mod_host::image_encoding("yuv422_uyvy") != -1 || mod_host::image_encoding("bayer_rggb8") != -1 || mod_host::image_encoding("") != -1) bad++;
  mod_host::Image m;
  m.width = 1280; m.height = 720; m.encoding = "yuv422_yuy2";                 // a side-by-side message of two 640-pixel panes
  ModImageLayout l{};
  if (!mod_host::image_layout(m, 3, 5, &l) || l.encoding != 6 || l.width != 1280 || l.step != 2560 || l.x0 != 3 || l.y0 != 5) bad++;
  if (!mod_host::image_layout(m, 3, 5, &l, true) || l.width != 640 || l.height != 720 || l.step != 2560) bad++;
  m.width = 1281;
  if (mod_host::image_layout(m, 0, 0, &l, true)) bad++;                       // an odd width holds no two panes
  std::printf("bad %d\n", bad);
  return bad;
}
"""


def test_messages_hpp_knows_all_seven_encodings(tmp_path):
    src = tmp_path / "encodings.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "encodings"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "moving_object_detector_amd", "host"),
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
