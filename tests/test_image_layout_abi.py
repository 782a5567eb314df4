"""CPU: ModImageLayout and the encoding constants of include/mod_sf.h match the ctypes binding (size 24, field offsets), and the
helpers capi.image_layout / capi.centred_window."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "mod_sf.h")).read()


def test_layout_struct_matches_the_header():
    from moving_object_detector_amd import capi
    src = _header()
    body = re.search(r"typedef struct ModImageLayout \{(.*?)\} ModImageLayout;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in re.findall(r"int32_t\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert fields == [f for f, _ in capi.ModImageLayout._fields_] == ["encoding", "width", "height", "step", "x0", "y0"]
    assert C.sizeof(capi.ModImageLayout) == 24
    assert [getattr(capi.ModImageLayout, f).offset for f in fields] == [0, 4, 8, 12, 16, 20]


def test_encoding_constants_match_the_header():
    from moving_object_detector_amd import capi
    src = _header()
    for name, val in capi.ENCODINGS.items():
        m = re.search(r"#define MOD_ENCODING_%s\s+(\d+)" % name.upper(), src)
        assert m and int(m.group(1)) == val == getattr(capi, "MOD_ENCODING_" + name.upper())


def test_layout_helpers():
    from moving_object_detector_amd import capi
    l = capi.image_layout("bgra8", 1920, 1080)
    assert (l.encoding, l.width, l.height, l.step, l.x0, l.y0) == (capi.MOD_ENCODING_BGRA8, 1920, 1080, 7680, 0, 0)
    l = capi.image_layout(capi.MOD_ENCODING_BGR8, 1281, 721, step=3845, x0=1, y0=1)
    assert (l.step, l.x0, l.y0) == (3845, 1, 1)
    assert capi.centred_window(1920, 1080, 1280, 720) == (320, 180)
    assert capi.centred_window(1281, 721, 1280, 720) == (0, 0)   # image_crop.cpp: integer (W - w) / 2
    with pytest.raises(ValueError):
        capi.centred_window(100, 100, 101, 10)
