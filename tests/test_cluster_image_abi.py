"""CPU: the cluster-image ABI (mod_set_cluster_image / mod_get_cluster_image / mod_cluster_image_dev / mod_cluster_color and
mod_cluster_palette) — struct size, exports, what the header promises, and the host-only colour calls against the model."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mod_sf.h")
CSRC = os.path.join(ROOT, "moving_object_detector_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests", "models"))
import cluster_image_model as M  # noqa: E402

NAMES = ("mod_set_cluster_image", "mod_get_cluster_image", "mod_cluster_image_dev", "mod_cluster_color", "mod_cluster_palette")
KS = (1, 2, 3, 7, 254, 255, 256, 257, 511, 9216, 20736)


def test_struct_is_32_bytes_and_mirrors_the_header():
    from moving_object_detector_amd import capi
    fields = ["image", "host_image", "palette_bgr", "reserved"]
    assert C.sizeof(capi.ModClusterImage) == 32
    assert [n for n, _ in capi.ModClusterImage._fields_] == fields
    assert capi.ModClusterImage.reserved.offset == 24 and capi.ModClusterImage.reserved.size == 8
    src = open(HEADER).read()
    body = re.search(r"typedef struct ModClusterImage \{(.*?)\} ModClusterImage;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == fields


def test_header_declares_the_calls_and_the_version_stays():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, flags=re.M), name
    assert "#define MOD_ABI_VERSION 2" in src
    assert re.search(r"#define MOD_STAGE_COUNT\s+7\b", src)
    from moving_object_detector_amd import capi
    assert capi.load().mod_abi_version() == 2


def test_symbols_pass_the_export_map_and_are_bound():
    from moving_object_detector_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    assert re.search(r"global:\s*mod_\*;", text) and re.search(r"local:\s*\*;", text)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert name in names and name in capi.EXPORTS, name
    lib = capi.load()
    assert lib.mod_set_cluster_image.argtypes[1]._type_ is capi.ModClusterImage
    assert lib.mod_get_cluster_image.argtypes[1]._type_ is capi.ModClusterImage
    assert len(lib.mod_cluster_image_dev.argtypes) == 6 and len(lib.mod_cluster_color.argtypes) == 4
    # a NULL context is refused before anything else, like every other setter
    assert lib.mod_set_cluster_image(None, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_cluster_image(None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_cluster_image_dev(None, 1, None, None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_header_states_the_table_and_the_rules():
    src = " ".join(re.sub(r"\n \*(?!/)", "\n", open(HEADER).read()).split())
    doc = src[src.index("The cluster image and the markers' colours"):src.index("typedef struct ModClusterImage")]
    assert "(k * 255) / K" in doc and "NOT OpenCV's COLORMAP_HSV" in doc
    assert "t = 6 i, s = t >> 8 (0..5), f = t & 255, g = 255 - f" in doc
    assert "Entry 0 is (0, 0, 255), entry 255 is (5, 0, 255)" in doc
    assert "never indexes the table" in doc and "NULL = off" in doc
    assert "leaves host_image untouched" in doc and "the frame in flight keeps both" in doc
    assert "reserved != 0" in doc and "16-byte aligned" in doc


def test_the_built_in_table_is_the_models():
    from moving_object_detector_amd import capi
    lut = capi.cluster_palette()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert np.array_equal(lut, M.palette())


def test_cluster_color_equals_the_model_for_every_label():
    from moving_object_detector_amd import capi
    lib = capi.load()
    lut = M.palette()
    rnd = np.random.default_rng(20261019).integers(0, 256, (256, 3), dtype=np.uint8)
    rnd_c = capi.palette_bytes(rnd)
    out = (C.c_uint8 * 3)()
    for K in KS:
        for k in range(K):
            i = M.index(k, K)
            assert lib.mod_cluster_color(k, K, None, out) == capi.MOD_OK
            assert tuple(out) == tuple(lut[i]), (k, K)
            assert lib.mod_cluster_color(k, K, rnd_c, out) == capi.MOD_OK
            assert tuple(out) == tuple(rnd[i]), (k, K)
    assert capi.cluster_color(3, 7) == tuple(lut[109]) and capi.cluster_color(3, 7, rnd) == tuple(rnd[109])


def test_cluster_color_refuses_labels_outside_the_frame():
    from moving_object_detector_amd import capi
    lib = capi.load()
    out = (C.c_uint8 * 3)(7, 7, 7)
    for k, K in ((5, 5), (-1, 5), (0, 0), (0, -3), (6, 5)):
        assert lib.mod_cluster_color(k, K, None, out) == capi.MOD_ERR_INVALID_ARGUMENT
        assert tuple(out) == (7, 7, 7)
    assert lib.mod_cluster_color(0, 1, None, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_cluster_palette(None) == capi.MOD_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        capi.cluster_color(5, 5)


def test_the_kernel_host_and_test_program_read_one_header():
    kernel = open(os.path.join(CSRC, "label_image.hip")).read()
    host = open(os.path.join(CSRC, "mod_sf.hip")).read()
    assert '#include "label_palette.h"' in kernel and "palette_index_rcp(" in kernel
    assert "label_palette::palette_index(" in host and "label_palette::builtin_bgr(" in host
    hdr = open(os.path.join(CSRC, "label_palette.h")).read()
    assert hdr.count("uint32_t palette_index(") == 1 and hdr.count("uint32_t builtin_bgr(") == 1
