"""CPU: bench.py --dump-outputs writes the last step's outputs as float32 / float64 .npy files — every per-pixel output at one fixed
seeded sample of pixel positions, the objects of every frame in full — from a workspace laid out as pipeline.Context.workspace lays it out."""
import importlib
import os

import numpy as np
import pytest
import torch

from moving_object_detector_amd import capi
from moving_object_detector_amd.pipeline import PLANES, Context


@pytest.fixture
def bench(monkeypatch):
    # bench.py sets HSA_ENABLE_IPC_MODE_LEGACY at import: keep that out of the rest of the session
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return importlib.import_module("bench")


def _workspace(F, H, W, max_objects=12):
    g = torch.Generator().manual_seed(7)
    per, skew = F * H * W, 5
    ws = {"xy": True}
    flat = torch.randn(6 * per + 5 * skew, generator=g)
    flat[torch.randint(0, len(flat), (len(flat) // 4,), generator=g)] = float("nan")     # invalid pixels, as the path writes them
    flat[torch.randint(0, len(flat), (len(flat) // 20,), generator=g)] = float("inf")
    flat[torch.randint(0, len(flat), (len(flat) // 20,), generator=g)] = -float("inf")
    ws["planes"] = flat.as_strided((6, F, H, W), (per + skew, H * W, W, 1))
    ws["mask"] = torch.randint(-2 ** 62, 2 ** 62, (F, H, (W + 63) // 64), generator=g, dtype=torch.int64)
    ws["labels"] = torch.randint(-1, H * W, (F, H, W), generator=g, dtype=torch.int32)
    ws["objects"] = torch.randint(0, 256, (F, max_objects, capi.MOD_OBJECT_BYTES), generator=g, dtype=torch.uint8)
    ws["n_objects"] = torch.randint(0, 6, (F,), generator=g, dtype=torch.int32)
    ws["n_clusters"] = torch.randint(0, 9, (F,), generator=g, dtype=torch.int32)
    return ws


@pytest.mark.parametrize("F,H,W,max_pixels", [(3, 5, 130, 1 << 20), (4, 7, 70, 500)])
def test_dump_outputs(bench, tmp_path, F, H, W, max_pixels):
    ws = _workspace(F, H, W)
    bench.dump_outputs(str(tmp_path / "a"), ws, F, H, W, max_pixels=max_pixels)
    bench.dump_outputs(str(tmp_path / "b"), ws, F, H, W, max_pixels=max_pixels)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    for name, a in got.items():
        assert a.dtype in (np.float32, np.float64), name
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy"))), name   # the sample is fixed
    pos = got["pixel_index"].astype(np.int64)
    assert len(pos) == min(max_pixels, F * H * W) and np.all(np.diff(pos) > 0)
    codes = got["nonfinite"].astype(np.int64)
    for i, k in enumerate(PLANES):
        want = ws["planes"][i].numpy().reshape(-1)[pos]
        code = (codes >> (2 * i)) & 3
        back = np.select([code == 1, code == 2, code == 3], [np.nan, np.inf, -np.inf], got[k])
        assert got[k].dtype == np.float32 and np.array_equal(back, want, equal_nan=True), k
        assert (code == 1).any() and (code == 2).any() and (code == 3).any() and (code == 0).any(), k
    assert np.array_equal(got["labels"], ws["labels"].numpy().reshape(-1)[pos])
    bits = np.unpackbits(ws["mask"].numpy().view(np.uint8), axis=-1, bitorder="little")[..., :W]
    assert np.array_equal(got["dynamic_mask"], bits.reshape(-1)[pos])
    assert np.array_equal(got["n_objects"], ws["n_objects"].numpy()) and np.array_equal(got["n_clusters"], ws["n_clusters"].numpy())
    for f, o in enumerate(Context.objects_to_host(ws)):
        row = got["objects"][f]
        code = got["objects_nonfinite"][f]
        assert not row[len(o):].any() and not code[len(o):].any()
        for j in range(len(o)):
            want = np.concatenate([[o["id"][j], o["n_points"][j]], o["center"][j], o["orientation"][j], o["velocity"][j], o["bounding_box"][j]])
            back = np.select([code[j] == 1, code[j] == 2, code[j] == 3], [np.nan, np.inf, -np.inf], row[j])
            assert np.array_equal(back, want, equal_nan=True)

