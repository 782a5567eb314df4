"""Shared helpers for the parity tests."""
import ctypes as C
import os

import numpy as np

PLANES = ("x", "y", "z", "vx", "vy", "vz")
CHECKED_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "moving_object_detector_amd", "libmod_sf_checked.so")


class EgoChecked:
    """A context of the diagnostic build, which can read the ego-motion estimator's scratch (mod_debug_read 5, 6, 7).  The library
    lays the correspondences out as [max_frames][9][cap] with cap the grid size of the smallest stride this context has seen
    (ensure_ego_scratch), so the reads use that stride, not the call's."""

    def __init__(self, W, H, F, cam):
        from moving_object_detector_amd import capi, synth
        from moving_object_detector_amd.host_calls import HostCalls
        import moving_object_detector_amd.pipeline  # noqa: F401  (torch first: one HIP runtime)
        L = capi.bind(CHECKED_LIB)
        self.L, self.h = L, C.c_void_p()
        assert L.mod_create(C.byref(capi.ModConfig(0, W, H, F, 0, 0, None)), C.byref(self.h)) == 0
        assert L.mod_set_camera(self.h, C.byref(capi.camera_struct(cam))) == 0
        assert L.mod_set_params(self.h, C.byref(capi.params_struct(synth.Params()))) == 0
        self.W, self.H, self.F = W, H, F
        self.min_stride = None
        self.calls = HostCalls()
        self.calls.lib, self.calls.h, self.calls.width, self.calls.height = L, self.h, W, H

    def run(self, dp, dn, fl, prm):
        """One mod_egomotion_dev call on device tensors -> transforms (F, 7), results (EGO_RESULT_DTYPE), correspondence counts
        [max_frames], correspondences [max_frames][9][cap], hypothesis counts [F][hypotheses]."""
        import torch
        from moving_object_detector_amd.pipeline import EGO_RESULT_DTYPE
        F = dn.shape[0]
        tf = torch.empty((F, 7), dtype=torch.float64, device=dn.device)
        res = torch.empty((F, 24), dtype=torch.uint8, device=dn.device)
        assert self.L.mod_egomotion_dev(self.h, F, dp.data_ptr(), dn.data_ptr(), fl.data_ptr(), C.byref(prm), tf.data_ptr(), res.data_ptr()) == 0
        assert self.L.mod_synchronize(self.h) == 0
        self.min_stride = prm.stride if self.min_stride is None else min(self.min_stride, prm.stride)
        s = self.min_stride
        cap = -(-self.W // s) * -(-self.H // s)
        n = np.zeros(self.F, np.int32)
        corr = np.zeros((self.F, 9, cap), np.float64)
        cnt = np.zeros(F * prm.hypotheses, np.int32)          # [frames][hypotheses] of this call
        for which, a in ((5, n), (6, corr), (7, cnt)):
            self.calls.debug_read(which, a)
        cnt = cnt.reshape(F, prm.hypotheses)
        return tf.cpu().numpy(), np.frombuffer(res.cpu().numpy().tobytes(), dtype=EGO_RESULT_DTYPE), n, corr, cnt

    def host(self, d_prev, d_now, flow, prm):
        """mod_egomotion_host of one frame of host arrays -> return code, ModTransform bytes, ModEgoResult bytes."""
        rc, ht, hr = self.calls.egomotion_host(*[np.ascontiguousarray(a, np.float32) for a in (d_prev, d_now, flow)], prm)
        return rc, bytes(ht), bytes(hr)

    def close(self):
        self.L.mod_destroy(self.h)


def bits_equal(a, b):
    """Bit-exact float comparison that treats every NaN as equal to every NaN (payload/sign of NaN is not part of
    the contract: x86 produces 0xFFC00000 for invalid operations, gfx950 0x7FC00000)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def bits_equal64(a, b):
    """bits_equal for f64: the same bits everywhere, NaN == NaN by position."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def assert_ego_frame(tf, res, n, corr, cnt, m, where):
    """One frame of EgoChecked.run (transform (7,), result record, correspondence count, correspondences [9][cap], hypothesis counts)
    against ego_model.estimate's dict m, bit for bit: the correspondence list, every hypothesis's inlier count, every ModEgoResult field
    (rms_px included) and the transform."""
    k = len(m["corr"]["pix"])
    assert n == k == res["correspondences"], (where, n, k, res["correspondences"])
    want = np.concatenate([m["corr"]["P"].T, m["corr"]["Q"].T, m["corr"]["O"].T])
    assert bits_equal64(corr[:, :k], want), (where, "correspondences")
    assert np.array_equal(cnt, m["counts"]), (where, "hypothesis counts", np.flatnonzero(cnt != m["counts"])[:8])
    got = (int(res["status"]), int(res["inliers"]), int(res["iterations"]))
    assert got == (m["status"], m["inliers"], m["iterations"]), (where, "status, inliers, iterations", got, m["status"], m["inliers"], m["iterations"])
    assert bits_equal64(res["rms_px"], m["rms"]), (where, "rms", float(res["rms_px"]), m["rms"])
    assert bits_equal64(tf, m["transform"]), (where, "transform", tf.tolist(), m["transform"].tolist())


def first_mismatch(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    bad = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    idx = np.argwhere(bad)
    if idx.size == 0:
        return None
    i = tuple(idx[0])
    return {"count": int(bad.sum()), "index": i, "a": float(a[i]), "b": float(b[i])}


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    m = ~(np.isnan(a) | np.isnan(b))
    if not m.any():
        return 0.0
    d = np.abs(a[m] - b[m])
    s = np.maximum(np.abs(a[m]), np.abs(b[m]))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(s > 0, d / s, 0.0)
    return float(np.nanmax(r))


def compare_objects(gpu_objs, orc_objs, strict_velocity=True):
    """gpu_objs: structured array (pipeline.OBJECT_DTYPE); orc_objs: list of dicts from pyoracle / numpy_ref."""
    assert len(gpu_objs) == len(orc_objs), (len(gpu_objs), len(orc_objs))
    for g, o in zip(gpu_objs, orc_objs):
        assert int(g["id"]) == int(o["id"])
        assert int(g["n_points"]) == int(o["n_points"])
        assert np.array_equal(g["center"], np.asarray(o["center"])), (g["center"], o["center"])
        assert np.array_equal(g["bounding_box"], np.asarray(o["bounding_box"]))
        assert np.array_equal(g["orientation"], np.array([0.0, 0.0, 0.0, 1.0]))
        if o.get("ambiguous", False) and not strict_velocity:
            # tie on ||v|| between different vectors and an expected value that does not come from std::sort (the numpy
            # goldens): only the norm is comparable.  Against the C++ oracle (real std::sort) use strict_velocity=True:
            # k_median_ties replays libstdc++'s introsort and must return the very same member
            ng = np.float32(np.sqrt(np.float32(g["velocity"][0]) ** 2 + (np.float32(g["velocity"][1]) ** 2 + np.float32(g["velocity"][2]) ** 2)))
            no = np.float32(np.sqrt(np.float32(o["velocity"][0]) ** 2 + (np.float32(o["velocity"][1]) ** 2 + np.float32(o["velocity"][2]) ** 2)))
            assert ng == no
        else:
            assert np.array_equal(g["velocity"], np.asarray(o["velocity"])), (g["velocity"], o["velocity"], o.get("ambiguous"))


def compare_objects_bits(gpu_objs, orc_objs):
    """compare_objects for records that may hold NaN or inf: id and n_points as integers, center, bounding_box and velocity as F64 bit
    patterns, a NaN matching a NaN at the same position (bits_equal64).  Velocities are always strict: the oracle's std::sort decides."""
    assert len(gpu_objs) == len(orc_objs), (len(gpu_objs), len(orc_objs))
    for g, o in zip(gpu_objs, orc_objs):
        assert int(g["id"]) == int(o["id"]), (int(g["id"]), int(o["id"]))
        assert int(g["n_points"]) == int(o["n_points"]), (int(o["id"]), int(g["n_points"]), int(o["n_points"]))
        for k in ("center", "bounding_box", "velocity"):
            assert bits_equal64(g[k], np.asarray(o[k], np.float64)), (int(o["id"]), k, g[k].tolist(), np.asarray(o[k]).tolist(), o.get("ambiguous"))
        assert np.array_equal(g["orientation"], np.array([0.0, 0.0, 0.0, 1.0]))


def assert_same_stream(a, b, keys, frames=None):
    """Two finished host_stream.HostStream runs gave the same: first, rc and n of every frame in `frames` (None: all), and for the frames
    that took a ticket, byte for byte, the outputs named in `keys` ("cloud", "labels", "disparity", "flow"; "transform" and "ego" for
    the estimator's records) and the object records the library reported.  A failure names (key, frame)."""
    for f in range(len(a.first)) if frames is None else frames:
        for k in ("first", "rc", "n"):
            assert getattr(a, k)[f] == getattr(b, k)[f], (k, f, getattr(a, k)[f], getattr(b, k)[f])
        if a.first[f] != 0:
            continue
        for k in keys:
            if k in ("transform", "ego"):
                same = getattr(a, k + "_bytes")(f) == getattr(b, k + "_bytes")(f)
            else:
                same = getattr(a, k)[f].tobytes() == getattr(b, k)[f].tobytes()
            assert same, (k, f)
        assert a.objects_bytes(f) == b.objects_bytes(f), ("objects", f)
