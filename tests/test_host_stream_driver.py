"""host_stream.HostStream against a context whose library only records its calls and returns scripted codes (no GPU): the order of
submits and collects, tickets and skip codes, errors, NULL arguments, the argument lists against capi's argtypes table, the one object
slicing rule; and tests/util.py's assert_same_stream on synthetic results that differ in one byte."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from moving_object_detector_amd import capi  # noqa: E402
from moving_object_detector_amd.host_stream import HostStream  # noqa: E402
from util import assert_same_stream  # noqa: E402

W, H, CAP, DT = 6, 4, 3, 0.1
SUBMITS = ("frame", "stereo", "images", "odometry", "depth")
OUTPUTS = ("cloud", "labels", "disparity", "flow")


class FakeLib:
    """records (name, args after the context); a submit returns the next scripted code and hands out tickets 100, 101, ..."""

    def __init__(self, codes=(), counts=()):
        self.calls, self.codes, self.counts, self.next_ticket = [], list(codes), list(counts), 100
        for kind in SUBMITS:
            setattr(self, f"mod_submit_{kind}_host", lambda h, *a, _n=kind: self._submit(_n, a))

    def _submit(self, name, args):
        self.calls.append((name, args))
        rc = self.codes.pop(0) if self.codes else 0
        if rc == 0:
            args[-1]._obj.value = self.next_ticket
            self.next_ticket += 1
        return rc

    def mod_collect_frame_host(self, h, ticket, count):
        self.calls.append(("collect", (ticket,)))
        count._obj.value = self.counts.pop(0) if self.counts else 0
        return 0

    def mod_forget_previous(self, h):
        self.calls.append(("forget", ()))
        return 0

    def mod_last_error(self, h):
        return b"the scripted error"


def _ctx(**kw):
    return types.SimpleNamespace(lib=FakeLib(**kw), h=C.c_void_p(1), width=W, height=H)


def _inputs():
    img, plane = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32)
    sp, fp, ep, tf = capi.ModSgmParams(), capi.flow_params(), capi.ego_params(), capi.ModTransform()
    return {"frame": (plane, plane, plane, tf, DT), "stereo": (img, img, sp, plane, tf, DT), "images": (img, img, sp, fp, tf, DT),
            "odometry": (img, img, sp, fp, ep, DT), "depth": (img, img, fp, ep, tf, DT)}


def test_every_submit_past_the_depth_collects_the_oldest_first():
    assert capi.MOD_PIPELINE_DEPTH == 3
    ctx = _ctx(counts=range(7))
    s = HostStream(ctx, 7, CAP)
    s.forget_previous()
    for f in range(7):
        assert s.submit_odometry(f, *_inputs()["odometry"]) == 0
    names = [(n, a[0]) if n == "collect" else n for n, a in ctx.lib.calls]
    assert names == ["forget"] + ["odometry"] * 3 + [x for k in range(4) for x in (("collect", 100 + k), "odometry")]
    del ctx.lib.calls[:]
    assert s.finish() is s
    assert ctx.lib.calls == [("collect", (t,)) for t in (104, 105, 106)]          # the rest, in submission order
    assert s.first == [0] * 7 and s.rc == [0] * 7 and s.n == list(range(7))


def test_a_positive_code_takes_no_ticket_and_a_negative_one_raises():
    ctx = _ctx(codes=[capi.MOD_SKIP_NO_FLOW, 0, capi.MOD_ERR_INVALID_ARGUMENT])
    s = HostStream(ctx, 3, CAP)
    assert s.submit_images(0, *_inputs()["images"]) == capi.MOD_SKIP_NO_FLOW
    assert s.submit_images(1, *_inputs()["images"]) == 0
    with pytest.raises(capi.ModError, match="the scripted error") as e:
        s.submit_images(2, *_inputs()["images"])
    assert e.value.code == capi.MOD_ERR_INVALID_ARGUMENT
    s.finish()
    assert s.first == [capi.MOD_SKIP_NO_FLOW, 0, capi.MOD_ERR_INVALID_ARGUMENT] and s.rc == [None, 0, None]
    assert [c for c in ctx.lib.calls if c[0] == "collect"] == [("collect", (100,))]


def test_a_frame_with_a_ticket_outstanding_cannot_be_submitted_again():
    s = HostStream(_ctx(), 2, CAP)
    s.submit_frame(0, *_inputs()["frame"])
    with pytest.raises(ValueError, match="outstanding"):
        s.submit_frame(0, *_inputs()["frame"])
    s.finish()
    assert s.submit_frame(0, *_inputs()["frame"]) == 0


def test_outputs_not_requested_and_none_inputs_are_null():
    ctx = _ctx()
    s = HostStream(ctx, 1, 0, outputs=("disparity",))
    assert s.cloud is None and s.labels is None and s.flow is None
    s.submit_depth(0, None, None, capi.flow_params(), None, None, DT)
    image, depth, _, ego_prm, tf, dt, cloud, labels, objects, cap, disp, flow = ctx.lib.calls[0][1][:12]
    assert (image, depth, ego_prm, tf, cloud, labels, objects, cap, flow) == (None, None, None, None, None, None, None, 0, None)
    assert disp == s.disparity[0].ctypes.data and dt == DT
    full = HostStream(ctx, 2, CAP)
    pinned = types.SimpleNamespace(ptr=4096, nbytes=H * W)
    full.submit_stereo(1, pinned, pinned, capi.ModSgmParams(), None, (np.zeros(3), np.array([0, 0, 0, 1.0])), DT)
    a = ctx.lib.calls[1][1]
    assert a[:2] == (4096, 4096) and a[3] is None and a[4]._obj.q[3] == 1.0
    assert a[6:11] == (full.cloud[1].ctypes.data, full.labels[1].ctypes.data, full.objects[1], CAP, full.disparity[1].ctypes.data)
    assert (full.labels == -7).all() and (full.cloud == -7).all()


@pytest.mark.parametrize("kind", SUBMITS)
def test_argument_lists_match_the_argtypes_table(kind):
    argtypes = getattr(capi.load(), f"mod_submit_{kind}_host").argtypes
    ctx = _ctx()
    s = HostStream(ctx, 1, CAP)
    getattr(s, f"submit_{kind}")(0, *_inputs()[kind])
    args = (ctx.h,) + ctx.lib.calls[0][1]
    assert len(args) == len(argtypes)
    for i, (a, t) in enumerate(zip(args, argtypes)):
        if isinstance(t._type_, type):                                                  # a POINTER(...): that very type, by reference
            assert isinstance(a._obj, t._type_), (i, t)
        elif t is C.c_void_p:
            assert a is None or isinstance(a, (int, C.c_void_p, C.Array)), (i, a)
        else:
            assert isinstance(a, {C.c_double: float, C.c_int32: int}[t]), (i, a)


def test_objects_bytes_slices_by_the_smaller_of_count_and_capacity():
    s = HostStream(_ctx(counts=[CAP - 1, CAP, CAP + 5]), 3, CAP)
    for f in range(3):
        s.submit_frame(f, *_inputs()["frame"])
    s.finish()
    assert [len(s.objects_bytes(f)) for f in range(3)] == [112 * (CAP - 1), 112 * CAP, 112 * CAP]
    assert len(s.transform_bytes(0)) == 56 and len(s.ego_bytes(0)) == 24


def _result():
    s = HostStream(_ctx(codes=[capi.MOD_SKIP_NO_FLOW, 0, 0], counts=[2, 1]), 3, CAP, transform=((9, 9, 9), (9, 9, 9, 9)), ego=(-9, -9, -9, -9, -9.0))
    for f in range(3):
        s.submit_odometry(f, *_inputs()["odometry"])
    return s.finish()


def _flip(s, key, f=1):
    if key in OUTPUTS:
        getattr(s, key)[f].view(np.uint8).reshape(-1)[5] ^= 1
    elif key in ("first", "rc", "n"):
        getattr(s, key)[f] += 1
    else:
        rec = {"objects": s.objects[f], "transform": s.transforms[f], "ego": s.ego[f]}[key]
        C.cast(C.byref(rec), C.POINTER(C.c_uint8))[3] ^= 1


@pytest.mark.parametrize("key", OUTPUTS + ("first", "rc", "n", "objects", "transform", "ego"))
def test_the_comparer_names_the_key_and_frame_of_one_differing_byte(key):
    keys = OUTPUTS + ("transform", "ego")
    a, b = _result(), _result()
    assert a.transforms[1].t[0] == 9 and a.ego[1].status == -9
    assert_same_stream(a, b, keys)
    _flip(b, key)
    with pytest.raises(AssertionError) as e:
        assert_same_stream(a, b, keys)
    assert f"('{key}', 1" in str(e.value)
