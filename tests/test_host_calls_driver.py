"""host_calls.HostCalls against a library that only records its calls and returns scripted codes (no GPU): the argument lists against
capi.SIGNATURES, NULL arguments, outputs in place, skip codes and errors, contiguity; and capi.bind / capi.declare against the
signature tables."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from moving_object_detector_amd import capi
from moving_object_detector_amd.host_calls import HostCalls, objects_bytes

W, H, CAP, DT = 6, 4, 3, 0.1
IMG, PLANE, FLOW = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32), np.zeros((H, W, 2), np.float32)
CLOUD = np.zeros((H, W, 8), np.float32)
TF = capi.ModTransform()
# method -> (entry point, arguments)
CALLS = {
    "disparity_host": ("mod_sgm_compute_host", (IMG, IMG, capi.ModSgmParams())),
    "flow_host": ("mod_flow_compute_host", (IMG, IMG, capi.flow_params())),
    "egomotion_host": ("mod_egomotion_host", (PLANE, PLANE, FLOW, capi.ego_params())),
    "depth_image_host": ("mod_depth_image_host", (PLANE,)),
    "static_flow_host": ("mod_static_flow_host", (PLANE, TF)),
    "process_frame_host": ("mod_process_frame_host", (PLANE, PLANE, FLOW, TF, DT, CLOUD, np.zeros((H, W), np.int32), CAP)),
    "cluster_cloud_host": ("mod_cluster_cloud_host", (CLOUD, np.zeros((H, W), np.int32), CAP)),
}


class FakeLib:
    """records (name, args after the context) and returns the next scripted code; a count pointer gets the next scripted count"""

    def __init__(self, codes=(), counts=()):
        self.calls, self.codes, self.counts = [], list(codes), list(counts)
        for name, _ in CALLS.values():
            setattr(self, name, lambda h, *a, _n=name: self._call(_n, a))

    def _call(self, name, args):
        self.calls.append((name, args))
        if name in ("mod_process_frame_host", "mod_cluster_cloud_host") and args[-1] is not None:
            args[-1]._obj.value = self.counts.pop(0) if self.counts else 0
        return self.codes.pop(0) if self.codes else 0

    def mod_last_error(self, h):
        return b"the scripted error"


def _ctx(**kw):
    c = HostCalls()
    c.lib, c.h, c.width, c.height = FakeLib(**kw), C.c_void_p(1), W, H
    return c


@pytest.mark.parametrize("method", CALLS)
def test_argument_lists_match_the_signature_table(method):
    name, args = CALLS[method]
    ctx = _ctx()
    getattr(ctx, method)(*args)
    (called, rest), argtypes = ctx.lib.calls[0], capi.SIGNATURES[name]
    got = (ctx.h,) + rest
    assert called == name and len(got) == len(argtypes)
    for i, (a, t) in enumerate(zip(got, argtypes)):
        if isinstance(t._type_, type):                                                  # a POINTER(...): that very type, by reference
            assert a is None or isinstance(a._obj, t._type_), (i, t)
        elif t is C.c_void_p:
            assert a is None or isinstance(a, (int, C.c_void_p, C.Array)), (i, a)
        else:
            assert isinstance(a, {C.c_double: float, C.c_int32: int}[t]), (i, a)


def test_none_inputs_and_unrequested_outputs_are_null():
    ctx = _ctx()
    ctx.disparity_host(None, None, None)
    ctx.flow_host(None, None)
    ctx.depth_image_host(None)
    ctx.static_flow_host(None, None)
    ctx.egomotion_host(None, None, None)
    ctx.process_frame_host(None, None, None, None, DT, count=False)
    ctx.cluster_cloud_host(None)
    a = [args for _, args in ctx.lib.calls]
    assert a[0][:3] == (None, None, None) and a[1][:2] == (None, None) and a[2][0] is None and a[3][:2] == (None, None)
    assert a[1][2]._obj.levels == capi.flow_params().levels                               # params None: the header's defaults
    assert a[4][:3] == (None, None, None) and a[4][3]._obj.hypotheses == capi.ego_params().hypotheses
    assert a[5] == (None, None, None, None, DT, None, None, None, 0, None)               # count=False: a NULL count pointer
    assert a[6][:7] == (None, W, H, 32, 32 * W, None, None) and a[6][7] == 0 and isinstance(a[6][8]._obj, C.c_int32)
    assert all(isinstance(x[-1], int) and x[-1] != 0 for x in a[:4])                      # a required output is allocated


def test_outputs_the_caller_passes_are_the_pointers_handed_over():
    ctx = _ctx(counts=[CAP + 2, 1])
    disp, flow, depth, sflow = (np.full(s, -7, np.float32) for s in ((H, W), (H, W, 2), (H, W), (H, W, 2)))
    cloud, labels = np.full((H, W, 8), -7, np.float32), np.full((H, W), -7, np.int32)
    assert ctx.disparity_host(IMG, IMG, capi.ModSgmParams(), disp)[1] is disp
    assert ctx.flow_host(IMG, IMG, out=flow)[1] is flow
    assert ctx.depth_image_host(PLANE, depth)[1] is depth
    assert ctx.static_flow_host(PLANE, (np.zeros(3), np.array([0, 0, 0, 1.0])), sflow)[1] is sflow
    rc, n, objs = ctx.process_frame_host(PLANE, PLANE, FLOW, TF, DT, cloud, labels, CAP)
    assert (rc, n) == (0, CAP + 2) and len(objects_bytes(objs, n, CAP)) == 112 * CAP
    rc, n, objs2 = ctx.cluster_cloud_host(cloud, labels, CAP, width=W - 1, height=H - 1, row_step=999)
    assert (rc, n) == (0, 1) and len(objects_bytes(objs2, n, CAP)) == 112 and objects_bytes(None, 0, 0) == b""
    a = [args for _, args in ctx.lib.calls]
    assert [x[-1] for x in a[:4]] == [v.ctypes.data for v in (disp, flow, depth, sflow)]
    assert a[3][1]._obj.q[3] == 1.0
    assert a[4][5:9] == (cloud.ctypes.data, labels.ctypes.data, objs, CAP) and a[4][3]._obj is TF
    assert a[5][:8] == (cloud.ctypes.data, W - 1, H - 1, 32, 999, labels.ctypes.data, objs2, CAP)
    assert all((v == -7).all() for v in (disp, flow, depth, sflow, cloud, labels))      # the driver itself writes nothing
    pinned = types.SimpleNamespace(ptr=4096, nbytes=H * W)
    ctx.disparity_host(pinned, pinned, capi.ModSgmParams())
    assert ctx.lib.calls[-1][1][:2] == (4096, 4096)


@pytest.mark.parametrize("method", CALLS)
def test_a_positive_code_is_returned_and_a_negative_one_raises(method):
    _, args = CALLS[method]
    ctx = _ctx(codes=[capi.MOD_SKIP_NO_FLOW, capi.MOD_ERR_CAPACITY])
    assert getattr(ctx, method)(*args)[0] == capi.MOD_SKIP_NO_FLOW
    with pytest.raises(capi.ModError, match="the scripted error") as e:
        getattr(ctx, method)(*args)
    assert e.value.code == capi.MOD_ERR_CAPACITY


def test_an_allocated_output_is_none_after_a_skip():
    ctx = _ctx(codes=[capi.MOD_SKIP_NO_DISPARITY_NOW, 0])
    assert ctx.disparity_host(None, IMG, capi.ModSgmParams()) == (capi.MOD_SKIP_NO_DISPARITY_NOW, None)
    rc, disp = ctx.disparity_host(IMG, IMG, capi.ModSgmParams())
    assert rc == 0 and disp.shape == (H, W) and disp.dtype == np.float32


@pytest.mark.parametrize("method", CALLS)
def test_a_non_contiguous_input_raises_before_any_call(method):
    _, args = CALLS[method]
    ctx = _ctx()
    strided = np.zeros((H, 2 * W) + args[0].shape[2:], args[0].dtype)[:, ::2]
    assert strided.shape == args[0].shape
    with pytest.raises(ValueError, match="C-contiguous"):
        getattr(ctx, method)(strided, *args[1:])
    assert ctx.lib.calls == []


def test_bind_declares_every_name_of_the_table_on_the_product_build():
    assert capi.EXPORTS == list(capi.SIGNATURES)
    L = capi.bind(capi.LIB_PATH)
    for name, argtypes in capi.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes == argtypes, name
        assert fn.restype == {"mod_destroy": None, "mod_last_error": C.c_char_p}.get(name, C.c_int), name
    if "MOD_SF_LIB" not in os.environ:                                                  # (the product build, not a diagnostic one)
        for name in capi.DEBUG_SIGNATURES:                                              # absent, and no error
            assert not hasattr(L, name)
    assert capi.DEBUG_SIGNATURES["mod_debug_read"] == [C.c_void_p, C.c_int, C.c_void_p, C.c_ulonglong]
    assert capi.DEBUG_SIGNATURES["mod_debug_counters"] == [C.c_void_p, C.POINTER(C.c_uint64)]


def test_declare_names_a_missing_entry_point_unless_missing_ok():
    def stub(without=(), debug=False):
        names = [n for n in capi.SIGNATURES if n not in without] + (list(capi.DEBUG_SIGNATURES) if debug else [])
        return types.SimpleNamespace(**{n: types.SimpleNamespace(argtypes="unset", restype="unset") for n in names})
    with pytest.raises(AttributeError, match="mod_set_disparity_filters"):
        capi.declare(stub(without=("mod_set_disparity_filters",)))
    old = capi.declare(stub(without=("mod_set_disparity_filters", "mod_abi_version")), missing_ok=True)
    assert not hasattr(old, "mod_set_disparity_filters") and old.mod_sgm_compute_dev.argtypes == capi.SIGNATURES["mod_sgm_compute_dev"]
    assert old.mod_destroy.restype is None and old.mod_last_error.restype is C.c_char_p and old.mod_create.restype is C.c_int
    checked = capi.declare(stub(debug=True))
    assert checked.mod_debug_read.argtypes == capi.DEBUG_SIGNATURES["mod_debug_read"] and checked.mod_debug_counters.restype is C.c_int
    assert checked.mod_abi_version.argtypes == "unset"                                  # None in the table: left undeclared
