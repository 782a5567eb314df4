"""Python methods of the synchronous host entry points (include/mod_sf.h: mod_*_host but the submits, which host_stream.HostStream
drives).  They add nothing to the library: no torch, no copies, no shape or dtype checks of the inputs (the layout in force decides
what a message is).

Conventions, those of pipeline.Context and HostStream: a negative code raises capi.ModError (.code, the library's mod_last_error text),
a positive (skip) code is returned; None for an input or an optional output goes to the library as NULL; an output array the caller
passes is written in place, one the call requires and the caller does not pass is allocated (None is returned for it on a skip, when
nothing was written); inputs are numpy arrays or pinned buffers (Context.pinned_copy) and must be C-contiguous (ValueError)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


def _ptr(a):
    """address of a C-contiguous numpy array or of a pinned buffer (Context.pinned_copy), None = NULL"""
    if a is None:
        return None
    if hasattr(a, "ptr"):
        return a.ptr
    if not a.flags.c_contiguous:
        raise ValueError("arrays handed to the library must be C-contiguous (np.ascontiguousarray makes the copy)")
    return a.ctypes.data


def _ref(s):
    return C.byref(s) if s is not None else None


def _transform(tf):
    """a ModTransform, a pair (t, q), or None"""
    return tf if tf is None or isinstance(tf, capi.ModTransform) else capi.transforms_array([tf[0]], [tf[1]])[0]


def objects_bytes(objects, n, capacity):
    """the bytes of the records the library reported (`n`, which may exceed the `capacity` of `objects`): the one slicing rule"""
    return bytes(objects)[:capi.MOD_OBJECT_BYTES * min(n, capacity)] if capacity else b""


class HostCalls:
    """The synchronous host calls of one context: anything with lib, h, width, height (pipeline.Context inherits them)."""

    def _check(self, rc: int) -> int:
        if rc < 0:
            raise capi.ModError(rc, self.lib.mod_last_error(self.h).decode())
        return rc

    def _image(self, fn, inputs, out, tail, dtype):
        """(rc, out) of fn(h, *inputs, out): `out` the caller's array or a new (H, W) + tail one, None when new and skipped"""
        given = out is not None
        if not given:
            out = np.empty((self.height, self.width) + tail, dtype)
        rc = self._check(fn(self.h, *inputs, _ptr(out)))
        return rc, out if given or rc == 0 else None

    def disparity_host(self, left, right, params, out=None):
        """mod_sgm_compute_host: two images of the layout in force -> (rc, (H, W) float32 disparity)"""
        return self._image(self.lib.mod_sgm_compute_host, (_ptr(left), _ptr(right), _ref(params)), out, (), np.float32)

    def flow_host(self, prev, now, params=None, out=None):
        """mod_flow_compute_host: two images -> (rc, (H, W, 2) float32 flow); params None = capi.flow_params()"""
        prm = params if params is not None else capi.flow_params()
        return self._image(self.lib.mod_flow_compute_host, (_ptr(prev), _ptr(now), C.byref(prm)), out, (2,), np.float32)

    def depth_image_host(self, disparity_now, out=None):
        """mod_depth_image_host: -> (rc, (H, W) float32 depth)"""
        return self._image(self.lib.mod_depth_image_host, (_ptr(disparity_now),), out, (), np.float32)

    def static_flow_host(self, disparity_prev, transform, out=None):
        """mod_static_flow_host: -> (rc, (H, W, 2) float32 static flow); transform a ModTransform, (t, q) or None"""
        return self._image(self.lib.mod_static_flow_host, (_ptr(disparity_prev), _ref(_transform(transform))), out, (2,), np.float32)

    def egomotion_host(self, disp_prev, disp_now, flow, params=None):
        """mod_egomotion_host: -> (rc, ModTransform prev -> now, ModEgoResult); params None = capi.ego_params()"""
        prm = params if params is not None else capi.ego_params()
        tf, res = capi.ModTransform(), capi.ModEgoResult()
        rc = self._check(self.lib.mod_egomotion_host(self.h, _ptr(disp_prev), _ptr(disp_now), _ptr(flow), C.byref(prm), C.byref(tf),
                                                     C.byref(res)))
        return rc, tf, res

    def _clustered(self, fn, inputs, labels, capacity, count):
        """(rc, n, objects) of fn(h, *inputs, labels, objects, capacity, n_objects): `capacity` ModObject records (0: NULL) and
        the count (count=False: NULL, n None); objects_bytes(objects, n, capacity) are the reported records"""
        objects = (capi.ModObject * capacity)() if capacity else None
        n = C.c_int32(-1) if count else None
        rc = self._check(fn(self.h, *inputs, _ptr(labels), objects, capacity, _ref(n)))
        return rc, n.value if count else None, objects

    def process_frame_host(self, disparity_now, disparity_prev, flow, transform, dt, cloud=None, labels=None, capacity=0, count=True):
        """mod_process_frame_host: one frame -> (rc, n, objects); cloud (H, W, 8) float32 and labels (H, W) int32 are written in place
        when given.  With neither labels nor objects nor the count (nor a cluster image set) the library does not cluster."""
        return self._clustered(self.lib.mod_process_frame_host, (_ptr(disparity_now), _ptr(disparity_prev), _ptr(flow),
                                                                 _ref(_transform(transform)), float(dt), _ptr(cloud)), labels, capacity, count)

    def cluster_cloud_host(self, cloud, labels=None, capacity=0, count=True, point_step=32, row_step=None, width=None, height=None):
        """mod_cluster_cloud_host: the clusterer alone on a PointCloud2 payload -> (rc, n, objects); width and height default to the
        context's, row_step to point_step * width."""
        w, h = self.width if width is None else int(width), self.height if height is None else int(height)
        step = point_step * w if row_step is None else int(row_step)
        return self._clustered(self.lib.mod_cluster_cloud_host, (_ptr(cloud), w, h, int(point_step), step), labels, capacity, count)

    # ---- a build with the debug hooks (csrc/mod_sf_debug.h) ----------------------------------------------------
    def _debug(self, name: str):
        fn = getattr(self.lib, name, None)
        if fn is None:
            raise RuntimeError(f"this build of the library does not export {name}: build it with the debug hooks (csrc/mod_sf_debug.h)")
        return fn

    def debug_counters(self) -> np.ndarray:
        """The 96 uint64 counters of a build with the debug hooks (mod_debug_counters); RuntimeError on a build without them."""
        out = np.zeros(96, dtype=np.uint64)
        self._check(self._debug("mod_debug_counters")(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def debug_read(self, which: int, array: np.ndarray) -> np.ndarray:
        """Internal buffer `which` of a build with the debug hooks into `array` (mod_debug_read, array.nbytes bytes); returns it."""
        self._check(self._debug("mod_debug_read")(self.h, int(which), _ptr(array), array.nbytes))
        return array
