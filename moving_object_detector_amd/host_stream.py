"""One Python driver of the host frame stream (include/mod_sf.h: mod_submit_*_host, mod_collect_frame_host, mod_forget_previous) for
tests and tools (host_calls.HostCalls has the synchronous calls).  It adds nothing to the library: no threads, no torch, and the raw
``ctx.lib.mod_*`` route stays open to whoever wants to misuse the ABI on purpose."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import capi
from .host_calls import _ptr, _ref, _transform, objects_bytes

_SHAPES = {"cloud": ((8,), np.float32), "labels": ((), np.int32), "disparity": ((), np.float32), "flow": ((2,), np.float32)}


class HostStream:
    """The host buffers of `frames` frame indices and the ticket queue of one context (anything with lib, h, width, height).

    Per frame index: the (H, W[, k]) arrays named in `outputs` (attributes cloud, labels, disparity, flow: (frames, H, W[, k]), filled
    with `fill`; an output not named is None and goes to the library as NULL), `capacity` ModObject records (objects[f]; capacity 0:
    NULL), a ModTransform (transforms[f], built from `transform`'s (t, q) if given) and a ModEgoResult (ego[f], from `ego`'s fields).
    pinned=True takes the arrays from Context.pinned_copy.

    Every submit_* first collects the oldest ticket when MOD_PIPELINE_DEPTH are outstanding, stores the call's return code in first[f],
    queues the ticket on 0, raises capi.ModError on a negative code and returns the code.  collect() records rc[f] and n[f].

    The driver owns every buffer a ticket writes until that ticket is collected: the result stream writes them until then, so the
    arrays, objects_bytes(f), transform_bytes(f), ego_bytes(f) mean something for frame f only after its collect (finish() collects
    all), and a frame index cannot be submitted again while its ticket is outstanding."""

    def __init__(self, ctx, frames, capacity, outputs=("cloud", "labels", "disparity", "flow"), fill=-7, transform=None, ego=None,
                 before_collect=None, pinned=False):
        self.ctx, self.capacity, self.before_collect = ctx, capacity, before_collect
        H, W = ctx.height, ctx.width
        for k, (tail, dtype) in _SHAPES.items():
            a = np.full((frames, H, W) + tail, fill, dtype) if k in outputs else None
            if a is not None and pinned:
                a = ctx.pinned_copy(a).array
            setattr(self, k, a)
        self.objects = [(capi.ModObject * capacity)() if capacity else None for _ in range(frames)]
        self.transforms = [capi.ModTransform(*transform) if transform else capi.ModTransform() for _ in range(frames)]
        self.ego = [capi.ModEgoResult(*ego) if ego else capi.ModEgoResult() for _ in range(frames)]
        self.first, self.rc, self.n = [None] * frames, [None] * frames, [0] * frames
        self._pending, self._busy = [], [False] * frames
        self._ticket, self._count = C.c_int32(-1), C.c_int32(-1)
        at = lambda a, f: a[f].ctypes.data if a is not None else None   # noqa: E731
        # per frame: cloud_aos, labels, objects, max_objects | disparity | flow_out | transform_out, ego_out
        self._out = [((at(self.cloud, f), at(self.labels, f), self.objects[f], capacity), at(self.disparity, f), at(self.flow, f),
                      (C.byref(self.transforms[f]), C.byref(self.ego[f]))) for f in range(frames)]

    # ---- the stream -------------------------------------------------------------------------------------------
    def make_room(self):
        """Collect the oldest ticket if MOD_PIPELINE_DEPTH are outstanding: what every submit does first (a caller that changes a
        setting in front of a submit calls it ahead of the change, so that the collect sees the old setting)."""
        if len(self._pending) == capi.MOD_PIPELINE_DEPTH:
            self.collect()

    def _submit(self, f, fn, *args):
        self.make_room()
        if self._busy[f]:
            raise ValueError(f"frame {f} has a ticket outstanding: its buffers are the result stream's")
        rc = fn(self.ctx.h, *args, C.byref(self._ticket))
        self.first[f] = rc
        if rc == 0:
            self._pending.append((self._ticket.value, f))
            self._busy[f] = True
        elif rc < 0:
            raise capi.ModError(rc, self.ctx.lib.mod_last_error(self.ctx.h).decode())
        return rc

    def submit_frame(self, f, disparity_now, disparity_prev, flow, transform, dt):
        tail, _, _, _ = self._out[f]
        return self._submit(f, self.ctx.lib.mod_submit_frame_host, _ptr(disparity_now), _ptr(disparity_prev), _ptr(flow),
                            _ref(_transform(transform)), dt, *tail)

    def submit_stereo(self, f, left, right, sgm, flow, transform, dt):
        tail, disp, _, _ = self._out[f]
        return self._submit(f, self.ctx.lib.mod_submit_stereo_host, _ptr(left), _ptr(right), _ref(sgm), _ptr(flow),
                            _ref(_transform(transform)), dt, *tail, disp)

    def submit_images(self, f, left, right, sgm, flow_prm, transform, dt):
        tail, disp, flow, _ = self._out[f]
        return self._submit(f, self.ctx.lib.mod_submit_images_host, _ptr(left), _ptr(right), _ref(sgm), _ref(flow_prm),
                            _ref(_transform(transform)), dt, *tail, disp, flow)

    def submit_odometry(self, f, left, right, sgm, flow_prm, ego_prm, dt):
        tail, disp, flow, est = self._out[f]
        return self._submit(f, self.ctx.lib.mod_submit_odometry_host, _ptr(left), _ptr(right), _ref(sgm), _ref(flow_prm), _ref(ego_prm),
                            dt, *tail, disp, flow, *est)

    def submit_depth(self, f, image, depth, flow_prm, ego_prm, transform, dt):
        tail, disp, flow, est = self._out[f]
        return self._submit(f, self.ctx.lib.mod_submit_depth_host, _ptr(image), _ptr(depth), _ref(flow_prm), _ref(ego_prm),
                            _ref(_transform(transform)), dt, *tail, disp, flow, *est)

    def collect(self):
        """Collect the oldest ticket."""
        if self.before_collect:
            self.before_collect()
        ticket, f = self._pending.pop(0)
        self._busy[f] = False
        rc = self.ctx.lib.mod_collect_frame_host(self.ctx.h, ticket, C.byref(self._count))
        self.rc[f], self.n[f] = rc, self._count.value
        if rc < 0:
            raise capi.ModError(rc, self.ctx.lib.mod_last_error(self.ctx.h).decode())

    def finish(self):
        while self._pending:
            self.collect()
        return self

    def forget_previous(self):
        rc = self.ctx.lib.mod_forget_previous(self.ctx.h)
        if rc != 0:
            raise capi.ModError(rc, self.ctx.lib.mod_last_error(self.ctx.h).decode())

    # ---- results (of collected frames) ------------------------------------------------------------------------
    def objects_bytes(self, f):
        """the records the library reported for frame f: the one slicing rule"""
        return objects_bytes(self.objects[f], self.n[f], self.capacity)

    def transform_bytes(self, f):
        return bytes(self.transforms[f])

    def ego_bytes(self, f):
        return bytes(self.ego[f])


def stream_rate(stream, step, frames, warmup=10, ok=(0,)):
    """Frames per second of `frames` calls of step(i), one submit on `stream` each, after `warmup` calls, the final drain included:
    the figure of tools/time_*.py.  The collects' codes (of the last frame of every index) must lie in `ok`."""
    for i in range(warmup):
        step(i)
    t0 = time.perf_counter()
    for i in range(warmup, warmup + frames):
        step(i)
    stream.finish()
    dt = time.perf_counter() - t0
    if any(rc is not None and rc not in ok for rc in stream.rc):
        raise RuntimeError(f"collect returned {stream.rc}")
    return frames / dt
