"""Numpy restatement of k_to_mono and k_rectify's sampling (csrc/ingest.hip, csrc/rectify.hip) for the packed
YUV 4:2:2 encodings and for one pane of a side-by-side message.  TEST INFRASTRUCTURE ONLY.  Extends ingest_model.py (encodings,
layouts, grey) and rectify_model.py (maps, taps) by import; every byte is fetched by its address in the message:

  - yuv422 is UYVY (bytes U0 Y0 V0 Y1: the luma of pixel x is byte 2x + 1 of its row), yuv422_yuy2 is YUYV (Y0 U0 Y1 V0: byte 2x);
    two bytes per pixel, step >= 2 * width; grey = Y, unchanged; chroma is never read; any width and x0, odd ones included;
  - under rectification Y is one channel, interpolated like mono8;
  - side by side (pane = 0 left, 1 right; None: a plain message): the layout's width and height are ONE eye's, step is the whole
    row's (>= 2 * width * C), the pane of eye e starts at byte e * width * C of every row, (x0, y0) is the window inside the pane; a tap
    outside the pane reads 0, never the other eye's pixel.
"""
from __future__ import annotations

import numpy as np

import ingest_model as im
import rectify_model as rm

YUV422, YUV422_YUY2 = 5, 6
NAMES = dict(im.NAMES, yuv422=YUV422, yuv422_yuy2=YUV422_YUY2)
CHANNELS = dict(im.CHANNELS)                    # bytes per pixel
CHANNELS.update({YUV422: 2, YUV422_YUY2: 2})
GREY_AT = {im.MONO8: 0, YUV422: 1, YUV422_YUY2: 0}   # one grey channel: its byte within a pixel
Layout = im.Layout


def encoding_of(e) -> int:
    return NAMES[e] if isinstance(e, str) else int(e)


def check(layout, W: int, H: int, pane=None) -> None:
    enc = encoding_of(layout.encoding)
    if enc not in CHANNELS:
        raise ValueError("unknown encoding")
    if pane not in (None, 0, 1):
        raise ValueError("pane must be None, 0 or 1")
    if layout.width < 1 or layout.height < 1 or layout.step < (1 if pane is None else 2) * layout.width * CHANNELS[enc]:
        raise ValueError("step is too small for the row")
    if layout.x0 < 0 or layout.y0 < 0 or layout.x0 + W > layout.width or layout.y0 + H > layout.height:
        raise ValueError("the window does not fit inside the image")


def _rows(buf, layout, frames):
    a = np.frombuffer(bytes(buf) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).tobytes(), np.uint8)
    need = frames * layout.step * layout.height
    if a.size < need:
        raise ValueError("buffer smaller than frames * step * height")
    return a[:need].reshape(frames, layout.height, layout.step).astype(np.int64)


def _finish(enc, channel) -> np.ndarray:
    """grey from channel(k) -> the plane of byte k of every pixel"""
    if enc in GREY_AT:
        return channel(GREY_AT[enc]).astype(np.uint8)
    b, g, r = im.ORDER[enc]
    return im.grey(channel(b), channel(g), channel(r))


def to_mono(buf, layout, W: int, H: int, frames: int = 1, pane=None) -> np.ndarray:
    """k_to_mono: grey planes [frames][H][W] uint8 of the window of `frames` messages stacked in `buf` (of pane `pane` of each)."""
    check(layout, W, H, pane)
    enc = encoding_of(layout.encoding)
    C = CHANNELS[enc]
    a = _rows(buf, layout, frames)
    first = (pane or 0) * layout.width * C + (layout.x0 + np.arange(W)) * C      # byte of each window pixel within its row
    rows = a[:, layout.y0:layout.y0 + H, :]
    return _finish(enc, lambda k: rows[:, :, first + k])


def rectify(buf, layout, qmap, frames: int = 1, pane=None) -> np.ndarray:
    """k_rectify: grey planes [frames][H][W] uint8 sampled through `qmap` (rectify_model.build_map) from the width x height message,
    or from pane `pane` of a side-by-side message."""
    check(layout, 0, 0, pane)
    enc = encoding_of(layout.encoding)
    C = CHANNELS[enc]
    a = _rows(buf, layout, frames)
    base = (pane or 0) * layout.width * C
    ix, iy, ax, ay, inside = rm.taps(qmap, layout.width, layout.height)

    def channel(k):
        t = []
        for (dy, dx), ok in zip(((0, 0), (0, 1), (1, 0), (1, 1)), inside):
            xx = np.clip(ix + dx, 0, layout.width - 1)
            yy = np.clip(iy + dy, 0, layout.height - 1)
            t.append(np.where(ok[None], a[:, yy, base + xx * C + k], 0))
        top = (32 - ax) * t[0] + ax * t[1]
        bot = (32 - ax) * t[2] + ax * t[3]
        return ((32 - ay) * top + ay * bot + 512) >> 10

    return _finish(enc, channel)


def cut_pane(buf, layout, pane: int, frames: int = 1):
    """The pane of a side-by-side message as a message of its own, rows packed: (uint8 [frames][height][width * C], its Layout)."""
    check(layout, 0, 0, pane)
    C = CHANNELS[encoding_of(layout.encoding)]
    row = layout.width * C
    a = _rows(buf, layout, frames)[:, :, pane * row:(pane + 1) * row].astype(np.uint8)
    return np.ascontiguousarray(a), layout._replace(step=row)
