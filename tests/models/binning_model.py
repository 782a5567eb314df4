"""Numpy restatement of k_bin_mono (csrc/binning.hip) on integers.  TEST INFRASTRUCTURE ONLY.

  - G is a full-resolution grey plane [.., by H, bx W] uint8 (what the path without binning makes of a camera of (bx W) x (by H));
  - bin_mean:    out(X, Y) = (sum over j < by, i < bx of G(bx X + i, by Y + j) + ((bx by) >> 1)) // (bx by)
  - bin_nearest: out(X, Y) = G(bx X, by Y)
  - the whole-path helpers compose ingest_model, yuv422_model, bayer_model and rectify_model at the FULL window with one of the two.
"""
from __future__ import annotations

import numpy as np

import bayer_model as bm
import rectify_model as rm
import yuv422_model as ym

MEAN, NEAREST = 0, 1


def _blocks(G, bx: int, by: int) -> np.ndarray:
    G = np.asarray(G)
    if G.dtype != np.uint8 or G.ndim < 2 or bx < 1 or by < 1 or G.shape[-2] % by or G.shape[-1] % bx:
        raise ValueError("G must be uint8 [.., by H, bx W]")
    H, W = G.shape[-2] // by, G.shape[-1] // bx
    return G.reshape(G.shape[:-2] + (H, by, W, bx))


def bin_mean(G, bx: int, by: int) -> np.ndarray:
    s = _blocks(G, bx, by).astype(np.int64).sum(axis=(-3, -1))
    return ((s + ((bx * by) >> 1)) // (bx * by)).astype(np.uint8)


def bin_nearest(G, bx: int, by: int) -> np.ndarray:
    return _blocks(G, bx, by)[..., :, 0, :, 0].copy()


def bin_grey(G, bx: int, by: int, mode: int) -> np.ndarray:
    if mode not in (MEAN, NEAREST):
        raise ValueError("unknown mode")
    return bin_mean(G, bx, by) if mode == MEAN else bin_nearest(G, bx, by)


def is_bayer(encoding) -> bool:
    return (encoding in bm.NAMES) if isinstance(encoding, str) else int(encoding) in bm.PATTERNS


def full_grey(buf, layout, W: int, H: int, bx: int, by: int, frames: int = 1, pane=None) -> np.ndarray:
    """the full-resolution grey window [frames][by H][bx W] of `frames` messages stacked in `buf` (of pane `pane` of each)"""
    if is_bayer(layout.encoding):
        return bm.to_mono(buf, layout, bx * W, by * H, frames, pane)
    return ym.to_mono(buf, layout, bx * W, by * H, frames, pane)


def to_mono(buf, layout, W: int, H: int, bx: int, by: int, mode: int, frames: int = 1, pane=None) -> np.ndarray:
    """mod_image_to_mono_dev with a binning set: grey planes [frames][H][W]"""
    return bin_grey(full_grey(buf, layout, W, H, bx, by, frames, pane), bx, by, mode)


def full_map(cal, layout, W: int, H: int, bx: int, by: int) -> np.ndarray:
    """mod_rectify_map_host with a binning set: the full window's map [by H][bx W][2]"""
    return rm.build_map(cal, layout.x0, layout.y0, bx * W, by * H)


def rectify(buf, layout, cal, W: int, H: int, bx: int, by: int, mode: int, frames: int = 1, pane=None) -> np.ndarray:
    """mod_rectify_dev with a binning set: the message (Bayer: its demosaic as mono8 of step width) sampled through the full window's
    map, then binned"""
    qmap = full_map(cal, layout, W, H, bx, by)
    if is_bayer(layout.encoding):
        grey = bm.demosaic_messages(buf, layout, frames, pane)
        full = ym.rectify(grey, ym.Layout("mono8", layout.width, layout.height, layout.width, layout.x0, layout.y0), qmap, frames)
    else:
        full = ym.rectify(buf, layout, qmap, frames, pane)
    return bin_grey(full, bx, by, mode)
