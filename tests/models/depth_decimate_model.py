"""numpy restatement of k_depth_decimate (csrc/depth_decimate.hip; include/mod_sf.h, "The depth decimation"): depth messages in, packed
depth messages of the same encoding out, word for word.  All np.float32, one operation at a time (numpy contracts nothing).  z and
valid0 are depth_model's, words / raw / enc depth_spatial_model's (the rule of the depth path itself), not restated here.

The rule.  All arithmetic is F32, one operation at a time, no contraction.  x, z = x * unit, valid0 (z > 0 and finite) and enc(m) are
those of the spatial stage.
  Output sample (X, Y) reads the block of message pixels (x0 + dx X + i, y0 + dy Y + j), i < dx, j < dy.  "Row-major order" is j
  ascending, then i ascending.  V is the set of the block's samples with valid0.  The "no reading" word is 0 for 16UC1 and
  0x7fc00000 for 32FC1.
  MOD_DEPTH_DECIMATE_MEDIAN (0, the default).  If |V| < max(min_valid, 1): no reading.  Otherwise sort V ascending by
    (z, row-major index).  The output is the INPUT WORD of element (|V| - 1) / 2, the lower median.  Every valid output word is one
    of the block's input words.
  MOD_DEPTH_DECIMATE_MIN (1).  Same min_valid test.  The output is the input word of the first element of that order, the nearest
    surface.  This is the z-buffer's rule, what the registered path does when several samples land on one pixel.
  MOD_DEPTH_DECIMATE_MEAN (2).  Same min_valid test.  a = the z of the lower median.  t = tol_abs + tol_rel * a, one multiply and
    then one add.  Members are the q in V with fabsf(z_q - a) <= t.  The median itself is always a member.
    sum = 0.0f; sum = sum + x_q, member by member in row-major order.  m = sum / (float)n.  The output is enc(m).
    For 16UC1 the sum is exact, because 16 * 65535 < 2^24.
  MOD_DEPTH_DECIMATE_NEAREST (3).  The output is the block's top-left input word, bit for bit, whatever it is.  This is
    crop_decimate's default.  min_valid and the tolerances are ignored.
  dx = dy = 1, or a NULL struct, means the stage is off.  The stage alone then copies the window's words bit for bit."""
from dataclasses import dataclass

import numpy as np

import depth_model as dm
import depth_spatial_model as dsm

MEDIAN, MIN, MEAN, NEAREST = 0, 1, 2, 3
MODES = {"median": MEDIAN, "min": MIN, "mean": MEAN, "nearest": NEAREST}
NO_READING = {0: np.uint16(0), 1: np.uint32(0x7FC00000)}


@dataclass
class Decimation:
    dx: int = 2
    dy: int = 2
    mode: int = MEDIAN
    min_valid: int = 1
    tol_abs: float = 0.0
    tol_rel: float = 0.02


def out_size(lay, d):
    return (lay.width - lay.x0) // d.dx, (lay.height - lay.y0) // d.dy


def blocks(a, lay, d):
    """[frames][height][width] -> [frames][out_h][out_w][dy * dx]: the blocks' samples in row-major order"""
    ow, oh = out_size(lay, d)
    win = a[:, lay.y0:lay.y0 + d.dy * oh, lay.x0:lay.x0 + d.dx * ow]
    return win.reshape(a.shape[0], oh, d.dy, ow, d.dx).transpose(0, 1, 3, 2, 4).reshape(a.shape[0], oh, ow, d.dy * d.dx)


def evaluate(buf, lay, d, frames=1):
    """dict of [frames][out_h][out_w] arrays: `out` the output words, `count` = |V|, `reading` (the min_valid test passed; NEAREST:
    the word has valid0), `n` MEAN's members"""
    f32 = np.float32
    assert 1 <= d.dx <= 4 and 1 <= d.dy <= 4 and 0 <= d.min_valid <= d.dx * d.dy
    unit = dm.unit_of(lay)
    w = blocks(dsm.words(buf, lay, frames), lay, d)
    x = blocks(dsm.raw(buf, lay, frames), lay, d)
    with np.errstate(all="ignore"):
        z = x * unit
        assert z.dtype == np.float32
        ok = dm.valid(z)
        count = ok.sum(axis=-1)
        if d.mode == NEAREST or d.dx * d.dy == 1:
            return {"out": w[..., 0].copy(), "count": count, "reading": ok[..., 0], "n": np.zeros(count.shape, np.int32)}
        enough = count >= max(d.min_valid, 1)
        # ascending by (z, row-major index): a stable sort of z with the samples outside V behind every member of it
        key = np.where(ok, z, f32(np.inf))
        order = np.argsort(key, axis=-1, kind="stable")
        # (inf never is a valid z, so V's elements come first, ties in row-major order)
        pos = np.where(d.mode == MIN, 0, (np.maximum(count, 1) - 1) // 2)
        pick = np.take_along_axis(order, pos[..., None], axis=-1)
        word = np.take_along_axis(w, pick, axis=-1)[..., 0]
        n = np.zeros(count.shape, np.int32)
        if d.mode == MEAN:
            a = np.take_along_axis(z, pick, axis=-1)                       # the z of the lower median
            prod = f32(d.tol_rel) * a                                      # one multiply ...
            t = f32(d.tol_abs) + prod                                      # ... then one add
            assert t.dtype == np.float32
            member = ok & (np.abs(z - a) <= t)
            s = np.zeros(count.shape, f32)
            for k in range(d.dx * d.dy):                                   # row-major order
                s = np.where(member[..., k], s + x[..., k], s)
            assert s.dtype == np.float32
            n = member.sum(axis=-1).astype(np.int32)
            m = s / n.astype(f32)
            assert m.dtype == np.float32
            word = dsm.enc(m, lay.enc)
        out = np.where(enough, word, NO_READING[lay.enc]).astype(dsm.WORD[lay.enc])
    return {"out": out, "count": count, "reading": enough, "n": np.where(enough, n, 0)}


def decimate_messages(buf, lay, d, frames=1):
    """the output messages, packed: uint8 [frames][out_h][out_w * B]; d None: the stage off, the window's words"""
    if d is None:
        d = Decimation(1, 1)
    out = evaluate(buf, lay, d, frames)["out"]
    return np.ascontiguousarray(out).view(np.uint8).reshape(frames, out.shape[1], -1)


def decimated_layout(lay, d):
    """the layout of decimate_messages' result"""
    ow, oh = out_size(lay, d if d is not None else Decimation(1, 1))
    return dm.Layout(lay.encoding, ow, oh, ow * dm.BYTES[lay.enc], 0, 0, lay.unit)
