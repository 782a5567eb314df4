"""numpy restatement of k_depth_temporal (csrc/depth_temporal.hip; include/mod_sf.h, "The temporal depth filter with hold"): consecutive
depth messages in, depth messages of the same layout out, word for word, with the per-pixel state (s, age) carried along.  All
np.float32, one operation at a time (numpy contracts nothing): the gate is one multiply, then one add; the average is subtract,
multiply, add.  z and valid0 are depth_model's (the rule of the depth path itself), not restated here.  Besides the messages and the
state, filter_messages returns how often each branch of the rule was taken, so that a test can assert that it exercised what it means to."""
from dataclasses import dataclass

import numpy as np

import depth_model as dm

WORD = {0: "<u2", 1: "<u4"}
EMPTY = 255
COUNTERS = ("started", "blended", "restarted", "held", "expired", "passed", "ties", "clamped")


@dataclass
class Temporal:
    alpha: float = 0.4
    delta_abs: float = 0.02
    delta_rel: float = 0.0
    hold: int = 0


def words(buf, lay, frames=1):
    """the samples' raw words [frames][height][width] (uint16 / uint32)"""
    b = np.ascontiguousarray(buf).view(np.uint8).reshape(frames, lay.height, lay.step)
    return np.ascontiguousarray(b[:, :, :lay.width * dm.BYTES[lay.enc]]).view(WORD[lay.enc])


def empty_state(lay):
    """(s, age) of a state that holds nothing: [height][width] float32 zeros and uint8 255"""
    return np.zeros((lay.height, lay.width), np.float32), np.full((lay.height, lay.width), EMPTY, np.uint8)


def enc(s, e, counters=None, where=None):
    """the output word of an average s: 16UC1 rounds to nearest even and clamps to 1 .. 65535, 32FC1 is the bits of s"""
    if e == 1:
        return s.astype(np.float32).view(np.uint32)
    with np.errstate(all="ignore"):
        r = np.rint(s)                                             # ties to even
        c = np.fmin(np.fmax(r, np.float32(1.0)), np.float32(65535.0))   # fmaxf / fminf: a NaN gives the other operand
        if counters is not None:
            counters["ties"] += int(np.count_nonzero(where & (np.abs(s - np.trunc(s)) == np.float32(0.5))))
            counters["clamped"] += int(np.count_nonzero(where & ~(c == r)))
    return c.astype(np.uint16)


def filter_messages(buf, lay, prm, frames=1, state=None):
    """(messages uint8 [frames][height][step], (s, age), counters).  state None: empty; the given planes are not modified.  Bytes of a
    row beyond width samples (not defined) are the input's."""
    f32 = np.float32
    e = lay.enc
    alpha, dabs, drel, hold = f32(prm.alpha), f32(prm.delta_abs), f32(prm.delta_rel), int(prm.hold)
    unit = dm.unit_of(lay)
    s, age = empty_state(lay) if state is None else (np.array(state[0], np.float32).reshape(lay.height, lay.width),
                                                     np.array(state[1], np.uint8).reshape(lay.height, lay.width))
    out = np.ascontiguousarray(buf).view(np.uint8).reshape(frames, lay.height, lay.step).copy()
    w_all = words(buf, lay, frames)
    n = dict.fromkeys(COUNTERS, 0)
    for f in range(frames):
        w = w_all[f]
        with np.errstate(all="ignore"):
            x = w.astype(f32) if e == 0 else w.view(f32)
            z = x * unit
            v = dm.valid(z)
            has = age != EMPTY
            zs = s * unit
            prod = drel * zs                                       # one multiply ...
            t = dabs + prod                                        # ... then one add
            near = np.abs(z - zs) <= t                             # a NaN compares false
            d = x - s
            ad = alpha * d
            avg = s + ad
            assert all(a.dtype == np.float32 for a in (x, z, zs, prod, t, d, ad, avg))
        start, blend, restart = v & ~has, v & has & near, v & has & ~near
        hold_ = ~v & has & (age < hold)
        drop = ~v & ~hold_
        n["started"] += int(start.sum()); n["blended"] += int(blend.sum()); n["restarted"] += int(restart.sum())
        n["held"] += int(hold_.sum()); n["expired"] += int((drop & has).sum()); n["passed"] += int((drop & ~has).sum())
        s = np.where(blend, avg, np.where(v, x, np.where(hold_, s, f32(0.0)))).astype(f32)
        age = np.where(v, 0, np.where(hold_, age.astype(np.int32) + 1, EMPTY)).astype(np.uint8)
        coded = blend | restart | hold_                            # the outputs that are enc(s); the others are the input word
        res = np.where(coded, enc(s, e, n, coded), w).astype(WORD[e])
        out[f, :, :lay.width * dm.BYTES[e]] = res.view(np.uint8).reshape(lay.height, -1)
    return out, (s, age), n
