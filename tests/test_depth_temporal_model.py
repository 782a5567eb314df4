"""CPU: tests/models/depth_temporal_model.py, the restatement of the temporal depth filter's rule (include/mod_sf.h), against a scalar
pure-Python loop that follows the header's text line by line; the identity at alpha = 1, hold = 0; that only hold > 0 fills a hole; and
the exponential average's steady state, whose variance ratio alpha / (2 - alpha) is derived, not measured."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_model as dm  # noqa: E402
import depth_temporal_model as dtm  # noqa: E402
import depth_temporal_cases as tc  # noqa: E402

f32 = np.float32


def _scalar(buf, lay, prm, frames):
    """the header's rule, one pixel and one frame at a time"""
    e = lay.enc
    unit = dm.unit_of(lay)
    alpha, dabs, drel = f32(prm.alpha), f32(prm.delta_abs), f32(prm.delta_rel)
    w = dtm.words(buf, lay, frames)
    out = w.copy()
    s = [[f32(0.0)] * lay.width for _ in range(lay.height)]
    age = [[255] * lay.width for _ in range(lay.height)]

    def enc(v):
        if e == 1:
            return np.array([v], f32).view(np.uint32)[0]
        r = f32(np.rint(v))
        return np.uint16(min(max(r, f32(1.0)), f32(65535.0)))

    with np.errstate(all="ignore"):
        for f in range(frames):
            for y in range(lay.height):
                for x_ in range(lay.width):
                    word = w[f, y, x_]
                    x = f32(word) if e == 0 else np.array([word], np.uint32).view(f32)[0]
                    z = f32(x * unit)
                    if z > 0 and np.isfinite(z):
                        if age[y][x_] == 255:
                            s[y][x_] = x
                        else:
                            zs = f32(s[y][x_] * unit)
                            t = f32(dabs + f32(drel * zs))
                            if abs(f32(z - zs)) <= t:
                                s[y][x_] = f32(s[y][x_] + f32(alpha * f32(x - s[y][x_])))
                            else:
                                s[y][x_] = x
                            out[f, y, x_] = enc(s[y][x_])
                        age[y][x_] = 0
                    elif age[y][x_] != 255 and age[y][x_] < prm.hold:
                        age[y][x_] += 1
                        out[f, y, x_] = enc(s[y][x_])
                    else:
                        age[y][x_] = 255
                        s[y][x_] = f32(0.0)
    return out, np.array(s, f32), np.array(age, np.uint8)


@pytest.mark.parametrize("hold", [0, 2])
@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_the_model_is_the_scalar_loop(encoding, hold):
    msg, lay = tc.sequence(encoding, 7, 5, 6, padded=True, seed=3)
    prm = dtm.Temporal(0.5, 0.004, 0.002, hold)
    out, (s, age), n = dtm.filter_messages(msg, lay, prm, 6)
    want, ws, wage = _scalar(msg, lay, prm, 6)
    assert dtm.words(out, lay, 6).tobytes() == want.tobytes()
    assert s.tobytes() == ws.tobytes() and age.tobytes() == wage.tobytes()
    assert n["started"] > 0 and n["blended"] > 0 and n["restarted"] > 0 and n["passed"] > 0, n
    assert (n["held"] > 0 and n["expired"] > 0) if hold else n["held"] == 0, n


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_alpha_one_without_hold_is_the_identity(encoding):
    msg, lay = tc.sequence(encoding, 37, 9, 5, padded=True, seed=4)
    out, _, n = dtm.filter_messages(msg, lay, dtm.Temporal(1.0, 0.004, 0.002, 0), 5)
    assert out.tobytes() == np.ascontiguousarray(msg).tobytes()
    assert n["blended"] > 0 and n["restarted"] > 0 and n["passed"] > 0 and n["held"] == 0, n


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_only_a_hold_fills_a_hole(encoding):
    msg, lay = tc.sequence(encoding, 37, 9, 5, padded=False, seed=5)
    v_in = dm.valid(dm.samples(msg, lay, 5))
    out0, _, _ = dtm.filter_messages(msg, lay, dtm.Temporal(0.5, 0.004, 0.002, 0), 5)
    assert (dm.valid(dm.samples(out0, lay, 5)) == v_in).all()
    out2, _, n = dtm.filter_messages(msg, lay, dtm.Temporal(0.5, 0.004, 0.002, 2), 5)
    v_out = dm.valid(dm.samples(out2, lay, 5))
    assert (v_out | ~v_in).all() and int((v_out & ~v_in).sum()) == n["held"] > 0


def test_the_state_carries_from_call_to_call():
    msg, lay = tc.sequence("16UC1", 37, 9, 5, padded=True, seed=6)
    prm = dtm.Temporal(0.5, 0.004, 0.002, 2)
    whole, st, _ = dtm.filter_messages(msg, lay, prm, 5)
    state, parts = None, []
    for f in range(5):
        o, state, _ = dtm.filter_messages(msg[f:f + 1], lay, prm, 1, state)
        parts.append(o)
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    assert state[0].tobytes() == st[0].tobytes() and state[1].tobytes() == st[1].tobytes()


def test_the_averages_steady_state_variance():
    """A static 32FC1 scene with Gaussian noise and a gate that never trips: s_n = (1 - a) s_(n-1) + a x_n has, once the start has
    decayed ((1 - a)^80 here), the variance a^2 / (1 - (1 - a)^2) = a / (2 - a) of the input's.  Compared within 15 %: the sampling
    error of a variance estimate from 4096 samples is sqrt(2 / 4095) = 2.2 %."""
    W = H = 64
    frames, alpha, sigma = 40, 0.4, 0.004
    rng = np.random.default_rng(7)
    x = (2.0 + sigma * rng.standard_normal((frames, H, W))).astype(f32)
    lay = dm.Layout("32FC1", W, H, 4 * W)
    out, _, n = dtm.filter_messages(x.view(np.uint8).reshape(frames, H, 4 * W), lay, dtm.Temporal(alpha, 1.0, 0.0, 0), frames)
    assert n["restarted"] == 0 and n["blended"] == (frames - 1) * W * H and n["started"] == W * H, n
    y = dtm.words(out, lay, frames).view(f32)[-1].astype(np.float64)
    ratio = y.var() / x[-1].astype(np.float64).var()
    want = alpha / (2.0 - alpha)
    assert abs(ratio - want) <= 0.15 * want, (ratio, want)
