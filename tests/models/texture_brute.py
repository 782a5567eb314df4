"""Scalar reference of the texture rule, written from the prose of include/mod_sf.h and DESIGN.md section 3.4d — not from
tests/models/texture_model.py or csrc/texture.hip, whose padding and separable sums it does not share.  TEST INFRASTRUCTURE ONLY.

Plain Python over pixels and window taps.  Slow: meant for images of a few hundred pixels.

`rules` names deviations from the documented behaviour — the plausible mistakes.  tests/test_texture_model.py shows that the tiny
cases tell every one of them from the default, so a kernel (or model) that made the mistake could not equal the reference there."""
from __future__ import annotations

RULES = {
    "mirrored_border": "the column beyond the border is the mirrored one (I(-1) = I(1), I(W) = I(W - 2)) instead of the clamped one",
    "taps_clamped": "a window tap outside the image takes g of the clamped pixel instead of adding 0",
    "cap_on_sum": "the cap is applied to the window sum (w * w * c) instead of to every g",
    "reject_on_equal": "a pixel is rejected when T <= t instead of T < t",
}


def _column(x, W, mirrored):
    if 0 <= x < W:
        return x
    if not mirrored:
        return 0 if x < 0 else W - 1
    m = -x if x < 0 else 2 * (W - 1) - x
    return min(max(m, 0), W - 1)                 # (W = 1: there is nothing to mirror)


def texture(I, w, c, rules=()):
    """T as a list of rows of Python ints for an image given as rows of ints 0..255"""
    unknown = set(rules) - set(RULES)
    assert not unknown, unknown
    H, W = len(I), len(I[0])
    r = (w - 1) // 2
    mirrored = "mirrored_border" in rules

    def g(x, y):
        d = abs(int(I[y][_column(x + 1, W, mirrored)]) - int(I[y][_column(x - 1, W, mirrored)]))
        return d if "cap_on_sum" in rules else min(d, c)

    out = []
    for y in range(H):
        row = []
        for x in range(W):
            total = 0
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    xx, yy = x + i, y + j
                    if 0 <= xx < W and 0 <= yy < H:
                        total += g(xx, yy)
                    elif "taps_clamped" in rules:
                        total += g(min(max(xx, 0), W - 1), min(max(yy, 0), H - 1))
            row.append(min(total, w * w * c) if "cap_on_sum" in rules else total)
        out.append(row)
    return out


def rejected(I, t, w, c, rules=()):
    T = texture(I, w, c, rules)
    if "reject_on_equal" in rules:
        return [[v <= t for v in row] for row in T]
    return [[v < t for v in row] for row in T]
