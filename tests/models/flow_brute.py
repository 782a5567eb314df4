"""Scalar reference of the census optical flow, written from the prose of DESIGN.md sections 3.5 and 3.5a — not from
tests/models/flow_model.py, flow_prop_model.py or csrc/flow.hip, whose key packing and array tricks it does not share.
TEST INFRASTRUCTURE ONLY.

Plain Python over pixels, candidates and taps: the winner is the lexicographic minimum of the tuple (cost, |ex| + |ey|, raster
index), five seeds are a loop with a strict "lower cost wins", the sub-pixel delta is the exact rational num / (2 den) rounded once
to float32 and then clamped, NaN is the quiet NaN 0x7fc00000.  Census words come from oracle.sgm_numpy.census (pinned elsewhere).
Slow: meant for images of a few thousand pixels.

`rules` names deviations from the documented behaviour — the plausible mistakes.  tests/test_flow_cases.py shows that the hostile
cases tell every one of them from the default, so a kernel (or model) that made the mistake could not equal the reference there.
"""
from __future__ import annotations

import os
import sys
from fractions import Fraction

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle.sgm_numpy import census  # noqa: E402

RULES = {
    "out_cost_30": "a prev sample outside the image costs 30 instead of 31",
    "tap_outside_31": "a window tap outside the image costs 31 instead of 0",
    "tap_outside_scored": "a window tap outside the image is scored like one inside, with a census word of 0, instead of adding 0",
    "no_l1_term": "ties broken by the raster index alone, without |ex| + |ey|",
    "last_raster_index": "ties (after |ex| + |ey|) go to the last candidate in raster order",
    "seed_tie_to_higher": "of two seeds with the same cost the higher one wins",
    "parent_wraps": "the parent of the last odd column / row is x >> 1 modulo W1 instead of min(x >> 1, W1 - 1)",
    "one_sided_on_the_rim": "a winner without an evaluated neighbour on one side takes its own cost for it (one-sided difference)",
    "den0_minus_half": "den <= 0 gives -0.5 instead of 0",
    "fb_strict": "the forward-backward test passes on < t instead of <= t",
    "outside_passes": "a prev position outside the image passes the forward-backward check",
}
SEED_OFFSETS = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))
QUIET_NAN = 0x7FC00000


def _pyramid(img, levels):
    out = [[[int(v) for v in row] for row in img]]
    for _ in range(1, levels):
        a = out[-1]
        h, w = len(a) >> 1, len(a[0]) >> 1
        out.append([[(a[2 * y][2 * x] + a[2 * y][2 * x + 1] + a[2 * y + 1][2 * x] + a[2 * y + 1][2 * x + 1] + 2) >> 2 for x in range(w)]
                    for y in range(h)])
    return out


def _census(img):
    return [[int(v) for v in row] for row in census(np.array(img, np.uint8))]


class _Level:
    """Costs of one level in one direction: cn is searched for in cp."""

    def __init__(self, cn, cp, window, rules):
        self.cn, self.cp, self.H, self.W = cn, cp, len(cn), len(cn[0])
        self.r = window // 2
        self.out_cost = 30 if "out_cost_30" in rules else 31
        self.tap_outside = 31 if "tap_outside_31" in rules else 0
        self.tap_scored = "tap_outside_scored" in rules
        self.taps, self.found = {}, {}

    def _tap_plane(self, dx, dy):
        """For every tap position q inside the image: popcount(cn(q) ^ cp(q - d)), or the outside cost where q - d leaves the image."""
        W, H, cn, cp = self.W, self.H, self.cn, self.cp
        plane = []
        for qy in range(H):
            py = qy - dy
            row = []
            for qx in range(W):
                px = qx - dx
                row.append(bin(cn[qy][qx] ^ cp[py][px]).count("1") if 0 <= px < W and 0 <= py < H else self.out_cost)
            plane.append(row)
        return plane

    def cost(self, x, y, dx, dy):
        plane = self.taps.get((dx, dy))
        if plane is None:
            plane = self.taps[(dx, dy)] = self._tap_plane(dx, dy)
        r, total, inside = self.r, 0, 0
        x0, x1 = max(x - r, 0), min(x + r, self.W - 1)
        for qy in range(max(y - r, 0), min(y + r, self.H - 1) + 1):      # the taps of the window that lie inside the image
            total += sum(plane[qy][x0:x1 + 1])
            inside += x1 + 1 - x0
        if self.tap_scored:
            for qy in range(y - r, y + r + 1):
                for qx in range(x - r, x + r + 1):
                    if not (0 <= qx < self.W and 0 <= qy < self.H):
                        px, py = qx - dx, qy - dy
                        total += bin(self.cp[py][px]).count("1") if 0 <= px < self.W and 0 <= py < self.H else self.out_cost
        return total + self.tap_outside * ((2 * r + 1) ** 2 - inside)

    def search(self, x, y, cx, cy, span, rules):
        """Winner over c + [-span, span]^2: (cost, dx, dy, sub) with sub = (num_x, den_x, num_y, den_y), None on an axis without both
        neighbours.  Remembered per (pixel, centre): the five seeds of a pixel mostly share one centre."""
        if (x, y, cx, cy) in self.found:
            return self.found[(x, y, cx, cy)]
        costs, best = {}, None
        idx = 0
        for ey in range(-span, span + 1):
            for ex in range(-span, span + 1):
                c = costs[(ex, ey)] = self.cost(x, y, cx + ex, cy + ey)
                l1 = 0 if "no_l1_term" in rules else abs(ex) + abs(ey)
                key = (c, l1, -idx if "last_raster_index" in rules else idx)
                if best is None or key < best[0]:
                    best = (key, ex, ey)
                idx += 1
        c0, bx, by = best[0][0], best[1], best[2]
        sub = []
        for ax, (lo, hi) in enumerate((((bx - 1, by), (bx + 1, by)), ((bx, by - 1), (bx, by + 1)))):
            cm, cq = costs.get(lo), costs.get(hi)
            if "one_sided_on_the_rim" in rules and (cm is None) != (cq is None):
                cm, cq = (c0 if cm is None else cm), (c0 if cq is None else cq)
            sub += [None, None] if cm is None or cq is None else [cm - cq, cm - 2 * c0 + cq]
        self.found[(x, y, cx, cy)] = c0, cx + bx, cy + by, tuple(sub)
        return self.found[(x, y, cx, cy)]


def _integer_flow(prev, now, levels, radius, window, seeds, rules):
    """Level-0 winners F[y][x] = (dx, dy) (indexed at `now`, prev = now - F) and their sub-pixel terms."""
    pn, pp = _pyramid(now, levels), _pyramid(prev, levels)
    F = sub = None
    for l in range(levels - 1, -1, -1):
        lev = _Level(_census(pn[l]), _census(pp[l]), window, rules)
        H, W = lev.H, lev.W
        G, gsub = [[None] * W for _ in range(H)], [[None] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                if l == levels - 1:
                    _, dx, dy, s = lev.search(x, y, 0, 0, radius, rules)
                    G[y][x], gsub[y][x] = (dx, dy), s
                    continue
                H1, W1 = len(F), len(F[0])
                if "parent_wraps" in rules:
                    X, Y = (x >> 1) % W1, (y >> 1) % H1
                else:
                    X, Y = min(x >> 1, W1 - 1), min(y >> 1, H1 - 1)
                win = None
                for ox, oy in SEED_OFFSETS[:seeds]:
                    fx, fy = F[min(max(Y + oy, 0), H1 - 1)][min(max(X + ox, 0), W1 - 1)]
                    found = lev.search(x, y, 2 * fx, 2 * fy, 1, rules)
                    if win is None or found[0] < win[0] or ("seed_tie_to_higher" in rules and found[0] == win[0]):
                        win = found
                G[y][x], gsub[y][x] = (win[1], win[2]), win[3]
        F, sub = G, gsub
    return F, sub


def _delta(num, den, rules):
    if num is None:
        return np.float32(0)
    if den <= 0:
        return np.float32(-0.5 if "den0_minus_half" in rules else 0)
    # |num| and den are below 2^12, so the exact quotient is never within a double's rounding of a float32 tie: rounding the
    # rational to double and then to float32 rounds it once
    d = np.float32(float(Fraction(num, 2 * den)))
    return min(max(d, np.float32(-0.5)), np.float32(0.5))


def flow(prev, now, levels=4, radius=4, window=5, subpixel=1, fb_check=1, seeds=1, rules=()):
    """Optical flow [H][W][2] float32 from `prev` to `now` (uint8 [H][W]); `rules`: names from RULES, default the documented behaviour."""
    rules = frozenset(rules)
    assert rules <= set(RULES) and seeds in (1, 5)
    H, W = len(now), len(now[0])
    F, sub = _integer_flow(prev, now, levels, radius, window, seeds, rules)
    G = _integer_flow(now, prev, levels, radius, window, seeds, rules)[0] if fb_check >= 0 else None
    bits = np.empty((H, W, 2), np.uint32)
    for y in range(H):
        for x in range(W):
            fx, fy = F[y][x]
            o = [np.float32(fx), np.float32(fy)]
            if subpixel:
                s = sub[y][x]
                o = [o[0] + _delta(s[0], s[1], rules), o[1] + _delta(s[2], s[3], rules)]
            ok = True
            if G is not None:
                px, py = x - fx, y - fy
                if 0 <= px < W and 0 <= py < H:
                    gx, gy = G[py][px]
                    if "fb_strict" in rules:
                        ok = abs(fx + gx) < fb_check and abs(fy + gy) < fb_check
                    else:
                        ok = abs(fx + gx) <= fb_check and abs(fy + gy) <= fb_check
                else:
                    ok = "outside_passes" in rules
            for i in range(2):
                bits[y, x, i] = np.array(o[i], np.float32).view(np.uint32) if ok else QUIET_NAN
    return bits.view(np.float32)
