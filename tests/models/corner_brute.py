"""Scalar reference of the min-eigenvalue rule, written from the prose of include/mod_sf.h and DESIGN.md section 3.5b — not from
tests/models/corner_model.py or csrc/corner.hip, whose padding, separable sums and floating-point root it does not share.  TEST
INFRASTRUCTURE ONLY.

Plain Python integers over pixels and window taps, math.isqrt for the root.  Slow: meant for images of a few hundred pixels."""
from __future__ import annotations

import math


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def tensor(I, w, c):
    """(S, D) as lists of rows of Python ints for an image given as rows of ints 0..255"""
    H, W = len(I), len(I[0])
    r = (w - 1) // 2

    def gx(x, y):
        return _clamp(int(I[y][min(x + 1, W - 1)]) - int(I[y][max(x - 1, 0)]), -c, c)

    def gy(x, y):
        return _clamp(int(I[min(y + 1, H - 1)][x]) - int(I[max(y - 1, 0)][x]), -c, c)

    S, D = [], []
    for y in range(H):
        rs, rd = [], []
        for x in range(W):
            A = B = C = 0
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    xx, yy = x + i, y + j
                    if 0 <= xx < W and 0 <= yy < H:
                        u, v = gx(xx, yy), gy(xx, yy)
                        A += u * u
                        B += u * v
                        C += v * v
            rs.append(A + C)
            rd.append((A - C) * (A - C) + 4 * B * B)
        S.append(rs)
        D.append(rd)
    return S, D


def strength(I, w, c):
    """E as a list of rows of Python ints"""
    S, D = tensor(I, w, c)
    out = []
    for rs, rd in zip(S, D):
        row = []
        for s, d in zip(rs, rd):
            q = math.isqrt(d)
            q += q * q < d                         # the smallest integer whose square is >= d
            assert s >= q
            row.append((s - q) >> 1)
        out.append(row)
    return out


def rejected(I, t, w, c):
    return [[e < t for e in row] for row in strength(I, w, c)]
