"""CPU: the numpy restatement of the on-GPU census optical flow (tests/models/flow_model.py, csrc/flow.hip) — exact on integer
translations up to the documented largest displacement, NaN where the forward-backward check fails, and pinned by a fixture."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import flow_model as fm  # noqa: E402

GOLD = os.path.join(HERE, "golden", "flow", "flow_320x240.npz")


def texture(H, W, seed):
    """Multi-scale (roughly 1/f) random texture: fine detail for level 0, coarse detail for the coarse levels."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((H, W), np.float32)
    for s in (1, 2, 4, 8, 16, 32):
        n = rng.standard_normal((H // s + 2, W // s + 2)).astype(np.float32)
        up = np.kron(n, np.ones((s, s), np.float32))[:H, :W]
        if s > 1:
            k = np.ones(s, np.float32) / s
            up = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, up)
            up = np.apply_along_axis(lambda c: np.convolve(c, k, mode="same"), 0, up)
        acc += up * np.sqrt(s)
    acc = (acc - acc.mean()) / acc.std()
    return np.clip(acc * 40 + 128, 0, 255).astype(np.uint8)


def translated(W, H, dx, dy, seed=1, pad=48):
    base = texture(H + 2 * pad, W + 2 * pad, seed)
    prev = base[pad:pad + H, pad:pad + W]
    now = base[pad - dy:pad - dy + H, pad - dx:pad - dx + W]           # now(x) = prev(x - d): flow d everywhere
    return np.ascontiguousarray(prev), np.ascontiguousarray(now)


def test_largest_displacement_is_39_px_at_the_defaults():
    p = fm.FlowParams()
    assert fm.max_displacement(p.levels, p.radius) == 39
    assert fm.max_displacement(1, 4) == 4 and fm.max_displacement(5, 2) == 47


def _interior(dx, dy, W=512, H=384):
    p = fm.FlowParams(subpixel=0)
    prev, now = translated(W, H, dx, dy)
    f = fm.flow(prev, now, p)
    # the border scales with the pyramid: a coarse-level window reaches (window/2 + 4) coarse pixels (its half-width plus the census
    # border, where the census word is 0), that many times 2^(levels-1) full-resolution pixels, plus the displacement itself
    b = (p.window // 2 + 4) * (1 << (p.levels - 1)) + max(abs(dx), abs(dy))
    inner = f[b:H - b, b:W - b]
    assert inner.size > 0
    return (inner[..., 0] == dx) & (inner[..., 1] == dy)


@pytest.mark.parametrize("dx,dy", [(0, 0), (8, -8), (-16, 24), (32, 0), (-32, 32)])
def test_translation_on_the_level_grid_is_recovered_exactly(dx, dy):
    """A displacement that is a multiple of 2^(levels-1) is an integer translation on every level: found exactly everywhere away
    from the border."""
    ok = _interior(dx, dy)
    assert ok.all(), (dx, dy, float(1 - ok.mean()))


@pytest.mark.parametrize("dx,dy", [(3, -2), (-12, 7), (25, -31), (36, 0), (-35, 35)])
def test_any_integer_translation_up_to_39_px(dx, dy):
    """Other displacements are fractional on the coarse levels, where a wrong winner cannot be undone by the +-1 refinement: still
    found on at least 99.9 % of the interior.  Right at the largest displacement (39 px at the defaults) the coarsest level must
    settle on its edge candidate, and there the share drops (5 - 13 % wrong at 39 px): a caller expecting such motion adds a level."""
    ok = _interior(dx, dy)
    assert ok.mean() >= 0.999, (dx, dy, float(1 - ok.mean()))


def test_subpixel_stays_within_half_a_pixel_of_the_winner():
    W, H = 256, 192
    prev, now = translated(W, H, 5, -3, seed=4)
    p = fm.FlowParams(fb_check=-1)
    fx, fy, _ = fm.integer_flow(prev, now, p)
    f = fm.flow(prev, now, p)
    assert np.all(np.abs(f[..., 0] - fx) <= 0.5) and np.all(np.abs(f[..., 1] - fy) <= 0.5)
    assert not np.isnan(f).any()


def test_forward_backward_check_marks_a_disoccluded_strip():
    """A strip that appears in `now` (covered in `prev` by a foreground band that moved away) has no consistent match: NaN."""
    W, H = 256, 192
    bg = texture(H, W, 7)
    fg = texture(H, W + 64, 8)
    prev = bg.copy()
    now = bg.copy()
    prev[:, 96:160] = fg[:, 96:160]                # a band over columns 96..159 in prev ...
    now[:, 120:184] = fg[:, 96:160]                # ... moved 24 px to the right in now: columns 96..119 of now are disoccluded
    f = fm.flow(prev, now, fm.FlowParams())
    strip = f[40:H - 40, 100:116]
    assert np.isnan(strip).all(axis=2).mean() > 0.9, float(np.isnan(strip).all(axis=2).mean())
    assert (np.isnan(f[..., 0]) == np.isnan(f[..., 1])).all()       # both components or neither
    far = f[40:H - 40, 8:60]
    assert (~np.isnan(far[..., 0])).mean() > 0.9
    off = fm.flow(prev, now, fm.FlowParams(fb_check=-1))
    assert not np.isnan(off).any()


def test_argument_checks():
    img = np.zeros((64, 64), np.uint8)
    with pytest.raises(ValueError):
        fm.flow(img, img, fm.FlowParams(levels=4))                  # coarsest 8 x 8 < 16
    with pytest.raises(ValueError):
        fm.flow(img, img, fm.FlowParams(levels=1, window=4))


def test_model_reproduces_the_fixture():
    g = np.load(GOLD)
    for k in range(int(g["pairs"])):
        p = fm.FlowParams(*[int(v) for v in g["params"][k]])
        got = fm.flow(g["prev"][k], g["now"][k], p)
        want = g["flow"][k]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
