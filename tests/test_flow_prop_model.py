"""CPU: the numpy restatement of the optical flow with neighbour-seed propagation (tests/models/flow_prop_model.py, csrc/flow.hip
k_flow_match_seeds) — flow_model bit for bit at seeds = 1, exact on a translation, pinned by a fixture, and the clamp of the parent
and of its neighbours pinned by hand."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, HERE)
import flow_model as fm  # noqa: E402
import flow_prop_model as fp  # noqa: E402

GOLD = os.path.join(HERE, "golden", "flow", "flow_prop_320x240.npz")


def _bits(a):
    return a.view(np.uint32)


def test_one_seed_is_flow_model_bit_for_bit():
    """150 x 77 at 3 levels: odd sizes on levels 0 and 1 (75 x 38, 37 x 19), so the parent clamps in x and in y."""
    from moving_object_detector_amd import synth
    m = synth.make_moving_images(150, 77, seed=5, n_boxes=2, shift=(4, 12))
    for kw in (dict(), dict(subpixel=0, fb_check=-1), dict(window=3, fb_check=0)):
        p = fm.FlowParams(levels=3, **kw)
        want, got = fm.flow(m["left0"], m["left1"], p), fp.flow(m["left0"], m["left1"], p, seeds=1)
        assert np.array_equal(_bits(got), _bits(want)), kw
    assert not np.array_equal(_bits(fp.flow(m["left0"], m["left1"], fm.FlowParams(levels=3), seeds=5)),
                              _bits(fm.flow(m["left0"], m["left1"], fm.FlowParams(levels=3))))      # and five seeds are not one


def test_translation_is_recovered_exactly_with_five_seeds():
    from test_flow_model import translated
    W, H, dx, dy = 256, 192, 8, -8
    p = fm.FlowParams(subpixel=0)
    prev, now = translated(W, H, dx, dy)
    f = fp.flow(prev, now, p, seeds=5)
    b = (p.window // 2 + 4) * (1 << (p.levels - 1)) + max(abs(dx), abs(dy))     # test_flow_model._interior's border
    inner = f[b:H - b, b:W - b]
    assert inner.size > 0
    assert ((inner[..., 0] == dx) & (inner[..., 1] == dy)).all()


def test_model_reproduces_the_fixture():
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(HERE, "golden", "flow", "flow_320x240.npz"))
    assert int(g["pairs"]) == 2 and int(g["seeds"]) == 5
    assert [tuple(int(v) for v in r[3:]) for r in g["params"]] == [(1, 1), (0, -1)]
    for k in range(int(g["pairs"])):
        p = fm.FlowParams(*[int(v) for v in g["params"][k]])
        got = fp.flow(g["prev"][k], g["now"][k], p, int(g["seeds"]))
        want = g["flow"][k]
        assert np.array_equal(_bits(got), _bits(want)), (k, int((_bits(got) != _bits(want)).sum()))


def test_parent_clamp_by_hand():
    """A 5-wide level over a 2-wide parent level: x = 4 has x >> 1 = 2, clamped to X = 1; its seeds sit at X = 1 (the parent), 0 (left),
    then 1 again for the right neighbour (clamped) and for the two vertical ones."""
    par, lo, hi = fp.seed_parents(5, 2)
    assert par.tolist() == [0, 0, 1, 1, 1]
    assert lo.tolist() == [0, 0, 0, 0, 0]
    assert hi.tolist() == [1, 1, 1, 1, 1]
    by_offset = {0: par, -1: lo, 1: hi}
    assert fp.SEED_OFFSETS == ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))
    assert [int(by_offset[ox][4]) for ox, _ in fp.SEED_OFFSETS] == [1, 0, 1, 1, 1]
    # the same through the model: a coarse field whose two columns differ, read at x = 4 of a 5 x 2 level
    coarse = np.array([[10, 20]])                                 # F(X = 0) = 10, F(X = 1) = 20 on a 2 x 1 parent level
    ys, xs = fp.seed_parents(2, 1), fp.seed_parents(5, 2)
    centres = []
    for ox, oy in fp.SEED_OFFSETS:
        yk = ys[0] if oy == 0 else ys[1] if oy < 0 else ys[2]
        xk = xs[0] if ox == 0 else xs[1] if ox < 0 else xs[2]
        centres.append(int((2 * coarse[yk][:, xk])[0, 4]))
    assert centres == [40, 20, 40, 40, 40]
