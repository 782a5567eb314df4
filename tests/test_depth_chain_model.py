"""CPU: the cases of tests/depth_chain_cases.py have the properties tests/test_gpu_depth_chain_batches.py relies on, and the composed
model of tests/models/depth_chain_model.py is a fit reference for it.

The layouts: the "off grid" ones keep the step and step * height off the multiples of 16, the "on grid" ones on them.  With every
stage on, over the six frames: each stage changes more than 100 sample words and the temporal filter takes every branch of its rule
(started, blended, restarted, held, expired, passed).  The MODEL is invariant under the split of the six frames into calls while the
state is carried, so a difference the GPU test finds between splits is the library's.  The planted pixels do what they are there for:
a hole the spatial stage filled reaches the temporal stage as a start; the pixels meant to drop out have a reading behind the spatial
stage in the frames around the drop and none in it (lone pixels while the filter is off, blocks in every setting), and the temporal
stage then holds them for one frame.  Every disparity plane has more than 100 valid pixels, and switching any one stage off changes
the planes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_chain_cases as cc  # noqa: E402
import depth_chain_model as cm  # noqa: E402
import depth_filter_model as dfm  # noqa: E402
import depth_model as dm  # noqa: E402
import depth_temporal_model as dtm  # noqa: E402

BRANCHES = ("started", "blended", "restarted", "held", "expired", "passed")


def _rigs():
    """(id, layout, messages, path) of every rig the GPU test runs with all stages on"""
    out = []
    for encoding in cc.ENCODINGS:
        for kind in cc.PAD:
            for unit in cc.UNITS[encoding]:
                lay = cc.layout(encoding, kind, unit)
                out.append((f"{encoding}, {kind}, unit {unit}", lay, cc.messages(lay), "plain"))
        lay = cc.registered_layout(encoding)
        for path in cc.PATHS[1:]:
            out.append((f"{encoding}, {path}", lay, cc.messages(lay, 12), path))
    return out


RIGS = _rigs()
PLAIN = [r for r in RIGS if r[3] == "plain"]


def _chain(msg, lay, subset, path, state=None, frames=cc.FRAMES):
    return cm.chain(msg, lay, *cc.settings(subset), state, frames, **cc.path_args(path))


def _valid_behind(msg, lay, subset, stage):
    """valid0 [FRAMES][height][width] of the messages behind `stage` (the input where it is off)"""
    behind, _, _, _ = cm.stages(msg, lay, *cc.settings(subset), None, cc.FRAMES)
    return dm.valid(dm.samples(behind.get(stage, msg), lay, cc.FRAMES))


def test_the_layouts_are_off_and_on_the_16_byte_grid():
    for encoding in cc.ENCODINGS:
        B = dm.BYTES[dm.ENCODINGS[encoding]]
        off, on = cc.layout(encoding, "off grid"), cc.layout(encoding, "on grid")
        assert (off.width, off.height, off.x0, off.y0) == (45, 19, 3, 2) and (cc.W, cc.H) == (40, 16)
        assert off.step % 16 != 0 and (off.step * off.height) % 16 != 0 and off.step % B == 0 and (off.step - off.width * B) % 4 == 0
        assert on.step % 16 == 0 and (on.step * on.height) % 16 == 0
        assert on.step * on.height > off.step * off.height           # (the growth test relies on it)
        # frames 1 .. of a batch, and of the library's scratches, lie off the grid: more than one residue, for more than one frame
        assert len({(f * off.step * off.height) % 16 for f in range(cc.FRAMES)} - {0}) >= 2
    assert cc.layout("16UC1", "off grid").step == 94 and 94 * 19 % 16 == 10
    assert len(cc.SUBSETS) == 7 and cc.ALL_ON in cc.SUBSETS
    assert all(sum(s) == cc.FRAMES for s in cc.SPLITS)


@pytest.mark.parametrize("name,lay,msg,path", PLAIN, ids=[r[0] for r in PLAIN])
def test_every_stage_and_every_branch_of_the_temporal_rule_takes_part(name, lay, msg, path):
    _, _, n = _chain(msg, lay, cc.ALL_ON, path)
    assert all(n["changed"][stage] > 100 for stage in cm.STAGES), n["changed"]
    assert all(n[k] > 0 for k in BRANCHES), n


@pytest.mark.parametrize("name,lay,msg,path", RIGS, ids=[r[0] for r in RIGS])
def test_the_messages_hold_what_they_say(name, lay, msg, path):
    w = dfm.words(msg, lay, cc.FRAMES)
    for f in range(cc.FRAMES):
        if lay.enc == 0:
            assert (w[f] == 1).any() and (w[f] == 65535).any()
        else:
            assert all((w[f] == h).any() for h in cc.fc.HOSTILE32)
    z = dm.samples(msg, lay, cc.FRAMES)
    oy, ox = cc.origin_of(lay)
    gate = z[:, oy + cc.GATE[0], ox + cc.GATE[1]]
    assert abs((gate[cc.JUMP_AT] - gate[cc.JUMP_AT - 1]) - 1.0) < 0.01 and abs(gate[1] - gate[0]) < 0.01     # a metre, far outside the gate
    holes = ~dm.valid(z)
    assert 0.01 < holes[:, :, ox + 15:].mean() < 0.12                   # 2 % and the hostile words of 32FC1, beside the planted holes
    # the padding holds noise, and the stages carry it (nothing downstream reads it)
    B = dm.BYTES[lay.enc]
    assert lay.step > lay.width * B and len(np.unique(msg[:, :, lay.width * B:])) > 8
    _, m, _, _ = cm.stages(msg, lay, *cc.settings(cc.ALL_ON), None, cc.FRAMES)
    assert m[:, :, lay.width * B:].tobytes() == msg[:, :, lay.width * B:].tobytes()


@pytest.mark.parametrize("subset", cc.SUBSETS, ids=cc.subset_id)
@pytest.mark.parametrize("name,lay,msg,path", RIGS, ids=[r[0] for r in RIGS])
def test_the_model_does_not_depend_on_the_split(name, lay, msg, path, subset):
    want, state, n = _chain(msg, lay, subset, path)
    frame = lay.step * lay.height
    for split in cc.SPLITS[1:]:
        st, f0, total = None, 0, dict.fromkeys(dtm.COUNTERS, 0)
        for k in split:
            got, st, c = _chain(msg.reshape(-1)[f0 * frame:(f0 + k) * frame], lay, subset, path, st, k)
            assert got.tobytes() == want[f0:f0 + k].tobytes(), (split, f0)
            total = {key: total[key] + c[key] for key in total}
            f0 += k
        assert total == {key: n[key] for key in total}, split
        if subset[2]:
            assert st[0].tobytes() == state[0].tobytes() and st[1].tobytes() == state[1].tobytes(), split


@pytest.mark.parametrize("subset", cc.SUBSETS, ids=cc.subset_id)
@pytest.mark.parametrize("name,lay,msg,path", RIGS, ids=[r[0] for r in RIGS])
def test_the_planted_pixels_drop_out_behind_the_spatial_stage(name, lay, msg, path, subset):
    """so that the hold is not tested on nothing.  The depth filter removes a lone pixel in every frame; the blocks serve every setting."""
    flt, spa, tmp = cc.settings(subset)
    valid = _valid_behind(msg, lay, subset, "spatial" if spa else "filter")     # what the temporal stage is given
    names = ("block1", "block3") if flt else ("lone1", "lone3", "block1", "block3")
    for key in names:
        for (r, c) in cc.planted(lay)[key]:
            got = [bool(valid[f, r, c]) for f in range(cc.FRAMES)]
            assert got == [f not in cc.DROPS[key] for f in range(cc.FRAMES)], (key, (r, c), got)
    if flt:
        for key in ("lone1", "lone3"):
            (r, c), = cc.planted(lay)[key]
            assert not valid[:, r, c].any(), "a lone pixel has no support"
    if not tmp:
        return
    # ... and the temporal stage holds each of them for exactly one frame: the one-frame drop is bridged, the three-frame drop is
    # held once and is gone for the two frames after it
    behind, _, _, _ = cm.stages(msg, lay, flt, spa, tmp, None, cc.FRAMES)
    out = dm.valid(dm.samples(behind["temporal"], lay, cc.FRAMES))
    for key in names:
        for (r, c) in cc.planted(lay)[key]:
            got = [bool(out[f, r, c]) for f in range(cc.FRAMES)]
            assert got == ([True] * 6 if cc.DROPS[key] == cc.ONE_FRAME else [True, True, False, False, True, True]), (key, (r, c), got)


@pytest.mark.parametrize("name,lay,msg,path", PLAIN, ids=[r[0] for r in PLAIN])
def test_a_filled_hole_reaches_the_temporal_stage_as_a_start(name, lay, msg, path):
    """the samples without a reading in frame 0 that the spatial stage fills are started by the temporal stage there: with the spatial
    stage on, frame 0 starts more pixels than with it off, by exactly the number of holes filled"""
    for flt_on in (False, True):
        on, off = (flt_on, True, True), (flt_on, False, True)
        one = msg.reshape(-1)[:lay.step * lay.height]
        _, _, with_fill = cm.chain(one, lay, *cc.settings(on), None, 1, **cc.path_args(path))
        _, _, without = cm.chain(one, lay, *cc.settings(off), None, 1, **cc.path_args(path))
        before = _valid_behind(msg, lay, on, "filter")[0]
        after = _valid_behind(msg, lay, on, "spatial")[0]
        filled = int(np.count_nonzero(after & ~before))
        assert filled > 20 and not (before & ~after).any()
        assert with_fill["started"] - without["started"] == filled and with_fill["blended"] == 0


@pytest.mark.parametrize("name,lay,msg,path", RIGS, ids=[r[0] for r in RIGS])
def test_the_planes_are_worth_comparing(name, lay, msg, path):
    want, _, _ = _chain(msg, lay, cc.ALL_ON, path)
    assert all(int((d > 0).sum()) > 100 for d in want), [int((d > 0).sum()) for d in want]
    for k in range(3):
        subset = tuple(on and i != k for i, on in enumerate(cc.ALL_ON))
        other, _, _ = _chain(msg, lay, subset, path)
        assert all(int((d > 0).sum()) > 100 for d in other)
        assert other.tobytes() != want.tobytes(), ("switching a stage off changed nothing", cm.STAGES[k])
    # a history matters: frames 3 .. 5 from an empty state are not frames 3 .. 5 of the six (what the reset tests rely on)
    frame = lay.step * lay.height
    fresh, _, _ = _chain(msg.reshape(-1)[3 * frame:], lay, cc.ALL_ON, path, None, 3)
    assert all(fresh[f].tobytes() != want[3 + f].tobytes() for f in range(3))


def test_the_paths_differ():
    """the registered, footprint and distorted rigs give three different sets of planes for the same messages"""
    for encoding in cc.ENCODINGS:
        planes = {r[3]: _chain(r[2], r[1], cc.ALL_ON, r[3])[0].tobytes() for r in RIGS if r[3] != "plain" and r[1].encoding == encoding}
        assert len(planes) == 3 and len(set(planes.values())) == 3
