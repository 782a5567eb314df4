"""GPU: the optical-flow kernels (csrc/flow.hip) on the hostile cases of tests/flow_cases.py — tie-rich, tiny and out-of-range inputs —
through mod_flow_compute_dev, bit for bit against the numpy model, with guards around the output; one context reused across calls of
different levels, seeds, sub-pixel and check settings; the host form against the device form.

tests/test_flow_cases.py (CPU) shows that the model equals an independent scalar reference on the tiny cases and that those cases
tell the plausible mistakes apart, so a kernel with one of them fails here.

Which instance of the match kernels a case runs follows from its parameters: the coarsest level runs k_flow_match<window, true>,
every finer level k_flow_match<window, false> (seeds 1) or k_flow_match_seeds<window> (seeds 5); test_every_family_reaches_every_kernel
checks that each family reaches all nine."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
sys.path.insert(0, HERE)
import flow_cases as fc  # noqa: E402

SENTINEL = 0x7FA5A5A5          # a NaN the kernels never write (theirs is 0x7fc00000)
QUIET_NAN = 0x7FC00000


@pytest.fixture(scope="module")
def contexts():
    """One context per (W, H, max_frames), shared by the cases of that shape: its flow scratch is allocated once and reused."""
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    made = {}

    def get(W, H, F):
        if (W, H, F) not in made:
            ctx = Context(W, H, max_frames=F)
            ctx.set_camera(synth.make_camera(W, H))
            ctx.set_params(synth.Params())
            made[(W, H, F)] = ctx
        return made[(W, H, F)]

    yield get
    for ctx in made.values():
        ctx.close()


def _gpu(ctx, prev, now, params, seeds):
    """mod_flow_compute_dev into the middle of an allocation of F + 2 frames filled with SENTINEL; returns the F frames as uint32 bits
    after checking that both guard frames are untouched and every float inside was written."""
    from moving_object_detector_amd import capi
    F, H, W = now.shape
    per = H * W * 2
    ctx.set_flow_propagation(seeds)
    tp, tn = torch.from_numpy(prev).to(ctx.device), torch.from_numpy(now).to(ctx.device)
    buf = torch.full(((F + 2) * per,), SENTINEL, dtype=torch.int32, device=ctx.device)
    prm = capi.flow_params(**params)
    rc = ctx.lib.mod_flow_compute_dev(ctx.h, F, tp.data_ptr(), tn.data_ptr(), C.byref(prm), buf.data_ptr() + 4 * per)
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    bits = buf.cpu().numpy().view(np.uint32)
    assert (bits[:per] == SENTINEL).all(), "the frame in front of the output was written"
    assert (bits[-per:] == SENTINEL).all(), "the frame behind the output was written"
    got = bits[per:-per].reshape(F, H, W, 2)
    assert not (got == SENTINEL).any(), ("pixels not written", int((got == SENTINEL).any(-1).sum()))
    return got


def _check(label, got, want):
    """uint32 bits; a NaN is 0x7fc00000 in both components or in neither."""
    want = np.ascontiguousarray(want).view(np.uint32)
    for f in range(got.shape[0]):
        nan = np.isnan(got[f].view(np.float32))
        assert (nan[..., 0] == nan[..., 1]).all() and (got[f][nan] == QUIET_NAN).all(), (label, f, "a NaN that is not 0x7fc00000 twice")
        bad = (got[f] != want[f]).any(-1)
        if bad.any():
            y, x = np.argwhere(bad)[0]
            pytest.fail("%s frame %d: %d pixels differ, first at (x %d, y %d): got %s, want %s"
                        % (label, f, int(bad.sum()), x, y, got[f][y, x].view(np.float32), want[f][y, x].view(np.float32)))


@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_case_matches_the_model_bit_for_bit(name, contexts):
    c = fc.BY_NAME[name]
    got = _gpu(contexts(c.W, c.H, c.F), c.prev, c.now, c.params, c.seeds)
    _check(name, got, fc.model_flow(name))


def kernels_of(c):
    w, out = c.params["window"], {("match_coarse", c.params["window"])}
    if c.params["levels"] >= 2:
        out.add(("match_seeds" if c.seeds == 5 else "match_fine", w))
    return out


def test_every_family_reaches_every_kernel():
    """k_flow_match<w, true>, k_flow_match<w, false> and k_flow_match_seeds<w> at w = 3, 5, 7: nine instances, each run by every family."""
    every = {(k, w) for k in ("match_coarse", "match_fine", "match_seeds") for w in (3, 5, 7)}
    for fam in fc.FAMILIES:
        reached = set().union(*[kernels_of(c) for c in fc.CASES if c.family == fam])
        assert reached == every, (fam, sorted(every - reached))


def test_one_context_reused_across_settings(contexts):
    """129 x 67, max_frames 3: five calls whose frame count, levels, seeds, sub-pixel and check settings all change, so every call finds
    the scratch (pyramids, census planes, the integer-field ping-pong, the sub-pixel terms) as another call left it; each result equals
    the model's for that call alone."""
    import flow_model as fm
    import flow_prop_model as fp
    W, H = 129, 67
    calls = (   # frames, levels, seeds, subpixel, fb_check, window
        (("flat", "blocks", "noise4"), 3, 5, 1, 1, 3),
        (("unrelated",), 1, 1, 0, -1, 7),
        (("stripes_v3", "border_left_at"), 2, 5, 1, 0, 5),
        (("noise4", "unrelated", "stripes_h2"), 3, 1, 0, 100, 3),
        (("blocks",), 3, 5, 1, 1, 5),
    )
    ctx = contexts(W, H, 3)
    for n, (variants, levels, seeds, subpixel, fb, window) in enumerate(calls):
        pairs = [fc.make_pair(v, W, H, levels, 1, 77 + n) for v in variants]
        prev, now = np.stack([p for p, _ in pairs]), np.stack([q for _, q in pairs])
        params = dict(levels=levels, radius=1, window=window, subpixel=subpixel, fb_check=fb)
        got = _gpu(ctx, prev, now, params, seeds)
        want = np.stack([fp.flow(prev[f], now[f], fm.FlowParams(**params), seeds) for f in range(len(variants))])
        _check("call %d %s" % (n, variants), got, want)


@pytest.mark.parametrize("name", ["flat_16x16_l1r8w7s0fb-1k1", "blocks_65x33_l2r2w3s1fb100k1"])
def test_host_form_equals_the_device_form(name, contexts):
    from moving_object_detector_amd import capi
    c = fc.BY_NAME[name]
    ctx = contexts(c.W, c.H, 1)
    dev = _gpu(ctx, c.prev, c.now, c.params, c.seeds)[0]
    host = np.full((c.H, c.W, 2), SENTINEL, np.uint32)
    pv, nw = np.ascontiguousarray(c.prev[0]), np.ascontiguousarray(c.now[0])
    prm = capi.flow_params(**c.params)
    assert ctx.flow_host(pv, nw, prm, host)[0] == 0
    assert np.array_equal(host, dev), (name, int((host != dev).any(-1).sum()))
