"""GPU: a context whose capacity (ModConfig) is larger than its camera.  The cluster scratch is allocated, cleared and grown for the
capacity, while the frames of a call lie the camera's strides apart inside it (mod_sf.hip: cluster_alloc, cluster_carve); the flow
estimator's level regions are sized for the capacity and walked with the camera's sizes (host_flow.hip: FlowPlan).  Every other test
sizes its context exactly to its camera and batch, where the two kinds of stride cannot differ.  Every comparison here is bit for bit,
against a fresh context sized exactly to the call and run in one chunk, and at chunk borders against the oracle."""
import functools

import numpy as np
import pytest

from test_gpu_chunks import _batch, _outputs, _same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CAP_W, CAP_H, CAP_F = 200, 72, 70          # the capacity: 4 mask words, 5 tile rows
H = 40                                      # the cameras: 132 x 40 and 130 x 40 (the two-pixel scene-flow kernel), 3 mask words, 3 tile rows
CLUSTER_SIZE = 10
MAX_OBJECTS = CAP_W * CAP_H // CLUSTER_SIZE + 1   # the same for every context: a record's place in `objects` is frame * max_objects + id


def _params(neighbor_distance=4):
    from moving_object_detector_amd import synth
    return synth.Params(dynamic_flow_diff=1, cluster_size=CLUSTER_SIZE, neighbor_distance=neighbor_distance)


@functools.lru_cache(maxsize=None)
def _sequence(W):
    from moving_object_detector_amd import synth
    return synth.make_sequence(W, H, CAP_F, seed=6)


def _context(width, height, frames, cam, prm, chunks):
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(width, height, max_frames=frames, max_objects=MAX_OBJECTS, batch_chunks=chunks)
    ctx.set_camera(cam); ctx.set_params(prm)
    return ctx


def _run(ctx, sq, lo, hi):
    ws = ctx.workspace(hi - lo)
    ws["planes"].fill_(-1.0); ws["labels"].fill_(-7); ws["objects"].zero_(); ws["n_objects"].fill_(-1); ws["n_clusters"].fill_(-1)
    assert ctx.process(_batch(ctx, sq, lo, hi), ws) == 0
    ctx.synchronize()
    return _outputs(ctx, ws), ws


@functools.lru_cache(maxsize=None)
def _reference(W, lo, hi, neighbor_distance=4):
    """Frames [lo, hi) of the camera's sequence on a fresh context of exactly that camera and that many frames, in one chunk."""
    cam, sq = _sequence(W)
    ctx = _context(W, H, hi - lo, cam, _params(neighbor_distance), 1)
    out, _ = _run(ctx, sq, lo, hi)
    ctx.close()
    return out


@pytest.mark.parametrize("W", [132, 130])
def test_capacity_larger_than_the_camera_chunked(oracle, W):
    """Calls of 64 (32 + 32), 70 (35 + 35), 63 (one chunk) and 64 frames again on one context of capacity 200 x 72 x 70."""
    from util import compare_objects_bits
    cam, sq = _sequence(W)
    prm = _params()
    ctx = _context(CAP_W, CAP_H, CAP_F, cam, prm, 2)
    assert (ctx.width, ctx.height, ctx.mask_words) == (W, H, 3)
    for lo, hi in ((0, 64), (0, 70), (7, 70), (0, 64)):
        want = _reference(W, lo, hi)
        assert int((want[2] > 0).sum()) > (hi - lo) // 2         # the sequence does hold objects
        got, ws = _run(ctx, sq, lo, hi)
        _same(got, want)
        objs = ctx.objects_to_host(ws)
        for f in (0, 31, 32, hi - lo - 1):                        # chunk borders of the 64-frame calls included
            g = lo + f
            ref = oracle.construct(cam, prm, sq["disparity"][g + 1], sq["disparity"][g], sq["flow"][g], sq["t"][g], sq["q"][g], float(sq["dt"][g]), "tidy")
            rl, ro, _ = oracle.cluster(ref, prm, "tidy", max_objects=W * H)
            assert np.array_equal(got[1][f], rl), (lo, hi, f)
            compare_objects_bits(objs[f], ro)
    ctx.close()


def test_requests_grow_with_the_neighbor_distance_and_stay():
    """neighbor_distance 2, 16, 2 on one context: the link-request scratch grows for 16 (to the capacity's tile count) and is kept."""
    W = 132
    cam, sq = _sequence(W)
    ctx = _context(CAP_W, CAP_H, 8, cam, _params(2), 0)
    for k, nd in enumerate((2, 16, 2)):
        ctx.set_params(_params(nd))
        lo = 4 * k
        want = _reference(W, lo, lo + 4, nd)
        assert int(want[2].sum()) > 0
        _same(_run(ctx, sq, lo, lo + 4)[0], want)
    ctx.close()


def test_clusterer_alone_between_two_fused_calls():
    """mod_cluster_dev on the oversized context, once with its own mask (k_dynamic_mask into the context's plane, k_tile_flags) and once
    with a caller's, on the planes of the fused call before; then a fused call that must find the scratch clean."""
    W = 132
    cam, sq = _sequence(W)
    ctx = _context(CAP_W, CAP_H, CAP_F, cam, _params(), 2)
    want, ws = _run(ctx, sq, 0, 64)
    _same(want, _reference(W, 0, 64))
    for mask_ready in (False, True):                             # (True: the mask plane the fused call wrote)
        ws["labels"].fill_(-7); ws["objects"].zero_(); ws["n_objects"].fill_(-1); ws["n_clusters"].fill_(-1)
        assert ctx.cluster(64, ws, mask_ready=mask_ready) == 0
        ctx.synchronize()
        got = _outputs(ctx, ws)
        assert np.array_equal(got[1], want[1]), mask_ready
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == want[4], mask_ready
    _same(_run(ctx, sq, 0, 70)[0], _reference(W, 0, 70))
    ctx.close()


def _image_pair(W, frames=2):
    """Smoothed noise that moves 2 px to the left between the images, and a block of it that also moves 3 px down."""
    rng = np.random.Generator(np.random.PCG64(11))
    t = rng.integers(0, 256, size=(frames, H + 8, W + 8)).astype(np.float32)
    for ax in (1, 2):
        t = (np.roll(t, 1, ax) + 2 * t + np.roll(t, -1, ax)) / 4
    t = t.astype(np.uint8)
    prev, now = t[:, 4:4 + H, 4:4 + W].copy(), t[:, 4:4 + H, 6:6 + W].copy()
    now[:, 10:30, 40:90] = t[:, 1:21, 46:96]
    return prev, now


def test_flow_levels_of_a_context_larger_than_its_camera():
    """mod_flow_compute_dev at 1 and 2 levels (the coarsest is 66 x 20), with and without the forward-backward check, on a context of
    capacity 200 x 72 and on one of exactly 132 x 40: equal.  3 levels would make a 33 x 10 level, which both refuse."""
    from moving_object_detector_amd import capi
    W, F = 132, 2
    cam, _ = _sequence(W)
    prev, now = _image_pair(W, F)
    results = []
    for width, height in ((CAP_W, CAP_H), (W, H)):
        ctx = _context(width, height, F, cam, _params(), 0)
        p, n = torch.from_numpy(prev).to(ctx.device), torch.from_numpy(now).to(ctx.device)
        flows = {}
        for levels in (1, 2, 1):                                 # (1 again: the level regions of the two-level call are behind it)
            for fb in (1, -1):
                out = ctx.estimate_flow(p, n, capi.flow_params(levels=levels, radius=4, window=5, subpixel=True, fb_check=fb))
                ctx.synchronize()
                got = out.cpu().numpy().view(np.uint32).copy()
                assert np.array_equal(flows.setdefault((levels, fb), got), got)
        with pytest.raises(capi.ModError) as e:
            ctx.estimate_flow(p, n, capi.flow_params(levels=3))
        assert e.value.code == capi.MOD_ERR_INVALID_ARGUMENT
        ctx.close()
        results.append(flows)
    big, exact = results
    for key, want in exact.items():
        assert np.isfinite(want.view(np.float32)).mean() > 0.5, key   # the estimator did find the motion
        assert np.array_equal(big[key], want), key
