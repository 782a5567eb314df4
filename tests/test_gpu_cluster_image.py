"""GPU: the renderer of the cluster image alone (mod_cluster_image_dev, k_cluster_image) on synthetic label planes, bit for bit against
tests/models/cluster_image_model.py.  The shapes put a frame's first pixel at every residue of the flat array's four-pixel grid, make
groups straddle two frames, and at 144 x 144 carry every label 0 .. 20735 exactly once: the exactness sweep of (k * 255) / K at the
largest K a 1080p context's default capacity can hold."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import cluster_image_model as M  # noqa: E402

SHAPES = [(1, 1), (3, 1), (5, 7), (64, 3), (144, 144)]          # W x H: H * W = 1, 3, 35, 192, 20736
FRAMES = [1, 3, 5]
I32_MAX, I32_MIN = 2**31 - 1, -2**31
CANARY = 64


def _ks(N, F, salt):
    pool = [0, 1, 2, 255, 256, 257, N]
    return [pool[(salt + 3 * f) % len(pool)] for f in range(F)]


def _labels(rng, N, K, permutation):
    if permutation:
        return rng.permutation(N).astype(np.int32)
    lab = rng.integers(-1, max(K, 0) + 2, N).astype(np.int64)       # -1 .. K + 1: inside, -1, K and K + 1
    special = [-1, K, K + 1, I32_MAX, I32_MIN, 0, max(K - 1, 0)]
    where = rng.permutation(N)[:len(special)]
    for j, p in enumerate(where):
        lab[p] = special[(j + int(rng.integers(0, 7))) % 7] if N < 7 else special[j]
    return lab.astype(np.int32)


@pytest.fixture(scope="module")
def contexts():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    made = {}
    for W, H in SHAPES:
        ctx = Context(W, H, max_frames=max(FRAMES))
        ctx.set_camera(synth.make_camera(W, H)); ctx.set_params(synth.Params())
        made[(W, H)] = ctx
    yield made
    for ctx in made.values():
        ctx.close()


def _render(ctx, lab, Ks, palette, misalign=0):
    """lab (F, N) int32 through mod_cluster_image_dev; returns the image (F, N, 3) and checks the canary behind it."""
    F, N = lab.shape
    store = torch.zeros(F * N + 4, dtype=torch.int32, device=ctx.device)
    dev = store[misalign:misalign + F * N]
    dev.copy_(torch.from_numpy(lab.reshape(-1)))
    buf = torch.full((3 * F * N + CANARY,), 0xA5, dtype=torch.uint8, device=ctx.device)
    out = buf[:3 * F * N]
    ctx.render_clusters(dev.view(F, N), torch.tensor(Ks, dtype=torch.int32, device=ctx.device), palette, out=out)
    ctx.synchronize()
    host = buf.cpu().numpy()
    assert (host[3 * F * N:] == 0xA5).all(), "bytes behind the image were written"
    return host[:3 * F * N].reshape(F, N, 3)


@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_renderer_matches_the_model(contexts, shape, F):
    W, H = shape
    N = W * H
    ctx = contexts[shape]
    rng = np.random.default_rng(1000 * N + F)
    rnd = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    for salt in range(3):
        Ks = _ks(N, F, salt + SHAPES.index(shape))
        perm = N == 20736 and salt == 0
        if perm:
            Ks[-1] = N                                           # one frame carries every label 0 .. N - 1 exactly once
        lab = np.stack([_labels(rng, N, Ks[f], perm and f == F - 1) for f in range(F)])
        if perm:
            assert np.array_equal(np.sort(lab[-1]), np.arange(N))
        for palette in (None, rnd):
            got = _render(ctx, lab, Ks, palette)
            want = M.render(lab, Ks, palette)
            assert np.array_equal(got, want), (shape, F, Ks, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("shape", [(5, 7), (144, 144)], ids=lambda s: "%dx%d" % s)
def test_label_plane_off_the_16_byte_grid(contexts, shape):
    """A caller's plane need only be an int32 array: the kernel's dword-load variant."""
    W, H = shape
    N, F = W * H, 3
    rng = np.random.default_rng(N)
    Ks = [N, 257, 2]
    lab = np.stack([_labels(rng, N, Ks[f], f == 0 and N > 7) for f in range(F)])
    for mis in (1, 2, 3):
        assert np.array_equal(_render(contexts[shape], lab, Ks, None, misalign=mis), M.render(lab, Ks))


def test_negative_and_zero_cluster_counts_are_black(contexts):
    ctx = contexts[(64, 3)]
    rng = np.random.default_rng(3)
    lab = rng.integers(-3, 300, (3, 192)).astype(np.int32)
    lab[:, :5] = [0, -1, I32_MAX, I32_MIN, 1]
    got = _render(ctx, lab, [0, -1, I32_MIN], None)
    assert not got.any()


def test_arguments_are_checked(contexts):
    from moving_object_detector_amd import capi
    ctx = contexts[(5, 7)]
    lab = torch.zeros(35, dtype=torch.int32, device=ctx.device)
    K = torch.ones(1, dtype=torch.int32, device=ctx.device)
    img = torch.zeros(3 * 35 + 16, dtype=torch.uint8, device=ctx.device)
    lib, E = ctx.lib, capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_cluster_image_dev(ctx.h, 1, None, K.data_ptr(), None, img.data_ptr()) == E
    assert lib.mod_cluster_image_dev(ctx.h, 1, lab.data_ptr(), None, None, img.data_ptr()) == E
    assert lib.mod_cluster_image_dev(ctx.h, 1, lab.data_ptr(), K.data_ptr(), None, None) == E
    assert lib.mod_cluster_image_dev(ctx.h, 1, lab.data_ptr(), K.data_ptr(), None, img.data_ptr() + 4) == E      # not 16-byte aligned
    assert lib.mod_cluster_image_dev(ctx.h, 0, lab.data_ptr(), K.data_ptr(), None, img.data_ptr()) == E
    assert lib.mod_cluster_image_dev(ctx.h, 6, lab.data_ptr(), K.data_ptr(), None, img.data_ptr()) == capi.MOD_ERR_CAPACITY
    ctx.synchronize()
    assert not img.cpu().numpy().any()
