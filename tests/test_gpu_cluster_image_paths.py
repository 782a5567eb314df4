"""GPU: the cluster image through every call that writes it (mod_set_cluster_image), at 64 x 48.  The expected image is always
tests/models/cluster_image_model.py's render() of the labels and the cluster count the same call returned.

ModConfig.max_objects is 1536, not 1024: mod_set_params refuses cluster_size = 2 on a 64 x 48 context whose capacity is below
max_width * max_height / cluster_size = 1536.  The domino cloud's K still lies in (256, 1024]."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from util import PLANES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import cluster_image_model as M  # noqa: E402

W, H, N = 64, 48, 64 * 48
CAP = 1536
FILL = 0x5A


def _prm():
    from moving_object_detector_amd import synth
    return synth.Params(dynamic_flow_diff=1, cluster_size=2, neighbor_distance=1)


def _cloud(dyn):
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    v = np.where(dyn, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    zero = np.zeros((H, W), np.float32)
    return {"x": xs * np.float32(0.01), "y": ys * np.float32(0.01), "z": np.full((H, W), 5.0, np.float32), "vx": v, "vy": zero, "vz": zero}


def _clouds():
    """Two-pixel horizontal dominoes two columns and one row apart (16 x 24 = 384 of them); nothing dynamic; one 40 x 30 block."""
    ys, xs = np.mgrid[0:H, 0:W]
    dominoes = (xs % 4 < 2) & (ys % 2 == 0)
    block = (xs >= 10) & (xs < 50) & (ys >= 9) & (ys < 39)
    return [_cloud(dominoes), _cloud(np.zeros((H, W), bool)), _cloud(block)]


def _ctx(F, chunks=0):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F, max_objects=CAP, batch_chunks=chunks)
    ctx.set_camera(synth.make_camera(W, H)); ctx.set_params(_prm())
    return ctx


def _load(ws, clouds):
    for f, cl in enumerate(clouds):
        for i, k in enumerate(PLANES):
            ws["planes"][i, f].copy_(torch.from_numpy(cl[k]))


def _expect(ws, F, lut=None):
    return M.render(ws["labels"][:F].cpu().numpy(), ws["n_clusters"][:F].cpu().numpy(), lut)


def test_the_domino_cloud_has_more_clusters_than_table_entries(oracle):
    Ks = [oracle.cluster(cl, _prm(), "tidy", max_objects=N)[2] for cl in _clouds()]
    assert 256 < Ks[0] <= 1024 and Ks[0] == 384 and Ks[1] == 0 and Ks[2] == 1


def test_cluster_dev_draws_every_frame(oracle):
    clouds = _clouds()
    ctx = _ctx(3)
    ws = ctx.workspace(3, image=True)
    _load(ws, clouds)
    rnd = np.random.default_rng(8).integers(0, 256, (256, 3), dtype=np.uint8)
    for lut in (None, rnd):
        ws["image"].fill_(FILL)
        ctx.set_cluster_image(ws, palette=lut)
        assert ctx.cluster(3, ws, mask_ready=False) == 0
        ctx.synchronize()
        K = ws["n_clusters"].cpu().numpy()
        assert list(K) == [384, 0, 1]
        for f, cl in enumerate(clouds):
            assert np.array_equal(ws["labels"][f].cpu().numpy(), oracle.cluster(cl, _prm(), "tidy", max_objects=N)[0])
        img = ws["image"].cpu().numpy()
        assert np.array_equal(img, _expect(ws, 3, lut))
        assert not img[1].any() and len(np.unique(img[0].reshape(-1, 3), axis=0)) > 200
    # what was set is what is reported
    m, on = ctx.get_cluster_image()
    assert on and m.image == ws["image"].data_ptr() and not m.host_image and m.palette_bgr and m.reserved == 0
    assert bytes((C.c_uint8 * 768).from_address(m.palette_bgr)) == rnd.tobytes()
    ctx.set_cluster_image(ws)
    m, on = ctx.get_cluster_image()
    assert on and not m.palette_bgr
    ctx.set_cluster_image(None)
    m, on = ctx.get_cluster_image()
    assert not on and bytes(m) == bytes(32)
    ctx.close()


def test_refusals_leave_the_setting_and_the_outputs_alone():
    from moving_object_detector_amd import capi
    ctx = _ctx(3)
    ws = ctx.workspace(3, image=True)
    _load(ws, _clouds())
    ctx.set_cluster_image(ws)
    before, _ = ctx.get_cluster_image()
    host = np.zeros((H, W, 3), np.uint8)
    for bad in (capi.ModClusterImage(ws["image"].data_ptr(), None, None, 1),
                capi.ModClusterImage(None, None, None, 0),
                capi.ModClusterImage(ws["image"].data_ptr() + 4, host.ctypes.data, None, 0)):
        assert ctx.lib.mod_set_cluster_image(ctx.h, C.byref(bad)) == capi.MOD_ERR_INVALID_ARGUMENT
        now, on = ctx.get_cluster_image()
        assert on and bytes(now) == bytes(before)
    # labels NULL while the image is on: refused, nothing drawn, and the setting survives
    ws["image"].fill_(FILL)
    nolab = ctx.workspace(3, labels=False)
    _load(nolab, _clouds())
    pl, out = ctx._planes_struct(nolab, with_mask=False), ctx._cluster_struct(nolab)
    assert ctx.lib.mod_cluster_dev(ctx.h, 3, C.byref(pl), C.byref(out)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert b"labels" in ctx.lib.mod_last_error(ctx.h)
    # ... and so is n_clusters NULL: the renderer needs the frames' K
    _load(ws, _clouds())
    pl, out = ctx._planes_struct(ws, with_mask=False), ctx._cluster_struct(ws)
    out.n_clusters = None
    assert ctx.lib.mod_cluster_dev(ctx.h, 3, C.byref(pl), C.byref(out)) == capi.MOD_ERR_INVALID_ARGUMENT
    assert b"n_clusters" in ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    assert bool((ws["image"] == FILL).all())
    now, on = ctx.get_cluster_image()
    assert on and bytes(now) == bytes(before)
    assert ctx.cluster(3, ws, mask_ready=False) == 0
    ctx.synchronize()
    assert np.array_equal(ws["image"].cpu().numpy(), _expect(ws, 3))
    ctx.close()


@pytest.fixture(scope="module")
def sequence():
    from moving_object_detector_amd import synth
    cam, sq = synth.make_sequence(W, H, 3, seed=4)
    return cam, sq


def _batch(ctx, sq, F):
    """F frames that cycle through the sequence's three."""
    idx = np.arange(F) % 3
    d = torch.from_numpy(sq["disparity"]).to(ctx.device)
    return ctx.make_batch(d[idx + 1].contiguous(), d[idx].contiguous(), torch.from_numpy(sq["flow"][idx]).to(ctx.device), sq["t"][idx], sq["q"][idx], sq["dt"][idx])


@pytest.mark.parametrize("chunks", [0, 2])
def test_process_dev_chunked_or_not(sequence, chunks):
    cam, sq = sequence
    F = 64                                                       # two chunks of 32 frames when batch_chunks = 2
    ctx = _ctx(F, chunks)
    ctx.set_camera(cam)
    batch = _batch(ctx, sq, F)
    ws = ctx.workspace(F, image=True)
    ws["image"].fill_(FILL)
    ctx.set_cluster_image(ws)
    assert ctx.process(batch, ws) == 0
    ctx.synchronize()
    K = ws["n_clusters"].cpu().numpy()
    assert K[:3].sum() >= 2, K[:3]
    img = ws["image"].cpu().numpy()
    assert np.array_equal(img, _expect(ws, F))
    assert np.array_equal(img[:3], img[60:63]) and img[:3].any()
    # off again: the image is not touched, and the outputs equal those of a context that never had the setting
    ctx.set_cluster_image(None)
    ws["image"].fill_(FILL)
    assert ctx.process(batch, ws) == 0
    ctx.synchronize()
    assert bool((ws["image"] == FILL).all())
    mine = (ws["labels"].cpu().numpy().tobytes(), ws["objects"].cpu().numpy().tobytes(), ws["n_objects"].cpu().numpy().tobytes(), K.tobytes())
    ctx.close()
    fresh = _ctx(F, chunks)
    fresh.set_camera(cam)
    ws2 = fresh.workspace(F)
    assert fresh.process(_batch(fresh, sq, F), ws2) == 0
    fresh.synchronize()
    n = ws2["n_objects"].cpu().numpy()
    theirs = (ws2["labels"].cpu().numpy().tobytes(), ws2["objects"].cpu().numpy().tobytes(), n.tobytes(), ws2["n_clusters"].cpu().numpy().tobytes())
    fresh.close()
    assert mine == theirs


def _frame_args(sq, f):
    from moving_object_detector_amd import capi
    tf = capi.transforms_array(sq["t"][f:f + 1], sq["q"][f:f + 1])
    flow = np.ascontiguousarray(sq["flow"][f])
    now, prev = np.ascontiguousarray(sq["disparity"][f + 1]), np.ascontiguousarray(sq["disparity"][f])
    return (now, prev, flow, tf), (now.ctypes.data, prev.ctypes.data, flow.ctypes.data, C.byref(tf[0]), float(sq["dt"][f]))


def test_host_calls_with_and_without_labels(sequence):
    from moving_object_detector_amd import capi
    cam, sq = sequence
    ctx = _ctx(1)
    ctx.set_camera(cam)
    keep, args = _frame_args(sq, 0)
    images = []
    labels = np.full((H, W), -7, np.int32)
    for want_labels in (True, False):
        host = np.full((H, W, 3), FILL, np.uint8)
        ctx.set_cluster_image(None, host_image=host)
        assert ctx.process_frame_host(*keep[:3], keep[3][0], args[4], labels=labels if want_labels else None, capacity=CAP * want_labels,
                                      count=want_labels)[0] == 0
        images.append(host.copy())
    K = int(labels.max()) + 1
    assert K >= 1
    assert np.array_equal(images[0], M.render(labels[None], [K])[0])
    assert np.array_equal(images[1], images[0])                  # the image request alone runs the cluster stage
    # mod_cluster_cloud_host on the domino cloud
    cl = _clouds()[0]
    rec = np.zeros((H, W, 8), np.float32)
    for j, k in zip((0, 1, 2, 4, 5, 6), PLANES):
        rec[..., j] = cl[k]
    images = []
    for want_labels in (True, False):
        host = np.full((H, W, 3), FILL, np.uint8)
        ctx.set_cluster_image(None, host_image=host)
        assert ctx.cluster_cloud_host(rec, labels if want_labels else None, CAP)[0] == 0
        images.append(host.copy())
    assert int(labels.max()) + 1 == 384
    assert np.array_equal(images[0], M.render(labels[None], [384])[0]) and np.array_equal(images[1], images[0])
    for k in (0, 1, 200, 383):                                   # the markers' colours are the image's
        u, v = np.argwhere(labels.T == k)[0]
        assert tuple(images[0][v, u]) == capi.cluster_color(k, 384)
    del keep
    ctx.close()


def test_three_tickets_keep_their_own_buffer_and_table(sequence):
    from moving_object_detector_amd import capi
    cam, sq = sequence
    ctx = _ctx(1)
    ctx.set_camera(cam)
    rnd = np.random.default_rng(11).integers(0, 256, (256, 3), dtype=np.uint8)
    hosts = [np.full((H, W, 3), FILL, np.uint8) for _ in range(4)]
    labels = [np.full((H, W), -7, np.int32) for _ in range(3)]
    # a first frame without a previous disparity ends at the guard: no ticket, and its buffer keeps its fill
    keep0, a0 = _frame_args(sq, 0)
    ctx.set_cluster_image(None, host_image=hosts[3])
    t = C.c_int32(-5)
    rc = ctx.lib.mod_submit_frame_host(ctx.h, a0[0], None, a0[2], a0[3], a0[4], None, None, None, 0, C.byref(t))
    assert rc == capi.MOD_SKIP_NO_DISPARITY_PREV and t.value == -1
    keeps, tickets = [], []
    for f in range(3):
        ctx.set_cluster_image(None, host_image=hosts[f], palette=rnd if f == 2 else None)     # rotated with tickets outstanding
        keep, args = _frame_args(sq, f)
        keeps.append(keep)
        t = C.c_int32(-1)
        assert ctx.lib.mod_submit_frame_host(ctx.h, *args, None, labels[f].ctypes.data, None, 0, C.byref(t)) == 0, ctx.lib.mod_last_error(ctx.h)
        tickets.append(t.value)
    ctx.set_cluster_image(None)                                  # frames in flight keep what their submit read
    for f in range(3):
        n = C.c_int32(-1)
        assert ctx.lib.mod_collect_frame_host(ctx.h, tickets[f], C.byref(n)) == 0
        K = int(labels[f].max()) + 1
        assert np.array_equal(hosts[f], M.render(labels[f][None], [K], rnd if f == 2 else None)[0]), f
    assert sum(int(l.max()) + 1 for l in labels) >= 2
    assert not np.array_equal(hosts[0], hosts[1]) or not hosts[0].any()
    assert (hosts[3] == FILL).all()
    # off: a submit writes no image
    hosts[0][:] = FILL
    t, n = C.c_int32(-1), C.c_int32(-1)
    keep1, a1 = _frame_args(sq, 0)
    assert ctx.lib.mod_submit_frame_host(ctx.h, *a1, None, labels[0].ctypes.data, None, 0, C.byref(t)) == 0
    assert ctx.lib.mod_collect_frame_host(ctx.h, t.value, C.byref(n)) == 0
    assert (hosts[0] == FILL).all()
    del keep0, keep1, keeps
    ctx.close()
