"""GPU: every instance of the scene-flow kernel (k_scene_flow_v4<XY> / v2 / v1, each also as ...i with the frame constants in the kernel
arguments, the v4 kernels with and without the XCD remap of their workgroups) against the oracle on the hostile batches of
tests/sceneflow_cases.py: batches of frames whose transforms and dt differ, with static pixels at tame and at extreme coordinates (the
finite-bound shortcut of stage 2a fires, declines, and stage 2b gives 0 or NaN) and residuals on the threshold and one ulp on either
side of it.  tests/test_sceneflow_cases.py (CPU) checks that the batches hold all that."""
import numpy as np
import pytest

import sceneflow_cases as sc
from util import PLANES, first_mismatch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -1234.5
SENTINEL_WORD = 0x5A5A5A5A5A5A5A5A


def _same(got, want):
    """None when got and want agree bit for bit (NaN == NaN), else where they first differ"""
    return first_mismatch(np.ascontiguousarray(got), np.ascontiguousarray(want))


def _mask_bits(words, W):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")[..., :W].astype(bool)


def _mask_tail(words, W):
    """the bits at columns W .. 64 mask_words - 1 of every row (no columns when W % 64 == 0)"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")[..., W:].astype(bool)


def _context(case, frames):
    from moving_object_detector_amd.pipeline import Context
    cam, prm, b = sc.make_case(case.name)
    assert prm.cluster_size == 3
    ctx = Context(case.W, case.H, max_frames=frames, max_objects=case.W * case.H // 3 + 1)
    ctx.set_camera(cam)
    ctx.set_params(prm)
    dev = ctx.device
    batch = ctx.make_batch(torch.from_numpy(b["disparity_now"].copy()).to(dev), torch.from_numpy(b["disparity_prev"].copy()).to(dev),
                           torch.from_numpy(b["flow"].copy()).to(dev), b["t"], b["q"], b["dt"])
    return ctx, batch


def _fill(ws):
    for k in ("planes", "aos", "depth", "static_flow"):
        if ws.get(k) is not None:
            ws[k].fill_(SENTINEL)
    ws["mask"].fill_(SENTINEL_WORD)


def _check_velocity_planes(case, planes, mask, keys):
    """frames 0 .. F-1 of the planes `keys` and of the mask against the oracle"""
    from oracle import numpy_ref
    _, prm, _ = sc.make_case(case.name)
    for f, ref in enumerate(sc.reference(case.name)):
        where = (case.name, "frame", f, sc.kind_of(case, f), "dt", sc.dt_of(case, f))
        for k in keys:
            bad = _same(planes[PLANES.index(k), f], ref[k])
            assert bad is None, (where, k, bad)
        want = numpy_ref.dynamic_mask(prm, ref["vx"], ref["vy"], ref["vz"])
        got = _mask_bits(mask[f], case.W)
        assert np.array_equal(got, want), (where, "mask", int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        # the cluster kernels read mask words whole: the bits of a row's last word at columns >= W are 0
        tail = _mask_tail(mask[f], case.W)
        assert not tail.any(), (where, "mask bits at columns >= W", np.argwhere(tail)[:4].tolist())


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_scene_flow_alone(name):
    case = sc.BY_NAME[name]
    F, H, W = case.F, case.H, case.W
    ctx, batch = _context(case, F + 1)
    ws = ctx.workspace(F + 1, aos=case.aos, extras=True)
    _fill(ws)
    assert ctx.scene_flow(batch, ws) == 0
    ctx.synchronize()
    planes, mask = np.ascontiguousarray(ws["planes"].cpu().numpy()), ws["mask"].cpu().numpy()
    depth, sflow = ws["depth"].cpu().numpy(), ws["static_flow"].cpu().numpy()
    aos = ws["aos"].cpu().numpy() if case.aos else None
    ctx.close()
    _check_velocity_planes(case, planes, mask, PLANES)
    for f, ref in enumerate(sc.reference(name)):
        where = (name, "frame", f, sc.kind_of(case, f))
        bad = _same(sflow[f], ref["static_flow"])
        assert bad is None, (where, "static_flow", bad)
        bad = _same(depth[f], ref["depth"])
        assert bad is None, (where, "depth", bad)
        if case.aos:                                     # the records hold the very bits of the planes; the pads are +0
            rec = aos[f].view(np.uint32)
            for j, k in zip((0, 1, 2, 4, 5, 6), range(6)):
                assert np.array_equal(rec[..., j], planes[k, f].view(np.uint32)), (where, "aos", PLANES[k])
            assert not rec[..., 3].any() and not rec[..., 7].any(), (where, "aos pads")
    # frame F of every output belongs to nobody: the call wrote F frames
    sent = np.float32(SENTINEL)
    assert (planes[:, F] == sent).all() and (depth[F] == sent).all() and (sflow[F] == sent).all()
    assert (mask[F].view(np.uint64) == np.uint64(SENTINEL_WORD)).all()
    if case.aos:
        assert (aos[F] == sent).all()


def _cluster_outputs(ctx, ws, F):
    return {"labels": ws["labels"].cpu().numpy()[:F].copy(), "n_objects": ws["n_objects"].cpu().numpy()[:F].copy(),
            "n_clusters": ws["n_clusters"].cpu().numpy()[:F].copy(), "objects": [o.tobytes() for o in ctx.objects_to_host(ws)[:F]]}


@pytest.mark.parametrize("name", [c.name for c in sc.CASES if c.fused])
def test_fused_call(name, oracle):
    case = sc.BY_NAME[name]
    F, H, W = case.F, case.H, case.W
    _, prm, _ = sc.make_case(name)
    xy = case.fused == "xy"
    # the unfused sequence on a context of its own: scene flow, then the clustering with its own mask and tile flags
    ctx, batch = _context(case, F)
    ws = ctx.workspace(F)
    assert ctx.scene_flow(batch, ws) == 0
    assert ctx.cluster(F, ws, mask_ready=False) == 0
    ctx.synchronize()
    unfused = _cluster_outputs(ctx, ws, F)
    ctx.close()
    # the fused call, twice: the second call runs over the tile headers and depth ranges the first one left
    ctx, batch = _context(case, F)
    ws = ctx.workspace(F, xy=xy)
    _fill(ws)
    for call in (1, 2):
        assert ctx.process(batch, ws) == 0
        ctx.synchronize()
        planes, mask = np.ascontiguousarray(ws["planes"].cpu().numpy()), ws["mask"].cpu().numpy()
        fused = _cluster_outputs(ctx, ws, F)
        _check_velocity_planes(case, planes, mask, PLANES if xy else PLANES[2:])
        if not xy:
            assert (planes[:2] == np.float32(SENTINEL)).all(), (name, "call", call, "x / y planes written")
        for f, ref in enumerate(sc.reference(name)):
            labels, _, K = oracle.cluster(ref, prm, "tidy")
            where = (name, "call", call, "frame", f, sc.kind_of(case, f))
            assert np.array_equal(fused["labels"][f], labels), (where, "labels", int((fused["labels"][f] != labels).sum()))
            assert int(fused["n_clusters"][f]) == K, (where, "n_clusters", int(fused["n_clusters"][f]), K)
        assert np.array_equal(fused["labels"], unfused["labels"]), (name, "call", call)
        assert np.array_equal(fused["n_objects"], unfused["n_objects"]) and np.array_equal(fused["n_clusters"], unfused["n_clusters"])
        for f in range(F):
            assert fused["objects"][f] == unfused["objects"][f], (name, "call", call, "frame", f, "object records")
    ctx.close()
