"""GPU: the on-GPU census optical flow (csrc/flow.hip) through the C ABI — bit for bit against the numpy restatement
(tests/models/flow_model.py) over sizes, frame counts and parameters, the host form against the device form, argument checks, and
accuracy on synthetic moving boxes with known flow."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
GOLD = os.path.join(HERE, "golden", "flow", "flow_320x240.npz")


def _ctx(W, H, F):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(synth.Params())
    return ctx


def _pairs(W, H, F, seed):
    from moving_object_detector_amd import synth
    ms = [synth.make_moving_images(W, H, seed=seed + f, n_boxes=3, shift=(2, 14)) for f in range(F)]
    return np.stack([m["left0"] for m in ms]), np.stack([m["left1"] for m in ms])


def _gpu(ctx, prev, now, prm):
    from moving_object_detector_amd import capi
    F, H, W = now.shape
    dev = ctx.device
    tp, tn = torch.from_numpy(prev).to(dev), torch.from_numpy(now).to(dev)
    out = torch.full((F, H, W, 2), -7.0, dtype=torch.float32, device=dev)
    return ctx.estimate_flow(tp, tn, prm, out).cpu().numpy()   # (.cpu() waits: the context runs on torch\'s stream)


def _same(a, b):
    """bit for bit, NaN = NaN"""
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


CASES = [
    (320, 240, 3, dict()),
    (1280, 720, 1, dict()),
    (333, 197, 1, dict(levels=3, window=7, subpixel=0, fb_check=-1)),
    (333, 197, 2, dict(levels=2, radius=5, window=3, subpixel=1, fb_check=0)),
    (320, 240, 1, dict(levels=1, radius=3, window=3, subpixel=1, fb_check=1)),
    (320, 240, 1, dict(levels=3, radius=2, window=7, subpixel=1, fb_check=-1)),
    (320, 240, 2, dict(levels=4, radius=4, window=5, subpixel=0, fb_check=2)),
    (512, 384, 1, dict(levels=5, radius=2, window=5, subpixel=1, fb_check=1)),
]


@pytest.mark.parametrize("W,H,F,kw", CASES)
def test_flow_matches_the_model_bit_for_bit(W, H, F, kw):
    import flow_model as fm
    from moving_object_detector_amd import capi
    prev, now = _pairs(W, H, F, seed=W + F)
    prm = capi.flow_params(**kw)
    ctx = _ctx(W, H, F)
    got = _gpu(ctx, prev, now, prm)
    ctx.close()
    mp = fm.FlowParams(prm.levels, prm.radius, prm.window, prm.subpixel, prm.fb_check)
    for f in range(F):
        want = fm.flow(prev[f], now[f], mp)
        assert _same(got[f], want), (kw, f, int((~((got[f].view(np.uint32) == want.view(np.uint32)) | (np.isnan(got[f]) & np.isnan(want)))).sum()))


def test_fixture_host_form_and_argument_checks():
    from moving_object_detector_amd import capi
    g = np.load(GOLD)
    H, W = g["prev"].shape[1:]
    ctx = _ctx(W, H, 2)
    for k in range(int(g["pairs"])):
        prm = capi.ModFlowParams(*[int(v) for v in g["params"][k]])
        dev = _gpu(ctx, g["prev"][k][None], g["now"][k][None], prm)[0]
        assert _same(dev, g["flow"][k]), k
        host = np.full((H, W, 2), -7.0, np.float32)
        pv, nw = np.ascontiguousarray(g["prev"][k]), np.ascontiguousarray(g["now"][k])
        assert ctx.flow_host(pv, nw, prm, host)[0] == 0
        assert _same(host, dev), k
    # the pipeline wrapper, on device tensors
    tp, tn = torch.from_numpy(g["prev"][0]).to(ctx.device), torch.from_numpy(g["now"][0]).to(ctx.device)
    wrapped = ctx.estimate_flow(tp, tn, capi.ModFlowParams(*[int(v) for v in g["params"][0]]))
    ctx.synchronize()
    assert _same(wrapped.cpu().numpy(), g["flow"][0])
    # what cannot work is an error; a missing image is a skip, like a failed estimateOpticalFlow
    pv, nw = np.ascontiguousarray(g["prev"][0]), np.ascontiguousarray(g["now"][0])
    out = torch.empty((3, H, W, 2), dtype=torch.float32, device=ctx.device)
    t3 = torch.zeros((3, H, W), dtype=torch.uint8, device=ctx.device)
    for bad in (capi.flow_params(window=4), capi.flow_params(window=9), capi.flow_params(levels=5), capi.flow_params(levels=0),
                capi.flow_params(levels=7), capi.flow_params(radius=0), capi.flow_params(radius=9), capi.ModFlowParams(4, 4, 5, 2, 1)):
        assert ctx.lib.mod_flow_compute_dev(ctx.h, 1, t3.data_ptr(), t3.data_ptr(), C.byref(bad), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
        assert ctx.lib.mod_flow_compute_host(ctx.h, pv.ctypes.data, nw.ctypes.data, C.byref(bad), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT   # a device pointer as the host output
    assert b"16 px" in ctx.lib.mod_last_error(ctx.h) or b"must" in ctx.lib.mod_last_error(ctx.h)
    ok = capi.flow_params()
    assert ctx.lib.mod_flow_compute_dev(ctx.h, 3, t3.data_ptr(), t3.data_ptr(), C.byref(ok), out.data_ptr()) == capi.MOD_ERR_CAPACITY
    assert ctx.lib.mod_flow_compute_dev(ctx.h, 0, t3.data_ptr(), t3.data_ptr(), C.byref(ok), out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
    assert ctx.lib.mod_flow_compute_dev(ctx.h, 1, None, t3.data_ptr(), C.byref(ok), out.data_ptr()) == capi.MOD_SKIP_NO_FLOW
    assert ctx.lib.mod_flow_compute_dev(ctx.h, 1, t3.data_ptr(), None, C.byref(ok), out.data_ptr()) == capi.MOD_SKIP_NO_FLOW
    assert ctx.lib.mod_flow_compute_host(ctx.h, None, nw.ctypes.data, C.byref(ok), out.data_ptr()) == capi.MOD_SKIP_NO_FLOW   # a device pointer as the host output
    assert ctx.lib.mod_flow_compute_dev(ctx.h, 1, t3.data_ptr(), t3.data_ptr(), None, out.data_ptr()) == capi.MOD_ERR_INVALID_ARGUMENT
    assert ctx.lib.mod_flow_compute_dev(ctx.h, 1, t3.data_ptr(), t3.data_ptr(), C.byref(ok), None) == capi.MOD_ERR_INVALID_ARGUMENT
    ctx.close()


def test_accuracy_on_moving_boxes_at_720p():
    """make_moving_images at 1280 x 720 (boxes moving by up to 20 px, camera still): on pixels at least 8 px from any box edge and from
    the image border, >= 95 % are valid and >= 99 % of the valid ones round to the true flow."""
    from moving_object_detector_amd import capi, synth
    W, H = 1280, 720
    ctx = _ctx(W, H, 1)
    for seed in (1, 2):
        m = synth.make_moving_images(W, H, seed=seed, n_boxes=4)
        f = _gpu(ctx, m["left0"][None], m["left1"][None], capi.flow_params())[0]
        truth = m["flow"]
        near = np.zeros((H, W), bool)
        near[:8] = near[-8:] = True
        near[:, :8] = near[:, -8:] = True
        for (x0, y0, bw, bh), (sx, sy), _ in m["boxes"]:
            for X0, Y0 in ((x0, y0), (x0 + sx, y0 + sy)):
                ring = np.zeros((H, W), bool)
                ring[max(0, Y0 - 8):Y0 + bh + 8, max(0, X0 - 8):X0 + bw + 8] = True
                ring[Y0 + 8:Y0 + bh - 8, X0 + 8:X0 + bw - 8] = False
                near |= ring
        sel = ~near & ~np.isnan(truth[..., 0])
        valid = ~np.isnan(f[..., 0])
        good = valid & (np.round(f[..., 0]) == truth[..., 0]) & (np.round(f[..., 1]) == truth[..., 1])
        assert valid[sel].mean() >= 0.95, (seed, float(valid[sel].mean()))
        assert good[sel].sum() >= 0.99 * (valid & sel).sum(), (seed, float(good[sel].sum() / (valid & sel).sum()))
    ctx.close()


def test_sources_and_symbols():
    src = open(os.path.join(ROOT, "moving_object_detector_amd", "csrc", "flow.hip")).read()
    assert "getenv" not in src
    sys.path.insert(0, HERE)
    from test_abi import declared_functions
    from moving_object_detector_amd import capi
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert names == sorted(declared_functions())
    for n in ("mod_flow_compute_dev", "mod_flow_compute_host", "mod_submit_images_host"):
        assert n in names
