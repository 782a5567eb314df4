"""GPU: scene-flow stage against the oracle on hostile inputs — random cameras with non-zero Tx/Ty, unnormalised
quaternions, negative / tiny dt, disparities spanning denormals..inf, flows spanning 0..1e30, NaN everywhere; also
transforms with huge entries.

The flows here are random and unrelated to the static flow, so under the random poses no pixel that gets a velocity is static: this test
does not exercise the "certainly finite" shortcut of stage 2a (FrameConst.pad[0]) — neither its firing at hostile coordinates nor its
declining beyond the bound — and its batches are single frames of the inline kernels.  tests/test_gpu_sceneflow_variants.py covers both: static and threshold-tied pixels at tame and
extreme coordinates, batches of differing frames, every kernel variant."""
import numpy as np
import pytest

from util import PLANES, bits_equal, first_mismatch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _hostile_frame(rng, W, H):
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, 1e-38, 1e-20, 1e20, 3e38, -1.0, 0.25, 64.0, 127.99, 128.0, 128.01], np.float32)
    def disp():
        d = rng.uniform(0.0, 130.0, (H, W)).astype(np.float32)
        m = rng.random((H, W)) < 0.25
        d[m] = rng.choice(specials, int(m.sum()))
        return d
    flow = (rng.standard_normal((H, W, 2)) * rng.choice([0.3, 3.0, 30.0, 3000.0], (H, W, 1))).astype(np.float32)
    m = rng.random((H, W, 2)) < 0.1
    flow[m] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.5, -0.5, 1.5, 2.5, 2147483648.0, -2147483904.0], np.float32), int(m.sum()))
    return disp(), disp(), flow


@pytest.mark.parametrize("seed", range(10))
def test_hostile_inputs(oracle, seed):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    rng = np.random.default_rng(1000 + seed)
    W, H = [(132, 70), (131, 67), (130, 69)][seed % 3]      # 4 px / thread, 1 px / thread (odd width), 2 px / thread (W % 4 == 2)
    cam = synth.make_camera(W, H)
    cam.fx, cam.fy = float(rng.uniform(50, 900)), float(rng.uniform(50, 900))
    cam.cx, cam.cy = float(rng.uniform(0, W)), float(rng.uniform(0, H))
    cam.Tx, cam.Ty = float(rng.uniform(-30, 30)), float(rng.uniform(-5, 5))
    cam.disp_f, cam.disp_T = np.float32(cam.fx), np.float32(rng.uniform(0.05, 0.6))
    cam.min_disparity, cam.max_disparity = np.float32(rng.choice([0.0, -4.0, 1.0])), np.float32(rng.choice([128.0, 64.0, 3.4e38]))
    prm = synth.Params(dynamic_flow_diff=int(rng.integers(1, 8)), cluster_size=100, dynamic_speed=float(rng.uniform(0.01, 1.0)))
    d_now, d_prev, flow = _hostile_frame(rng, W, H)
    q = rng.standard_normal(4) * rng.choice([1.0, 0.5, 2.0])          # not normalised on purpose
    t = rng.standard_normal(3) * rng.choice([0.1, 10.0])
    dt = float(rng.choice([0.1, 1.0 / 15.0, 1e-9, -0.1, 3.0]))
    if seed == 4:
        q = q * 1e18                                                  # rotation entries ~1e36 (no pixel is static here: see the docstring)
    if seed == 5:
        t = np.array([np.inf, 0.0, np.nan])
    # the kernel's division shortcuts (csrc/exact_div.h) and their fall-backs
    if seed == 6:
        dt = 0.0                                                      # reciprocal of dt unusable: inf / NaN velocities
    if seed == 7:
        dt = 1e-70                                                    # outside the reciprocal window: IEEE division path
    if seed == 8:                                                     # identity motion, integer principal point, no Tx/Ty:
        q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)            # zero numerators (+0 and -0) in the projection
        cam.cx, cam.cy, cam.Tx, cam.Ty = float(W // 2), float(H // 2), 0.0, 0.0
    if seed == 9:
        q, t = q * 1e-40, t * 1e-90                                   # tiny transformed coordinates: operands leave the window
    ref = oracle.construct(cam, prm, d_now, d_prev, flow, t, q, dt, "tidy")
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(prm)
    ws = ctx.workspace(1, aos=False, extras=True)
    dev = ctx.device
    b = ctx.make_batch(torch.from_numpy(d_now[None]).to(dev), torch.from_numpy(d_prev[None]).to(dev), torch.from_numpy(flow[None]).to(dev),
                       [t], [q], [dt])
    assert ctx.scene_flow(b, ws) == 0
    ctx.synchronize()
    for i, k in enumerate(PLANES):
        got = ws["planes"][i, 0].cpu().numpy()
        assert bits_equal(got, ref[k]), (k, first_mismatch(got, ref[k]))
    assert bits_equal(ws["static_flow"][0].cpu().numpy(), ref["static_flow"])
    # the mask equals calculateDynamicMap of the produced velocities
    from oracle import numpy_ref
    bits = np.unpackbits(ws["mask"][0].cpu().numpy().view(np.uint8), axis=-1, bitorder="little")[:, :W].astype(bool)
    assert np.array_equal(bits, numpy_ref.dynamic_mask(prm, ref["vx"], ref["vy"], ref["vz"]))
    ctx.close()
