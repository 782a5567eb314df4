"""GPU: the stand-alone kernels that restate parts of the fused scene-flow kernel — k_static_flow (mod_static_flow_dev), k_depth
(mod_depth_image_dev) and k_dynamic_mask (mod_dynamic_mask_dev) — against the oracle, bit for bit, on the hostile batches of
tests/sceneflow_cases.py (odd widths, H % 4 != 0, frames whose transforms differ, disparities from denormal to inf, half turns of
1e10 ... 1e19, inf / NaN translations) and, k_static_flow, on the targeted projection frames of tests/static_flow_cases.py (the
wave-uniform IEEE fallback of exact_div::div2_shared on lanes whose result is a number, the za / zb branches, tz of 0, < 0, inf and
denormal).  tests/test_static_flow_cases.py (CPU) checks that the targeted frames hold all that.  Every output lies in front of a
sentinel frame (word) that the call must leave alone; masks are compared as whole words: the bits at columns >= W must be 0."""
import numpy as np
import pytest

import sceneflow_cases as sc
import static_flow_cases as sfc
from util import first_mismatch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = np.float32(-1234.5)
SENTINEL_WORD = 0x5A5A5A5A5A5A5A5A
GUARD = 16                                                       # floats in front of the static flow
HOSTILE = [c.name for c in sc.CASES]


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == SENTINEL.view(np.uint32)).all())


def _static_flow(label, cam, d_prev, t, q, want, kind):
    """mod_static_flow_dev over all frames of d_prev (F, H, W) in one call, then over frames [k:] through offset views, against want[f]
    (H, W, 2); kind(f) names frame f in a failure"""
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    F, H, W = d_prev.shape
    n = H * W * 2
    ctx = Context(W, H, max_frames=1)                            # the call is not held to max_frames
    ctx.set_camera(cam)
    ctx.set_params(synth.Params())
    d_dev = torch.from_numpy(d_prev.copy()).to(ctx.device)
    tf_dev = torch.from_numpy(np.concatenate([t, q], axis=1)).to(ctx.device)
    assert tf_dev.shape == (F, 7) and tf_dev.dtype == torch.float64
    buf = torch.full((GUARD + (F + 1) * n,), float(SENTINEL), dtype=torch.float32, device=ctx.device)
    for k in (0, 1) if F > 1 else (0,):                          # k = 1: bases that are not frame 0's (odd W H: d_prev 4-byte aligned only)
        buf.fill_(float(SENTINEL))
        out = buf[GUARD + k * n:GUARD + F * n]
        assert d_dev[k:].data_ptr() == d_dev.data_ptr() + 4 * k * H * W and tf_dev[k:].data_ptr() == tf_dev.data_ptr() + 56 * k
        got = ctx.static_flow(d_dev[k:], tf_dev[k:], out=out)
        assert got.data_ptr() == out.data_ptr()
        ctx.synchronize()
        host = buf.cpu().numpy()
        frames = host[GUARD:].reshape(F + 1, H, W, 2)
        for f in range(k, F):
            bad = first_mismatch(frames[f], want[f])
            assert bad is None, (label, "frames [%d:]" % k, "frame", f, kind(f), bad)
        assert _untouched(host[:GUARD]), (label, k, "guard floats in front of the output")
        assert _untouched(frames[:k]), (label, k, "frames in front of the view")
        assert _untouched(frames[F]), (label, k, "sentinel frame behind the output")
    ctx.close()


@pytest.mark.parametrize("name", HOSTILE)
def test_static_flow_on_hostile_batch(name):
    case = sc.BY_NAME[name]
    cam, _, b = sc.make_case(name)
    want = [ref["static_flow"] for ref in sc.reference(name)]
    _static_flow(name, cam, b["disparity_prev"], b["t"], b["q"], want, lambda f: sc.kind_of(case, f))


@pytest.mark.parametrize("name", [c.name for c in sfc.CASES])
def test_static_flow_on_targeted_frames(name):
    cam, d, t, q = sfc.make_case(name)
    _static_flow(name, cam, d, t, q, sfc.reference(name), lambda f: sfc.FRAME_NAMES[f])


def _context(case):
    from moving_object_detector_amd.pipeline import Context
    cam, prm, _ = sc.make_case(case.name)
    ctx = Context(case.W, case.H, max_frames=case.F, max_objects=case.W * case.H // 3 + 1)      # held to max_frames = F
    ctx.set_camera(cam)
    ctx.set_params(prm)
    return ctx


@pytest.mark.parametrize("name", HOSTILE)
def test_depth_image_on_hostile_batch(name):
    case = sc.BY_NAME[name]
    F, H, W = case.F, case.H, case.W
    if W % 2:
        assert (F * W * H) % 256 != 0                            # k_depth's last block is ragged
    _, _, b = sc.make_case(name)
    ctx = _context(case)
    dn = torch.from_numpy(b["disparity_now"].copy()).to(ctx.device)
    out = torch.full((F + 1, H, W), float(SENTINEL), dtype=torch.float32, device=ctx.device)
    assert ctx.lib.mod_depth_image_dev(ctx.h, F, dn.data_ptr(), out.data_ptr()) == 0
    ctx.synchronize()
    host = out.cpu().numpy()
    ctx.close()
    for f, ref in enumerate(sc.reference(name)):
        bad = first_mismatch(host[f], ref["depth"])
        assert bad is None, (name, "frame", f, bad)
    assert _untouched(host[F]), (name, "sentinel frame behind the output")


def mask_words(bits):
    """(H, W) bool -> (H, ceil(W / 64)) uint64, bit b of word k of a row = pixel 64 k + b, the bits at columns >= W zero"""
    H, W = bits.shape
    padded = np.zeros((H, -(-W // 64) * 64), np.uint8)
    padded[:, :W] = bits
    return np.packbits(padded, axis=-1, bitorder="little").view(np.uint64)


@pytest.mark.parametrize("name", HOSTILE)
def test_dynamic_mask_on_hostile_batch(name):
    from oracle import numpy_ref
    case = sc.BY_NAME[name]
    F, H, W = case.F, case.H, case.W
    MW = -(-W // 64)
    _, prm, _ = sc.make_case(name)
    ref = sc.reference(name)
    v = {k: np.stack([r[k] for r in ref]) for k in ("vx", "vy", "vz")}
    allv = np.stack(list(v.values()))
    # what the planes hold (a batch of 8 frames or more has a frame with dt = 0: infinite velocities)
    assert np.isnan(allv).any() and (allv == 0).any() and (F < 8 or np.isinf(allv).any())
    ctx = _context(case)
    dev = {k: torch.from_numpy(a).to(ctx.device) for k, a in v.items()}
    mask = torch.full((F * H * MW + 1,), SENTINEL_WORD, dtype=torch.int64, device=ctx.device)
    assert ctx.lib.mod_dynamic_mask_dev(ctx.h, F, dev["vx"].data_ptr(), dev["vy"].data_ptr(), dev["vz"].data_ptr(), mask.data_ptr()) == 0
    ctx.synchronize()
    host = mask.cpu().numpy().view(np.uint64)
    ctx.close()
    got = host[:-1].reshape(F, H, MW)
    for f in range(F):
        want = mask_words(numpy_ref.dynamic_mask(prm, v["vx"][f], v["vy"][f], v["vz"][f]))
        diff = got[f] ^ want
        tail = diff[:, -1] >> np.uint64(W % 64) if W % 64 else np.zeros(H, np.uint64)
        assert not diff.any(), (name, "frame", f, sc.kind_of(case, f), "rows whose words differ", np.flatnonzero(diff.any(axis=1))[:4].tolist(),
                                "rows with bits at columns >= W", np.flatnonzero(tail)[:4].tolist())
    assert host[-1] == np.uint64(SENTINEL_WORD), (name, "sentinel word behind the mask")
