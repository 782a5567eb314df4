"""The kernel cases of k_rectify (csrc/rectify.hip), shared by tests/test_gpu_rectify.py (the product build: direct gathers) and
tests/rectify_staged_worker.py (the build with the LDS-staged tap path compiled in).  A plain module, not a conftest: no fixtures.

A Case is one window of one message size under one pair of calibrations; it is run in every encoding it lists.  Each case carries
`check`, what tests/models/rectify_model.py::staged_plan must show for it (which workgroup tiles are border / staged / fallback, and
where their boxes lie): run() asserts it on the CPU before anything is launched, so a case that has stopped exercising its branch
fails instead of passing idly.  The expected planes are rectify_model.rectify's, compared with np.array_equal; the 0xA5 guard bytes
around the planes must survive."""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import ingest_model as im  # noqa: E402
import rectify_model as rm  # noqa: E402

ENCODINGS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8")
F = 3                                                     # frames per call: blockIdx.z and frame_bytes matter

Case = namedtuple("Case", "name cals mw mh W H x0 y0 pad encodings check to_mono eye")
Case.__new__.__defaults__ = (None,)                      # eye None: the encodings alternate between the two


class Mismatch(AssertionError):
    """The planes differ from the model's: .info says where, and what the plan says about the first differing pixel's tile."""

    def __init__(self, info):
        super().__init__(str(info))
        self.info = info


def channels(enc):
    return im.CHANNELS[im.NAMES[enc]]


def layout(case, enc):
    """(encoding, width, height, step, x0, y0).  pad None: an odd step with 3 or 4 bytes of padding; else step = width * C + pad[C]."""
    row = case.mw * channels(enc)
    pad = (3 if row % 2 == 0 else 4) if case.pad is None else case.pad[channels(enc)]
    return (enc, case.mw, case.mh, row + pad, case.x0, case.y0)


def offsets(case, k):
    """(src_off, dst_off, eye, seed) of the case's k-th encoding: byte offsets in 1..3 that differ between the encodings."""
    n = sum(case.name.encode())
    return 1 + (k + n) % 3, 1 + (k + n // 3) % 3, (k + n) % 2 if case.eye is None else case.eye, 1000 * (n % 97) + k


def outcomes(plan):
    return sorted({t.outcome for t in plan.values()})


# ---- what the plan must show ---------------------------------------------------------------------------------------------------------
def all_staged(case, enc, plan, qmap, src_off):
    """every tile with a tap inside the message is staged; a tile of the grid's size may also be all border"""
    assert "fallback" not in outcomes(plan) and "staged" in outcomes(plan), outcomes(plan)


def identity_ends(case, enc, plan, qmap, src_off):
    """Window = message: the first tile's box starts at the message's first byte and the last tile's ends at its last pixel; in some
    frame the aligned dword that holds each of them lies astride the message's first / last byte (byte-by-byte staging), and the
    window's last column reads ix = width - 1, whose right neighbour is outside (in0 && !in1)."""
    assert outcomes(plan) == ["staged"], outcomes(plan)
    first, last = plan[min(plan)], plan[max(plan)]
    assert first.box[0] == 0 and first.box[2] == 0 and last.box[1] == case.mw - 1 and last.box[3] == case.mh - 1
    assert (qmap[:, -1, 0] >> 5 == case.mw - 1).all()
    Cn, step = channels(enc), layout(case, enc)[3]
    fb = step * case.mh
    starts = [(src_off + z * fb) & 3 for z in range(F)]                        # the message's first byte = the first box's
    assert any(starts), starts
    astride_end = []
    for z in range(F):
        end = src_off + (z + 1) * fb
        last_byte = end - (step - case.mw * Cn) - 1                            # of the last pixel of the last row
        astride_end.append((last_byte & ~3) + 4 > end)
    assert any(astride_end), astride_end


def near_limit(case, enc, plan, qmap, src_off):
    """one tile just under 16 KiB (staged) and one just over (falls back), in one image"""
    size = {k: t.rows * t.pitch for k, t in plan.items()}
    assert any(3500 <= s <= 4096 and plan[k].outcome == "staged" for k, s in size.items()), size
    assert any(4096 < s <= 4700 and plan[k].outcome == "fallback" for k, s in size.items()), size


def middle_falls_back(case, enc, plan, qmap, src_off):
    """the 9x map: the tiles in the middle do not fit, those at the rim, whose box the message's edge cuts down, are staged"""
    by, bx = max(k[0] for k in plan), max(k[1] for k in plan)
    assert plan[(by // 2, bx // 2)].outcome == "fallback", plan[(by // 2, bx // 2)]
    rim = [t for (j, i), t in plan.items() if j in (0, by) or i in (0, bx)]
    assert any(t.outcome == "staged" for t in rim), [t.outcome for t in rim]
    assert "fallback" in outcomes(plan) and "staged" in outcomes(plan)


def border_tile(case, enc, plan, qmap, src_off):
    """at least one tile without any tap inside the message, and one staged tile whose box the message's edge cuts: some of its pixels
    have taps outside the message"""
    assert "border" in outcomes(plan) and "staged" in outcomes(plan), outcomes(plan)
    _, _, _, _, inside = rm.taps(qmap, case.mw, case.mh)
    part = ~(inside[0] & inside[1] & inside[2] & inside[3])
    ys, xs = np.nonzero(part)
    by, bx = rm.tile_of(xs, ys, case.W, offsets(case, case.encodings.index(enc))[1])
    assert any(plan[(int(j), int(i))].outcome == "staged" for j, i in zip(by, bx))


def clamps(case, enc, plan, qmap, src_off):
    """the map holds -2^24 (a non-finite entry among them) and +2^24: those pixels have no tap inside the message"""
    assert (qmap == -rm.QMAX).any() and (qmap == rm.QMAX).any()
    assert "border" in outcomes(plan), outcomes(plan)


def thin(case, enc, plan, qmap, src_off):
    """a message one or two pixels wide or high: every pixel has a tap outside it, and some tap inside"""
    assert min(case.mw, case.mh) in (1, 2)
    _, _, _, _, inside = rm.taps(qmap, case.mw, case.mh)
    assert not (inside[0] & inside[1] & inside[2] & inside[3]).all() and (inside[0] | inside[3]).any()
    assert "staged" in outcomes(plan), outcomes(plan)


# ---- the calibrations ----------------------------------------------------------------------------------------------------------------
def scaling(mw, mh, s, eye):
    """R = I, D = 0, K's focal lengths s times P's: the map is a pure magnification about the principal point"""
    f = 100.0
    cx, cy = 0.5 * mw + 0.3 - 0.5 * eye, 0.5 * mh - 0.2
    return rm.calibration(mw, mh, [s * f, 0, cx, 0, s * f, cy, 0, 0, 1], [0.0] * 5, np.eye(3), [f, 0, cx, 0, 0, f, cy, 0, 0, 0, 1, 0])


# s per channel count, found with staged_plan on the CPU (near_limit holds for both eyes); the first guess for mono8 was 3.8
LIMIT_SCALE = {1: 4.05, 3: 2.3, 4: 2.0}


def not_smooth(mw, mh):
    """the calibrations of tests/test_gpu_rectify.py::test_a_map_that_is_not_smooth_takes_the_direct_path"""
    return [rm.calibration(mw, mh, [900.4, 0, 550.3 + 20 * s, 0, 899.1, 160.2, 0, 0, 1], [-0.05, 0.01, 0.001 * s, -0.002, 0.0],
                           rm.rotation(0.01 * s, -0.02, 0.015), [100.0, 0, 549.5, 0, 0, 100.0, 159.5, 0, 0, 0, 1, 0]) for s in (1.0, -1.0)]


def pushed_off(mw, mh, eye):
    """rm.distorted with K's principal point moved right by 0.6 of the width and down a little: the window's right part samples
    past the message's right edge"""
    c = rm.distorted(mw, mh, eye)
    K = list(c.K)
    K[2] += 0.6 * mw
    K[5] += 3.0
    return rm.calibration(mw, mh, K, c.D, c.R, c.P)


def turned(mw, mh):
    """the 90-degree `odd` calibration of test_map_is_the_models_on_the_distorted_fixture: non-finite entries where Wd = 0, both
    clamps beside them"""
    return rm.calibration(mw, mh, [1e9, 0, 30.5, 0, 1e9, 20.5, 0, 0, 1], [0] * 5, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
                          [50, 0, 30.0, 0, 0, 50, 20.0, 0, 0, 0, 1, 0])


def gentle(mw, mh, eye):
    """for messages too small for rm.distorted (its focal lengths follow the width): mild distortion, a small rotation, fractions in
    both axes, taps on both sides of every edge"""
    s = 1.0 if eye == 0 else -1.0
    K = [41.3, 0, 0.5 * mw - 0.2 + 0.4 * s, 0, 40.1, 0.5 * mh - 0.3, 0, 0, 1]
    P = [37.0, 0, 0.5 * mw - 0.5, 0, 0, 37.0, 0.5 * mh - 0.5, 0, 0, 0, 1, 0]
    return rm.calibration(mw, mh, K, [0.08 * s, -0.02, 0.001, -0.002 * s, 0.0], rm.rotation(0.01 * s, -0.008, 0.02 * s), P)


def zed_like(mw, mh, eye):
    """A ZED-like 1080p calibration (as tests/test_gpu_rectify.py::_zed_like): k1 about -0.17, a small rectifying rotation, P's focal
    a little below K's."""
    s = 1.0 if eye == 0 else -1.0
    K = [1400.3, 0, 0.5 * mw + 11.2 * s, 0, 1399.1, 0.5 * mh - 7.9, 0, 0, 1]
    D = [-0.172 + 0.003 * s, 0.026, 0.0004 * s, -0.0003, 0.0012]
    P = [1350.0, 0, 0.5 * mw, -162.0 * (eye != 0), 0, 1350.0, 0.5 * mh, 0, 0, 0, 1, 0]
    return rm.calibration(mw, mh, K, D, rm.rotation(0.003 * s, -0.004, 0.002 * s), P)


def _pair(fn, *a):
    return [fn(*a, eye) for eye in (0, 1)]


def _cases():
    out = []
    grid = [(W, H) for W in (2, 3, 15, 17, 63, 64, 65, 130) for H in (1, 7)] + [(W, H) for W in (63, 65) for H in (16, 17, 33)]
    for W, H in grid:                                                          # widths around the runs and the tile, rows around 16
        out.append(Case(f"grid {W}x{H}", _pair(rm.distorted, W + 7, H + 7), W + 7, H + 7, W, H, 3, 5, None, ENCODINGS, all_staged, False))
    # window = message, packed rows where that is an odd step (1 and 3 channels), one byte of padding for 4 channels
    out.append(Case("identity over the whole message 67x19", _pair(lambda mw, mh, eye: rm.identity(mw, mh, 70.5, 69.25, 33.3, 9.7), 67, 19),
                    67, 19, 67, 19, 0, 0, {1: 0, 3: 0, 4: 1}, ENCODINGS, identity_ends, True))
    for Cn, encs in ((1, ("mono8",)), (3, ("bgr8", "rgb8")), (4, ("bgra8", "rgba8"))):
        s = LIMIT_SCALE[Cn]
        W, H = 130, 31
        mw, mh = int(s * W) + 24, int(s * H) + 16
        out.append(Case(f"16 KiB limit, {Cn} channels, s = {s}", _pair(scaling, mw, mh, s), mw, mh, W, H, (mw - W) // 2, (mh - H) // 2, None,
                        encs, near_limit, False))
    out.append(Case("9x map that is not smooth", not_smooth(1100, 320), 1100, 320, 130, 37, 485, 141, {1: 1, 3: 1, 4: 1}, ENCODINGS,
                    middle_falls_back, False, 1))                              # (the left eye's rim is all border: no staged tile)
    out.append(Case("a whole tile of border", _pair(pushed_off, 150, 40), 150, 40, 130, 20, 11, 9, None, ENCODINGS, border_tile, False))
    out.append(Case("clamps through the kernel", [turned(61, 40)] * 2, 61, 40, 48, 32, 7, 5, None, ENCODINGS, clamps, False))
    for mw, mh, W, H, x0, y0 in ((1, 9, 1, 9, 0, 0), (2, 9, 2, 7, 0, 1), (23, 1, 17, 1, 3, 0), (23, 2, 17, 2, 3, 0)):
        out.append(Case(f"message {mw}x{mh}", _pair(gentle, mw, mh), mw, mh, W, H, x0, y0, None, ENCODINGS, thin, False))
    return out


def large():
    """The one large shape, the bgra8 case of tests/test_gpu_rectify.py::test_two_frames_at_1080p (the staged worker runs it once):
    (cals, lay, W, H, frames, eye, qmap, plan).  No tile of its plan falls back: every tap comes out of LDS; four tiles of the top
    row look past the message and are all border."""
    W, H, frames, eye = 1920, 1080, 2, 1
    cals = [zed_like(W, H, e) for e in (0, 1)]
    lay = ("bgra8", W, H, W * 4, 0, 0)
    qmap = rm.build_map(cals[eye], 0, 0, W, H)
    plan = rm.staged_plan(qmap, im.Layout(*lay), 0)
    assert "fallback" not in outcomes(plan) and sum(t.outcome == "staged" for t in plan.values()) > 2000, outcomes(plan)
    return cals, lay, W, H, frames, eye, qmap, plan


CASES = _cases()
NAMES = [c.name for c in CASES]


def prepare(case, k):
    """CPU side of the case's k-th encoding: (lay, payload, qmap, want, src_off, dst_off, eye, plan), with the plan's check made."""
    enc = case.encodings[k]
    lay = layout(case, enc)
    src_off, dst_off, eye, seed = offsets(case, k)
    qmap = rm.build_map(case.cals[eye], case.x0, case.y0, case.W, case.H)
    plan = rm.staged_plan(qmap, im.Layout(*lay), dst_off)
    case.check(case, enc, plan, qmap, src_off)
    payload = np.random.default_rng(seed).integers(0, 256, size=F * lay[3] * case.mh, dtype=np.uint8)
    want = rm.rectify(payload, im.Layout(*lay), qmap, F)
    if case.to_mono:
        assert np.array_equal(want, im.to_mono(payload, im.Layout(*lay), case.W, case.H, F))
    return lay, payload, qmap, want, src_off, dst_off, eye, plan


def run(case, make_ctx, cams):
    """The case through mod_rectify_dev of the library the process has loaded, in every encoding of the case.  make_ctx(W, H) -> a
    Context with a camera; cams(cals) -> ModRectifyCamera pair.  Raises Mismatch where the planes differ."""
    import torch
    from moving_object_detector_amd import capi
    ctx = make_ctx(case.W, case.H)
    ctx.set_rectification(*cams(case.cals))
    try:
        for k, enc in enumerate(case.encodings):
            lay, payload, qmap, want, src_off, dst_off, eye, plan = prepare(case, k)
            dev = ctx.device
            src = torch.empty(payload.size + src_off, dtype=torch.uint8, device=dev)
            src[src_off:] = torch.from_numpy(payload).to(dev)
            n = F * case.H * case.W
            dst = torch.full((n + dst_off + 64,), 0xA5, dtype=torch.uint8, device=dev)
            assert src.data_ptr() % 4 == 0 and dst.data_ptr() % 4 == 0        # the plan's heads and the astride bytes assume it
            out = dst[dst_off:dst_off + n].view(F, case.H, case.W)
            assert np.array_equal(ctx.rectification_map(eye, capi.image_layout(*lay)), qmap), (case.name, enc, "map")
            ctx.rectify(src[src_off:], capi.image_layout(*lay), eye, out=out)
            ctx.synchronize()
            d = dst.cpu().numpy()
            assert (d[:dst_off] == 0xA5).all() and (d[dst_off + n:] == 0xA5).all(), (case.name, enc, "wrote outside the grey planes")
            got = d[dst_off:dst_off + n].reshape(F, case.H, case.W)
            if not np.array_equal(got, want):
                f, y, x = (int(v[0]) for v in np.nonzero(got != want))
                by, bx = (int(v) for v in rm.tile_of(x, y, case.W, dst_off))
                t = plan[(by, bx)]
                raise Mismatch({"case": case.name, "encoding": enc, "count": int((got != want).sum()), "first": [f, y, x],
                                "got": int(got[f, y, x]), "want": int(want[f, y, x]), "tile": [by, bx],
                                "tile_outcome_in_frame_0": t.outcome, "box": t.box, "rows": t.rows, "pitch": t.pitch})
            if case.check is clamps:                                           # BORDER_CONSTANT: the clamped entries read 0
                far = (np.abs(qmap) == rm.QMAX).any(axis=-1)
                assert (got[:, far] == 0).all()
    finally:
        ctx.close()
