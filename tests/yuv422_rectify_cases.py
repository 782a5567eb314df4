"""The kernel cases of k_rectify (csrc/rectify.hip) for the packed YUV 4:2:2 encodings: the maps and windows of
tests/rectify_cases.py, run in yuv422 and yuv422_yuy2 against tests/models/yuv422_model.py, shared by
tests/test_gpu_yuv422_rectify.py (the product build: direct gathers) and tests/yuv422_rectify_worker.py (the build with the
LDS-staged tap path compiled in).  A plain module, not a conftest: no fixtures.

rectify_cases' own machinery does the work (its layouts, offsets, plan checks and run()); this module hands it the two encodings —
ingest_model's tables are extended for the length of a call, never for good — and the expected planes of yuv422_model.  The cases
that rectify_cases builds per channel count (a box just under and just over 16 KiB of LDS) are rebuilt here for a pitch of two bytes."""
import contextlib
import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import rectify_cases as rc  # noqa: E402
import yuv422_model as ym  # noqa: E402

im, rm = rc.im, rc.rm
ENCODINGS = ("yuv422", "yuv422_yuy2")
F = rc.F
LIMIT_SCALE_2 = 2.85                                     # found with staged_plan on the CPU, like rectify_cases.LIMIT_SCALE: near_limit holds for both eyes


@contextlib.contextmanager
def two_more_encodings():
    """ingest_model's tables with the two encodings, while rectify_cases and rectify_model.staged_plan look them up"""
    with mock.patch.dict(im.NAMES, {n: ym.NAMES[n] for n in ENCODINGS}), mock.patch.dict(im.CHANNELS, {ym.NAMES[n]: 2 for n in ENCODINGS}):
        yield


def _cases():
    out = []
    for c in rc.CASES:
        if c.check is rc.near_limit:                      # built per channel count: see below
            continue
        pad = {**c.pad, 2: 1} if isinstance(c.pad, dict) else c.pad   # (the identity case: an odd step for two bytes per pixel too)
        out.append(c._replace(encodings=ENCODINGS, pad=pad))
    s = LIMIT_SCALE_2
    W, H = 130, 31
    mw, mh = int(s * W) + 24, int(s * H) + 16
    out.append(rc.Case(f"16 KiB limit, pitch 2, s = {s}", rc._pair(rc.scaling, mw, mh, s), mw, mh, W, H, (mw - W) // 2, (mh - H) // 2, None,
                       ENCODINGS, rc.near_limit, False))
    return out


CASES = _cases()
NAMES = [c.name for c in CASES]


def prepare(case, k):
    """rectify_cases.prepare for the case's k-th encoding, the expected planes from yuv422_model"""
    enc = case.encodings[k]
    lay = rc.layout(case, enc)
    src_off, dst_off, eye, seed = rc.offsets(case, k)
    qmap = rm.build_map(case.cals[eye], case.x0, case.y0, case.W, case.H)
    plan = rm.staged_plan(qmap, im.Layout(*lay), dst_off)
    case.check(case, enc, plan, qmap, src_off)
    payload = np.random.default_rng(seed).integers(0, 256, size=F * lay[3] * case.mh, dtype=np.uint8)
    want = ym.rectify(payload, ym.Layout(*lay), qmap, F)
    if case.to_mono:
        assert np.array_equal(want, ym.to_mono(payload, ym.Layout(*lay), case.W, case.H, F))
    return lay, payload, qmap, want, src_off, dst_off, eye, plan


def run(case, make_ctx, cams):
    """rectify_cases.run with this module's prepare: the case through mod_rectify_dev of the library the process has loaded"""
    with two_more_encodings(), mock.patch.object(rc, "prepare", prepare):
        rc.run(case, make_ctx, cams)


def large(enc="yuv422_yuy2"):
    """Two frames at 1080p under rectify_cases.zed_like, the right eye: (cals, lay, W, H, frames, eye, qmap, payload, want)."""
    W, H, frames, eye = 1920, 1080, 2, 1
    cals = [rc.zed_like(W, H, e) for e in (0, 1)]
    lay = (enc, W, H, W * 2 + 2, 0, 0)
    qmap = rm.build_map(cals[eye], 0, 0, W, H)
    payload = np.random.default_rng(11).integers(0, 256, size=frames * lay[3] * H, dtype=np.uint8)
    return cals, lay, W, H, frames, eye, qmap, payload, ym.rectify(payload, ym.Layout(*lay), qmap, frames)


PANES = "side-by-side panes"


def run_panes(make_ctx, cams):
    """Pane isolation through mod_rectify_dev of the loaded library, side by side on, bgr8 and yuv422_yuy2: two stacked messages
    whose left pane is all 255 and whose rows end in 64 random bytes; the window is the whole pane under rectify_model.distorted, so
    the right eye's taps cross the pane's left and right edges.  The right image must be the model's on the cut-out right pane (a tap
    beyond the pane reads 0) and must not change when the left pane and the padding are random anew; the left image likewise.
    Then the same without padding and with one byte of it (an odd step): without padding the right pane's last pixel byte is the
    message's last byte, a tap reads it, and the two source offsets put it on and off the dword grid, so the image depends on the
    loadable extent the kernel is given for the pane (the staged build loads a dword astride it byte by byte)."""
    import torch
    from moving_object_detector_amd import capi
    mw, mh, frames = 70, 37, 2
    cals = [rm.distorted(mw, mh, e) for e in (0, 1)]
    q = [rm.build_map(c, 0, 0, mw, mh) for c in cals]
    ix, iy = q[1][..., 0] >> 5, q[1][..., 1] >> 5
    rows_in = (iy >= 0) & (iy + 1 < mh)
    assert ((ix == -1) & rows_in).any() and ((ix == mw - 1) & rows_in).any()      # half in, half out, at both edges of the pane
    ax, ay = q[1][..., 0] & 31, q[1][..., 1] & 31
    wx = np.where(ix == mw - 1, 32 - ax, np.where(ix == mw - 2, ax, 0))
    wy = np.where(iy == mh - 1, 32 - ay, np.where(iy == mh - 2, ay, 0))
    assert ((wx > 0) & (wy > 0)).any()                                            # a tap with weight on the pane's last pixel
    ctx = make_ctx(mw, mh)
    ctx.set_rectification(*cams(cals))
    try:
        for enc in ("bgr8", "yuv422_yuy2"):
            for pad in (64, 0, 1):
                Cn = ym.CHANNELS[ym.NAMES[enc]]
                row = mw * Cn
                lay = (enc, mw, mh, 2 * row + pad, 0, 0)
                rng = np.random.default_rng(Cn + pad)
                a = rng.integers(0, 256, size=(frames, mh, lay[3]), dtype=np.uint8)
                a[:, :, :row] = 255
                b = rng.integers(0, 256, size=a.shape, dtype=np.uint8)    # the left pane and the padding anew ...
                b[:, :, row:2 * row] = a[:, :, row:2 * row]    # ... the right pane kept
                ctx.set_image_layout(capi.image_layout(*lay))
                ctx.set_side_by_side(True)
                want = [ym.rectify(m, ym.Layout(*lay), q[1], frames, 1) for m in (a, b)]
                cut, cl = ym.cut_pane(a, ym.Layout(*lay), 1, frames)
                assert np.array_equal(want[0], ym.rectify(cut, cl, q[1], frames)) and np.array_equal(want[0], want[1])
                edge = ((ix == -1) | (ix == mw - 1)) & rows_in
                assert (want[0][:, edge] != 255).any()
                for k, m in enumerate((a, b)):
                    for src_off in (0, 1):    # the message's last byte on and off the dword grid
                        src = torch.empty(src_off + m.size, dtype=torch.uint8, device=ctx.device)
                        src[src_off:] = torch.from_numpy(m.ravel()).to(ctx.device)
                        got = ctx.rectify(src[src_off:], None, capi.MOD_EYE_RIGHT)
                        ctx.synchronize()
                        got = got.cpu().numpy()
                        if not np.array_equal(got, want[k]):
                            f, y, x = (int(v[0]) for v in np.nonzero(got != want[k]))
                            raise rc.Mismatch({"case": PANES, "encoding": enc, "pad": pad, "message": k, "src_off": src_off,
                                               "first": [f, y, x], "count": int((got != want[k]).sum()), "got": int(got[f, y, x]),
                                               "want": int(want[k][f, y, x])})
                left = ctx.rectify(torch.from_numpy(a.ravel()).to(ctx.device), None, capi.MOD_EYE_LEFT)
                ctx.synchronize()
                assert np.array_equal(left.cpu().numpy(), ym.rectify(a, ym.Layout(*lay), q[0], frames, 0))
                ctx.set_side_by_side(False)
                ctx.set_image_layout(None)
    finally:
        ctx.close()
