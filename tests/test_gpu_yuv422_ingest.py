"""GPU: k_to_mono (csrc/ingest.hip) for the packed YUV 4:2:2 encodings through mod_image_to_mono_dev, bit for bit against
tests/models/yuv422_model.py, on the grid of tests/test_gpu_ingest.py::test_matches_the_model — widths around the 16-pixel runs and
the dword grid, exact and padded steps, window origins (odd x0 included), frame counts, source and destination addresses off the
dword grid, guard bytes round the output.  Every case runs twice: the second time every byte that is not a LUMA byte of the window
(the chroma inside the window, the padding, the rest of the message, the bytes behind the last frame) is random anew and the output
must not change."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import yuv422_model as ym  # noqa: E402

ENCODINGS = (("yuv422", 1), ("yuv422_yuy2", 0))          # name, the byte of a pixel that holds its luma
TAIL = 32                                                # bytes behind the last frame, in the device allocation


def _ctx(W, H):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(synth.make_camera(W, H))
    return ctx


def _convert(ctx, payload, tail, lay, F, src_off, dst_off):
    """payload: F frames of step * height bytes, `tail`: the bytes behind them; the device copy starts src_off bytes into its
    allocation, the grey planes dst_off bytes into theirs.  Returns the grey planes; the bytes round them must survive."""
    from moving_object_detector_amd import capi
    dev = ctx.device
    src = torch.empty(src_off + payload.size + tail.size, dtype=torch.uint8, device=dev)
    src[src_off:] = torch.from_numpy(np.concatenate([payload, tail])).to(dev)
    n = F * ctx.height * ctx.width
    dst = torch.full((n + dst_off + 64,), 0xA5, dtype=torch.uint8, device=dev)
    out = dst[dst_off:dst_off + n].view(F, ctx.height, ctx.width)
    ctx.image_to_mono(src[src_off:src_off + payload.size], capi.image_layout(*lay), out=out)
    ctx.synchronize()
    d = dst.cpu().numpy()
    assert (d[:dst_off] == 0xA5).all() and (d[dst_off + n:] == 0xA5).all(), "wrote outside the grey planes"
    return d[dst_off:dst_off + n].reshape(F, ctx.height, ctx.width)


@pytest.mark.parametrize("W", [2, 3, 15, 17, 63, 64, 65, 1281])
def test_matches_the_model(W):
    H = 5
    ctx = _ctx(W, H)
    rng = np.random.default_rng(100 + W)
    mw, mh = W + 7, H + 5
    origins = [(0, 0), (1, 1), (3, 2), ((mw - W) // 2, (mh - H) // 2)]
    case = 0
    for enc, luma in ENCODINGS:
        for pad in (0, 1, 3, 64):
            step = mw * 2 + pad
            for (x0, y0) in origins:
                for F in (1, 3):
                    case += 1
                    lay = (enc, mw, mh, step, x0, y0)
                    a = rng.integers(0, 256, size=F * step * mh, dtype=np.uint8)
                    tail = rng.integers(0, 256, size=TAIL, dtype=np.uint8)
                    want = ym.to_mono(a, ym.Layout(*lay), W, H, F)
                    src_off, dst_off = case % 5, (case // 5) % 3
                    got = _convert(ctx, a, tail, lay, F, src_off, dst_off)
                    assert np.array_equal(got, want), (enc, pad, x0, y0, F, src_off, dst_off)
                    # everything but the window's luma bytes anew: the same output
                    b = rng.integers(0, 256, size=a.size, dtype=np.uint8)
                    keep = np.zeros((F, mh, step), bool)
                    keep[:, y0:y0 + H, 2 * x0 + luma:2 * (x0 + W):2] = True
                    assert keep.sum() == F * H * W
                    b[keep.ravel()] = a[keep.ravel()]
                    tail2 = rng.integers(0, 256, size=TAIL, dtype=np.uint8)
                    assert np.array_equal(_convert(ctx, b, tail2, lay, F, src_off, dst_off), got), (enc, pad, x0, y0, F, "second run")
    ctx.close()


@pytest.mark.parametrize("enc", [e for e, _ in ENCODINGS])
def test_eight_frames_at_1080p(enc):
    W, H, F = 1920, 1080, 8
    ctx = _ctx(W, H)
    mw, mh = 1936, 1090
    lay = (enc, mw, mh, mw * 2 + 3, 9, 5)
    a = np.random.default_rng(7).integers(0, 256, size=F * lay[3] * mh, dtype=np.uint8)
    assert np.array_equal(_convert(ctx, a, np.zeros(0, np.uint8), lay, F, 1, 0), ym.to_mono(a, ym.Layout(*lay), W, H, F))
    ctx.close()
