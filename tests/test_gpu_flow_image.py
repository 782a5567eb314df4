"""GPU: the flow image and the residual-flow image (mod_flow_image_dev, mod_flow_residual_image_dev; k_flow_image) bit for bit
against tests/models/flow_image_model.py.  Shapes 37 x 5 (W no multiple of 4: frame 1 starts one pixel into a four-pixel group),
64 x 3 (W a multiple of 16) and 4 x 1 (a single run), two frames each; the field holds every octant, exact zeros, +-0, denormals, NaN
in x only, in y only and in both, +-inf, +-1e6 and vectors at max_px (1 +- 1 ulp).  Written with out= into a buffer with guard bytes
on both sides."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import flow_image_model as M  # noqa: E402

f32 = np.float32
SHAPES = [(37, 5), (64, 3), (4, 1)]          # W x H
F = 2
MAX_PX = 6.5
GUARD = 64


def _specials(max_px):
    r = f32(max_px)
    lo, hi = np.nextafter(r, f32(0)), np.nextafter(r, f32(np.inf))
    nan, inf = np.nan, np.inf
    rows = [(0, 0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0),
            (1e-40, 0), (0, -1e-41), (1e-39, 1e-39), (-1e-20, 1e-38), (1.1754944e-38, 0),
            (nan, 1), (1, nan), (nan, nan), (inf, 1), (1, -inf), (-inf, inf), (inf, nan),
            (1e6, 1e6), (-1e6, 1e6), (1e6, -1e6), (-1e6, -1e6), (1e6, 0), (0, -1e6),
            (r, 0), (lo, 0), (hi, 0), (0, r), (0, lo), (0, hi), (-r, 0), (0, -lo), (-hi, 0)]
    for k in range(16):                                            # two vectors in every octant, short and long
        a = (k + 0.5) * np.pi / 8
        rows.append((2.5 * np.cos(a), 2.5 * np.sin(a)))
    return np.array(rows, f32)


def _field(shape, seed, max_px):
    W, H = shape
    rng = np.random.default_rng(seed)
    flow = (rng.standard_normal((F, H * W, 2)) * 4.0).astype(f32)
    sp = _specials(max_px)
    for f in range(F):                                             # as many specials as fit, a different stretch of them per frame
        n = min(len(sp), H * W)
        where = rng.permutation(H * W)[:n]
        flow[f, where] = np.roll(sp, -11 * f - seed, axis=0)[:n]
    return flow.reshape(F, H, W, 2)


@pytest.fixture(scope="module")
def contexts():
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    made = {}
    for W, H in SHAPES:
        ctx = Context(W, H, max_frames=F)
        ctx.set_camera(synth.make_camera(W, H)); ctx.set_params(synth.Params())
        made[(W, H)] = ctx
    yield made
    for ctx in made.values():
        ctx.close()


def _render(ctx, flow, still=None, misalign=0):
    """flow (F, H, W, 2) through Context.flow_image with out= inside guarded bytes; misalign: floats the planes start off the 16-byte grid."""
    n = flow.size
    def dev(a):
        store = torch.zeros(n + 4, dtype=torch.float32, device=ctx.device)
        t = store[misalign:misalign + n]
        t.copy_(torch.from_numpy(a.reshape(-1)))
        return t
    nbytes = 3 * n // 2
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=ctx.device)
    out = buf[GUARD:GUARD + nbytes]
    got = ctx.flow_image(dev(flow), MAX_PX, static=None if still is None else dev(still), out=out)
    assert got.data_ptr() == out.data_ptr()
    ctx.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + nbytes:] == 0xA5).all(), "bytes outside the image were written"
    return host[GUARD:GUARD + nbytes].reshape(flow.shape[:-1] + (3,))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_flow_image_matches_the_model(contexts, shape):
    flow = _field(shape, 1, MAX_PX)
    got, want = _render(contexts[shape], flow), M.flow_image(flow, MAX_PX)
    assert np.array_equal(got, want), (shape, np.argwhere(got != want)[:4])
    if shape != (4, 1):                                            # the field is what the docstring says it is
        fx, fy = flow[..., 0].ravel(), flow[..., 1].ravel()
        assert (np.isnan(fx) & ~np.isnan(fy)).any() and (~np.isnan(fx) & np.isnan(fy)).any() and (np.isnan(fx) & np.isnan(fy)).any()
        assert np.isinf(fx).any() and (np.abs(fx) == 1e6).any() and ((fx == 0) & (fy == 0)).any()
        assert (want == 255).all(-1).any() and (want == 0).all(-1).any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_planes_off_the_16_byte_grid(contexts, shape):
    flow = _field(shape, 2, MAX_PX)
    for mis in (1, 2, 3):
        assert np.array_equal(_render(contexts[shape], flow, misalign=mis), M.flow_image(flow, MAX_PX))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_residual_image_matches_the_model(contexts, shape):
    W, H = shape
    flow = _field(shape, 3, MAX_PX)
    flow = np.where(np.isnan(flow), f32(1.25), flow)               # NaN in the static plane only
    rng = np.random.default_rng(4)
    still = (rng.standard_normal(flow.shape) * 2.0).astype(f32)
    flat = still.reshape(F, H * W, 2)
    for f in range(F):
        flat[f, (f + 1) % (H * W), 0] = np.nan
        flat[f, (f + 2) % (H * W), 1] = np.nan
        flat[f, (f + 3) % (H * W)] = flow.reshape(F, H * W, 2)[f, (f + 3) % (H * W)]      # equal vectors: at rest, or inf - inf
    assert not np.isnan(flow).any() and np.isnan(still).any()
    for mis in (0, 2):
        got, want = _render(contexts[shape], flow, still, misalign=mis), M.flow_image(flow, MAX_PX, static=still)
        assert np.array_equal(got, want), (shape, mis, np.argwhere(got != want)[:4])
    assert (want[0].reshape(-1, 3)[1 % (H * W)] == 0).all()


def test_legend_agrees_with_the_image(contexts):
    from moving_object_detector_amd import capi
    flow = _field((64, 3), 5, MAX_PX)
    got = _render(contexts[(64, 3)], flow).reshape(-1, 3)
    for k in range(0, got.shape[0], 7):
        fx, fy = flow.reshape(-1, 2)[k]
        assert capi.flow_color(float(fx), float(fy), MAX_PX) == tuple(got[k]), (fx, fy)
