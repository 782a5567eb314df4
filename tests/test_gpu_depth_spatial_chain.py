"""GPU: the spatial stage (mod_set_depth_spatial) inside the chain from depth messages to disparity planes: depth filter, then the
spatial stage, then the temporal filter, then registration or conversion, whoever runs it.  Every comparison is between two runs of the
same kernels and is exact.  The rig is tests/test_gpu_depth_chain.py's, copied: a 40 x 24 camera, a 48 x 30 message, four frames, ONE
frame a call (the contexts have max_frames = 1).  Batches of frames a call, and the comparison of the chain with the composed numpy
models, are tests/test_gpu_depth_chain_batches.py's.

(a) Composition: mod_depth_filter_dev, then mod_depth_spatial_dev, then mod_depth_temporal_dev on caller-owned state, then
mod_depth_to_disparity_dev with no setting on the context give, frame after frame, what mod_depth_to_disparity_dev gives with the three
settings on the context, and what mod_submit_depth_host returns as `disparity`: filter off / window 5, spatial window 3 / 7, temporal
off / on, unregistered / registered / registered with footprints.
(b) Origins (1, 3) and (8, 6) with filter window 5 and spatial window 7: the summed apron of 2 + 3 = 5 message pixels is clamped on the
left, top and bottom, and on the right and bottom; both encodings.  A spatial neighbour outside the window has then itself been
filtered with its full neighbourhood, or the stream would differ from the whole-message calls.
(c) The synchronous call never writes its input.  (d) A ticket keeps the spatial setting of its submit.  (e) After
set_depth_spatial(None) the synchronous and the stream outputs are byte for byte those of a context on which it was never set.
Each compared plane has more than 100 valid pixels, and with the stage on at least one plane differs from the plane with it off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from moving_object_detector_amd import capi  # noqa: E402

W, H, FR, DT = 40, 24, 4, 1.0 / 15.0
MW, MH = 48, 30                              # the unregistered message
PAD = {"16UC1": 6, "32FC1": 8}               # bytes of row padding: 6, and for 32FC1 the next multiple of the sample size (the ABI wants one)
DW, DH = 24, 16                              # the depth camera of the registered cases
ORIGINS = [(1, 3), (8, 6)]
BYTES = {"16UC1": 2, "32FC1": 4}
DROPPED, GATE = (12, 20), (6, 30)            # (row, column) in the unregistered message: inside the window at either origin
TF = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))


def _filter(window):
    return capi.depth_filter(0.3, 6.0, window, {3: 3, 5: 8}[window], 0.03, 0.02) if window else None


def _spatial(window):
    return capi.depth_spatial(window, True, {3: 3, 5: 6, 7: 8}[window], 0.03, 0.02) if window else None


def _temporal(on, alpha=0.5):
    return capi.depth_temporal(alpha, 0.05, 0.01, 1) if on else None


def _messages(encoding, width, height, dropped, gate, seed):
    """FR messages of a wall at about 2 m, millimetre noise from frame to frame (inside the gate), flying pixels and holes for the
    spatial stages, `dropped` without a reading in frames 1 and 2, and a 3 x 3 block at `gate` that jumps by a metre in frame 2"""
    rng = np.random.default_rng(seed)
    B, step = BYTES[encoding], width * BYTES[encoding] + PAD[encoding]
    base = 2.0 + 0.3 * np.sin(np.arange(width) / 7.0)[None, :] + 0.01 * np.arange(height)[:, None]
    flying = rng.random((height, width)) < 0.04
    out = []
    for f in range(FR):
        z = base + rng.normal(0.0, 0.004, size=base.shape)
        z[flying] += rng.uniform(0.3, 1.0, size=int(flying.sum()))
        z[rng.random(z.shape) < 0.02] = 0.0                              # no reading
        z[gate[0] - 1:gate[0] + 2, gate[1] - 1:gate[1] + 2] = base[gate] + (1.0 if f >= 2 else 0.0)
        z[dropped] = 0.0 if f in (1, 2) else base[dropped]
        if encoding == "16UC1":
            img = np.rint(1000.0 * z).astype("<u2")
        else:
            img = np.where(z > 0.0, z, np.nan).astype("<f4")
        msg = rng.integers(0, 256, size=(height, step), dtype=np.uint8)    # the padding holds noise
        msg[:, :width * B] = img.view(np.uint8).reshape(height, width * B)
        out.append(msg)
    return out


class Rig:
    """A context with its camera, layout and registration (`kind`: "plain", "registered" or "splat"), and its messages"""

    def __init__(self, kind, encoding="16UC1", origin=ORIGINS[0]):
        from moving_object_detector_amd import synth
        from moving_object_detector_amd.pipeline import Context
        self.kind, self.encoding = kind, encoding
        self.ctx = Context(W, H, max_frames=1, max_objects=16)
        cam = synth.make_camera(W, H)
        cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(63.0)
        self.ctx.set_camera(cam)
        self.ctx.set_params(synth.Params())
        B = BYTES[encoding]
        if kind == "plain":
            self.msgs = _messages(encoding, MW, MH, DROPPED, GATE, 11)
            self.lay = self.layout(origin)
        else:
            a = np.radians(0.5)
            R = [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)]
            s = DW / W * 1.05                                               # a little more than the window's field of view
            self.ctx.set_depth_registration(capi.depth_registration(cam.fx * s, cam.fy * s, (DW - 1) / 2.0, (DH - 1) / 2.0, R, (0.01, 0.002, 0.0)))
            self.ctx.set_depth_splat(kind == "splat")
            self.msgs = _messages(encoding, DW, DH, (8, 12), (4, 5), 12)
            self.lay = capi.depth_layout(encoding, DW, DH, DW * B + PAD[encoding])
        self.ctx.set_depth_layout(self.lay)
        self.image = [np.random.default_rng(20 + f).integers(0, 256, size=(H, W), dtype=np.uint8) for f in range(FR)]

    def layout(self, origin):
        return capi.depth_layout(self.encoding, MW, MH, MW * BYTES[self.encoding] + PAD[self.encoding], *origin)

    def settings(self, flt, spa, tmp):
        self.ctx.set_depth_filter(flt)
        self.ctx.set_depth_spatial(spa)
        self.ctx.set_depth_temporal(tmp)          # (every call empties the context's state)

    def dev(self, f):
        return torch.from_numpy(self.msgs[f].reshape(-1).copy()).to(self.ctx.device)

    def composed(self, flt, spa, tmp, frames=range(FR)):
        """the stand-alone calls in sequence, no setting on the context, the temporal filter's state the caller's"""
        self.settings(None, None, None)
        n = self.lay.width * self.lay.height
        state = (torch.zeros(n, dtype=torch.float32, device=self.ctx.device), torch.full((n,), 255, dtype=torch.uint8, device=self.ctx.device))
        out = []
        for f in frames:
            m = self.dev(f)
            if flt is not None:
                m = self.ctx.depth_filter(m, self.lay, flt)
            if spa is not None:
                m = self.ctx.depth_spatial(m, self.lay, spa)
            if tmp is not None:
                m = self.ctx.depth_temporal(m, self.lay, tmp, state=state)
            out.append(self.ctx.depth_to_disparity(m, self.lay)[0].cpu().numpy())
        return out

    def synchronous(self, flt, spa, tmp, frames=range(FR), configure=True):
        """mod_depth_to_disparity_dev with the settings on the context; the caller's messages must come back untouched"""
        if configure:
            self.settings(flt, spa, tmp)
        out = []
        for f in frames:
            m = self.dev(f)
            out.append(self.ctx.depth_to_disparity(m, self.lay)[0].cpu().numpy())
            assert m.cpu().numpy().tobytes() == self.msgs[f].tobytes(), "the caller's input was written"
        return out

    def stream(self, flt, spa, tmp, frames=range(FR), between=None, configure=True):
        """mod_submit_depth_host, caller-transform kind, scene flow only: the tickets' disparity planes (None: the frame took no ticket);
        between(f, stream) runs after the submit of frame f, while its ticket is outstanding"""
        from moving_object_detector_amd.host_stream import HostStream
        if configure:
            self.settings(flt, spa, tmp)
        s = HostStream(self.ctx, FR, 0, outputs=("disparity",))
        s.forget_previous()
        for f in frames:
            s.submit_depth(f, self.image[f], self.msgs[f], capi.flow_params(levels=1), None, TF, DT)
            if between:
                between(f, s)
        s.finish()
        assert all(s.rc[f] == 0 for f in frames if s.first[f] == 0), s.rc
        return [s.disparity[f].copy() if s.first[f] == 0 else None for f in range(FR)], s.first

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def rigs():
    """one context per (kind, encoding, origin), made when first asked for and shared by the tests (each sets what it needs)"""
    made = {}

    def get(kind, encoding="16UC1", origin=ORIGINS[0]):
        key = (kind, encoding, origin if kind == "plain" else None)
        if key not in made:
            made[key] = Rig(*key[:2], origin)
        return made[key]
    yield get
    for r in made.values():
        r.close()


def _same(a, b, what):
    assert a.tobytes() == b.tobytes(), (what, np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:6])


def _composition(rig, window, spatial, temporal):
    flt, spa, tmp = _filter(window), _spatial(spatial), _temporal(temporal)
    want = rig.composed(flt, spa, tmp)
    got = rig.synchronous(flt, spa, tmp)
    for f in range(FR):
        _same(got[f], want[f], ("synchronous", f))
    tickets, first = rig.stream(flt, spa, tmp)
    assert first == [capi.MOD_SKIP_NO_FLOW, 0, 0, 0]                    # no previous image yet: the chain ran all the same
    for f in range(1, FR):
        _same(tickets[f], want[f], ("stream", f))
    rig.settings(None, None, None)
    assert all((d > 0).sum() > 100 for d in want), "hardly a valid pixel: the comparison would be weak"
    off = rig.composed(flt, None, tmp)
    assert any(want[f].tobytes() != off[f].tobytes() for f in range(FR)), "the spatial stage changed nothing"
    return want, off


@pytest.mark.parametrize("kind", ["plain", "registered", "splat"])
@pytest.mark.parametrize("temporal", [False, True], ids=["temporal off", "temporal on"])
@pytest.mark.parametrize("spatial", [3, 7], ids=["spatial 3", "spatial 7"])
@pytest.mark.parametrize("window", [0, 5], ids=["filter off", "filter 5"])
def test_composition(rigs, window, spatial, temporal, kind):
    want, off = _composition(rigs(kind), window, spatial, temporal)
    if kind == "plain" and not window and not temporal:                 # the stage fills holes: more valid pixels than with it off
        assert sum(int((d > 0).sum()) for d in want) > sum(int((d > 0).sum()) for d in off)


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
@pytest.mark.parametrize("origin,clamped", zip(ORIGINS, [{"left", "top", "bottom"}, {"right", "bottom"}]), ids=["left, top and bottom", "right and bottom"])
def test_origins(rigs, origin, clamped, encoding):
    room = {"left": origin[0], "top": origin[1], "right": MW - origin[0] - W, "bottom": MH - origin[1] - H}
    assert {side for side, pixels in room.items() if pixels < 5 // 2 + 7 // 2} == clamped      # where the summed apron of 5 does not fit
    _composition(rigs("plain", encoding, origin), 5, 7, True)


def test_the_apron_is_the_sum_of_both(rigs):
    """with the window at (8, 6) there is room on the left and on top: a stream that staged the filter's apron alone, or the spatial
    stage's alone, would hand the spatial stage unfiltered or missing neighbours along those two sides.  The composition holds with
    either stage alone too (the other's apron is 0)."""
    rig = rigs("plain", "16UC1", ORIGINS[1])
    _composition(rig, 0, 7, False)
    want, _ = _composition(rig, 5, 7, False)
    alone = rig.composed(None, _spatial(7), None)
    assert any(want[f].tobytes() != alone[f].tobytes() for f in range(FR)), "the depth filter changed nothing ahead of the stage"


@pytest.mark.parametrize("window", [0, 5], ids=["spatial alone", "behind the filter"])
def test_the_synchronous_call_does_not_write_its_input(rigs, window):
    rig = rigs("plain")
    rig.synchronous(_filter(window), _spatial(7), None)                # (asserts it, frame by frame)
    rig.synchronous(_filter(window), _spatial(3), _temporal(True))
    rig.settings(None, None, None)


def test_a_ticket_keeps_the_spatial_setting_of_its_submit(rigs):
    rig = rigs("plain")
    ctx = rig.ctx
    a = (_filter(5), _spatial(3), _temporal(True))

    def change(f, s):
        if f == 1:                                                      # ticket 1 is outstanding
            ctx.set_depth_spatial(_spatial(7))

    def off(f, s):
        if f == 1:
            ctx.set_depth_spatial(None)
    try:
        throughout, _ = rig.stream(*a, frames=range(3))
        for between in (change, off):
            changed, first = rig.stream(*a, frames=range(3), between=between)
            assert first[:3] == [capi.MOD_SKIP_NO_FLOW, 0, 0]
            _same(changed[1], throughout[1], "the frame submitted before the change")
            assert changed[2].tobytes() != throughout[2].tobytes(), "the change did not reach the next frame"
    finally:
        rig.settings(None, None, None)


@pytest.mark.parametrize("kind", ["plain", "splat"])
def test_off_is_byte_identical_to_never_set(rigs, kind):
    """a context that had the stage on and then off against a fresh one that never heard of it: the synchronous call and the stream,
    with the other two filters on (their scratch and apron are what the stage shares)"""
    flt, tmp = _filter(5), _temporal(True)
    fresh = Rig(kind)
    try:
        fresh.ctx.set_depth_filter(flt)
        fresh.ctx.set_depth_temporal(tmp)
        want_sync = fresh.synchronous(None, None, None, configure=False)
        fresh.ctx.set_depth_temporal(tmp)                               # (empties the state)
        want_stream, _ = fresh.stream(None, None, None, configure=False)
        assert bytes(fresh.ctx.get_depth_spatial()) == bytes(32)
    finally:
        fresh.close()
    rig = rigs(kind)
    try:
        on = rig.synchronous(flt, _spatial(7), tmp)
        rig.stream(flt, _spatial(7), tmp)
        rig.ctx.set_depth_spatial(None)
        assert bytes(rig.ctx.get_depth_spatial()) == bytes(32)
        rig.ctx.set_depth_temporal(tmp)
        got_sync = rig.synchronous(None, None, None, configure=False)
        rig.ctx.set_depth_temporal(tmp)
        got_stream, first = rig.stream(None, None, None, configure=False)
        assert first == [capi.MOD_SKIP_NO_FLOW, 0, 0, 0]
        for f in range(FR):
            _same(got_sync[f], want_sync[f], ("synchronous", f))
        for f in range(1, FR):
            _same(got_stream[f], want_stream[f], ("stream", f))
        assert any(on[f].tobytes() != want_sync[f].tobytes() for f in range(FR)), "the stage had changed nothing while it was on"
        assert all((d > 0).sum() > 100 for d in want_sync)
    finally:
        rig.settings(None, None, None)
