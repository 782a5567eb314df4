"""GPU: the chain from depth messages to disparity planes (filter, then temporal filter, then registration or conversion) is one chain,
whoever runs it.  Every comparison is between two runs of the same kernels and is exact, and every call here carries ONE frame (the
contexts have max_frames = 1): batches of frames a call, and the comparison of the chain with the composed numpy models, are
tests/test_gpu_depth_chain_batches.py's.

(a) Composition: mod_depth_filter_dev, then mod_depth_temporal_dev on caller-owned state, then mod_depth_to_disparity_dev with no filter
set on the context give, frame after frame, what mod_depth_to_disparity_dev gives with the filters set on the context, and what
mod_submit_depth_host returns as `disparity` for the same messages: filter off / window 3 / window 5, temporal filter off / on with
hold 1, unregistered / registered / registered with footprints.  Four consecutive frames a case (the stream's first frame finds no
previous image and takes no ticket: its three others are compared), with a pixel that drops out for two frames (held once, then
emptied) and a block that leaves the gate.
(b) Shapes, the smallest at which the arithmetic of the staged window can go wrong: a 40 x 24 camera; unregistered, a 48 x 30 message
with 6 bytes of row padding (32FC1: 8, since a step must be a multiple of the sample size) and the window at (1, 3) (a window-5 apron
is clamped on the left only) and at (8, 6) (clamped right and bottom), both encodings; registered, a 24 x 16 depth camera whose whole
message is scattered into the window.
(c) The synchronous call never writes its input, with the temporal filter alone and with both filters.
(d) A ticket keeps the settings of its submit: filter, temporal filter and footprints all change while it is outstanding.
(e) What empties the temporal filter's state: mod_set_depth_temporal, mod_reset_depth_temporal, mod_forget_previous, a depth submit
skipped for a NULL depth, and a layout of another origin; and nothing else."""
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


def _temporal(on, alpha=0.5):
    return capi.depth_temporal(alpha, 0.05, 0.01, 1) if on else None


def _messages(encoding, width, height, dropped, gate, seed):
    """FR messages of a wall at about 2 m, millimetre noise from frame to frame (inside the gate), flying pixels and holes for the
    spatial filter, `dropped` without a reading in frames 1 and 2, and a 3 x 3 block at `gate` that jumps by a metre in frame 2"""
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

    def settings(self, flt, tmp):
        self.ctx.set_depth_filter(flt)
        self.ctx.set_depth_temporal(tmp)          # (every call empties the context's state)

    def dev(self, f):
        return torch.from_numpy(self.msgs[f].reshape(-1).copy()).to(self.ctx.device)

    def composed(self, flt, tmp, frames=range(FR)):
        """the stand-alone calls, no filter set on the context, the temporal filter's state the caller's"""
        self.settings(None, None)
        n = self.lay.width * self.lay.height
        state = (torch.zeros(n, dtype=torch.float32, device=self.ctx.device), torch.full((n,), 255, dtype=torch.uint8, device=self.ctx.device))
        out = []
        for f in frames:
            m = self.dev(f)
            if flt is not None:
                m = self.ctx.depth_filter(m, self.lay, flt)
            if tmp is not None:
                m = self.ctx.depth_temporal(m, self.lay, tmp, state=state)
            out.append(self.ctx.depth_to_disparity(m, self.lay)[0].cpu().numpy())
        return out

    def synchronous(self, flt, tmp, frames=range(FR)):
        """mod_depth_to_disparity_dev with the filters set on the context; the caller's messages must come back untouched"""
        self.settings(flt, tmp)
        out = []
        for f in frames:
            m = self.dev(f)
            out.append(self.ctx.depth_to_disparity(m, self.lay)[0].cpu().numpy())
            assert m.cpu().numpy().tobytes() == self.msgs[f].tobytes(), "the caller's input was written"
        return out

    def stream(self, flt, tmp, frames=range(FR), between=None):
        """mod_submit_depth_host, caller-transform kind, scene flow only: the tickets' disparity planes (None: the frame took no ticket);
        between(f, stream) runs after the submit of frame f, while its ticket is outstanding"""
        from moving_object_detector_amd.host_stream import HostStream
        self.settings(flt, tmp)
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


def _composition(rig, window, temporal):
    flt, tmp = _filter(window), _temporal(temporal)
    want = rig.composed(flt, tmp)
    got = rig.synchronous(flt, tmp)
    for f in range(FR):
        _same(got[f], want[f], ("synchronous", f))
    tickets, first = rig.stream(flt, tmp)
    assert first == [capi.MOD_SKIP_NO_FLOW, 0, 0, 0]                    # no previous image yet: the chain ran all the same
    for f in range(1, FR):
        _same(tickets[f], want[f], ("stream", f))
    rig.settings(None, None)
    return want


@pytest.mark.parametrize("kind", ["plain", "registered", "splat"])
@pytest.mark.parametrize("temporal", [False, True], ids=["temporal off", "temporal on"])
@pytest.mark.parametrize("window", [0, 3, 5])
def test_composition(rigs, window, temporal, kind):
    rig = rigs(kind)
    want = _composition(rig, window, temporal)
    assert all((d > 0).sum() > 100 for d in want), "hardly a valid pixel: the comparison would be weak"
    plain = rig.composed(None, None)
    if window or temporal:
        assert any(want[f].tobytes() != plain[f].tobytes() for f in range(FR)), "the filters changed nothing"
    if kind == "plain" and temporal and not window:                     # the scene holds what it says it holds
        x0, y0 = ORIGINS[0]
        drop, gate = (DROPPED[0] - y0, DROPPED[1] - x0), (GATE[0] - y0, GATE[1] - x0)
        assert plain[1][drop] < 0 and want[1][drop] > 0, "the dropped pixel is held for one frame"
        assert plain[2][drop] < 0 and want[2][drop] < 0, "... and emptied after it"
        assert want[2][gate] == plain[2][gate], "the block leaves the gate in frame 2: a restart, and a blend would lie half a metre off"


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
@pytest.mark.parametrize("origin,clamped", zip(ORIGINS, [{"left"}, {"right", "bottom"}]), ids=["left", "right and bottom"])
def test_shapes_plain(rigs, origin, clamped, encoding):
    room = {"left": origin[0], "top": origin[1], "right": MW - origin[0] - W, "bottom": MH - origin[1] - H}
    assert {side for side, pixels in room.items() if pixels < 5 // 2} == clamped      # where a window-5 apron does not fit
    _composition(rigs("plain", encoding, origin), 5, True)


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_shapes_registered(rigs, encoding):
    _composition(rigs("registered", encoding), 5, True)


@pytest.mark.parametrize("window", [0, 3], ids=["temporal alone", "both filters"])
def test_the_synchronous_call_does_not_write_its_input(rigs, window):
    rig = rigs("plain")
    rig.synchronous(_filter(window), _temporal(True))                  # (asserts it, frame by frame)
    rig.settings(None, None)


def test_a_ticket_keeps_the_settings_of_its_submit(rigs):
    rig = rigs("splat")
    ctx = rig.ctx
    a = (_filter(3), _temporal(True))

    def change(f, s):
        if f == 1:                                                      # ticket 1 is outstanding
            ctx.set_depth_filter(_filter(5))
            ctx.set_depth_temporal(None)
            ctx.set_depth_splat(False)
    try:
        throughout, _ = rig.stream(*a, frames=range(3))
        changed, first = rig.stream(*a, frames=range(3), between=change)
        assert first[:3] == [capi.MOD_SKIP_NO_FLOW, 0, 0]
        _same(changed[1], throughout[1], "the frame submitted before the change")
        assert changed[2].tobytes() != throughout[2].tobytes(), "the change did not reach the next frame"
    finally:
        ctx.set_depth_splat(True)
        rig.settings(None, None)


def _skipped_submit(rig):
    from moving_object_detector_amd.host_stream import HostStream
    s = HostStream(rig.ctx, 1, 0, outputs=("disparity",))
    assert s.submit_depth(0, rig.image[0], None, capi.flow_params(levels=1), None, TF, DT) == capi.MOD_SKIP_NO_DISPARITY_NOW


RESETS = {
    "mod_set_depth_temporal": lambda rig: rig.ctx.set_depth_temporal(_temporal(True)),
    "mod_reset_depth_temporal": lambda rig: rig.ctx.reset_depth_temporal(),
    "mod_forget_previous": lambda rig: rig.ctx._check(rig.ctx.lib.mod_forget_previous(rig.ctx.h)),
    "a skipped depth submit": _skipped_submit,
    "nothing": None,
}


@pytest.fixture(scope="module")
def fresh_first_frames():
    """message 2 as the first frame of a context without history, at both origins (computed once; the tests leave it unchanged)"""
    out = {}
    for origin in ORIGINS:
        rig = Rig("plain", "16UC1", origin)
        try:
            out[origin] = rig.synchronous(None, _temporal(True), frames=[2])[0]
        finally:
            rig.close()
    return out


@pytest.mark.parametrize("reset", list(RESETS))
def test_what_empties_the_temporal_state(rigs, fresh_first_frames, reset):
    """frames 0 and 1 through the synchronous call, the reset, then frame 2: the first frame of a fresh context, unless nothing was reset"""
    rig = rigs("plain")
    try:
        rig.synchronous(None, _temporal(True), frames=[0, 1])
        if RESETS[reset]:
            RESETS[reset](rig)
        m = rig.dev(2)
        got = rig.ctx.depth_to_disparity(m, rig.lay)[0].cpu().numpy()
        if RESETS[reset]:
            _same(got, fresh_first_frames[ORIGINS[0]], reset)
        else:
            assert got.tobytes() != fresh_first_frames[ORIGINS[0]].tobytes(), "the history did not matter: the resets would show nothing"
    finally:
        rig.settings(None, None)


def test_a_layout_of_another_origin_empties_the_temporal_state(rigs, fresh_first_frames):
    """the stream stages the window: with the window elsewhere in the message the state's lattice lies elsewhere, and the history is gone.
    The same submits without the change carry it."""
    rig = rigs("plain")

    def move(f, s):
        if f == 1:
            rig.ctx.set_depth_layout(rig.layout(ORIGINS[1]))
    try:
        moved, first = rig.stream(None, _temporal(True), frames=range(3), between=move)
        assert first[:3] == [capi.MOD_SKIP_NO_FLOW, 0, 0]
        _same(moved[2], fresh_first_frames[ORIGINS[1]], "frame 2, the window at another origin")
        rig.ctx.set_depth_layout(rig.lay)
        stayed, _ = rig.stream(None, _temporal(True), frames=range(3))
        assert stayed[2].tobytes() != fresh_first_frames[ORIGINS[0]].tobytes()
    finally:
        rig.ctx.set_depth_layout(rig.lay)
        rig.settings(None, None)
