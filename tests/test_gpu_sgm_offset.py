"""GPU: the disparity estimator (csrc/sgm.hip) with a minimum-disparity offset (mod_set_disparity_offset), through the C ABI, bit for
bit against tests/models/sgm_offset_model.py on the cases of tests/sgm_offset_cases.py.  What each case reaches is asserted on the CPU,
from the model alone, by tests/test_sgm_offset_model.py.

Every output sits between two guard bands, every pixel of it is written, and an invalid pixel is exactly -1.0f whatever the offset.

Kernels reached with an offset: k_sgm_paths_all<UH, UV> (D = 128; 4 and 8 paths), k_sgm_path_q<.., COST = true> with the padded copy of the
right plane (mod_sgm_path_dev), k_sgm_path_h / k_sgm_path_line (every other D, even and odd), k_sgm_wta16 and k_sgm_wta in their SUB x UNIQ
variants, k_sgm_lr for both left-map types."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import sgm_offset_cases as oc  # noqa: E402
import sgm_filters_model as fm  # noqa: E402

om = oc.om
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD = 1024                        # elements in front of and behind every output
FILL = 0xA5
UNSET = -7.0


def _ctx(W, H, F, d0=None):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(synth.Params())
    if d0 is not None:
        ctx.set_disparity_offset(d0)
    return ctx


def _compute(ctx, left, right, D, P, paths=8, lr_check=True, median=True):
    """mod_sgm_compute_dev on uint8 [F][H][W] -> float32 [F][H][W]; the plane lies between two guard bands."""
    from moving_object_detector_amd import capi
    F, H, W = left.shape
    n = F * H * W
    prm = capi.ModSgmParams(D, P[0], P[1], paths, int(lr_check), int(median))
    buf = torch.full((n + 2 * GUARD,), UNSET, dtype=torch.float32, device=ctx.device)
    tl, tr = torch.from_numpy(np.array(left)).to(ctx.device), torch.from_numpy(np.array(right)).to(ctx.device)
    rc = ctx.lib.mod_sgm_compute_dev(ctx.h, F, tl.data_ptr(), tr.data_ptr(), C.byref(prm), buf.data_ptr() + 4 * GUARD)
    assert rc == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    a = buf.cpu().numpy()
    assert (a[:GUARD] == UNSET).all() and (a[-GUARD:] == UNSET).all()
    out = a[GUARD:-GUARD].reshape(F, H, W)
    assert not (out == UNSET).any()                                   # every pixel is written
    return out


def _check_plane(got, want, d0, D, key):
    assert np.array_equal(got, want), (key, int((got != want).sum()))
    assert ((got == -1.0) | ((got >= d0) & (got <= d0 + D - 1))).all(), key      # invalid is exactly -1, whatever the offset


MODES = [(bits, u, lr, med) for bits in (0, 4) for u in (0, 50) for lr in (True, False) for med in (True, False)]


def _estimator_against_model(W, H, D, d0, modes, P=oc.PENALTIES):
    left, right = oc.shifted_pair(W, H, D, d0, oc.seed_of(W, H, D, d0))
    ctx = _ctx(W, H, 1, d0)
    for paths in (8, 4):
        _, S = oc.volumes(W, H, D, d0, oc.seed_of(W, H, D, d0), paths, P)
        for bits, u, lr_check, median in modes:
            ctx.set_disparity_subpixel(bits)
            ctx.set_disparity_filters(uniqueness_ratio=u)
            got = _compute(ctx, left[None], right[None], D, P, paths, lr_check, median)[0]
            _check_plane(got, om.finish(S, d0, lr_check, median, bits, u), d0, D, (paths, bits, u, lr_check, median))
    ctx.close()


def _paths_against_model(ctx, W, H, D, d0, P, F):
    """mod_sgm_path_dev, all eight directions, on arbitrary 31-bit words: matching cost and path cost, guard bands around both."""
    from moving_object_detector_amd import capi
    wl, wr = oc.stage_words(W, H, D, d0, F)
    dev = ctx.device
    cl, cr = torch.from_numpy(wl.view(np.int32)).to(dev), torch.from_numpy(wr.view(np.int32)).to(dev)
    prm = capi.ModSgmParams(D, P[0], P[1], 8, 1, 1)
    n = F * H * W * D
    Cref = [om.cost_volume(wl[f], wr[f], D, d0) for f in range(F)]
    for direction in range(8):
        L = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        Cv = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        rc = ctx.lib.mod_sgm_path_dev(ctx.h, F, cl.data_ptr(), cr.data_ptr(), C.byref(prm), direction, L.data_ptr() + GUARD, Cv.data_ptr() + GUARD)
        assert rc == 0, ctx.lib.mod_last_error(ctx.h)
        ctx.synchronize()
        Lh, Ch = L.cpu().numpy(), Cv.cpu().numpy()
        for a in (Lh, Ch):
            assert (a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all(), direction
        Lh, Ch = Lh[GUARD:-GUARD].reshape(F, H, W, D), Ch[GUARD:-GUARD].reshape(F, H, W, D)
        for f in range(F):
            assert np.array_equal(Ch[f], Cref[f]), (d0, D, P, f, direction, int((Ch[f] != Cref[f]).sum()))
            want = om.ref.aggregate(Cref[f], P[0], P[1], direction)
            assert np.array_equal(Lh[f], want), (d0, D, P, f, direction, int((Lh[f] != want).sum()))
    return Cref


# ---- a. the four-line D = 128 path ------------------------------------------------------------------------------------------------------
FOUR_LINE = [(W, H, d0) for W, H in oc.FOUR_LINE_SHAPES for d0 in oc.FOUR_LINE_OFFSETS] + [oc.FOUR_LINE_WIDE]


@pytest.mark.parametrize("W,H,d0", FOUR_LINE, ids=lambda v: str(v))
def test_four_line_kernels_with_an_offset(W, H, d0):
    _estimator_against_model(W, H, 128, d0, MODES)


# ---- b. the edges of existence ------------------------------------------------------------------------------------------------------------
def test_an_image_no_wider_than_the_offset_is_all_border():
    """W <= d0 (38 x 12 at d0 = 64): every cost is 31 and every pixel is invalid under the check (exempt from the valid-share condition
    by design: there is nothing to match)."""
    W, H, D, d0 = oc.ALL_BORDER
    left, right = oc.shifted_pair(W, H, D, d0, oc.seed_of(W, H, D, d0))
    ctx = _ctx(W, H, 2, d0)
    for Cf in _paths_against_model(ctx, W, H, D, d0, (6, 96), 2):
        assert (Cf == 31).all()
    for paths in (8, 4):
        for bits in (0, 4):
            ctx.set_disparity_subpixel(bits)
            assert (_compute(ctx, left[None], right[None], D, (6, 96), paths, True, True) == -1.0).all()
            assert (_compute(ctx, left[None], right[None], D, (6, 96), paths, False, True) == float(d0)).all()
    ctx.close()


@pytest.mark.parametrize("W,H,D,d0", oc.EDGES, ids=lambda v: str(v))
def test_widths_at_the_edges_of_the_window(W, H, D, d0):
    """W = d0 + 1 (one column with one disparity), W = d0 + D - 1 and W = d0 + D (the first width with a column free of the border)."""
    assert W in (d0 + 1, d0 + D - 1, d0 + D)
    ctx = _ctx(W, H, 2, d0)
    _paths_against_model(ctx, W, H, D, d0, (6, 96), 2)
    ctx.close()
    _estimator_against_model(W, H, D, d0, [(0, 0, True, True), (4, 0, True, False), (0, 50, False, True), (4, 50, True, True)])


# ---- c. the one-line kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d0", oc.ONE_LINE_OFFSETS)
@pytest.mark.parametrize("D", oc.ONE_LINE_D)
def test_one_line_kernels_with_an_offset(D, d0):
    """Even and odd D; W > d0 + D - 1, so the column x = d0 + D - 1 exists where an odd D's last lane owns its disparity alone and its
    pair of right words was read at word 0 (the relative of the bug DESIGN.md 3.4 records)."""
    W, H = oc.one_line_width(D, d0), oc.ONE_LINE_H
    ctx = _ctx(W, H, 1, d0)
    Cref = _paths_against_model(ctx, W, H, D, d0, (6, 96), 1)
    ctx.close()
    x = d0 + D - 1
    assert (Cref[0][:, x, :] != 31).any() and (Cref[0][:, x - 1, D - 1] == 31).all()     # the last disparity starts to exist at that column
    _estimator_against_model(W, H, D, d0, [(0, 0, True, True), (4, 0, True, True), (0, 50, True, False), (4, 50, False, False), (0, 0, False, True)])


# ---- d. mod_sgm_path_dev ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d0", oc.STAGE_OFFSETS)
@pytest.mark.parametrize("W", oc.STAGE_W)
def test_path_stage_on_arbitrary_words(W, d0):
    """Arbitrary 31-bit words (the zeroed lead in front of the padded right plane would give popcount(word), not 31, if it were
    used), two frames, all eight directions, the matching cost included."""
    ctx = _ctx(W, oc.STAGE_H, 2, d0)
    for D in oc.STAGE_D:
        for P in oc.STAGE_PENALTIES:
            _paths_against_model(ctx, W, oc.STAGE_H, D, d0, P, 2)
    ctx.close()


# ---- e. one context, the offset switched between calls --------------------------------------------------------------------------------------
def test_one_context_switches_the_offset_between_batches():
    """A 3-frame batch at d0 = 64, then 0, then 128, then 0: every call is the model's under its own offset, and the d0 = 0 results are
    those of a context that never set one."""
    W, H, D, F = 140, 12, 128, 3
    pairs = [oc.shifted_pair(W, H, D, 64, 8100 + f) for f in range(F)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    S = {}
    for d0 in (0, 64, 128):
        for f in range(F):
            C_ = om.cost_volume(om.ref.census(left[f]), om.ref.census(right[f]), D, d0)
            S[d0, f] = om.path_sums(C_, 6, 96, 8)[1]
    fresh = _ctx(W, H, F)
    never = _compute(fresh, left, right, D, (6, 96))
    fresh.close()
    ctx = _ctx(W, H, F)
    zero = []
    for d0 in (64, 0, 128, 0):
        ctx.set_disparity_offset(d0)
        got = _compute(ctx, left, right, D, (6, 96))
        for f in range(F):
            _check_plane(got[f], om.finish(S[d0, f], d0), d0, D, (d0, f))
        if d0 == 0:
            zero.append(got)
    ctx.close()
    for got in zero:
        assert np.array_equal(got.view(np.uint32), never.view(np.uint32))
    valid = [float((om.finish(S[d0, 0], d0) >= 0).mean()) for d0 in (0, 64)]
    assert 0.20 <= valid[1] <= 0.95 and valid[0] != valid[1]


def test_speckle_stage_keeps_its_rule_with_an_offset():
    """The estimator's speckle stage behind an offset: pixels >= 0 take part, removed pixels become -1 (not d0 - 1)."""
    W, H, D, d0 = 140, 12, 128, 17
    left, right = oc.shifted_pair(W, H, D, d0, oc.seed_of(W, H, D, d0))
    _, S = oc.volumes(W, H, D, d0, oc.seed_of(W, H, D, d0), 8)
    ctx = _ctx(W, H, 1, d0)
    removed = 0
    for bits in (0, 4):
        ctx.set_disparity_subpixel(bits)
        ctx.set_disparity_filters(0, 12, 1)
        before = om.finish(S, d0, True, True, bits)
        want = fm.speckle(before, 12, 1, 0.0, -1.0)
        removed += int((want != before).sum())
        _check_plane(_compute(ctx, left[None], right[None], D, oc.PENALTIES)[0], want, d0, D, bits)
    assert removed > 0
    ctx.close()


# ---- f. the stream: a frame in flight keeps the offset of its submit, and why the feature exists ---------------------------------------------
def test_stream_tickets_complete_with_the_offset_of_their_submit():
    """mod_submit_stereo_host on the 150-px pair: frame 1 is submitted at d0 = 96, frame 2 at d0 = 0 while frame 1 is in flight, then
    the offset changes again before either is collected.  Frame 1's disparity copy is the model's at 96 (it recovers the shift), frame
    2's the model's at 0 (it cannot)."""
    from moving_object_detector_amd import capi, synth
    from moving_object_detector_amd.pipeline import Context
    W, H, D, shift = oc.NEAR
    left, right = (np.array(a) for a in oc.near_pair())
    cam = synth.make_camera(W, H)
    cam.min_disparity, cam.max_disparity = np.float32(0.0), np.float32(255.0)
    sp = capi.ModSgmParams(D, 6, 96, 8, 1, 1)
    tf = capi.transforms_array(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]))
    flow = np.zeros((H, W, 2), np.float32)
    plane = {d0: om.compute(left, right, D, 6, 96, 8, True, True, d0) for d0 in (0, oc.NEAR_OFFSET)}
    settings = [0, oc.NEAR_OFFSET, 0]
    ctx = Context(W, H, max_frames=1)
    ctx.set_camera(cam)
    ctx.set_params(synth.Params(cluster_size=150))
    n_px = H * W
    disp = np.full((len(settings), n_px + 2 * GUARD), UNSET, np.float32)
    objs = [(capi.ModObject * 8)() for _ in settings]
    t, n = C.c_int32(-1), C.c_int32(-1)
    tickets = []
    for f, d0 in enumerate(settings):
        ctx.set_disparity_offset(d0)                                  # frame f - 1 is still in flight
        rc = ctx.lib.mod_submit_stereo_host(ctx.h, left.ctypes.data, right.ctypes.data, C.byref(sp), flow.ctypes.data, C.byref(tf[0]), 1.0 / 15.0,
                                            None, None, objs[f], 8, disp[f, GUARD:].ctypes.data if f else None, C.byref(t))
        if f == 0:
            assert rc == capi.MOD_SKIP_NO_DISPARITY_PREV and t.value == -1
        else:
            assert rc == 0, ctx.lib.mod_last_error(ctx.h)
            tickets.append(t.value)
    ctx.set_disparity_offset(128)                                     # changing it now does not reach the frames in flight
    for tk in tickets:
        assert ctx.lib.mod_collect_frame_host(ctx.h, tk, C.byref(n)) == 0, ctx.lib.mod_last_error(ctx.h)
    ctx.close()
    interior = np.zeros((H, W), bool)
    interior[3:H - 3, shift + 4:W - 4] = True
    for f in (1, 2):
        d0 = settings[f]
        assert (disp[f, :GUARD] == UNSET).all() and (disp[f, -GUARD:] == UNSET).all()
        got = disp[f, GUARD:-GUARD].reshape(H, W)
        _check_plane(got, plane[d0], d0, D, f)
    assert float((disp[1, GUARD:-GUARD].reshape(H, W)[interior] == shift).mean()) >= 0.95
    assert float((disp[2, GUARD:-GUARD].reshape(H, W)[interior] == shift).mean()) <= 0.03
