"""GPU: the disparity estimator (csrc/sgm.hip) on the hostile cases of tests/sgm_cases.py — tie-rich images, penalties at their limits,
winners at the last disparity and at the lane boundaries, disparity counts and image sizes at the kernel-selection edges — bit for bit
against oracle/sgm_ref.cpp (census, cost, every path, S) and the models of tests/models (everything behind S).  What each case
reaches is asserted on the CPU, from the reference alone, by tests/test_sgm_cases.py.

Kernels reached.  Stage by stage: k_sgm_census; k_sgm_path_h<RTL> and k_sgm_path_line<RX, RY> (D != 128: even D with the 2-byte store,
odd D and the last lane of D = 15, 17, 127 with byte stores); k_sgm_path_q<RX, RY, UNIFORM, COST = true> in both UNIFORM variants of
rows and columns and the ragged diagonals, partly filled waves included.  Complete estimator: k_sgm_paths_all<UH, UV> (D = 128, 4 and
8 paths: <true, true> 140 x 12 and 8 x 8, <true, false> 38 x 12, <false, true> 36 x 10, <false, false> the other tiny images), the
one-line kernels on their side streams otherwise;
k_sgm_wta16 / k_sgm_wta <SUB, TL, UNIQ> in all four SUB x UNIQ variants each; k_sgm_median3<uint8_t / uint16_t>; k_sgm_lr<TL, UNIQ>
for both left-map types."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import sgm_cases as sc  # noqa: E402
import sgm_filters_model as fm  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD = 4096                        # bytes in front of and behind every volume the path kernels write
FILL = 0xA5


def _ctx(W, H, F):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context
    ctx = Context(W, H, max_frames=F)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(synth.Params())
    return ctx


def _compute(ctx, left, right, D, P1, P2, paths=8, lr_check=True, median=True):
    from moving_object_detector_amd import capi
    F, H, W = left.shape
    prm = capi.ModSgmParams(D, P1, P2, paths, int(lr_check), int(median))
    out = torch.full((F, H, W), -7.0, dtype=torch.float32, device=ctx.device)
    tl, tr = torch.from_numpy(np.array(left)).to(ctx.device), torch.from_numpy(np.array(right)).to(ctx.device)      # (copies: the cases are read-only)
    return ctx.estimate_disparity(tl, tr, prm, out).cpu().numpy()   # (.cpu() waits: the context runs on torch\'s stream)


def _sums(left, right, D, P1, P2, paths):
    from oracle import pysgm
    return pysgm.compute(left, right, D, P1, P2, paths, True, True, want_S=True)[1]


# ---- a. stage by stage ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D,P,F", sc.STAGE, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_census_cost_and_all_eight_paths_at_the_edges(W, H, D, P, F):
    from moving_object_detector_amd import capi
    from oracle import pysgm
    left, right, wl, wr = sc.stage_inputs(W, H, D, F)
    ctx = _ctx(W, H, F)
    dev = ctx.device
    # census, on images (W < 9 or H < 7: every word is 0)
    for img in (left, right):
        t = torch.from_numpy(img).to(dev)
        cen = torch.full((F, H, W), -1, dtype=torch.int32, device=dev)
        assert ctx.lib.mod_sgm_census_dev(ctx.h, F, t.data_ptr(), cen.data_ptr()) == 0, ctx.lib.mod_last_error(ctx.h)
        ctx.synchronize()
        got = cen.cpu().numpy().view(np.uint32)
        for f in range(F):
            assert np.array_equal(got[f], pysgm.census(img[f])), f
        if W < 9 or H < 7:
            assert not got.any()
    # cost and paths, on arbitrary 31-bit words; every volume sits between two guard bands
    cl, cr = torch.from_numpy(wl.view(np.int32)).to(dev), torch.from_numpy(wr.view(np.int32)).to(dev)
    prm = capi.ModSgmParams(D, P[0], P[1], 8, 1, 1)
    n = F * H * W * D
    Cref = [pysgm.cost(wl[f], wr[f], D) for f in range(F)]
    top = 0
    for direction in range(8):
        L = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        Cv = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        rc = ctx.lib.mod_sgm_path_dev(ctx.h, F, cl.data_ptr(), cr.data_ptr(), C.byref(prm), direction, L.data_ptr() + GUARD, Cv.data_ptr() + GUARD)
        assert rc == 0, ctx.lib.mod_last_error(ctx.h)
        ctx.synchronize()
        for name, t in (("L", L), ("C", Cv)):
            a = t.cpu().numpy()
            assert (a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all(), (name, direction)
        Lh, Ch = L.cpu().numpy()[GUARD:-GUARD].reshape(F, H, W, D), Cv.cpu().numpy()[GUARD:-GUARD].reshape(F, H, W, D)
        for f in range(F):
            assert np.array_equal(Ch[f], Cref[f]), (f, direction)
            want = pysgm.aggregate(Cref[f], P[0], P[1], direction)
            assert np.array_equal(Lh[f], want), (f, direction, int((Lh[f] != want).sum()))
            top = max(top, int(want.max()))
    if P[1] == 224 and W >= 130 and D >= 127:
        assert top == 255                                           # the top of the uint8 the kernels store is reached, and matched
    ctx.close()


# ---- b. the complete estimator on every case -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_complete_estimator_on_the_hostile_cases(name):
    c = sc.CASES[name]
    left, right = sc.images(name)
    ctx = _ctx(c.W, c.H, 1)
    for paths in (8, 4):
        S = sc.sums(name, paths)
        for bits in (0, 4):
            ctx.set_disparity_subpixel(bits)
            for u in (0,) + sc.UNIQUENESS:
                ctx.set_disparity_filters(uniqueness_ratio=u)
                for median in (True, False):
                    for lr_check in (True, False):
                        got = _compute(ctx, left[None], right[None], c.D, c.P1, c.P2, paths, lr_check, median)[0]
                        want = fm.compute(S, lr_check, median, bits, uniqueness_ratio=u)
                        assert np.array_equal(got, want), (paths, bits, u, median, lr_check, int((got != want).sum()))
    ctx.close()


# ---- c. different cases as the frames of one call, then the same batch with the mode switched ------------------------------------------
BATCH_FAMILIES = ("tie_rich", "last_disparity", "lane_edges", "flat", "identical", "binary", "saturating_shift")


@pytest.mark.parametrize("W,H,D,P", [(140, 12, 128, (0, 1)), (96, 24, 33, (6, 96))], ids=["d128_paths_all", "d33_side_streams"])
def test_a_batch_of_different_cases_and_mode_switches(W, H, D, P):
    """20 frames go as groups of 7 + 7 + 6: two groups plus a partial one, and the first set of census planes and volumes is used
    twice.  Every frame holds another family (or another seed of it), so a frame that leaked into its neighbour, or a group that read
    the other set, cannot agree with its own model."""
    F = 20
    pairs = [sc.make(BATCH_FAMILIES[f % len(BATCH_FAMILIES)], W, H, D, 300 + f) for f in range(F)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    S = [_sums(left[f], right[f], D, P[0], P[1], 8) for f in range(F)]
    assert len({s.tobytes() for s in S}) >= F - 2                   # (the flat frames are the same frame)
    ctx = _ctx(W, H, F)
    for bits, u in ((4, 50), (0, 50), (0, 0), (4, 0), (4, 50)):     # sub-pixel on then off, uniqueness on then off, and back
        ctx.set_disparity_subpixel(bits)
        ctx.set_disparity_filters(uniqueness_ratio=u)
        got = _compute(ctx, left, right, D, P[0], P[1])
        for f in range(F):
            want = fm.compute(S[f], True, True, bits, uniqueness_ratio=u)
            assert np.array_equal(got[f], want), (bits, u, f, int((got[f] != want).sum()))
    ctx.close()


# ---- d. tiny images end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D,P,F", sc.TINY, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tiny_images_end_to_end(W, H, D, P, F):
    """W < 9 or H < 7: every census word is 0, every cost is 0 or the border's 31 — the result must still be the model's."""
    left, right, _, _ = sc.stage_inputs(W, H, D, F)
    ctx = _ctx(W, H, F)
    for paths in (8, 4):
        S = [_sums(left[f], right[f], D, P[0], P[1], paths) for f in range(F)]
        for bits, u in ((0, 0), (4, 0), (0, 50), (4, 99)):
            ctx.set_disparity_subpixel(bits)
            ctx.set_disparity_filters(uniqueness_ratio=u)
            for median, lr_check in ((True, True), (False, False)):
                got = _compute(ctx, left, right, D, P[0], P[1], paths, lr_check, median)
                for f in range(F):
                    want = fm.compute(S[f], lr_check, median, bits, uniqueness_ratio=u)
                    assert np.array_equal(got[f], want), (paths, bits, u, median, lr_check, f, got[f], want)
    ctx.close()


def test_an_image_one_pixel_wide_is_refused_with_its_reason():
    """The only size the estimator refuses (the path kernels read the right census words in pairs): an error code and a message that
    names the reason, from the complete estimator and from the path stage — never a silent no-op — and nothing is written."""
    from moving_object_detector_amd import capi
    W, H = 1, 5
    ctx = _ctx(W, H, 1)
    dev = ctx.device
    prm = capi.ModSgmParams(8, 6, 96, 8, 1, 1)
    img = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
    out = torch.full((1, H, W), -7.0, dtype=torch.float32, device=dev)
    with pytest.raises(capi.ModError, match="at least 2 pixels wide") as e:
        ctx.estimate_disparity(img, img, prm, out)
    assert e.value.code == capi.MOD_ERR_INVALID_ARGUMENT
    cen = torch.zeros((1, H, W), dtype=torch.int32, device=dev)
    L = torch.full((1, H, W, 8), FILL, dtype=torch.uint8, device=dev)
    assert ctx.lib.mod_sgm_path_dev(ctx.h, 1, cen.data_ptr(), cen.data_ptr(), C.byref(prm), 0, L.data_ptr(), None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert b"at least 2 pixels wide" in ctx.lib.mod_last_error(ctx.h)
    ctx.synchronize()
    assert bool((out == -7.0).all()) and bool((L == FILL).all())
    ctx.close()
