"""GPU: the median / object stage (cluster_median.hip: k_median, k_box_nan, k_median_ties) at its edges — the clusterer alone on
caller planes, bit for bit against the C++ oracle (real std::sort, pcl's min / max fold):

  a. tied clusters on the right edge of large frames, where the tie replay's row arithmetic used to be wrong (test_row_model.py);
  b. k_median's selection rounds: the most rounds the search can take, the kMedDirect boundary, norms of +inf, ties between identical
     vectors, the smallest clusters there are, clusters of exactly cluster_size members;
  c. coordinate boxes with NaN and +-inf in x and y (k_box_nan, box_to_object's +-FLT_MAX start values);
  d. a caller-supplied dynamic mask;
  e. tied frames inside a batch, twice on one workspace (the replay's scratch planes, the counters its last workgroup resets).

Every case first asserts on the host that its input has the property it is named for."""
import os
import sys

import numpy as np
import pytest

from util import bits_equal64, compare_objects_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import median_select_model as msm  # noqa: E402
import row_model  # noqa: E402
sys.path.insert(0, HERE)
import median_edge_cases as mec  # noqa: E402


def _check(ref, planes, prm, W, H):
    from test_gpu_cluster_stress import _cluster_gpu
    rl, ro, rK = ref
    lab, objs, K = _cluster_gpu(planes, prm, W, H)
    assert K == rK, (K, rK)
    assert np.array_equal(lab, rl), int((lab != rl).sum())
    compare_objects_bits(objs, ro)


def _norm_bits(planes, members):
    from oracle import numpy_ref
    return numpy_ref.norm3(planes["vx"][members], planes["vy"][members], planes["vz"][members]).view(np.uint32)


# ---- a. the tie replay's row arithmetic -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("blobs", ["corner", "corner_and_top_left"])
@pytest.mark.parametrize("W,H", mec.RIGHT_EDGE_SHAPES)
def test_tied_cluster_on_the_right_edge_of_a_large_frame(oracle, W, H, blobs):
    planes, prm, corner, first = mec.right_edge_tie_cloud(W, H, blobs == "corner_and_top_left")
    p = np.flatnonzero(corner.ravel()).astype(np.uint32)
    assert p.size >= prm.cluster_size and np.any(p % W == W - 1)
    assert np.any(row_model.row_float(p, W) != p // W), "the F32 row estimate is meant to be wrong for a member of this blob"
    ref = oracle.cluster(planes, prm, "tidy", max_objects=8)
    assert ref[2] == len(ref[1]) == (2 if first.any() else 1) and all(o["ambiguous"] for o in ref[1])
    if first.any():
        q = np.flatnonzero(first.ravel()).astype(np.uint32)
        assert np.array_equal(row_model.row_float(q, W), q // W), "... and right for the blob in the opposite corner"
    _check(ref, planes, prm, W, H)


# ---- b. selection rounds -----------------------------------------------------------------------------------------------------------
def _select_case(oracle, bits, seed, W=256, H=128, dynamic_speed=1e-4):
    from moving_object_detector_amd import synth
    planes, m = mec.norm_blob(W, H, bits, np.random.default_rng(seed))
    got = _norm_bits(planes, m)
    assert np.array_equal(np.sort(got), np.sort(np.asarray(bits, np.uint32))), "the members' norms are meant to have exactly these patterns"
    prm = synth.Params(cluster_size=100, neighbor_distance=2, dynamic_speed=dynamic_speed)
    ref = oracle.cluster(planes, prm, "tidy", max_objects=8)
    assert ref[2] == 1 and ref[1][0]["n_points"] == len(bits)
    return planes, prm, ref, msm.select(got)


def test_selection_takes_two_rounds_and_ends_in_direct_ranking(oracle):
    """Several thousand distinct norms inside fewer than 2^12 consecutive patterns, outliers at 1e-3 and 1e3: the first round's bin of
    the rank holds the whole band, the second round's (64 patterns) ends in direct ranking with shift != 0.  Two rounds is the most such
    a search can have: a round takes 11 bits off a range of at most 31, so a third round always has shift 0
    (median_select_model.py, test_median_select_model.py) — the next test runs that one."""
    W, H = 256, 128
    bits = np.concatenate([mec.band_bits(np.random.default_rng(1)), [mec.F32_1EM3] * 3, [mec.F32_1E3] * 3])
    planes, prm, ref, (rounds, exact, value, nties) = _select_case(oracle, bits, 11)
    assert len(rounds) == 2 and not exact and all(r["shift"] != 0 for r in rounds), rounds
    assert rounds[0]["inbin"] > msm.K_MED_DIRECT >= rounds[1]["inbin"] and nties == 1, rounds
    _check(ref, planes, prm, W, H)


def test_selection_takes_three_rounds(oracle):
    """The same band with outliers at 1e-3 and +inf: shifts 20, 9, 0 — three rounds, the most there can be, more than kMedDirect members
    in the rank's bin after the first two."""
    W, H = 256, 128
    bits = np.concatenate([mec.band_bits(np.random.default_rng(2)), [mec.F32_1EM3] * 3, [mec.F32_INF] * 3])
    planes, prm, ref, (rounds, exact, value, nties) = _select_case(oracle, bits, 12)
    assert [r["shift"] for r in rounds] == [20, 9, 0] and exact and nties == 1, rounds
    assert rounds[0]["inbin"] > msm.K_MED_DIRECT and rounds[1]["inbin"] > msm.K_MED_DIRECT, rounds
    _check(ref, planes, prm, W, H)


@pytest.mark.parametrize("inbin", [255, 256, 257])
def test_selection_at_the_direct_ranking_boundary(oracle, inbin):
    """The rank's bin holds exactly kMedDirect - 1, kMedDirect, kMedDirect + 1 members after the first round: ranked directly, or narrowed once more."""
    W, H = 256, 128
    planes, prm, ref, (rounds, exact, value, nties) = _select_case(oracle, mec.boundary_bits(inbin), 20 + inbin)
    assert rounds[0]["inbin"] == inbin and rounds[0]["shift"] == 17 and not exact, rounds
    assert len(rounds) == (1 if inbin <= msm.K_MED_DIRECT else 2), rounds
    assert rounds[-1]["shift"] != 0 and rounds[-1]["inbin"] <= msm.K_MED_DIRECT, rounds
    _check(ref, planes, prm, W, H)


@pytest.mark.parametrize("n_inf,median_is_inf", [(200, False), (700, True)])
def test_norms_of_infinity(oracle, n_inf, median_is_inf):
    """Members with a component of +-inf, and members with 3e38 whose squared norm overflows: ||v|| = +inf, below or at the median."""
    from moving_object_detector_amd import synth
    from oracle import numpy_ref
    W, H, size = 256, 128, 1200
    rng = np.random.default_rng(n_inf)
    m = mec.blob_mask(W, H, 5, 3, 100, size)
    vec = np.stack([1.0 + rng.random(size), 0.1 * rng.standard_normal(size), 0.1 * rng.standard_normal(size)], -1).astype(np.float32)
    hot = np.array([[np.inf, 0.5, 0.0], [0.0, -np.inf, 1.0], [3e38, 3e38, 0.0], [-3e38, 0.0, 0.0], [np.inf, -np.inf, np.inf]], np.float32)
    who = rng.permutation(size)[:n_inf]
    vec[who] = hot[rng.integers(0, len(hot), size=n_inf)]
    v = np.zeros((H, W, 3), np.float32)
    v[m] = vec
    planes = mec.grid_planes(W, H, v)
    nrm = numpy_ref.norm3(vec[:, 0], vec[:, 1], vec[:, 2])
    assert not np.isnan(nrm).any() and int(np.isposinf(nrm).sum()) == n_inf
    assert np.isposinf(numpy_ref.norm3(*hot[2])) and np.isfinite(hot[2]).all(), "3e38: finite components, norm overflows"
    rounds, exact, value, nties = msm.select(nrm.view(np.uint32))
    assert (value == mec.F32_INF) == median_is_inf and (nties == n_inf if median_is_inf else nties == 1), (value, nties)
    prm = synth.Params(cluster_size=100, neighbor_distance=2)
    ref = oracle.cluster(planes, prm, "tidy", max_objects=8)
    assert ref[2] == 1 and bool(np.isposinf(numpy_ref.norm3(*ref[1][0]["velocity"].astype(np.float32)))) == median_is_inf
    _check(ref, planes, prm, W, H)


def test_every_member_has_the_same_vector(oracle):
    """nties = size > 1 and nothing ambiguous: the canonical pick stands, no tie replay."""
    from moving_object_detector_amd import synth
    W, H, size = 256, 128, 1500
    m = mec.blob_mask(W, H, 5, 3, 100, size)
    v = np.zeros((H, W, 3), np.float32)
    v[m] = np.array([0.6, -0.7, 0.2], np.float32)
    planes = mec.grid_planes(W, H, v)
    rounds, exact, value, nties = msm.select(_norm_bits(planes, m))
    assert exact and len(rounds) == 1 and nties == size > 1
    prm = synth.Params(cluster_size=100, neighbor_distance=2)
    ref = oracle.cluster(planes, prm, "tidy", max_objects=8)
    assert ref[2] == 1 and not ref[1][0]["ambiguous"]
    _check(ref, planes, prm, W, H)


def test_smallest_clusters(oracle):
    """cluster_size = 1.  The reference labels a pixel only through a link to a neighbour, so an isolated pixel is no cluster and the
    smallest cluster has two members (rank size / 2 = 1: the smaller norm); a one-member cluster cannot exist."""
    from moving_object_detector_amd import synth
    from test_gpu_cluster_stress import _make_cloud
    W, H = 96, 64
    rng = np.random.default_rng(8)
    ys, xs = np.mgrid[0:H, 0:W]
    alone = (xs % 6 == 0) & (ys % 8 == 0)
    pair = ((ys % 8 == 3) & (xs % 6 <= 1)) | ((xs % 6 == 3) & (ys % 8 >= 5) & (ys % 8 <= 6) & (xs > 40))      # horizontal, vertical
    pair |= (ys % 8 == 5) & (xs % 6 == 0) & (xs <= 36) | (ys % 8 == 6) & (xs % 6 == 1) & (xs <= 37)            # diagonal (up-left)
    planes = _make_cloud(W, H, alone | pair, np.full((H, W), 5.0), rng)
    prm = synth.Params(cluster_size=1, neighbor_distance=1)
    ref = oracle.cluster(planes, prm, "tidy", max_objects=W * H)
    sizes = [o["n_points"] for o in ref[1]]
    assert ref[2] == len(sizes) > 50 and set(sizes) == {2}, (ref[2], set(sizes))
    assert np.all(ref[0][alone] == -1) and np.all(ref[0][pair] >= 0)
    _check(ref, planes, prm, W, H)


def test_cluster_of_exactly_cluster_size_members(oracle):
    from moving_object_detector_amd import synth
    from test_gpu_cluster_stress import _make_cloud
    W, H, size = 128, 64, 300
    rng = np.random.default_rng(9)
    keep, drop = mec.blob_mask(W, H, 4, 4, 20, size), mec.blob_mask(W, H, 60, 4, 23, size - 1)
    planes = _make_cloud(W, H, keep | drop, np.full((H, W), 5.0), rng)
    prm = synth.Params(cluster_size=size, neighbor_distance=2)
    ref = oracle.cluster(planes, prm, "tidy", max_objects=8)
    assert ref[2] == 1 and ref[1][0]["n_points"] == size and np.all(ref[0][drop] == -1) and np.all(ref[0][keep] == 0)
    _check(ref, planes, prm, W, H)


# ---- c. boxes ---------------------------------------------------------------------------------------------------------------------
BOX_W, BOX_H = 200, 150


def _box_cloud(oracle):
    """Several blobs with distinct velocities, and the oracle's labels of the clean cloud (x and y never decide a link)."""
    from moving_object_detector_amd import synth
    from test_gpu_cluster_stress import _make_cloud
    W, H = BOX_W, BOX_H
    rng = np.random.default_rng(21)
    ys, xs = np.mgrid[0:H, 0:W]
    dyn = ((xs // 50 + ys // 50) % 2 == 0) & (xs % 50 < 40) & (ys % 50 < 38) & (rng.random((H, W)) < 0.9)
    planes = _make_cloud(W, H, dyn, np.full((H, W), 5.0), rng)
    prm = synth.Params(cluster_size=100, neighbor_distance=2)
    lab, objs, K = oracle.cluster(planes, prm, "tidy", max_objects=64)
    assert K == len(objs) == 6
    return planes, prm, lab, rng


def _column_major_ends(lab, k):
    """Pixel (y, x) of cluster k's first and last member in column-major order (smallest / largest x * H + y)."""
    ys, xs = np.nonzero(lab == k)
    key = xs * lab.shape[0] + ys
    return (ys[key.argmin()], xs[key.argmin()]), (ys[key.argmax()], xs[key.argmax()])


def _scatter(rng, plane, members, frac, values):
    hit = members & (rng.random(plane.shape) < frac)
    plane[hit] = rng.choice(np.asarray(values, np.float32), size=int(hit.sum()))
    return hit


@pytest.mark.parametrize("case", ["nan_x", "nan_y", "nan_xyz", "last_member_nan_x", "first_member_nan_x", "inf_xy", "inf_and_nan_xy"])
def test_boxes_with_nan_and_inf_coordinates(oracle, case):
    planes, prm, lab, rng = _box_cloud(oracle)
    W, H = BOX_W, BOX_H
    members = lab >= 0
    inf = [np.inf, -np.inf]
    if case in ("nan_x", "nan_y"):
        assert _scatter(rng, planes[case[-1]], members, 0.05, [np.nan]).sum() > 20
    elif case == "nan_xyz":
        for k in ("x", "y", "z"):                            # (NaN depth links everything in the window: other labels than the clean cloud's)
            assert _scatter(rng, planes[k], members, 0.05, [np.nan, -np.nan]).sum() > 20
    elif case == "last_member_nan_x":
        planes["x"][_column_major_ends(lab, 1)[1]] = np.nan
    elif case == "first_member_nan_x":
        planes["x"][_column_major_ends(lab, 2)[0]] = np.nan
    elif case == "inf_xy":
        assert _scatter(rng, planes["x"], members, 0.03, inf).sum() > 20 and _scatter(rng, planes["y"], members, 0.03, inf).sum() > 20
        planes["x"][lab == 3] = np.inf                       # every member at +inf: the minimum keeps its FLT_MAX start value
        planes["y"][lab == 4] = -np.inf                      # ... and the maximum its -FLT_MAX
    else:
        for k in ("x", "y"):
            assert _scatter(rng, planes[k], members, 0.06, inf + [np.nan]).sum() > 40
        planes["x"][lab == 3] = np.inf
        planes["x"][_column_major_ends(lab, 3)[0]] = np.nan  # the NaN replaces the start value: min = max = +inf after it, inf - inf
    ref = oracle.cluster(planes, prm, "tidy", max_objects=64)
    if case != "nan_xyz":
        assert np.array_equal(ref[0], lab)
    box = np.array([o["bounding_box"] for o in ref[1]])
    ctr = np.array([o["center"] for o in ref[1]])
    if case == "last_member_nan_x":
        assert np.isnan(box[1, 0]) and np.isnan(ctr[1, 0]) and int(np.isnan(box).sum()) == 1, "the oracle's box is meant to be NaN"
    elif case == "first_member_nan_x":
        assert np.isfinite(box).all() and np.isfinite(ctr).all(), "a NaN that the next member replaces leaves no trace"
        xs = planes["x"][lab == 2]
        xs = xs[~np.isnan(xs)]
        assert box[2, 0] == np.float64(xs.max() - xs.min())
    elif case == "inf_xy":
        fmax = np.float32(3.402823466e38)
        assert np.isposinf(box[3, 0]) and np.isposinf(ctr[3, 0]) and np.isposinf(box[4, 1]) and np.isneginf(ctr[4, 1])
        assert ctr[3, 0] == np.float64((fmax + np.float32(np.inf)) / np.float32(2)) and not np.isnan(box).any()
    elif case == "inf_and_nan_xy":
        assert np.isnan(box[3, 0]) and np.isposinf(ctr[3, 0]), (box[3], ctr[3])
        assert np.isnan(box).any() or np.isinf(box).any()
    else:
        assert np.isnan(planes[case[-1] if case != "nan_xyz" else "x"][ref[0] >= 0]).any()
    _check(ref, planes, prm, W, H)


# ---- d. a caller's dynamic mask ---------------------------------------------------------------------------------------------------
def _pack_mask(dyn, words):
    """[H][words] little-endian 64-bit words: bit b of word k of a row = pixel 64 k + b (mod_sf.h, mod_mask_words)."""
    H, W = dyn.shape
    padded = np.zeros((H, words * 64), np.uint8)
    padded[:, :W] = dyn
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").astype(np.uint64).view(np.int64).reshape(H, words)


def test_callers_dynamic_mask(oracle):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context, PLANES
    from oracle import numpy_ref
    from test_gpu_cluster_stress import _make_cloud
    W, H = 200, 150
    rng = np.random.default_rng(31)
    z = 5.0 + 0.1 * rng.integers(0, 3, size=(H, W))
    planes = _make_cloud(W, H, rng.random((H, W)) < 0.15, z, rng)
    prm = synth.Params(cluster_size=5, neighbor_distance=2)
    dyn = numpy_ref.dynamic_mask(prm, planes["vx"], planes["vy"], planes["vz"])
    assert 0.1 < dyn.mean() < 0.2 and W % 64 != 0
    ref = oracle.cluster(planes, prm, "tidy", max_objects=W * H)
    assert ref[2] > 3

    ctx = Context(W, H, max_frames=1, max_objects=W * H // prm.cluster_size + 1)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(prm)
    ws = ctx.workspace(1)
    assert ctx.mask_words == (W + 63) // 64 and tuple(ws["mask"].shape) == (1, H, ctx.mask_words)

    def run(mask_ready):
        for k in ("labels", "objects", "n_objects", "n_clusters"):
            ws[k].fill_(0x55 if k == "objects" else -7)      # nothing of the call before survives
        assert ctx.cluster(1, ws, mask_ready=mask_ready) == 0
        ctx.synchronize()
        return ws["labels"][0].cpu().numpy(), int(ws["n_clusters"][0]), int(ws["n_objects"][0]), ws["objects"][0].cpu().numpy().copy()

    for i, k in enumerate(PLANES):
        ws["planes"][i, 0].copy_(torch.from_numpy(planes[k]))
    ws["mask"].fill_(-1)                                     # (not read by a call without a mask)
    own = run(False)
    assert own[1] == ref[2] and np.array_equal(own[0], ref[0])
    compare_objects_bits(ctx.objects_to_host(ws)[0], ref[1])
    ws["mask"][0].copy_(torch.from_numpy(_pack_mask(dyn, ctx.mask_words)))
    given = run(True)
    assert given[1] == own[1] and given[2] == own[2] and np.array_equal(given[0], own[0])
    assert np.array_equal(given[3][:own[2]], own[3][:own[2]]), "object bytes differ with the caller's mask"
    ctx.close()


# ---- e. tied frames in a batch, twice on one workspace ------------------------------------------------------------------------------
def test_batch_of_tied_frames_twice_on_one_workspace(oracle):
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context, PLANES
    from test_gpu_cluster_stress import _make_cloud
    W, H, F = 160, 96, 4
    ys, xs = np.mgrid[0:H, 0:W]
    prm = synth.Params(cluster_size=200, neighbor_distance=3)
    clouds = []
    for f, seed in ((0, 41), (2, 43)):
        rng = np.random.default_rng(seed)
        dyn = (xs > 8 + 10 * f) & (xs < 120 + 10 * f) & (ys > 6) & (ys < 80) & (rng.random((H, W)) < 0.93)
        clouds.append(mec.tie_cloud(W, H, rng, dyn, 3))
    rng = np.random.default_rng(42)
    distinct = _make_cloud(W, H, (rng.random((H, W)) < 0.8) & (xs > 30), np.full((H, W), 5.0), rng)
    empty = _make_cloud(W, H, np.zeros((H, W), bool), np.full((H, W), 5.0), rng)
    clouds = [clouds[0], distinct, clouds[1], empty]
    refs = [oracle.cluster(cl, prm, "tidy", max_objects=64) for cl in clouds]
    assert all(refs[f][2] >= 1 and all(o["ambiguous"] for o in refs[f][1]) for f in (0, 2))
    assert refs[1][2] >= 1 and not any(o["ambiguous"] for o in refs[1][1]) and refs[3][2] == 0
    assert not bits_equal64(refs[0][1][0]["velocity"], refs[2][1][0]["velocity"])
    ctx = Context(W, H, max_frames=F, max_objects=W * H // prm.cluster_size + 1)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(prm)
    ws = ctx.workspace(F)
    for f, cl in enumerate(clouds):
        for i, k in enumerate(PLANES):
            ws["planes"][i, f].copy_(torch.from_numpy(cl[k]))
    for _ in range(2):                                       # the second call runs over the scratch the first one's tie replay left behind
        assert ctx.cluster(F, ws, mask_ready=False) == 0
        ctx.synchronize()
    labels, objs, K = ws["labels"].cpu().numpy(), ctx.objects_to_host(ws), ws["n_clusters"].cpu().numpy()
    for f in range(F):
        assert int(K[f]) == refs[f][2] and np.array_equal(labels[f], refs[f][0]), f
        compare_objects_bits(objs[f], refs[f][1])
    ctx.close()
