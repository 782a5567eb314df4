"""GPU: the union-find tile body (csrc/ccl_tile.hip ccl_tile_body) where it works alone — neighbor_distance 11 .. 16, which
launch_ccl_tile serves with k_ccl_tile<16, 16, 4, false> over the whole grid — and its list instances off the default window, on the
cases of tests/ccl_tile_cases.py (tests/test_ccl_tile_cases.py shows on the CPU what each reaches).  Everything goes through the
clusterer alone (mod_cluster_dev on caller-supplied planes) against oracle.cluster(..., "tidy"): labels, cluster count and object
records bit for bit, then again without a labels plane.  No tolerances.

Instance of ccl_tile_body reached, and the internal limit crossed, per family:
  window_edge     grid <16,16,4,false> (n = 11 .. 16).  The window's edge: partners at distance n / n + 1 in the tile, the top halo (at
                  n = 16 a whole tile row: PH = 32, PW = 80), the left halo (mL) and the corner halo; up-right neighbours never link.
  bars            grid <16,16,4,false>.  Gaps n, n + 1, n + 2 along rows and columns; a partial last tile column (203 = 3 x 64 + 11).
  small_images    grid <16,16,4,false>.  Images narrower / lower than the window and than one tile: clamped halo loads.
  depth_hostile   grid <16,16,4,false> (n = 11 .. 16) and list <16,4,4,false> (n = 1, 3), <16,8,4,false> (n = 5, 8), <16,16,4,false>
                  (n = 9, 10).  Phase B's labels and its `same` shortcut: five classes, ramps, chains, NaN and infinite depth.
  job_queue       grid <16,16,4,false> (n = 11, 16), list <16,8,4,false> (n = 5), <16,16,4,false> (n = 9).  kJobCap = 128 unions per
                  wave: push_jobs unites in place from a wave's third row on.
  many_roots      grid <16,16,4,false> (n = 11, 16), list <16,8,4,false> (n = 8), <16,16,4,false> (n = 10).  kSlots = 32 tile roots in
                  LDS: 512 roots per tile, records initialised in HBM and fed with global atomics.
  full_requests   grid <16,16,4,false> (n = 11, 13, 16).  ccl_request_capacity(n) = n (64 + n) + 16 n link requests per tile: filled to
                  the last slot (checkerboard at n = 16, diagonal classes at n = 11, 13; the checkerboard at odd n stops two short), and
                  k_ccl_link consumes a full tile.
  mixed_batch     grid <16,16,4,false> (n = 12, 16).  Six frames, two calls on one workspace: headers, counters and requests per frame.
  fused path      grid <16,16,4,false> (n = 11, 14, 16) behind the scene-flow epilogue's tile headers instead of k_tile_flags'.
  one context     n = 2, 16, 11, 4 in turn: list <16,4,4,false>, grid, grid, list <16,4,4,true>; the request scratch grows and stays.

full_requests, small_images, many_roots and job_queue derive indices from the data, so they run through the CHECKED build first
(tests/ccl_tile_checked_worker.py in a child process): the product-build tests of these families fail without touching the GPU when
a violation counter is non-zero — an index error shows as a count, not as a fault."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ccl_tile_cases as cc
from test_gpu_ccl_bits import _fused
from test_gpu_cluster_stress import _check, _cluster_gpu, _make_cloud
from util import compare_objects, compare_objects_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _prm(case):
    from moving_object_detector_amd import synth
    return synth.Params(cluster_size=case.cluster_size, neighbor_distance=case.n, depth_diff=cc.DEPTH_DIFF, dynamic_speed=0.3)


def _cloud(case):
    return _make_cloud(case.W, case.H, case.dyn, case.z, np.random.default_rng(cc.seed_of(case)))


def _run(oracle, case):
    if np.isfinite(case.z[case.dyn]).all():
        return _check(oracle, _cloud(case), _prm(case), case.W, case.H)
    # NaN / infinite depth reaches the records (a small cluster's median depth): _check with NaN == NaN at the same position
    planes, prm = _cloud(case), _prm(case)
    lab, objs, K = _cluster_gpu(planes, prm, case.W, case.H)
    rl, ro, rK = oracle.cluster(planes, prm, "tidy", max_objects=case.W * case.H // 2 + 16)
    assert K == rK, (K, rK)
    assert np.array_equal(lab, rl), int((lab != rl).sum())
    compare_objects_bits(objs, ro)


def _check_batch(oracle, frames, calls=1):
    """_check for the frames of one batch (same size and parameters): one context, `calls` calls on one workspace."""
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context, PLANES
    W, H, F, prm = frames[0].W, frames[0].H, len(frames), _prm(frames[0])
    clouds = [_cloud(f) for f in frames]
    ctx = Context(W, H, max_frames=F, max_objects=W * H // prm.cluster_size + 1)
    ctx.set_camera(synth.make_camera(W, H))
    ctx.set_params(prm)
    ws = ctx.workspace(F)
    for f, cl in enumerate(clouds):
        for i, k in enumerate(PLANES):
            ws["planes"][i, f].copy_(torch.from_numpy(cl[k]))
    for _ in range(calls):                                            # a second call runs over the headers, lists and requests of the first
        assert ctx.cluster(F, ws, mask_ready=False) == 0
    ctx.synchronize()
    labels, objs, K = ws["labels"].cpu().numpy(), ctx.objects_to_host(ws), ws["n_clusters"].cpu().numpy()
    raw, n_obj = ws["objects"].cpu().numpy().copy(), ws["n_objects"].cpu().numpy().copy()
    for f, cl in enumerate(clouds):
        rl, ro, rK = oracle.cluster(cl, prm, "tidy", max_objects=W * H // 2 + 16)
        assert int(K[f]) == rK, (frames[f].name, int(K[f]), rK)
        assert np.array_equal(labels[f], rl), (frames[f].name, int((labels[f] != rl).sum()))
        compare_objects(objs[f], ro, strict_velocity=True)
    ws2 = ctx.workspace(F, labels=False)                              # the same batch without a labels plane: identical objects
    assert ws2["labels"] is None
    for f, cl in enumerate(clouds):
        for i, k in enumerate(PLANES):
            ws2["planes"][i, f].copy_(torch.from_numpy(cl[k]))
    ws2["objects"].zero_()
    for _ in range(calls):
        assert ctx.cluster(F, ws2, mask_ready=False) == 0
    ctx.synchronize()
    assert np.array_equal(ws2["n_objects"].cpu().numpy(), n_obj) and np.array_equal(ws2["n_clusters"].cpu().numpy(), K)
    raw2 = ws2["objects"].cpu().numpy()
    for f in range(F):
        assert np.array_equal(raw2[f, :n_obj[f]], raw[f, :n_obj[f]]), (frames[f].name, "objects differ without the labels plane")
    ctx.close()


@pytest.fixture(scope="module")
def checked():
    """The index-critical families through the checked build, in a fresh child process, before the product build runs them."""
    lib = os.path.join(ROOT, "moving_object_detector_amd", "libmod_sf_checked.so")
    if not os.path.exists(lib):                                       # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "moving_object_detector_amd", "csrc"), "checked"], stdout=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ccl_tile_checked_worker.py")], env=dict(os.environ, MOD_SF_LIB=lib),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _index_clean(checked, cases):
    """No GPU work on the product build unless the checked build ran these very cases without a violation (12, 13 in particular)."""
    assert all(v == 0 for v in checked["violations"].values()), checked["violations"]
    assert checked["violations"]["12"] == 0 and checked["violations"]["13"] == 0
    assert set(c.name for c in cases) <= set(checked["ran"])
    assert not set(c.name for c in cases) & set(checked["differ"]), checked["differ"]


def test_checked_build_ran_every_index_critical_case(checked):
    assert checked["ran"] == [c.name for c in cc.index_critical()]
    assert all(v == 0 for v in checked["violations"].values()), checked["violations"]
    assert checked["differ"] == []


@pytest.mark.parametrize("n", cc.NS_GRID)
def test_window_edge(oracle, n):
    _check_batch(oracle, cc.window_edge(n))


@pytest.mark.parametrize("n", cc.NS_GRID)
def test_bars(oracle, n):
    for case in cc.bars(n):
        _run(oracle, case)


@pytest.mark.parametrize("n", cc.NS_GRID)
def test_small_images(oracle, checked, n):
    _index_clean(checked, cc.small_images(n))
    for case in cc.small_images(n):
        _run(oracle, case)


@pytest.mark.parametrize("n", cc.NS_GRID + cc.NS_LIST)
def test_depth_hostile(oracle, n):
    for case in cc.depth_hostile(n):
        _run(oracle, case)


@pytest.mark.parametrize("n", cc.JOB_QUEUE_NS)
def test_job_queue(oracle, checked, n):
    _index_clean(checked, [cc.job_queue(n)])
    _run(oracle, cc.job_queue(n))


@pytest.mark.parametrize("n", cc.MANY_ROOTS_NS)
def test_many_roots(oracle, checked, n):
    _index_clean(checked, [cc.many_roots(n)])
    _run(oracle, cc.many_roots(n))


@pytest.mark.parametrize("n", cc.FULL_REQUEST_NS)
def test_full_requests(oracle, checked, n):
    _index_clean(checked, cc.full_requests(n))
    for case in cc.full_requests(n):
        _run(oracle, case)


@pytest.mark.parametrize("n", cc.MIXED_BATCH_NS)
def test_mixed_batch(oracle, n):
    _check_batch(oracle, cc.mixed_batch(n), calls=2)


@pytest.mark.parametrize("W,H", [(200, 60), (257, 33)])
@pytest.mark.parametrize("n", [11, 14, 16])
def test_fused_path(oracle, n, W, H):
    """mod_process_dev: the scene-flow epilogue, not k_tile_flags, writes the tile headers k_ccl_tile skips on."""
    from moving_object_detector_amd import synth
    cam = synth.make_camera(W, H)
    rng = np.random.default_rng(n * 1000 + W)
    xs = np.arange(W)[None, :] + np.zeros((H, 1), int)
    prm = synth.Params(dynamic_flow_diff=1, cluster_size=2, neighbor_distance=n, depth_diff=cc.DEPTH_DIFF, dynamic_speed=0.05)
    total = 0
    for z in (np.full((H, W), 4.0), np.where(xs % 64 < 50, 4.0, 4.6) + 0.0):
        for density in (0.35, 1.0):
            total += _fused(oracle, cam, prm, z, rng.random((H, W)) < density)
    assert total > 0


def test_one_context_across_windows(oracle):
    """n = 2, 16, 11, 4 on one context with one cloud: the list counters and the grid path alternate, the link-request scratch grows
    at n = 16 and stays.  Each result equals a fresh context's (and the oracle's)."""
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import Context, PLANES
    W, H = 200, 60
    rng = np.random.default_rng(21)
    planes = _make_cloud(W, H, rng.random((H, W)) < 0.6, 5.0 + 0.3 * rng.integers(0, 5, size=(H, W)), rng)
    ctx = Context(W, H, max_frames=1, max_objects=W * H // 3 + 1)
    ctx.set_camera(synth.make_camera(W, H))
    ws = ctx.workspace(1)
    for i, k in enumerate(PLANES):
        ws["planes"][i, 0].copy_(torch.from_numpy(planes[k]))
    for n in (2, 16, 11, 4):
        prm = synth.Params(cluster_size=3, neighbor_distance=n, depth_diff=cc.DEPTH_DIFF, dynamic_speed=0.3)
        ctx.set_params(prm)
        assert ctx.cluster(1, ws, mask_ready=False) == 0
        ctx.synchronize()
        lab, K, objs = ws["labels"][0].cpu().numpy(), int(ws["n_clusters"][0]), ctx.objects_to_host(ws)[0]
        flab, fobjs, fK = _cluster_gpu(planes, prm, W, H)
        assert K == fK and len(objs) == len(fobjs), (n, K, fK)
        assert np.array_equal(lab, flab), (n, int((lab != flab).sum()))
        assert objs.tobytes() == fobjs.tobytes(), n
        rl, ro, rK = oracle.cluster(planes, prm, "tidy", max_objects=W * H // 2 + 16)
        assert K == rK and np.array_equal(lab, rl), n
        compare_objects(objs, ro, strict_velocity=True)
    ctx.close()
