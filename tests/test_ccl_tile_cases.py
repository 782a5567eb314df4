"""CPU: the families of tests/ccl_tile_cases.py hold what they claim — shown from the planes and the oracle alone, so that a green run
of tests/test_gpu_ccl_tile_wide.py means the limits of ccl_tile_body (kJobCap, kSlots, the link-request capacity, the window's edge)
were in fact reached."""
import numpy as np
import pytest

import ccl_tile_cases as cc
from test_gpu_cluster_stress import _make_cloud


def _prm(case):
    from moving_object_detector_amd import synth
    return synth.Params(cluster_size=case.cluster_size, neighbor_distance=case.n, depth_diff=cc.DEPTH_DIFF, dynamic_speed=0.3)


def _oracle(oracle, case):
    planes = _make_cloud(case.W, case.H, case.dyn, case.z, np.random.default_rng(cc.seed_of(case)))
    return oracle.cluster(planes, _prm(case), "tidy", max_objects=case.W * case.H // 2 + 16)


@pytest.mark.parametrize("n", cc.NS_GRID)
def test_window_edge_pairs_straddle_the_reference_window(oracle, n):
    frames = cc.window_edge(n)
    assert all(f.W <= 320 and f.H <= 96 and f.cluster_size == 2 for f in frames)
    linked, upright, cols, rows = {}, [], set(), set()
    for f in frames:
        lab, objs, K = _oracle(oracle, f)
        pts = np.argwhere(f.dyn)
        assert len(pts) == 2 * len(f.info["pairs"])
        # no third pixel in reach of any pair: every other pixel is more than 2 n + 2 away
        d = np.abs(pts[:, None, :] - pts[None, :, :]).max(axis=2)
        assert ((d <= 2 * n + 2).sum(axis=1) == 2).all()
        for dx, dy, ur, (x, y), (px, py) in f.info["pairs"]:
            assert f.dyn[y, x] and f.dyn[py, px] and (py, px) == (y - dy, x + dx if ur else x - dx)
            a, b = int(lab[y, x]), int(lab[py, px])
            assert (a >= 0) == (b >= 0) and (a < 0 or a == b)
            if ur:
                upright.append(a >= 0)
            else:
                linked.setdefault((dx, dy), set()).add(a >= 0)
            cols.add(x % 64); rows.add(y % 16)
        assert K == sum(int(lab[y, x]) >= 0 for _, _, _, (x, y), _ in f.info["pairs"])
    assert cols == {0, n - 1, n, 63} and rows == {0, 15}                       # partner in the tile, the top, left and corner halo
    assert set(linked) == {(dx, dy) for dx in range(n + 2) for dy in range(n + 2)} - {(0, 0)}
    assert all(len(v) == 1 for v in linked.values())                            # an offset links everywhere or nowhere
    yes = {k for k, v in linked.items() if True in v}
    assert yes and len(yes) < len(linked)                                       # some pairs are clusters, some are not
    m = max(max(k) for k in yes)                                                # the reference's window, as the oracle shows it
    assert yes == {(dx, dy) for dx in range(m + 1) for dy in range(m + 1)} - {(0, 0)}
    assert m == n                                                               # so the offsets n and n + 1 straddle its edge
    assert len(upright) == 9 and not any(upright)                               # up-right neighbours are never tested


@pytest.mark.parametrize("n", cc.NS_GRID)
def test_bars_link_up_to_the_window_and_not_beyond(oracle, n):
    got = {}
    for c in cc.bars(n):
        assert (c.W, c.H) == (203, 50)
        got.setdefault(c.info["gap"], []).append(_oracle(oracle, c)[2])
    assert set(got) == {n, n + 1, n + 2}
    assert got[n] == [1, 1]                                                     # bars n apart link: one cluster
    for gap in (n + 1, n + 2):                                                  # further apart: every bar a cluster of its own
        assert got[gap] == [len(range(0, 203, gap)), len(range(0, 50, gap))]


@pytest.mark.parametrize("n", cc.NS_GRID)
def test_small_images_are_smaller_than_the_window_or_one_tile(n):
    shapes = [(c.W, c.H) for c in cc.small_images(n)]
    assert shapes == [(1, 40), (40, 1), (1, 1), (n - 1, n - 1), (n, n), (n + 1, 17), (15, 33), (65, 17), (63, 16)]
    for c in cc.small_images(n):
        assert c.dyn.any() or c.W * c.H == 1
        assert np.all(c.z == 5.0)


@pytest.mark.parametrize("n", cc.JOB_QUEUE_NS)
def test_job_queue_passes_the_job_capacity(oracle, n):
    c = cc.job_queue(n)
    assert c.dyn.all()
    counts = [cc.vertical_run_pairs(c, 1, 1, w) for w in range(cc.WAVES)]      # an interior tile of the 3 x 3
    assert min(counts) > cc.K_JOB_CAP, counts
    # 64 distinct pairs per row: the queue is full after two rows, the third is united in place
    assert all(k % 64 == 0 for k in counts)
    lab, _, K = _oracle(oracle, c)
    assert K == c.info["classes"] and (lab >= 0).all()
    if n <= 10:                                                                 # more classes than k_ccl_bits peels off: the tile is listed
        assert c.info["classes"] > 4 and len(np.unique(c.z[16:32, 64:128])) > 4


@pytest.mark.parametrize("n", cc.MANY_ROOTS_NS)
def test_many_roots_overflow_the_lds_slots(oracle, n):
    c = cc.many_roots(n)
    lab, objs, K = _oracle(oracle, c)
    assert K == c.info["dominoes"] == 2048 and len(objs) == K
    first = {}
    for p, l in enumerate(lab.ravel().tolist()):
        first.setdefault(l, p)
    in_tile = sum(1 for l, p in first.items() if l >= 0 and p // c.W < 16 and p % c.W < 64)
    assert in_tile > cc.K_SLOTS and in_tile == 512
    if n <= 10:
        assert len(np.unique(c.z[:16, :64])) > 4


@pytest.mark.parametrize("n", cc.FULL_REQUEST_NS)
def test_full_requests_fill_the_request_buffer(oracle, n):
    cap = n * (64 + n) + 16 * n
    assert cc.request_capacity(n) == cap
    full = 0
    for c in cc.full_requests(n):
        got = cc.own_requests(c, 1, 1)                                          # the interior tile (complete in 150 x 40 too)
        assert got == c.info["requests"] <= cap, (c.name, got)
        # the checkerboard misses the capacity by the two halo cells that see ONE tile pixel, of the other parity, when n is odd
        assert got == (cap if c.info["layout"] == "diagonal" or n % 2 == 0 else cap - 2)
        full += got == cap
        for tx in range((c.W + 63) // 64):                                      # no tile can ask for more than its share of the buffer
            for ty in range((c.H + 15) // 16):
                assert cc.own_requests(c, tx, ty) <= cap
        lab, _, K = _oracle(oracle, c)
        assert K == c.info["clusters"] and (lab >= 0).all()
        if c.info["layout"] == "checkerboard":
            assert K == 2
    assert full >= 1                                                            # every n has a case that fills the buffer to the last slot


@pytest.mark.parametrize("n", cc.NS_GRID + cc.NS_LIST)
def test_depth_hostile_layouts_cluster(oracle, n):
    cases = cc.depth_hostile(n)
    assert sorted({c.info["layout"] for c in cases}) == ["chain3", "chain3_halves", "five", "inf_rows", "nan", "ramp", "ramp_columns"]
    for c in cases:
        assert (c.W, c.H) == (200, 50)
        lab, objs, K = _oracle(oracle, c)
        assert K >= 1 and len(objs) == K, c.name
        if c.info["layout"] == "five":
            zt = c.z[16:32, 64:128][c.dyn[16:32, 64:128]]
            lv = np.unique(zt)
            assert len(lv) >= 5 and np.all(np.diff(lv) > cc.DEPTH_DIFF)         # five classes clear of each other in one tile
        if c.info["layout"] == "nan":
            assert np.isnan(c.z[c.dyn]).any()
        if c.info["layout"] == "inf_rows":
            assert np.isposinf(c.z).any() and np.isneginf(c.z).any()


@pytest.mark.parametrize("n", cc.MIXED_BATCH_NS)
def test_mixed_batch_frames(oracle, n):
    frames = cc.mixed_batch(n)
    assert len(frames) == 6 and all((f.W, f.H) == (192, 96) for f in frames)
    ks = [_oracle(oracle, f)[2] for f in frames]
    assert ks[0] == 0 and ks[5] == 0 and all(k >= 1 for k in ks[1:5]) and ks[2] == 2 and ks[3] == 2
    assert min(cc.vertical_run_pairs(frames[3], 1, 2, w) for w in range(cc.WAVES)) > cc.K_JOB_CAP
    assert cc.own_requests(frames[2], 1, 2) == cc.request_capacity(n) - (2 if n % 2 else 0)
