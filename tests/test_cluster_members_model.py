"""CPU: the member layout's model (tests/models/cluster_members_model.py) against a brute-force np.lexsort — random masks, combs,
single rows and columns; boxes of 1 cell, exactly one run, one cell more, several runs (run length 8 to keep this cheap); ymin not a
multiple of 64; row spans of 64, 65 and 128."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import cluster_members_model as model  # noqa: E402


def _brute(pixels, W):
    p = np.asarray(pixels, np.int64)
    v, u = p // W, p % W
    return p[np.lexsort((v, u))].tolist()               # u ascending, then v ascending


def _pixels(mask, x0, y0, W, rng):
    v, u = np.nonzero(mask)
    p = (v + y0) * W + (u + x0)
    return rng.permutation(p).tolist()                  # the list arrives in no particular order


def _check(mask, x0, y0, W, run, rng, want_runs=None, want_cells=None):
    px = _pixels(mask, x0, y0, W, rng)
    got, runs = model.layout(px, W, run)
    assert got == _brute(px, W)
    if want_cells is not None:
        assert model.cell_count(px, W) == want_cells
    if want_runs is not None:
        assert runs == want_runs
    return runs


@pytest.mark.parametrize("density", [0.05, 0.5, 1.0])
@pytest.mark.parametrize("run", [8, 512, 8192])
def test_random_masks(density, run):
    rng = np.random.default_rng(int(density * 100) + run)
    for (h, w, x0, y0, W) in [(30, 40, 3, 5, 130), (197, 6, 20, 3, 64), (70, 9, 0, 61, 97), (1, 1, 7, 7, 16)]:
        m = rng.random((h, w)) < density
        m[0, 0] = True
        _check(m, x0, y0, W, run, rng)


def test_combs_rows_and_columns():
    rng = np.random.default_rng(1)
    ys, xs = np.mgrid[0:30, 0:30]
    _check((xs % 3 == 0), 2, 1, 100, 8, rng)                      # comb of columns
    _check((ys % 3 == 0), 2, 1, 100, 8, rng)                      # comb of rows
    _check(((xs + 30 * ys) % 3 == 0), 2, 1, 100, 8, rng)          # holes inside every cell: ranks depend on the popcount below the bit
    _check(np.ones((1, 50), bool), 4, 9, 64, 8, rng, want_cells=50, want_runs=7)     # a single row
    _check(np.ones((200, 1), bool), 4, 9, 64, 8, rng, want_cells=4, want_runs=1)     # a single column: 200 rows from 9 = 4 cells


@pytest.mark.parametrize("cols,runs", [(1, 1), (8, 1), (9, 2), (29, 4)])
def test_cell_counts_around_the_run_length(cols, runs):
    """1 cell, exactly the run length (8), one more, several runs."""
    rng = np.random.default_rng(cols)
    m = rng.random((40, cols)) < 0.6
    m[0, :] = True
    m[-1, :] = True                                              # the box is 40 rows: one cell per column
    _check(m, 11, 70, 80, 8, rng, want_cells=cols, want_runs=runs)


@pytest.mark.parametrize("span", [64, 65, 128])
@pytest.mark.parametrize("ymin", [0, 1, 63, 64, 100])
def test_row_spans_and_unaligned_tops(span, ymin):
    rng = np.random.default_rng(span * 1000 + ymin)
    m = rng.random((span, 5)) < 0.7
    m[0, 0] = True
    m[-1, -1] = True
    nseg = (span - 1 + 64) // 64                                 # 1, 2, 2 cells per column
    _check(m, 3, ymin, 50, 8, rng, want_cells=5 * nseg)
    _check(np.ones((span, 5), bool), 3, ymin, 50, 8, rng, want_cells=5 * nseg)


def test_interleaved_clusters_share_a_box_but_not_their_lists():
    rng = np.random.default_rng(7)
    ys, xs = np.mgrid[0:30, 0:40]
    even, odd = (xs % 2 == 0), (xs % 2 == 1)
    a = model.layout(_pixels(even, 3, 5, 130, rng), 130, 8)[0]
    b = model.layout(_pixels(odd, 3, 5, 130, rng), 130, 8)[0]
    assert not set(a) & set(b) and len(a) == len(b) == 600
    assert all(p % 130 % 2 == 1 for p in a) and all(p % 130 % 2 == 0 for p in b)   # image origin (3, 5): even block columns are odd image columns
