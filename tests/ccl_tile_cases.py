"""The hostile clouds tests/test_ccl_tile_cases.py (CPU: what each family reaches, from the planes and the oracle alone) and
tests/test_gpu_ccl_tile_wide.py / tests/ccl_tile_checked_worker.py (GPU: csrc/ccl_tile.hip's ccl_tile_body against the oracle, bit
for bit) share.  A plain module, not a conftest: no fixtures, numpy only, every input generated deterministically from a fixed seed.

A case is one frame (`Case`): name, W, H, neighbor_distance n, cluster_size, the dynamic mask and the depth plane [H][W], plus `info`
(what the CPU test needs to know about the construction).  depth_diff is DEPTH_DIFF everywhere.  `_cloud(case)` in the GPU module and the worker's loop
turns it into planes with test_gpu_cluster_stress._make_cloud (velocities distinct per pixel).

ccl_tile_body has four instances: <16, 4, 4, true> (n = 4, tested elsewhere), <16, 4, 4, false> (n = 1 .. 3), <16, 8, 4, false>
(n = 5 .. 8) and <16, 16, 4, false> (n = 9 .. 16).  For n <= 10 it sees only the tiles k_ccl_bits lists (more than four depth
classes, a class not clear of the next, a NaN depth, more than 32 components); for n = 11 .. 16 (NS_GRID) k_ccl_tile<16, 16, 4, false>
runs it over every tile.  NS_LIST are the list windows off the default: 1, 3 -> NMAX 4; 5, 8 -> NMAX 8; 9, 10 -> NMAX 16.

Families:
  window_edge(n)    NS_GRID.  Isolated pixel pairs, one per offset (dx, dy) in [0, n + 1]^2 but (0, 0), the partner up-left of the lower
                    pixel, and up-right pairs (+dx, -dy), dx, dy in {1, n, n + 1}; every other pixel is more than 2 n + 2 away.  The
                    lower pixel sits at tile-local columns 0, n - 1, n, 63 and rows 0, 15, so the partner lies in the tile, the top
                    halo (at n = 16 a whole tile row), the left halo (mL) or the corner halo.  Frames of 320 x 96, one batch per n.
  bars(n)           NS_GRID.  One-pixel bars at gaps n, n + 1, n + 2, vertical and horizontal, 203 x 50 (partial last tile).
  small_images(n)   NS_GRID.  Images narrower / lower than the window or one tile: clamped halo loads, rows and columns outside the image.
  depth_hostile(n)  NS_GRID + NS_LIST.  Five classes (phase B's labels, > kMaxClasses of k_ccl_bits), a ramp and a three-level chain
                    (the `same` shortcut must not fire across a gate), NaN depth (links with everything), rows of +inf / -inf.
  job_queue(n)      11, 16 (grid) and 5, 9 (list, five classes by column).  Every pixel a run of its own linked to the pixel above: 64
                    jobs per row, so phase A2 passes kJobCap = 128 on a wave's third row and push_jobs unites in place.
  many_roots(n)     11, 16 (grid) and 8, 10 (list).  512 two-pixel components per tile: past kSlots = 32, records in HBM behind the
                    extra __syncthreads(), with a 16-wide halo (8 wide at n = 8).
  full_requests(n)  11, 13, 16.  A depth checkerboard: no halo cell has a direct edge to its left or upper neighbour, so every halo cell
                    linked to a tile pixel issues its own link request.  At n = 16 an interior tile fills the request buffer
                    (ccl_request_capacity(n) = n (64 + n) + 16 n) to the last slot; at odd n two halo cells — (row -n, column 63) and
                    (row 15, column -n) — see only one tile pixel, of the other parity, and the tile emits capacity - 2.  The
                    `diagonal` layout (class = (x + y) mod n) fills the buffer at odd n as well.
  mixed_batch(n)    12, 16.  Six frames of 192 x 96 for one call: empty, flat noise, full_requests, job_queue, five-class noise, static.
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name W H n cluster_size dyn z info")

DEPTH_DIFF = 0.15
NS_GRID = (11, 12, 13, 14, 15, 16)
NS_LIST = (1, 3, 5, 8, 9, 10)
TILE_W, TILE_H, WAVES = 64, 16, 4
K_JOB_CAP, K_SLOTS = 128, 32

JOB_QUEUE_NS = (11, 16, 5, 9)
MANY_ROOTS_NS = (11, 16, 8, 10)
FULL_REQUEST_NS = (11, 13, 16)
MIXED_BATCH_NS = (12, 16)


def nmax(n):
    """Halo width of the ccl_tile_body instance that serves window n (launch_ccl_tile)."""
    return 4 if n <= 4 else 8 if n <= 8 else 16


def request_capacity(n):
    return n * (TILE_W + n) + TILE_H * n


def _case(name, n, csize, dyn, z, **info):
    H, W = dyn.shape
    dyn = np.ascontiguousarray(dyn, bool)
    z = np.ascontiguousarray(np.broadcast_to(z, (H, W)), np.float64)
    dyn.setflags(write=False)
    z.setflags(write=False)
    return Case(name, W, H, n, csize, dyn, z, info)


def seed_of(case):
    """Seed of the velocities _make_cloud draws for the case: fixed per name."""
    return sum((i + 1) * ord(ch) for i, ch in enumerate(case.name)) % (2 ** 31)


# ---- window_edge ------------------------------------------------------------------------------------------------------------------
EDGE_W, EDGE_H = 320, 96


@functools.lru_cache(maxsize=None)
def window_edge(n):
    """Frames of one batch.  info["pairs"]: (dx, dy, upright, (x, y) of the lower pixel, (x, y) of the partner) per pair of the frame."""
    cols, rows = (0, n - 1, n, TILE_W - 1), (0, TILE_H - 1)
    anchors = [(cx, cy) for cy in rows for cx in cols]
    want = []                                                    # (dx, dy, upright, anchor or None = any, taken in turn)
    k = 0
    for dy in range(n + 2):
        for dx in range(n + 2):
            if dx or dy:
                want.append((dx, dy, False, anchors[k % 8])); k += 1
    for dy in (0, n, n + 1):                                      # the offsets around the edge of the window at EVERY anchor
        for dx in (0, n, n + 1):
            if dx or dy:
                want.extend((dx, dy, False, a) for a in anchors)
    k = 0
    for dy in (1, n, n + 1):
        for dx in (1, n, n + 1):
            want.append((dx, dy, True, anchors[k % 8])); k += 1
    far = 2 * n + 2                                               # every other pixel is MORE than this away (Chebyshev)
    frames = []                                                   # [list of pixels (x, y)], [pairs]
    for dx, dy, upright, (cx, cy) in want:
        placed = False
        for fr in frames + [None]:
            if fr is None:
                fr = ([], [])
                frames.append(fr)
            pts = np.array(fr[0], int).reshape(-1, 2)
            for ty in range(EDGE_H // TILE_H):
                for tx in range(EDGE_W // TILE_W):
                    x, y = tx * TILE_W + cx, ty * TILE_H + cy
                    px, py = (x + dx if upright else x - dx), y - dy
                    if px < 0 or px >= EDGE_W or py < 0:
                        continue
                    if len(pts):
                        d = np.minimum(np.abs(pts - (x, y)).max(axis=1), np.abs(pts - (px, py)).max(axis=1))
                        if d.min() <= far:
                            continue
                    fr[0].extend([(x, y), (px, py)])
                    fr[1].append((dx, dy, upright, (x, y), (px, py)))
                    placed = True
                    break
                if placed:
                    break
            if placed:
                break
        assert placed, (n, dx, dy, upright, cx, cy)
    out = []
    for i, (pts, pairs) in enumerate(frames):
        dyn = np.zeros((EDGE_H, EDGE_W), bool)
        for x, y in pts:
            dyn[y, x] = True
        out.append(_case(f"window_edge_n{n}_f{i}", n, 2, dyn, 5.0, pairs=tuple(pairs)))
    return tuple(out)


# ---- bars, small images -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bars(n):
    W, H = 203, 50
    out = []
    for gap in (n, n + 1, n + 2):
        d = np.zeros((H, W), bool); d[:, ::gap] = True
        out.append(_case(f"bars_n{n}_v{gap}", n, 2, d, 5.0, gap=gap))
        d = np.zeros((H, W), bool); d[::gap, :] = True
        out.append(_case(f"bars_n{n}_h{gap}", n, 2, d, 5.0, gap=gap))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def small_images(n):
    rng = np.random.default_rng(7700 + n)
    shapes = ((1, 40), (40, 1), (1, 1), (n - 1, n - 1), (n, n), (n + 1, 17), (15, 33), (65, 17), (63, 16))
    return tuple(_case(f"small_n{n}_{W}x{H}", n, 2, rng.random((H, W)) < 0.7, 5.0) for W, H in shapes)


# ---- depth_hostile ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def depth_hostile(n):
    W, H = 200, 50
    rng = np.random.default_rng(4100 + n)
    out = []

    def add(layout, density, z, **info):
        dyn = np.ones((H, W), bool) if density == 1.0 else rng.random((H, W)) < density
        out.append(_case(f"depth_n{n}_{layout}_{int(density * 100)}", n, 3, dyn, z, layout=layout, **info))

    five = 5.0 + 0.3 * rng.integers(0, 5, size=(H, W))             # five classes clear of each other
    add("five", 1.0, five, levels=5, step=0.3)
    add("five", 0.25, five, levels=5, step=0.3)
    add("ramp", 1.0, 5.0 + 0.05 * rng.integers(0, 8, size=(H, W)))  # 8 x 0.05: no class is clear of the next
    add("ramp_columns", 0.25, 5.0 + 0.05 * ((np.arange(W)[None, :] // 7) % 8) + np.zeros((H, 1)))
    add("chain3", 1.0, 5.0 + 0.1 * rng.integers(0, 3, size=(H, W)))  # 0.1 links, 0.2 does not: pairwise, not end to end
    add("chain3_halves", 0.25, 5.0 + 0.1 * (np.arange(H)[:, None] * 3 // H) + np.zeros((1, W)))
    z = np.full((H, W), 6.0)
    z[:, 100:] = 7.0
    z[rng.random((H, W)) < 0.02] = np.nan                           # NaN links with everything: bridges the two depths
    add("nan", 0.5, z)
    z = np.full((H, W), 6.0)
    z[10:20, :] = np.inf                                            # inf - inf = NaN links, inf - 6 does not: a class of its own
    z[30:35, :] = -np.inf
    add("inf_rows", 1.0, z)
    return tuple(out)


# ---- job_queue ----------------------------------------------------------------------------------------------------------------------
def _column_classes(W, H, n):
    """Depth constant per column, neighbouring columns more than DEPTH_DIFF apart: two classes on the grid path, five (so that
    k_ccl_bits gives the tile up) on the list path."""
    k = 2 if n > 10 else 5
    step = 1.0 if k == 2 else 0.3
    return 5.0 + step * (np.arange(W)[None, :] % k) + np.zeros((H, 1)), k


@functools.lru_cache(maxsize=None)
def job_queue(n):
    W, H = 192, 48
    z, k = _column_classes(W, H, n)
    return _case(f"job_queue_n{n}", n, 2, np.ones((H, W), bool), z, classes=k)


def vertical_run_pairs(case, tx, ty, w):
    """Distinct (run, run above) pairs that phase A2 queues for wave w of tile (tx, ty): the wave's tile rows w, w + 4, w + 8, w + 12
    and its halo rows (grid rows NMAX - 1 - w, NMAX - 5 - w, ... above NMAX - n), each against the row above, over the 64 tile columns.
    A run is a stretch of dynamic pixels each linked to its left neighbour; a pair counts when some column of it links vertically."""
    n, NM = case.n, nmax(case.n)
    x0, y0 = tx * TILE_W, ty * TILE_H
    zf = case.z.astype(np.float32)

    def runs(y):
        d, zr = case.dyn[y, x0:x0 + TILE_W], zf[y, x0:x0 + TILE_W]
        link = d[1:] & d[:-1] & ~(np.abs(zr[1:] - zr[:-1]) > np.float32(DEPTH_DIFF))
        return np.concatenate(([0], np.cumsum(~link)))
    grid_rows = [NM + w + WAVES * j for j in range(TILE_H // WAVES)] + list(range(NM - 1 - w, NM - n, -WAVES))
    total = 0
    for gr in grid_rows:
        y = y0 - NM + gr
        if y < 1 or y >= case.H:
            continue
        both = case.dyn[y, x0:x0 + TILE_W] & case.dyn[y - 1, x0:x0 + TILE_W]
        link = both & ~(np.abs(zf[y, x0:x0 + TILE_W] - zf[y - 1, x0:x0 + TILE_W]) > np.float32(DEPTH_DIFF))
        total += len(set(zip(runs(y)[link].tolist(), runs(y - 1)[link].tolist())))
    return total


# ---- many_roots ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_roots(n):
    W, H = 128, 32
    ys, xs = np.mgrid[0:H, 0:W]
    cls = (xs // 2) % 16 + 16 * (ys % 32)                           # no two dominoes within any 17 x 17 window share a class
    return _case(f"many_roots_n{n}", n, 2, np.ones((H, W), bool), 5.0 + 0.5 * cls, dominoes=W * H // 2)


# ---- full_requests ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_requests(n):
    """The depth checkerboard at 192 x 48 and 150 x 40 (two clusters), plus — at odd n, where the checkerboard stops two requests short
    of the capacity — the diagonal layout at 192 x 48: class (x + y) mod n, 1.0 apart (n clusters)."""
    out = []
    for W, H in ((192, 48), (150, 40)):
        ys, xs = np.mgrid[0:H, 0:W]
        out.append(_case(f"full_requests_n{n}_{W}x{H}", n, 2, np.ones((H, W), bool), np.where((xs + ys) % 2 == 0, 5.0, 6.0),
                         layout="checkerboard", clusters=2, requests=request_capacity(n) - (2 if n % 2 else 0)))
    if n % 2:
        W, H = 192, 48
        ys, xs = np.mgrid[0:H, 0:W]
        out.append(_case(f"full_requests_n{n}_diagonal", n, 2, np.ones((H, W), bool), 5.0 + 1.0 * ((xs + ys) % n),
                         layout="diagonal", clusters=n, requests=request_capacity(n)))
    return tuple(out)


def own_requests(case, tx, ty):
    """Link requests tile (tx, ty) issues by phase C's rule, counted for layouts in which a halo cell joins a tile pixel's set only by a
    direct edge: the dynamic halo cells (n rows above the tile over n + 64 columns, n columns left of its rows) with a tile pixel that
    passes the depth gate in their down-right window and no direct edge to their left or upper halo neighbour."""
    n = case.n
    x0, y0 = tx * TILE_W, ty * TILE_H
    zf = case.z.astype(np.float32)
    th = np.float32(DEPTH_DIFF)

    def edge(ax, ay, bx, by):
        return case.dyn[ay, ax] and case.dyn[by, bx] and not (np.abs(zf[ay, ax] - zf[by, bx]) > th)

    def is_halo(x, y):
        return x0 - n <= x < x0 + TILE_W and y0 - n <= y < y0 + TILE_H and (x < x0 or y < y0) and x >= 0 and y >= 0
    count = 0
    for y in range(max(y0 - n, 0), min(y0 + TILE_H, case.H)):
        for x in range(max(x0 - n, 0), min(x0 + TILE_W, case.W)):
            if not is_halo(x, y) or not case.dyn[y, x]:
                continue
            ys = slice(max(y, y0), min(y + n, y0 + TILE_H - 1, case.H - 1) + 1)
            xs = slice(max(x, x0), min(x + n, x0 + TILE_W - 1, case.W - 1) + 1)
            win = case.dyn[ys, xs] & ~(np.abs(zf[ys, xs] - zf[y, x]) > th)
            if not win.any():
                continue
            if (is_halo(x - 1, y) and edge(x, y, x - 1, y)) or (is_halo(x, y - 1) and edge(x, y, x, y - 1)):
                continue
            count += 1
    return count


# ---- mixed_batch --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_batch(n):
    W, H = 192, 96
    rng = np.random.default_rng(1200 + n)
    ys, xs = np.mgrid[0:H, 0:W]
    none, full = np.zeros((H, W), bool), np.ones((H, W), bool)
    frames = (("empty", none, np.full((H, W), np.nan)),
              ("flat_noise", rng.random((H, W)) < 0.5, 5.0),
              ("full_requests", full, np.where((xs + ys) % 2 == 0, 5.0, 6.0)),
              ("job_queue", full, _column_classes(W, H, n)[0]),
              ("five_noise", rng.random((H, W)) < 0.6, 5.0 + 0.3 * rng.integers(0, 5, size=(H, W))),
              ("static", none, 5.0 + 0.3 * rng.integers(0, 5, size=(H, W))))
    return tuple(_case(f"mixed_n{n}_{name}", n, 3, d, z) for name, d, z in frames)


# ---- what the checked build runs first (tests/ccl_tile_checked_worker.py): the families whose indices depend on the data -----------
def index_critical():
    out = []
    for n in FULL_REQUEST_NS:
        out.extend(full_requests(n))
    for n in NS_GRID:
        out.extend(small_images(n))
    out.extend(many_roots(n) for n in MANY_ROOTS_NS)
    out.extend(job_queue(n) for n in JOB_QUEUE_NS)
    return out
