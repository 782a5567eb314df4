"""The member layout of csrc/cluster_common.h (member_box / member_layout: k_median_ties, k_cluster_members) restated step for step on
Python integers: a cluster's pixel indices, in any order, come out in the reference's order (column-major: u ascending, then v
ascending, clusterMap2IndicesCluster, clusterer_nodelet.cpp:97-117) without a sort.

  box      image-space bounding box of the members (exact integer divide for row and column);
  cells    one column x 64 rows, numbered column-major: cell = (x - xmin) * nseg64 + ((y - ymin) >> 6), nseg64 = (ymax - ymin + 64) // 64;
  pass A   bit (y - ymin) & 63 of the member's cell is set in a 64-bit mask;
  prefix   exclusive prefix of the cell populations in cell order, continued from `base`;
  pass B   member -> slot start[cell] + popcount(mask[cell] below its bit);
  runs     a box of more cells than `run` (the LDS arrays: 8192 for a workgroup, 512 for a wave) takes passes A and B once per run
           of `run` cells; `base` carries the members of the runs before.
"""

MASK64 = (1 << 64) - 1


def row_col(p, W):
    y = p // W
    return y, p - y * W


def box(pixels, W):
    xs = [row_col(p, W)[1] for p in pixels]
    ys = [row_col(p, W)[0] for p in pixels]
    return min(xs), max(xs), min(ys), max(ys)


def layout(pixels, W, run=8192):
    """The members in the reference's order, and the number of runs taken."""
    size = len(pixels)
    assert size >= 1
    xmin, xmax, ymin, ymax = box(pixels, W)
    ncols = xmax - xmin + 1
    nseg64 = (ymax - ymin + 64) // 64
    ncell = ncols * nseg64

    def cell_of(p):
        y, x = row_col(p, W)
        ry = y - ymin
        return (x - xmin) * nseg64 + (ry >> 6), ry & 63

    out = [None] * size
    base, runs = 0, 0
    for g0 in range(0, ncell, run):
        ncl = min(run, ncell - g0)
        mask = [0] * run
        for p in pixels:                                  # pass A
            cl, bit = cell_of(p)
            cl -= g0
            if 0 <= cl < ncl:
                mask[cl] |= 1 << bit
        start, acc = [0] * run, base                      # prefix
        for i in range(run):
            start[i] = acc
            acc += bin(mask[i] & MASK64).count("1") if i < ncl else 0
        base = acc
        for p in pixels:                                  # pass B
            cl, bit = cell_of(p)
            cl -= g0
            if 0 <= cl < ncl:
                slot = start[cl] + bin(mask[cl] & ((1 << bit) - 1)).count("1")
                assert 0 <= slot < size and out[slot] is None
                out[slot] = p
        runs += 1
    assert base == size, "every member lies in exactly one cell"
    return out, runs


def cell_count(pixels, W):
    xmin, xmax, ymin, ymax = box(pixels, W)
    return (xmax - xmin + 1) * ((ymax - ymin + 64) // 64)
